// lstm_seq.h -- the caller side of the hot path: the parameter network that
// feeds hbvx_forward is an LSTM over the same [T, B] grid (delta-MG's CudnnLstmModel; not part of the
// reference repository).  Once the HBV recurrence costs well under a millisecond the per-step
// launches of a library LSTM dominate a training step, so the recurrence is one persistent kernel
// per direction:
//
//   gates_t = gx_t + h_{t-1} W_hh^T          (gx = x W_ih^T + b_ih + b_hh: one library GEMM, host side)
//   i, f, o = sigmoid, g = tanh;  c_t = f c_{t-1} + i g;  h_t = o tanh(c_t)      (torch.nn.LSTM)
//   (h_{-1}, c_{-1}) = (h0, c0), zeros when not given; backward: dc_{T-1} starts from grad_c_last, and
//   grad_c0 = dc_0 f_0 after the last (t = 0) step
//
// and a third one of the forward's shape, k_lstm_tan (at the end of this file), is its forward-mode derivative;
// k_lstm_dirs behind it runs that derivative along many directions at once, on (direction, row tile) pairs.
//
// Basins are independent, so the batch is cut into row tiles of 16 basins (the N of
// v_mfma_f32_16x16x4_f32: exact f32 products, a k-ordered fmaf chain) and only the H/16 workgroups
// that share a row tile ever talk to each other.  Forward: workgroup = 16 hidden units = four groups of
// 4 units x 4 gates (the 16 MFMA rows); wave w multiplies K quarter w of h_{t-1} (H/64 16-byte loads
// per lane) into all four groups (its W_hh entries live in H/4 VGPRs for the whole sequence), the
// partial tiles are summed through LDS in wave order and wave w finishes unit group w.  Backward: workgroup = 16 hidden units, its 4 waves
// split the 4H gate rows of dh_{t-1} = dgates_t W_hh (again H/4 VGPRs of W_hh each), partial tiles
// are summed through LDS in wave order, then one thread per (unit, basin) does the cell adjoint.
// Gate vectors use the (unit, gate) layout [T,B,H,4] so that a lane's four gates are one 16-byte access.
//
// Hand-off between the waves of a row tile, once per time step: the exchange buffer holds one slab per
// time step and row tile, never reused inside a launch and filled with the sentinel word 0xFFFFFFFF by
// k_lstm_arm (lstm.hip) before the launch.  A producer writes its slice with sc1 stores (write
// through, 4-byte granules are atomic) and goes on; a consumer re-issues its sc1 loads of the slab (L1
// bypassed: MI355X_MICROARCH.md "inter-workgroup visibility") until none of the words it needs is the
// sentinel -- the payload is its own flag, there are no counters, fences or barriers on the path, and a
// word that is not the sentinel can only be the value written in this launch.  h and the gate gradients
// are never the sentinel pattern (arithmetic NaNs are canonical 0x7FC00000).  One to three workgroups
// per CU (compiled for three waves per SIMD; the host sizes the LDS request so that exactly that many
// fit) and a launch never holds more workgroups than that, so all partners are resident.  Every spin
// is bounded: on a time-out the wave gives up, sets the error word (hbvx_lstm_check) and poisons its
// outputs.
//
// Measured and not kept (round 5, profiles/r05_lstm_xcd.jsonl; T = 730, B = 100, H = 256): a row tile's workgroups on
// ONE XCD (blocks b, b + 8, ... under the observed round-robin dispatch) with hand-off stores that stay in that XCD's L2
// (plain instead of sc1): forward 1.81 -> 1.67 ms, backward 2.28 -> 2.23; the mapping alone 1.71 / 2.66.  4 % of the
// pair for a protocol whose correctness would hang on placement (a run-time XCC_ID handshake could guard it): the
// hand-off's price sits in the consumer CU's memory queue, not in which cache serves it.
#pragma once
#include <hip/hip_runtime.h>

#define LSTM_ROWS 16                 // basins per row tile
#define LSTM_UNITS 16                // hidden units per workgroup
#define LSTM_SPIN_LIMIT (1u << 21)   // polls before a tile gives up (seconds, not minutes)
#define LSTM_SC1 16                  // buffer-instruction cache-policy bit: sc1

typedef float lstm_f4 __attribute__((ext_vector_type(4)));

struct LstmArgs {
    int T, B, tile0, ntile;          // this launch covers row tiles tile0 ..; ntile = tiles of the whole batch
    const float *w_hh;               // [4H,H], torch row order (i, f, g, o blocks)
    const float *gx;                 // forward: [T,B,H,4] input projection; backward: activated gates
    float *gates;                    // forward: activated gates (may alias gx); backward: grad of the pre-activations
    const float *c_in;               // backward: c_all
    const float *dh;                 // backward: grad_h [T,B,H]
    float *c_all, *h_all;            // forward outputs [T,B,H]
    const float *h0, *c0;            // initial state [B,H] (forward: h0 and c0; backward: c0); NULL = zeros
    const float *dc_last;            // backward: gradient w.r.t. c_{T-1} [B,H]; NULL = zeros
    float *dc0;                      // backward: gradient w.r.t. c0 [B,H]; NULL = not wanted
    float *xch;                      // exchange slabs, one per time step and row tile, sentinel-filled by k_lstm_arm
    unsigned *cnt;                   // cnt[0] = error word (zeroed by k_lstm_arm)
    unsigned spin_limit;             // polls before a hand-off gives up (LSTM_SPIN_LIMIT; lowered by the fault-injection test)
    int drop_wg;                     // fault injection (tests): this workgroup never publishes its slab; -1: none
};

// Gate non-linearities on the hardware transcendentals (v_exp_f32 / v_rcp_f32, about 1 ulp each): absolute
// error <= 2e-7 on values in [-1, 1], far inside the test tolerance, and 4-5 instructions instead of the
// ~30 of an IEEE division and the ~40 of ocml's tanhf -- the cell sits on the per-step latency chain.
// Saturation is exact: exp2 -> inf gives rcp -> 0.
__device__ __forceinline__ float lstm_sigmoid(float x)
{
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896341f));
}
__device__ __forceinline__ float lstm_tanh(float x)
{
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * 2.88539008177792681f));
}

#define LSTM_SENTINEL 0xFFFFFFFFu
#define LSTM_AUX (LSTM_SC1 | 0x80000000)   // sc1 + volatile: the polling loads are never hoisted or merged

// Loads the wave's KB 16-byte granules per lane (granule g0 + 4 j + kq of row n) until none of them
// holds a sentinel word.  false: timed out (error word set).
template <int KB, class A>
__device__ __forceinline__ bool lstm_fetch(const A &a, const float *slab_ptr, int slab_bytes, int g0,
                                           int kq, int n, lstm_f4 (&v)[KB])
{
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(slab_ptr), 0, slab_bytes, 0x00020000);
    for (unsigned spins = 0;; ++spins) {
#pragma unroll
        for (int j = 0; j < KB; ++j)
            v[j] = __builtin_bit_cast(lstm_f4, __builtin_amdgcn_raw_buffer_load_b128(r, ((g0 + 4 * j + kq) * LSTM_ROWS + n) * 16, 0, LSTM_AUX));
        unsigned mx = 0;
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            const auto u = __builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v[j]);
            mx = max(max(mx, u[0]), u[1]);
            mx = max(max(mx, u[2]), u[3]);
        }
        if (__ballot(mx == LSTM_SENTINEL) == 0) return true;
        if (spins > a.spin_limit) {
            if ((threadIdx.x & 63) == 0) __hip_atomic_store(&a.cnt[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
        __builtin_amdgcn_s_sleep(2);
        asm volatile("" ::: "memory");
    }
}

// UG: unit groups (4 units x 4 gates = the 16 MFMA rows) per workgroup: 4 (16 units, H/16 workgroups per
// row tile) or, when the batch is small enough for twice the workgroups to fit one launch, 2 (8 units: half
// the MFMAs per wave on the latency chain; waves 2 and 3 only multiply).
template <int H, int UG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_lstm_fwd(LstmArgs a)
{
    constexpr int NWG = H / (4 * UG), KQ = H / 64;     // KQ: 16-byte loads per lane = the wave's quarter of h
    __shared__ lstm_f4 part[2][4][UG][64];             // [buffer][K quarter][unit group][lane]
    const int tile = a.tile0 + blockIdx.x / NWG, s = blockIdx.x % NWG;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, kq = l >> 4, n = l & 15;
    const bool fin = w < UG;                        // this wave finishes unit group w
    const int u0 = (s * UG + (fin ? w : 0)) * 4;    // its four units
    const int unit = u0 + kq;
    const int row = tile * LSTM_ROWS + n, rowc = row < a.B ? row : a.B - 1;
    const bool live = row < a.B && fin;

    // Wave w multiplies K quarter w of h_{t-1} into all UG groups, so no byte of the slab is loaded
    // twice per workgroup.  A operand of group g: MFMA row m = 4*unit_local + gate; k of block (j, i) =
    // 4 (w H/16 + 4 j + kq) + i, like the loads.
    float wreg[UG][KQ * 4];
    {
        const int m = l & 15;
#pragma unroll
        for (int g = 0; g < UG; ++g) {
            const float *wr = a.w_hh + (size_t)((m & 3) * H + (s * UG + g) * 4 + (m >> 2)) * H + 4 * (w * (H / 16) + kq);
#pragma unroll
            for (int j = 0; j < KQ; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) wreg[g][j * 4 + i] = wr[16 * j + i];
        }
    }
    const size_t slab = (size_t)H * LSTM_ROWS;      // floats per (step, tile): [H/4][16 rows][4 units]
    // A hand-off time-out must never be silent: the wave that timed out raises this flag BEFORE the
    // step's barrier, every wave reads it AFTER the barrier, the finishing waves poison the last output
    // step and the whole workgroup leaves (a wave that simply returned would let the others sum stale
    // partial tiles into finite, wrong values).  Its row-tile partners time out on its missing slab.
    __shared__ int timed_out;
    if (threadIdx.x == 0) timed_out = 0;
    __syncthreads();
    const bool publish = (int)blockIdx.x != a.drop_wg;
    float c = a.c0 ? a.c0[(size_t)rowc * H + unit] : 0.0f;
    for (int t = 0; t < a.T; ++t) {
        const size_t e = ((size_t)t * a.B + rowc) * H + unit;
        lstm_f4 acc = {0, 0, 0, 0};
        if (fin) acc = *reinterpret_cast<const lstm_f4 *>(a.gx + e * 4);
        if (t > 0 || a.h0) {
            // step 0 of a stateful call takes h0 through the same MFMA chain and LDS sum as every later step
            // (its granules in the slab's [H/4][16 rows][4 units] order), so a run resumed from (h_{t-1}, c_{t-1})
            // gives the bits of the uninterrupted one
            lstm_f4 hv[KQ];
            if (t == 0) {
#pragma unroll
                for (int j = 0; j < KQ; ++j)
                    hv[j] = *reinterpret_cast<const lstm_f4 *>(a.h0 + (size_t)rowc * H + 4 * (w * (H / 16) + 4 * j + kq));
            } else if (!lstm_fetch<KQ>(a, a.xch + ((size_t)(t - 1) * a.ntile + tile) * slab, (int)(slab * 4), w * (H / 16), kq, n, hv))
                timed_out = 1;                      // every lane of the wave stores the same word
            lstm_f4 p[UG];
#pragma unroll
            for (int g = 0; g < UG; ++g) p[g] = lstm_f4{0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < KQ; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int g = 0; g < UG; ++g)
                        p[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[g][j * 4 + i], hv[j][i], p[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < UG; ++g) part[t & 1][w][g][l] = p[g];
            __syncthreads();                        // the only barrier of a step; part[] is two deep
            if (timed_out) {
                if (live) a.h_all[((size_t)(a.T - 1) * a.B + row) * H + unit] = __builtin_nanf("");
                return;
            }
            if (fin)
                acc += (part[t & 1][0][w][l] + part[t & 1][1][w][l]) + (part[t & 1][2][w][l] + part[t & 1][3][w][l]);
        }
        if (!fin) continue;
        const float ig = lstm_sigmoid(acc[0]), fg = lstm_sigmoid(acc[1]), gg = lstm_tanh(acc[2]), og = lstm_sigmoid(acc[3]);
        c = fg * c + ig * gg;
        const float h = og * lstm_tanh(c);
        if (live) {
            const lstm_f4 act = {ig, fg, gg, og};
            *reinterpret_cast<lstm_f4 *>(a.gates + e * 4) = act;
            a.c_all[e] = c;
            a.h_all[e] = h;
        }
        if (t + 1 < a.T && publish) {
            // the wave's 64 lanes cover 256 contiguous bytes: two whole lines, one store instruction
            float *xp = a.xch + ((size_t)t * a.ntile + tile) * slab + ((size_t)(u0 >> 2) * LSTM_ROWS + n) * 4 + kq;
            __hip_atomic_store(xp, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int H>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_lstm_bwd(LstmArgs a)
{
    constexpr int NWG = H / LSTM_UNITS, KB = H / 16;
    __shared__ float part[2][4][4][64];
    const int tile = a.tile0 + blockIdx.x / NWG, s = blockIdx.x % NWG;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, kq = l >> 4, n = l & 15;
    const int unit = s * LSTM_UNITS + 4 * kq + w;   // this thread's unit in the cell adjoint
    const int row = tile * LSTM_ROWS + n, rowc = row < a.B ? row : a.B - 1;
    const bool live = row < a.B;

    // A operand: MFMA row m = hidden unit 16 s + m; the wave's quarter of the gate rows:
    // k of block (j, i) = gate i of unit w H/4 + 4 j + kq
    float wreg[KB * 4];
    {
        const int m = l & 15;
#pragma unroll
        for (int j = 0; j < KB; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                wreg[j * 4 + i] = a.w_hh[(size_t)(i * H + w * (H / 4) + 4 * j + kq) * H + s * LSTM_UNITS + m];
    }
    const size_t slab = (size_t)H * LSTM_ROWS * 4;  // floats per (step, tile): [H units][16 rows][4 gates]
    __shared__ int timed_out;                       // as in k_lstm_fwd: raised before the barrier, acted on after it
    if (threadIdx.x == 0) timed_out = 0;
    __syncthreads();
    const bool publish = (int)blockIdx.x != a.drop_wg;
    float dc_carry = a.dc_last ? a.dc_last[(size_t)rowc * H + unit] : 0.0f;
    for (int t = a.T - 1; t >= 0; --t) {
        const size_t e = ((size_t)t * a.B + rowc) * H + unit;
        const lstm_f4 act = *reinterpret_cast<const lstm_f4 *>(a.gx + e * 4);
        const float ct = a.c_in[e];
        const float cp = t > 0 ? a.c_in[e - (size_t)a.B * H] : (a.c0 ? a.c0[e] : 0.0f);   // e = rowc H + unit at t = 0
        float dh = a.dh[e];
        if (t + 1 < a.T) {
            lstm_f4 gv[KB];
            if (!lstm_fetch<KB>(a, a.xch + ((size_t)(t + 1) * a.ntile + tile) * slab, (int)(slab * 4), w * (H / 4), kq, n, gv))
                timed_out = 1;
            lstm_f4 p0 = {0, 0, 0, 0}, p1 = {0, 0, 0, 0}, p2 = {0, 0, 0, 0}, p3 = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < KB; ++j) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float av = wreg[j * 4 + i], bv = gv[j][i];
                    if (i == 0) p0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, p0, 0, 0, 0);
                    else if (i == 1) p1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, p1, 0, 0, 0);
                    else if (i == 2) p2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, p2, 0, 0, 0);
                    else p3 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, p3, 0, 0, 0);
                }
            }
            p0 = (p0 + p1) + (p2 + p3);
            // result row m = 4 kq + i of the 16 units: thread (w, l) finishes i = w
#pragma unroll
            for (int i = 0; i < 4; ++i) part[t & 1][w][i][l] = p0[i];
            __syncthreads();                        // the only barrier of a step; part[] is two deep
            if (timed_out) {
                // poison this step's gate gradients (nothing overwrites them: the workgroup leaves); every
                // weight gradient sums over them, so the failure reaches the loss scaler / optimiser as NaN
                if (live) {
                    const lstm_f4 bad = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
                    *reinterpret_cast<lstm_f4 *>(a.gates + e * 4) = bad;
                    if (a.dc0) a.dc0[e - (size_t)t * a.B * H] = __builtin_nanf("");   // [rowc][unit]
                }
                return;
            }
            dh += (part[t & 1][0][w][l] + part[t & 1][1][w][l]) + (part[t & 1][2][w][l] + part[t & 1][3][w][l]);
        }
        const float ig = act[0], fg = act[1], gg = act[2], og = act[3];
        const float tc = lstm_tanh(ct);
        const float dc = dc_carry + dh * og * (1.0f - tc * tc);
        lstm_f4 d;
        d[0] = dc * gg * ig * (1.0f - ig);
        d[1] = dc * cp * fg * (1.0f - fg);
        d[2] = dc * ig * (1.0f - gg * gg);
        d[3] = dh * tc * og * (1.0f - og);
        dc_carry = dc * fg;
        if (live) *reinterpret_cast<lstm_f4 *>(a.gates + e * 4) = d;
        if (t == 0 && live && a.dc0) a.dc0[e] = dc_carry;   // dc_0 f_0: the gradient w.r.t. c0
        if (t > 0 && publish) {
            // 16 lanes of one store instruction cover a unit's 256-byte block: whole lines
            // (d comes out of VALU instructions: an inline-asm store placed straight after MFMAs would read the
            // accumulators before their write-back -- the compiler pads only the stores it can see)
            float *xp = a.xch + ((size_t)t * a.ntile + tile) * slab + ((size_t)unit * LSTM_ROWS + n) * 4;
            const lstm_f4 dx = live ? d : lstm_f4{0, 0, 0, 0};
            asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(xp), "v"(dx) : "memory");
        }
    }
}

// Forward-mode tangent of k_lstm_fwd along one direction (hbvx_lstm_tangent), on the primal the forward saved:
//
//   z'_t = gx'_t + h'_{t-1} W_hh^T      (gx' = every time-parallel term of the tangent: host-side GEMMs)
//   di = i(1-i) z'_i,  df = f(1-f) z'_f,  dg = (1-g^2) z'_g,  do = o(1-o) z'_o   (i, f, g, o: the saved gates)
//   c'_t = df c_{t-1} + f c'_{t-1} + di g + i dg;   tau = tanh(c_t);   h'_t = do tau + o (1-tau^2) c'_t
//   (h'_{-1}, c'_{-1}) = (h0', c0'), zeros when not given; c_{-1} = c0, zeros when not given
//
// Only h'_{t-1} W_hh^T sits on the sequential chain and it has the forward's shape, so this is k_lstm_fwd with
// another cell: the same row tiles, W_hh quarters in VGPRs, MFMA chain and LDS sum in wave order, the same
// sentinel-armed slabs (h'_t instead of h_t), bounded spins and time-out poisoning, the same residency.  The
// per-step inputs of the cell (gx'_t, gates_t, c_t: 36 B per lane) do not depend on the chain: they are issued a
// step ahead, right behind the previous step's hand-off, and nothing waits for them before the hand-off of their
// own step, whose poll waits for them anyway (vector loads return in order) -- a step after they were issued.
// (tests/test_lstm_jvp.py checks the ISA for a vmcnt wait between these loads and the barrier of their step.)
struct LstmTanArgs {
    int T, B, tile0, ntile;          // as in LstmArgs
    const float *w_hh;               // [4H,H], torch row order
    const float *gx_t;               // [T,B,H,4] tangent of the time-parallel term, (unit, gate) layout
    const float *gates;              // [T,B,H,4] activated gates of the forward
    const float *c_all;              // [T,B,H] c of the forward
    const float *c0;                 // [B,H] primal initial cell state; NULL = zeros
    const float *h0_t, *c0_t;        // [B,H] tangents of the initial state; NULL = zeros
    float *h_t;                      // output [T,B,H]: h'
    float *c_t_last;                 // output [B,H]: c'_{T-1}; NULL = not wanted
    float *xch;                      // exchange slabs, as in LstmArgs (the forward's [H/4][16 rows][4 units] slab)
    unsigned *cnt;                   // cnt[0] = error word
    unsigned spin_limit;
    int drop_wg;                     // fault injection (tests): this workgroup never publishes its slab; -1: none
};

template <int H, int UG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_lstm_tan(LstmTanArgs a)
{
    constexpr int NWG = H / (4 * UG), KQ = H / 64;
    __shared__ lstm_f4 part[2][4][UG][64];             // [buffer][K quarter][unit group][lane]
    const int tile = a.tile0 + blockIdx.x / NWG, s = blockIdx.x % NWG;
#include "lstm_tan_body.h"                             // shared with k_lstm_dirs, textually
}

// Many directions on one primal (hbvx_lstm_tangent_batch): D directions are D independent recurrences on the same
// gates, c_all, c0 and W_hh, so the unit of work is the pair (direction, row tile) instead of the row tile -- more
// tiles to share a SIMD, whose MFMAs hide each other's hand-offs.  tile0 counts pairs here, direction-major; the
// primal is indexed by the pair's basin rows alone, the tangent buffers [D, ...] and the exchange slabs
// [D][T][tiles] by its direction too.
template <int H, int UG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_lstm_dirs(LstmTanArgs a)
{
    constexpr int NWG = H / (4 * UG), KQ = H / 64;
    __shared__ lstm_f4 part[2][4][UG][64];             // [buffer][K quarter][unit group][lane]
    const int pair = a.tile0 + blockIdx.x / NWG, dir = pair / a.ntile;
    const int tile = pair - dir * a.ntile, s = blockIdx.x % NWG;
    {
        const size_t bh = (size_t)dir * a.B * H, tbh = bh * a.T;
        a.gx_t += tbh * 4;
        a.h_t += tbh;
        if (a.h0_t) a.h0_t += bh;
        if (a.c0_t) a.c0_t += bh;
        if (a.c_t_last) a.c_t_last += bh;
        a.xch += (size_t)dir * a.T * a.ntile * H * LSTM_ROWS;
    }
#include "lstm_tan_body.h"
}
