// hbv_gage_pop.h -- stage 2 of the hourly model's population evaluation (include/hbvx_gage_pop.h): every candidate's
// unit runoff routed to the gages and scored there.  Stage 1 is k_pop's runoff form (hbv_pop.h); launch_gage_pop.hip has
// the entry points.
//
// Why two stages: k_pop keeps a basin's window and chains in the registers of the wave that simulates it, because a
// daily basin IS the scored series.  Here a wave simulates units, and the scored series is a gage's: the area-weighted
// sum of up to thousands of units, each through a 72-tap pair hydrograph.  That sum crosses waves and workgroups, so the
// runoff goes through memory once ([P,T,U]) and three kernels take it from there:
//   k_gp_transpose  the runoff unit-major, [P,U,T], so that a pair's column is contiguous (k_transpose with a
//                   candidate axis);
//   k_gp_uh         candidate c's taps of every pair from its route_a / route_b / route_tau (k_gage_uh's statements with
//                   a candidate axis), only when the candidates move the routing parameters;
//   k_gp_route      one workgroup per (1024-hour tile, gage, candidate): loops over the gage's pairs in CSR order, stages
//                   the pair's column (tile + halo) and taps in LDS, forms its four outputs per thread with
//                   k_gage_lag_fwd's statements, adds them to the gage accumulators in pair order and divides by the
//                   gage's area once -- k_gage_lag_fwd followed by k_gage_sum_fwd, operation for operation, without the
//                   [P,NPAIR,T] series between them (4.4 GB at 64 candidates on 12 000 pairs x 2 160 hours).  The serial
//                   pair loop that lost to the pair-parallel form in the forward (hbv_gage.h) is the right shape here:
//                   the candidates supply the parallelism one gage lacks;
//   k_gp_score      lanes are gages, blockIdx.y the candidate: one ascending pass over the hours of [P,T,G], a PeriodMean
//                   and the period cursor of k_pop's period form, BasinStats::score<TR> at each close.
// A fifth kernel works on the series these leave behind:
//   k_gp_events     hbvx_gage_population_events (include/hbvx_gage_events.h): per (candidate, event, gage) the peak, its
//                   hour and the volume inside a window of hours fixed on the observed side.  It sits on the [P,T,G]
//                   series and not inside k_gp_route, whose workgroups own 1024-hour tiles: an event crosses tiles.
// Three more work on it for the flow-duration curve (include/hbvx_gage_fdc.h):
//   k_gp_fdc        hbvx_gage_population_fdc: per (candidate, level, gage) the scored hours above a threshold fixed on the
//                   observed side and the volume above it -- hbvx_pop_fdc.h's slot on the gage series, one ordered pass;
//   k_gp_keys, k_gp_quant   hbvx_gage_population_quantiles: the candidate's own curve.  The series gage-major as sortable
//                   keys, then one LDS sort per (candidate, gage) column and the flows at K ranks.  The sort sits on the
//                   series because k_pop and k_gp_route keep none: a quantile needs all hours of a column at once.
// The statements of hbv_gage.h are restated, not shared: that header defines its kernels (one translation unit may
// include it), and its kernels' code is pinned.  A change to either belongs in both; tests/test_hourly_population_gpu.py
// holds the gage series to hbvx_gage_route_forward's bits.
#pragma once

#include "hbv_pop.h"

#if defined(__HIPCC__)

#include "hbv_step.h"
#include "../../include/hbvx_gage_pop.h"
#include "../../include/hbvx_gage_events.h"
#include "../../include/hbvx_gage_fdc.h"

namespace hbvx {
namespace gagepop {

constexpr int TILE = 256;               // threads of k_gp_route; four outputs each
constexpr int TILE4 = 4 * TILE;
constexpr int MAXL = HBVX_GAGE_MAXLEN;
constexpr int COLN = TILE4 + MAXL + 8;
constexpr int HOURS = 16;               // hours k_gp_score loads ahead of its chains

struct Args {
    hbvx_gage_desc r;
    hbvx_gage_pop gp;
    float *qsT;             // [P or 1,U,T]
    int64_t qsT_c_stride;   // U * T, or 0 with one runoff for all
    float *uh;              // [P,NPAIR,L] with gp.dp, else gp.uh
    int64_t uh_c_stride;    // NPAIR * L, or 0
    float *series;          // [P,T,G]
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// out[c][col][row] = in[c][row][col]; in [R,C] row-major per candidate.  k_transpose (hbv_gage.h) with blockIdx.z.
__global__ void __launch_bounds__(256) k_gp_transpose(int R, int C, const float *__restrict__ in, int64_t in_c_stride,
                                                      float *__restrict__ out)
{
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float *src = in + (int64_t)blockIdx.z * in_c_stride;
    float *dst = out + (int64_t)blockIdx.z * R * C;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int r = r0 + ty + 8 * k, c = c0 + tx;
        tile[ty + 8 * k][tx] = (r < R && c < C) ? src[(int64_t)r * C + c] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = c0 + ty + 8 * k, r = r0 + tx;
        if (c < C && r < R) dst[(int64_t)c * R + r] = tile[tx][ty + 8 * k];
    }
}

// k_gage_uh's statements on candidate blockIdx.y's parameters of pair blockIdx.x.
__global__ void __launch_bounds__(128) k_gp_uh(const Args A)
{
    __shared__ float w[MAXL];
    __shared__ float ssum;
    const hbvx_gage_desc &r = A.r;
    const int p = blockIdx.x, k = threadIdx.x;
    const int64_t c = blockIdx.y;
    const int L = r.L;
    const float *dp = A.gp.dp + (c * r.NPAIR + p) * 3;
    const float a = descale_(dp[0], r.a_lo, r.a_hi);
    const float b = descale_(dp[1], r.b_lo, r.b_hi);
    const float tau = descale_(dp[2], r.tau_lo, r.tau_hi);
    const float aa = fmaxf(a, 0.0f) + 0.1f;
    const float theta = fmaxf(b, 0.0f) + 0.5f;
    const float kkf = r.lag_uh ? floorf(tau) : 0.0f;
    const float f = r.lag_uh ? tau - kkf : 0.0f;
    const float denom = expf(lgammaf(aa)) * powf(theta, aa);
    if (k < L) {
        const float t = (float)k + 0.5f;
        w[k] = 1.0f / denom * powf(t, aa - 1.0f) * expf(-t / theta);
    }
    __syncthreads();
    if (k == 0) {
        float sum = 0.0f;
        for (int j = 0; j < L; j++) sum += w[j];
        ssum = sum;
    }
    __syncthreads();
    if (k >= L) return;
    const float sum = ssum;
    float *dst = A.uh + (c * r.NPAIR + p) * L;
    if (!r.lag_uh) {
        dst[k] = w[k] / sum;
        return;
    }
    const int kk = (int)kkf;
    const int i0 = k - kk, i1 = k - kk - 1;
    const float w0 = (i0 >= 0 && i0 <= L - 1) ? w[i0] / sum : 0.0f;
    const float w1 = (i1 >= 0 && i1 <= L - 1) ? w[i1] / sum : 0.0f;
    dst[k] = (1.0f - f) * w0 + f * w1;
}

// hbvx_gage_population_events (include/hbvx_gage_events.h): the peak, its hour and the volume of event blockIdx.z's window
// at gage (blockIdx.x * 64 + lane) in candidate blockIdx.y's series.  Lanes are gages, so a wave's loads are coalesced
// ([t*G + g]); the wave walks the hours from the smallest start to the largest end among its lanes, both wave-uniform,
// EV_HOURS at a time into registers so that the serial pass waits on memory once per batch, and each lane pushes the
// hours of its OWN window into its EventSlot, in ascending order.  A lane reads hours of its wave's span alone, all
// within 0 .. T-1 whatever start / end hold; an inactive lane of a partial wave reads gage G-1 and stores nothing.
// (It stands before k_gp_route so that the code of that kernel, the last of this file's plain functions in the object, is
// byte for byte what it was, the padding behind it included: tools/compare_code.py.)
constexpr int EV_HOURS = 8;

struct EventArgs {
    hbvx_gage_events ev;
    int c0, e0;             // the first candidate and the first event of this launch (launch_gage_pop.hip splits the call
                            // so that no launch exceeds a grid dimension or 2^32 threads)
};

__global__ void __launch_bounds__(64) k_gp_events(const EventArgs A)
{
    const hbvx_gage_events &ev = A.ev;
    const int lane = threadIdx.x, G = ev.G, T = ev.T, E = ev.n_events;
    const int gl = blockIdx.x * 64 + lane;
    const bool active = gl < G;
    const int g = active ? gl : G - 1;
    const int64_t c = A.c0 + blockIdx.y;
    const int e = A.e0 + blockIdx.z;
    const int s = ev.start[(int64_t)e * G + g];
    int f = ev.end[(int64_t)e * G + g];
    f = f < T - 1 ? f : T - 1;
    const bool present = active && s >= 0 && f >= s;
    // the wave's span: present lanes have 0 <= s <= f <= T - 1
    int lo = present ? s : T, hi = present ? f : -1;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int ol = __shfl_xor(lo, m), oh = __shfl_xor(hi, m);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);
    const float *ser = ev.series + c * (int64_t)T * G + g;
    hbvx_popk::EventSlot slot;
    slot.start();
    for (int tb = lo; tb <= hi; tb += EV_HOURS) {
        float v[EV_HOURS];
#pragma unroll
        for (int i = 0; i < EV_HOURS; i++) {
            const int t = tb + i <= hi ? tb + i : hi;       // lo <= t <= hi <= T - 1
            v[i] = ser[(int64_t)t * G];
        }
#pragma unroll
        for (int i = 0; i < EV_HOURS; i++) {
            const int t = tb + i;
            if (present && t >= s && t <= f) slot.push(v[i], t);
        }
    }
    if (active) {
        const int64_t at = (c * E + e) * (int64_t)G + g;
        ev.peak[at] = slot.peak;
        ev.peak_hour[at] = slot.hour;
        ev.volume[at] = slot.vol;
    }
}

// hbvx_gage_population_fdc (include/hbvx_gage_fdc.h): the exceedance count and the volume above FDC_LEVELS thresholds,
// the block blockIdx.z of the call's K, at gage (blockIdx.x * 64 + lane) in candidate (c0 + blockIdx.y)'s series.  Lanes
// are gages, so the loads of the flows and of the mask ([t*G + g]) are coalesced; one ascending pass over the hours,
// FDC_HOURS at a time into registers, and each lane pushes the hours its mask lets in into its FdcSlots (hbv_pop.h).
// Threshold, count and volume of the block stay in registers: 3 x 8 of them, which leaves the kernel at eight waves per
// SIMD; all 32 levels would take 96 (tools/kernel_resources.py, profiles/r27_hourly_fdc.md).  A level from K on has a
// threshold of +inf and is not stored; an inactive lane of a partial wave reads gage G-1 and stores nothing.  (Like
// k_gp_events it stands before k_gp_route: tools/compare_code.py.)
constexpr int FDC_HOURS = 8;
constexpr int FDC_LEVELS = 8;

struct FdcArgs {
    hbvx_gage_fdc gf;
    int c0;                 // the first candidate of this launch (launch_gage_pop.hip splits the call so that no launch
                            // exceeds 2^32 threads)
};

__global__ void __launch_bounds__(64) k_gp_fdc(const FdcArgs A)
{
    const hbvx_gage_fdc &gf = A.gf;
    const int lane = threadIdx.x, G = gf.G, T = gf.T, K = gf.n_lev;
    const int gl = blockIdx.x * 64 + lane;
    const bool active = gl < G;
    const int g = active ? gl : G - 1;
    const int64_t c = A.c0 + blockIdx.y;
    const int k0 = blockIdx.z * FDC_LEVELS;
    const float *ser = gf.series + c * (int64_t)T * G + g;
    const uint8_t *msk = gf.scored + g;
    float thr[FDC_LEVELS];
    hbvx_popk::FdcSlot slot[FDC_LEVELS];
#pragma unroll
    for (int j = 0; j < FDC_LEVELS; j++) {
        thr[j] = k0 + j < K ? gf.thr[(int64_t)(k0 + j) * G + g] : INFINITY;
        slot[j].start();
    }
    for (int tb = 0; tb < T; tb += FDC_HOURS) {
        float v[FDC_HOURS];
        uint8_t m[FDC_HOURS];
#pragma unroll
        for (int i = 0; i < FDC_HOURS; i++) {
            const int t = tb + i < T ? tb + i : T - 1;      // 0 <= t <= T - 1
            v[i] = ser[(int64_t)t * G];
            m[i] = msk[(int64_t)t * G];
        }
#pragma unroll
        for (int i = 0; i < FDC_HOURS; i++) {
            if (tb + i < T && m[i]) {
#pragma unroll
                for (int j = 0; j < FDC_LEVELS; j++) slot[j].push(v[i], thr[j]);
            }
        }
    }
    if (active) {
#pragma unroll
        for (int j = 0; j < FDC_LEVELS; j++) {
            if (k0 + j < K) {
                const int64_t at = (c * K + (k0 + j)) * (int64_t)G + g;
                gf.count[at] = (int32_t)slot[j].n;
                gf.volume[at] = slot[j].vol;
            }
        }
    }
}

// hbvx_gage_population_quantiles (include/hbvx_gage_fdc.h), in two kernels.
//   k_gp_keys   keys[c][g][t] = the sortable image (hbvx_popk::quant_key) of series[c][t][g], QUANT_NONE where the hour is
//               not scored: k_gp_transpose's statements on a 32 x 32 tile (blockIdx.x: gages, blockIdx.y: hours,
//               blockIdx.z: candidates from c0), with the mask read beside the flows, so that both reads are rows of
//               [T,G] and the writes are rows of [G,T].  The sort then never sees the mask.
//   k_gp_quant  one workgroup per (gage g0 + blockIdx.x, candidate c0 + blockIdx.y): the column's T keys come from one
//               contiguous row into N = the next power of two >= T words of dynamic LDS (sized by the call's T, not by the
//               cap), QUANT_NONE behind them; a bitonic network sorts them descending, one barrier per step; then thread
//               k < K reads the key at rank[k][g].  QUANT_NONE is below every flow, so an index < n lands on a flow and
//               one >= n on QUANT_NONE: NaN.  QUANT_NAN is above every flow, so after the sort word 0 IS the workgroup's
//               flag "a scored hour is NaN" -- it costs no LDS beside the column, which at the cap is all 64 KB a
//               launch may ask for without an attribute.
constexpr int QUANT_THREADS = 256;

struct QuantArgs {
    hbvx_gage_fdc gf;
    uint32_t *keys;         // [P,G,T] of this CALL (c0 indexes into it)
    int c0, g0;             // the first candidate and the first gage of this launch
    int N;                  // the padded column: a power of two, T <= N < 2 T
};

__global__ void __launch_bounds__(256) k_gp_keys(const QuantArgs A)
{
    __shared__ uint32_t tile[32][33];
    const int T = A.gf.T, G = A.gf.G;
    const int g0 = blockIdx.x * 32, t0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t c = A.c0 + blockIdx.z;
    const float *src = A.gf.series + c * (int64_t)T * G;
    uint32_t *dst = A.keys + c * (int64_t)T * G;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int t = t0 + ty + 8 * k, g = g0 + tx;
        uint32_t key = hbvx_popk::QUANT_NONE;
        if (t < T && g < G && A.gf.scored[(int64_t)t * G + g]) key = hbvx_popk::quant_key(src[(int64_t)t * G + g]);
        tile[ty + 8 * k][tx] = key;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int g = g0 + ty + 8 * k, t = t0 + tx;
        if (g < G && t < T) dst[(int64_t)g * T + t] = tile[tx][ty + 8 * k];
    }
}

__global__ void __launch_bounds__(QUANT_THREADS) k_gp_quant(const QuantArgs A)
{
    extern __shared__ uint32_t quant_col[];         // [N]
    const hbvx_gage_fdc &gf = A.gf;
    const int T = gf.T, G = gf.G, K = gf.n_lev, N = A.N, tid = threadIdx.x;
    const int g = A.g0 + blockIdx.x;
    const int64_t c = A.c0 + blockIdx.y;
    const uint32_t *col = A.keys + (c * G + g) * (int64_t)T;
    for (int i = tid; i < N; i += QUANT_THREADS) quant_col[i] = i < T ? col[i] : hbvx_popk::QUANT_NONE;
    __syncthreads();
    // Comparator i of a step with distance j joins lo = (i with a zero bit inserted at j) and lo + j; inside a block of
    // 2 k words with bit k of lo clear the larger key goes first, with it set the smaller.  In the last stage k = N, so
    // the bit is clear everywhere: descending.  All indices are < N.
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int i = tid; i < (N >> 1); i += QUANT_THREADS) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                const int hi = lo + j;
                const uint32_t a = quant_col[lo], b = quant_col[hi];
                const bool desc = (lo & k) == 0;
                if (desc ? a < b : a > b) {
                    quant_col[lo] = b;
                    quant_col[hi] = a;
                }
            }
            __syncthreads();
        }
    if (tid < K) {
        const int r = gf.rank[(int64_t)tid * G + g];
        const bool any_nan = quant_col[0] == hbvx_popk::QUANT_NAN;
        const uint32_t key = (r >= 0 && r < N) ? quant_col[r] : hbvx_popk::QUANT_NONE;
        const bool none = any_nan || key == hbvx_popk::QUANT_NONE;
        gf.quantile[(c * K + tid) * (int64_t)G + g] = none ? __builtin_nanf("") : hbvx_popk::quant_value(key);
    }
}

// series[c][t][g] for the tile blockIdx.x, the gage blockIdx.y, the candidate blockIdx.z.
__global__ void __launch_bounds__(TILE) k_gp_route(const Args A)
{
    __shared__ __align__(16) float col[COLN];
    __shared__ __align__(16) float wsh[MAXL + 4];
    const hbvx_gage_desc &r = A.r;
    const int t0 = blockIdx.x * TILE4, g = blockIdx.y, tid = threadIdx.x;
    const int64_t c = blockIdx.z;
    const int T = r.T, L = r.L, nblk = (L + 3) >> 2;
    const float *qsT = A.qsT + c * A.qsT_c_stride;
    const float *uh = A.uh + c * A.uh_c_stride;
    const int p0 = clampi(r.gage_ptr[g], 0, r.NPAIR), p1 = clampi(r.gage_ptr[g + 1], 0, r.NPAIR);
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (int p = p0; p < p1; p++) {
        const int u = clampi(r.pair_unit[p], 0, r.U - 1);
        const float ar = r.areas[u];
        const float *w = uh + (int64_t)p * L;
        __syncthreads();        // the pair before has been read
        // col[x] = q at time t0 - 4 nblk + x (zero history, zero beyond the record)
        for (int x = tid; x < TILE4 + 4 * nblk; x += TILE) {
            const int ts = t0 - 4 * nblk + x;
            col[x] = (ts >= 0 && ts < T) ? qsT[(int64_t)u * T + ts] * ar : 0.0f;
        }
        for (int k = tid; k < MAXL + 4; k += TILE) wsh[k] = (k < L) ? w[k] : 0.0f;
        __syncthreads();
        const float4 *c4 = reinterpret_cast<const float4 *>(col) + tid + nblk;
        float4 cur = c4[0];
        float y0 = 0.0f, y1 = 0.0f, y2 = 0.0f, y3 = 0.0f;
        for (int b = 0; b < nblk; b++) {
            const float4 nxt = c4[-b - 1];
            const float4 q = reinterpret_cast<const float4 *>(wsh)[b];
            y0 += q.x * cur.x; y0 += q.y * nxt.w; y0 += q.z * nxt.z; y0 += q.w * nxt.y;
            y1 += q.x * cur.y; y1 += q.y * cur.x; y1 += q.z * nxt.w; y1 += q.w * nxt.z;
            y2 += q.x * cur.z; y2 += q.y * cur.y; y2 += q.z * cur.x; y2 += q.w * nxt.w;
            y3 += q.x * cur.w; y3 += q.y * cur.z; y3 += q.z * cur.y; y3 += q.w * cur.x;
            cur = nxt;
        }
        a0 += y0; a1 += y1; a2 += y2; a3 += y3;     // k_gage_sum_fwd's sum, in pair order
    }
    const float den = r.denom[g];
    const int t = t0 + tid * 4;
    float *dst = A.series + (c * T + t) * r.G + g;
    if (t < T) dst[0] = a0 / den;
    if (t + 1 < T) dst[(int64_t)r.G] = a1 / den;
    if (t + 2 < T) dst[(int64_t)2 * r.G] = a2 / den;
    if (t + 3 < T) dst[(int64_t)3 * r.G] = a3 / den;
}

// The four chains of gage (blockIdx.x * 64 + lane) and candidate blockIdx.y.  The hours come HOURS at a time into
// registers, and the targets, weights and closing hours of the next HOURS periods into LDS (a batch of HOURS hours closes
// at most HOURS periods), so that the serial pass waits on memory once per batch, not once per hour.
template <int TR>
__global__ void __launch_bounds__(64) k_gp_score(const Args A)
{
    __shared__ float sh_o[HOURS][64], sh_w[HOURS][64];
    __shared__ int sh_e[HOURS];
    const hbvx_gage_desc &r = A.r;
    const hbvx_gage_pop &gp = A.gp;
    const int lane = threadIdx.x, G = r.G, T = r.T, K = gp.n_periods;
    const int gl = blockIdx.x * 64 + lane;
    const bool active = gl < G;
    const int g = active ? gl : G - 1;
    const int64_t c = blockIdx.y;
    const float *ser = A.series + c * (int64_t)T * G + g;
    const float *tg = gp.target + g;
    const float *wt = gp.w ? gp.w + g : nullptr;
    float *sim = gp.sim ? gp.sim + c * (int64_t)K * G + g : nullptr;

    hbvx_popk::BasinStats bs;
    bs.start(false, gp.shift[g], TR == hbvx_popk::T_LOG ? gp.eps[g] : 0.0f);
    hbvx_popk::PeriodMean pm;
    pm.acc = 0.0f;
    int kf = 0, sf = 0, ef = -1;
    float pobs = 0.0f, pw = 1.0f;
    for (int tb = 0; tb < T && kf < K; tb += HOURS) {
        float v[HOURS];
#pragma unroll
        for (int i = 0; i < HOURS; i++) v[i] = tb + i < T ? ser[(int64_t)(tb + i) * G] : 0.0f;
        const int kf0 = kf;
        __syncthreads();        // the batch before has been read
#pragma unroll
        for (int i = 0; i < HOURS; i++) {
            const int k = kf0 + i < K ? kf0 + i : K - 1;
            sh_o[i][lane] = tg[(int64_t)k * G];
            sh_w[i][lane] = wt ? wt[(int64_t)k * G] : 1.0f;
        }
        if (lane < HOURS) sh_e[lane] = kf0 + lane < K ? gp.period_end[kf0 + lane] : -1;
        __syncthreads();
        ef = sh_e[0], pobs = sh_o[0][lane], pw = sh_w[0][lane];
#pragma unroll
        for (int i = 0; i < HOURS; i++) {
            const int t = tb + i;
            if (t < T && kf < K) {
                pm.add(v[i], t == sf);
                if (t == ef) {
                    const int n = ef - sf + 1;
                    const float mean = n == 1 ? pm.acc : pm.close(n);
                    bs.template score<TR>(mean, pobs, pw);
                    if (sim && active) sim[(int64_t)kf * G] = mean;     // the mean, not its transform
                    kf++;
                    sf = t + 1;
                    const int j = kf - kf0;
                    if (j < HOURS) ef = sh_e[j], pobs = sh_o[j][lane], pw = sh_w[j][lane];
                }
            }
        }
    }
    if (active) {
        const int64_t at = c * G + g;
        gp.sse[at] = bs.cost;
        gp.s1[at] = bs.s1;
        gp.s2[at] = bs.s2;
        gp.s3[at] = bs.s3;
    }
}

} // namespace gagepop
} // namespace hbvx

#endif // __HIPCC__
