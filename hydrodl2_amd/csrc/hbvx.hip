// hbvx.hip -- libhbvx.so: HIP implementation of include/hbvx.h for gfx950 (MI355X).
//
// Lane mapping (all kernels): one wavefront lane per (basin, ensemble member).
// A 64-lane wave holds 64/Mp basins x Mp members, Mp = next power of two >= M,
// so one basin's ensemble sits in Mp adjacent lanes and the ensemble mean
// (reference hbv.py:507-511) is an intra-wave butterfly, never memory traffic.
// The time axis is strictly serial per lane (explicit Euler recurrence).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared
#include "hbvx_host.h"
#include "../../include/hbvx_route_rows.h"
#include "../../include/hbvx_live_rows.h"
#include "../../include/hbvx_pop_ens.h"
#include "hbv_step.h"
#include "hbv_lane.h"
#include "hbv_gage.h"
#include "hbv_pop.h"      // hbvx_popk::gamma_denom / gamma_tap: the unit hydrograph's per-tap arithmetic

using namespace hbvx;
using namespace hbvx_host;

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";

int hbvx_host::fail(int code, const char *msg)
{
    snprintf(g_err, sizeof g_err, "%s", msg);
    return code;
}

int hbvx_host::hip_fail(hipError_t e, const char *what)
{
    snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    return HBVX_E_DEVICE;
}

// which kernel family took the last forward / adjoint call of the process (diagnostic: the tests assert that the
// family they mean to check is the one that ran).  The adjoint runs on autograd's thread, the asking test on the
// main one: process-wide under a mutex, handed out through a per-thread copy.
static std::mutex g_disp_mu;
static char g_disp[2][48] = {"", ""};
void hbvx_host::note_dispatch(int dir, const char *family)
{
    std::lock_guard<std::mutex> lock(g_disp_mu);
    snprintf(g_disp[dir & 1], sizeof g_disp[0], "%s", family);
}
extern "C" int hbvx_zero_in_launch(void) { return hbvx_host::zero_taken() ? 1 : 0; }

extern "C" const char *hbvx_last_dispatch(int direction)
{
    static thread_local char out[48];
    std::lock_guard<std::mutex> lock(g_disp_mu);
    snprintf(out, sizeof out, "%s", g_disp[direction & 1]);
    return out;
}

extern "C" int hbvx_version(void) { return HBVX_ABI_VERSION; }
extern "C" const char *hbvx_last_error(void) { return g_err; }
extern "C" const char *hbvx_backend(void) { return "hip:gfx950"; }
extern "C" uint64_t hbvx_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(hbvx_desc);
    case 1: return sizeof(hbvx_fwd_out);
    case 2: return sizeof(hbvx_bwd_io);
    case 3: return sizeof(hbvx_route_desc);
    case 6: return sizeof(hbvx_gage_desc);
    case 4: return sizeof(hbvx_param_src);
    case 5: return sizeof(hbvx_param_grad);
    case 7: return sizeof(hbvx_tan_io);
    case 8: return sizeof(hbvx_tan_batch);
    case 9: return sizeof(hbvx_gram_desc);
    case 10: return sizeof(hbvx_pop);
    case 11: return sizeof(hbvx_pop_stats);
    case 12: return sizeof(hbvx_pop_joint);
    case 13: return sizeof(hbvx_pop_period);
    case 14: return sizeof(hbvx_pop_ens);
    default: return 0;
    }
}

// ---------------------------------------------------------------------------
// forward recurrence (reference hbv.py:423-511 + parameter prep hbv.py:201-256)
// ---------------------------------------------------------------------------
struct FwdArgs {
    hbvx_desc d;
    hbvx_fwd_out o;
    int lgMp;
};

template <int MODEL, bool BETAET>
__global__ void __launch_bounds__(64) k_fwd(const FwdArgs A)
{
    constexpr int NP = NParam<MODEL, BETAET>::value;
    const hbvx_desc &d = A.d;
    const hbvx_fwd_out &o = A.o;
    const int lgMp = A.lgMp;
    const LaneId L = lane_id(d, lgMp);
    const int T = d.T;
    const int64_t N = (int64_t)d.B * d.M;
    const bool raw = d.raw_sigmoid != 0;
    const float nz = d.nearzero;
    const float ac = (MODEL == MODEL_HBV20 || MODEL == MODEL_HOURLY) ? d.ac[L.b] : 0.0f;
    const float elev = (MODEL == MODEL_HBV20 || MODEL == MODEL_HOURLY) ? d.elev[L.b] : 0.0f;

    float p[NPARAM_MAX];
    const float *dynp[NP];
    bool use_dyn[NP];
    unsigned dmask = 0;
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const hbvx_param_src &s = d.p[i];
        float v = s.sta[(int64_t)L.b * s.sta_b_stride + L.j];
        v = raw ? sigmoid_(v) : v;
        p[i] = descale_(v, s.lo, s.hi);
        dynp[i] = s.dyn ? s.dyn + (int64_t)L.b * s.dyn_b_stride + L.j : s.sta;
        use_dyn[i] = s.dyn && !(s.drop && s.drop[L.b]);
        if (s.dyn) dmask |= 1u << i;
    }
#pragma unroll
    for (int i = NP; i < NPARAM_MAX; i++) p[i] = 0.0f;

    float st[5];
#pragma unroll
    for (int k = 0; k < 5; k++) st[k] = d.state_in ? d.state_in[k * N + L.n] : 0.001f;

    const float *xb = d.x + (int64_t)L.b * d.x_b_stride;
    const float *mu = d.muwts ? d.muwts + (int64_t)L.b * d.mu_b_stride + L.j : nullptr;
    const float invM = 1.0f / (float)d.M;
    const int nf = o.n_flux;
    // HBVX_TRAJ_CKPT: only the storages entering every K-th day are kept, [ceil(T/K), 5, N]
    const int ckpt_k = (o.traj && HBVX_TRAJ_KIND(o.traj_layout) == HBVX_TRAJ_CKPT) ? HBVX_TRAJ_CKPT_DAYS(o.traj_layout) : 0;

    // one-step-ahead register prefetch of the per-step inputs
    float nxf[3], nxd[NP];
    {
        const float *xr = xb;
        nxf[0] = T > 0 ? xr[d.ch_prcp] : 0.f;
        nxf[1] = T > 0 ? xr[d.ch_tmean] : 0.f;
        nxf[2] = T > 0 ? xr[d.ch_pet] : 0.f;
#pragma unroll
        for (int i = 0; i < NP; i++) nxd[i] = ((dmask >> i) & 1) && T > 0 ? dynp[i][0] : 0.f;
    }

    for (int t = 0; t < T; t++) {
        Step<MODEL, BETAET> s;
        s.P = nxf[0]; s.Tf = nxf[1]; s.PET = nxf[2];
        float cur[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) cur[i] = nxd[i];
        {
            const int tn = t + 1 < T ? t + 1 : t;
            const float *xr = xb + (int64_t)tn * d.x_t_stride;
            nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
#pragma unroll
            for (int i = 0; i < NP; i++)
                if ((dmask >> i) & 1) nxd[i] = dynp[i][(int64_t)tn * d.p[i].dyn_t_stride];
        }
#pragma unroll
        for (int i = 0; i < NP; i++)
            if ((dmask >> i) & 1) {
                float v = raw ? sigmoid_dyn_(cur[i]) : cur[i];
                float pv = descale_(v, d.p[i].lo, d.p[i].hi);
                if (use_dyn[i]) p[i] = pv;
            }
        s.SP = st[0]; s.MW = st[1]; s.SM = st[2]; s.SUZ = st[3]; s.SLZ = st[4];
        s.template fwd<false, true>(p, nz, ac, elev, 0.f, 0.f);

        if (ckpt_k) {
            if (t % ckpt_k == 0 && L.active) {
#pragma unroll
                for (int k = 0; k < 5; k++) o.traj[((int64_t)(t / ckpt_k) * 5 + k) * N + L.n] = st[k];
            }
        } else if (o.traj && L.active) {
#pragma unroll
            for (int k = 0; k < 5; k++) o.traj[((int64_t)k * (T + 1) + t) * N + L.n] = st[k];
        }
        st[0] = s.SP3; st[1] = s.MW3; st[2] = s.SM4; st[3] = s.SUZ4; st[4] = s.SLZ2;

        if (o.flux) {
            const float act = L.active ? 1.0f : 0.0f;
            float wq = mu ? mu[(int64_t)t * d.mu_t_stride] : 1.0f;
            float f[HBVX_MAX_FLUX];
            f[HBVX_F_QSIM] = (mu ? s.Q * wq : s.Q) * act;
            f[HBVX_F_Q0] = s.Q0 * act;
            f[HBVX_F_Q1] = s.Q1 * act;
            f[HBVX_F_Q2] = s.Q2 * act;
            f[HBVX_F_AET] = s.ET * act;
            f[HBVX_F_SWE] = s.SP3 * act;
            f[HBVX_F_RECHARGE] = s.rech * act;
            f[HBVX_F_EXCS] = s.exc * act;
            f[HBVX_F_EVAPFACTOR] = s.ef * act;
            f[HBVX_F_TOSOIL] = s.tosoil * act;
            f[HBVX_F_PERC] = s.PERC * act;
            f[HBVX_F_CAPILLARY] = s.cap * act;
#pragma unroll
            for (int k = 0; k < HBVX_MAX_FLUX; k++) {
                if (k < nf) {
                    float v = ens_sum(f[k], lgMp);
                    if (!(k == HBVX_F_QSIM && mu)) v = v * invM;
                    if (L.leader) o.flux[((int64_t)k * T + t) * d.B + L.b] = v;
                }
            }
        }
    }
    if (L.active) {
#pragma unroll
        for (int k = 0; k < 5; k++) {
            o.state_out[k * N + L.n] = st[k];
            if (o.traj && !ckpt_k) o.traj[((int64_t)k * (T + 1) + T) * N + L.n] = st[k];
        }
    }
}

// ---------------------------------------------------------------------------
// adjoint recurrence (the autograd tape of the same lines)
// ---------------------------------------------------------------------------
struct BwdArgs {
    hbvx_desc d;
    hbvx_bwd_io io;
    int lgMp;
};

template <int MODEL, bool BETAET>
__global__ void __launch_bounds__(64) k_bwd(const BwdArgs A)
{
    constexpr int NP = NParam<MODEL, BETAET>::value;
    const hbvx_desc &d = A.d;
    const hbvx_bwd_io &io = A.io;
    const int lgMp = A.lgMp;
    const LaneId L = lane_id(d, lgMp);
    const int T = d.T;
    const int64_t N = (int64_t)d.B * d.M;
    const bool raw = d.raw_sigmoid != 0;
    const float nz = d.nearzero;
    const float ac = (MODEL == MODEL_HBV20 || MODEL == MODEL_HOURLY) ? d.ac[L.b] : 0.0f;
    const float elev = (MODEL == MODEL_HBV20 || MODEL == MODEL_HOURLY) ? d.elev[L.b] : 0.0f;
    const int nf = io.n_flux;

    float p[NPARAM_MAX], usta[NP], gsta[NP];
    const float *dynp[NP];
    float *gdyn[NP];
    bool use_dyn[NP];
    unsigned dmask = 0;
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const hbvx_param_src &s = d.p[i];
        float v = s.sta[(int64_t)L.b * s.sta_b_stride + L.j];
        usta[i] = raw ? sigmoid_(v) : v;
        p[i] = descale_(usta[i], s.lo, s.hi);
        dynp[i] = s.dyn ? s.dyn + (int64_t)L.b * s.dyn_b_stride + L.j : s.sta;
        gdyn[i] = io.g[i].dyn ? io.g[i].dyn + (int64_t)L.b * io.g[i].dyn_b_stride + L.j : nullptr;
        use_dyn[i] = s.dyn && !(s.drop && s.drop[L.b]);
        gsta[i] = 0.0f;
        if (s.dyn) dmask |= 1u << i;
    }
#pragma unroll
    for (int i = NP; i < NPARAM_MAX; i++) p[i] = 0.0f;

    const float *xb = d.x + (int64_t)L.b * d.x_b_stride;
    const float *mu = d.muwts ? d.muwts + (int64_t)L.b * d.mu_b_stride + L.j : nullptr;
    const float invM = 1.0f / (float)d.M;
    float a[5];
#pragma unroll
    for (int k = 0; k < 5; k++) a[k] = io.grad_state_out ? io.grad_state_out[k * N + L.n] : 0.0f;

    for (int t = T - 1; t >= 0; t--) {
        Step<MODEL, BETAET> s;
        const float *xr = xb + (int64_t)t * d.x_t_stride;
        s.P = xr[d.ch_prcp]; s.Tf = xr[d.ch_tmean]; s.PET = xr[d.ch_pet];
        s.SP = io.traj[((int64_t)0 * (T + 1) + t) * N + L.n];
        s.MW = io.traj[((int64_t)1 * (T + 1) + t) * N + L.n];
        s.SM = io.traj[((int64_t)2 * (T + 1) + t) * N + L.n];
        s.SUZ = io.traj[((int64_t)3 * (T + 1) + t) * N + L.n];
        s.SLZ = io.traj[((int64_t)4 * (T + 1) + t) * N + L.n];
        float ud[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) {
            ud[i] = usta[i];
            if ((dmask >> i) & 1) {
                float v = dynp[i][(int64_t)t * d.p[i].dyn_t_stride];
                v = raw ? sigmoid_dyn_(v) : v;
                if (use_dyn[i]) {
                    ud[i] = v;
                    p[i] = descale_(v, d.p[i].lo, d.p[i].hi);
                }
            }
        }
        s.template fwd<false>(p, nz, ac, elev, 0.0f, 0.0f);

        FluxGrad g;
        const int64_t fs = (int64_t)T * d.B;
        const int64_t go = (int64_t)t * d.B + L.b;
        auto GF = [&](int k) -> float {
            float v = io.grad_flux ? io.grad_flux[k * fs + go] : 0.0f;
            if (io.grad_flux4 && k < 4) v += io.grad_flux4[k * fs + go];
            return v;
        };
        const float gq = GF(HBVX_F_QSIM);
        const float wq = mu ? mu[(int64_t)t * d.mu_t_stride] : invM;
        g.gQ = gq * wq;
        g.gQ0 = GF(HBVX_F_Q0) * invM;
        g.gQ1 = GF(HBVX_F_Q1) * invM;
        g.gQ2 = GF(HBVX_F_Q2) * invM;
        g.gET = GF(HBVX_F_AET) * invM;
        g.gSWE = GF(HBVX_F_SWE) * invM;
        g.grech = GF(HBVX_F_RECHARGE) * invM;
        g.gexc = GF(HBVX_F_EXCS) * invM;
        g.gef = GF(HBVX_F_EVAPFACTOR) * invM;
        g.gtosoil = GF(HBVX_F_TOSOIL) * invM;
        g.gPERC = GF(HBVX_F_PERC) * invM;
        g.gcap = (nf > HBVX_F_CAPILLARY) ? GF(HBVX_F_CAPILLARY) * invM : 0.0f;
        if (io.grad_muwts && L.active) io.grad_muwts[((int64_t)t * d.B + L.b) * d.M + L.j] = gq * s.Q;

        float gp[NPARAM_MAX], gx[3];
#pragma unroll
        for (int i = 0; i < NPARAM_MAX; i++) gp[i] = 0.0f;
        s.bwd(p, nz, g, a, gp, gx);

#pragma unroll
        for (int i = 0; i < NP; i++) {
            float gu = gp[i] * (d.p[i].hi - d.p[i].lo);
            if ((dmask >> i) & 1) {
                float gr = raw ? gu * (ud[i] * (1.0f - ud[i])) : gu;
                if (gdyn[i] && L.active)
                    gdyn[i][(int64_t)t * io.g[i].dyn_t_stride] = use_dyn[i] ? gr : 0.0f;
                gsta[i] += use_dyn[i] ? 0.0f : gu;
            } else {
                gsta[i] += gu;
            }
        }
        if (io.grad_x) {
            const float act = L.active ? 1.0f : 0.0f;
            float g0 = ens_sum(gx[0] * act, lgMp), g1 = ens_sum(gx[1] * act, lgMp),
                  g2 = ens_sum(gx[2] * act, lgMp);
            if (L.leader) {
                float *gr = io.grad_x + (int64_t)t * d.x_t_stride + (int64_t)L.b * d.x_b_stride;
                gr[d.ch_prcp] = g0; gr[d.ch_tmean] = g1; gr[d.ch_pet] = g2;
            }
        }
    }
    if (L.active) {
#pragma unroll
        for (int i = 0; i < NP; i++) {
            if (!io.g[i].sta) continue;
            float gr = raw ? gsta[i] * (usta[i] * (1.0f - usta[i])) : gsta[i];
            float *dst = io.g[i].sta + (int64_t)L.b * io.g[i].sta_b_stride + L.j;
            *dst += gr;
        }
        if (io.grad_state_in) {
#pragma unroll
            for (int k = 0; k < 5; k++) io.grad_state_in[k * N + L.n] = a[k];
        }
    }
}

// ---------------------------------------------------------------------------
// unit-hydrograph routing (reference core/calc/uh_routing.py:5-57)
// ---------------------------------------------------------------------------
__device__ __forceinline__ void route_ab(const hbvx_route_desc &r, int b, float &ua, float &ub,
                                         float &a, float &bb)
{
    float va = r.ra[(int64_t)b * r.r_stride], vb = r.rb[(int64_t)b * r.r_stride];
    ua = r.raw_sigmoid ? sigmoid_(va) : va;
    ub = r.raw_sigmoid ? sigmoid_(vb) : vb;
    a = descale_(ua, r.a_lo, r.a_hi);
    bb = descale_(ub, r.b_lo, r.b_hi);
}

// uh_gamma (uh_routing.py:5-22): one thread per (basin, tap), 16 basins x 16 tap slots per workgroup.  Every thread
// forms its tap's 1 / denom * mid * right (hbvx_popk::gamma_denom / gamma_tap, hbv_pop.h: the text gamma_taps runs); the
// 15 values of a basin meet in LDS, every thread sums them k = 0..14 in that order, zeros from L on included, and
// divides its own.  One thread per basin walked 15 powf + 15 expf + lgammaf in series on 11 workgroups of 64
// (10-14 us at 671 basins).
#define UH_PB 16        // basins per block of k_uh_gamma
__global__ void __launch_bounds__(16 * UH_PB) k_uh_gamma(const hbvx_route_desc r, float *__restrict__ uh)
{
    static_assert(HBVX_UH_MAXLEN <= 16, "k_uh_gamma: 16 tap slots");
    __shared__ float sw[16][UH_PB];
    const int bl = threadIdx.x % UH_PB, k = threadIdx.x / UH_PB;
    const int b = blockIdx.x * UH_PB + bl;
    const bool mine = b < r.B && k < r.L;
    float v = 0.0f;
    if (mine) {
        float ua, ub, a, bb;
        route_ab(r, b, ua, ub, a, bb);
        float aa = fmaxf(a, 0.0f) + 0.1f;
        float theta = fmaxf(bb, 0.0f) + 0.5f;
        v = hbvx_popk::gamma_tap(hbvx_popk::gamma_denom(aa, theta), aa, theta, k);
    }
    sw[k][bl] = v;
    __syncthreads();
    if (!mine) return;
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < HBVX_UH_MAXLEN; j++) sum += sw[j][bl];
    uh[(int64_t)b * r.L + k] = v / sum;
}

// Routing kernels: the 64 lanes of a wave are 64 consecutive basins (256-byte coalesced accesses); a workgroup stages
// its days' rows in LDS, so every input element is read from memory once (plus a 14-day halo per workgroup), and the
// 15-tap window slides through registers.  ROUTE_CHUNK: the days of a wave in k_route_fwd, of a thread in
// k_route_tan_batch.
#ifndef ROUTE_CHUNK
#define ROUTE_CHUNK 32
#endif
// The adjoint's chunk: its tap-gradient partials are per chunk (their sums are part of the gradient's bits), so longer
// chunks halve the second stage's input.  Measured at the headline shape with one thread per (basin, chunk) and the
// hydrograph in a launch of its own (round 5, whole-library variants): forward 32 / 16 / 64 days: 81 / 78 / 82 us; adjoint:
// 68 / 84 / 57 us.  The workgroup forms below, kernel trace at config 2 (profiles/r20_route_bfi_fold.md): k_uh_gamma
// 13.7 -> 6 us, k_route_fwd 58.6 -> 47 us (four series), k_route_bwd 37.6 -> 35.5 us with the zeros of three more rows
// (a 10 us fill before), k_route_bwd_params 15.7 -> 12 us.
#ifndef ROUTE_CHUNK_BWD
#define ROUTE_CHUNK_BWD 64
#endif

// Block map of the routing and BFI kernels.  Workgroups are dealt round-robin over the 8 XCDs (block i runs on XCD
// i % 8: observed, not guaranteed -- it only matters for speed; hbv_chunked.h), each with its own L2.  A [T,B] row is
// 4-byte aligned only, so the 256-byte (64-byte) piece a workgroup takes of it shares its first and last 128-byte line
// with the neighbouring basins' workgroups; on the plain grid those run on other XCDs and the shared lines are
// fetched once per L2: 1.5 x the bytes (a micro-benchmark of k_route_fwd's loads and stores alone at config 2: 36 us on
// the plain grid, 25 us on this map, 23 us for a flat copy of the same bytes).  Here XCD c takes the contiguous run
// [c * per, (c + 1) * per) of the n logical blocks, basins fastest, so neighbours meet in one L2.
// The launch has xcd_grid(n) workgroups; -1: none for this one (uniform over the workgroup).
static inline unsigned xcd_grid(int64_t n) { return (unsigned)((n + 7) / 8 * 8); }
__device__ __forceinline__ int xcd_block()
{
    const int per = gridDim.x / 8;
    return (blockIdx.x % 8) * per + blockIdx.x / 8;
}

__device__ __forceinline__ void load_uh(const float *__restrict__ uh, int b, int L, float *w)
{
#pragma unroll
    for (int k = 0; k < HBVX_UH_MAXLEN; k++) w[k] = (k < L) ? uh[(int64_t)b * L + k] : 0.0f;
}

// uh_conv (uh_routing.py:25-57): y[s,t,b] = sum_k UH[b,k] * q[s,t-k,b], zero history.
// Workgroup (xcd_block: basins, then days, then series) = 64 basins x 4 * ROUTE_CHUNK days, wave p the days ROUTE_CHUNK p .. of them.  The tile's
// rows (with the 14 days before it) go to LDS with every thread's share of the loads issued at once: one round trip to
// memory per workgroup and a halo of 14 rows in 142 (a thread per (basin, chunk) loading for itself made five
// dependent round trips and re-read 14 rows in 46).
#define ROUTE_FWD_TILE (4 * ROUTE_CHUNK)
#define ROUTE_FWD_ROWS (ROUTE_FWD_TILE + HBVX_UH_MAXLEN - 1)
__global__ void __launch_bounds__(256) k_route_fwd(int T, int B, int S, int L,
                                                   const float *__restrict__ q,
                                                   const float *__restrict__ uh,
                                                   float *__restrict__ y)
{
    __shared__ float sq[ROUTE_FWD_ROWS][64];      // q[t0 - 14 + r], zero before the record and from T on
    constexpr int NLOAD = (ROUTE_FWD_ROWS + 3) / 4;
    const int lane = threadIdx.x & 63, part = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (a scalar: row addresses are)
    const int nx = (B + 63) / 64, ny = (T + ROUTE_FWD_TILE - 1) / ROUTE_FWD_TILE;
    const int blk = xcd_block();
    if (blk >= nx * ny * S) return;       // (the whole workgroup)
    const int b = (blk % nx) * 64 + lane;
    const int t0 = (blk / nx) % ny * ROUTE_FWD_TILE;
    const bool live = b < B;        // (no early return before the barrier)
    const int s = blk / (nx * ny);
    const float *qs = q + (int64_t)s * T * B;      // rows are addressed as (uniform row pointer)[b]
    float *ys = y + (int64_t)s * T * B;
    float v[NLOAD];
#pragma unroll
    for (int i = 0; i < NLOAD; i++) {
        const int r = part + 4 * i, t = t0 - (HBVX_UH_MAXLEN - 1) + r;
        v[i] = (live && r < ROUTE_FWD_ROWS && t >= 0 && t < T) ? (qs + (int64_t)t * B)[b] : 0.0f;
    }
    float w[HBVX_UH_MAXLEN];
    load_uh(uh, live ? b : B - 1, L, w);
#pragma unroll
    for (int i = 0; i < NLOAD; i++) {
        const int r = part + 4 * i;
        if (r < ROUTE_FWD_ROWS) sq[r][lane] = v[i];
    }
    __syncthreads();
    const int c0 = part * ROUTE_CHUNK;
    if (!live || t0 + c0 >= T) return;
    float win[HBVX_UH_MAXLEN];
#pragma unroll
    for (int k = 1; k < HBVX_UH_MAXLEN; k++) win[k] = sq[c0 + HBVX_UH_MAXLEN - 1 - k][lane];
#pragma unroll 8
    for (int d = 0; d < ROUTE_CHUNK; d++) {
        win[0] = sq[c0 + HBVX_UH_MAXLEN - 1 + d][lane];
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < HBVX_UH_MAXLEN; k++) acc += w[k] * win[k];
        if (t0 + c0 + d < T) (ys + (int64_t)(t0 + c0 + d) * B)[b] = acc;
#pragma unroll
        for (int k = HBVX_UH_MAXLEN - 1; k > 0; k--) win[k] = win[k - 1];
    }
}

// conv1d backward in one pass over the chunk:
//   gq[s,t,b] = sum_k UH[b,k] * gy[s,t+k,b]                      (w.r.t. the input)
//   ws[(chunk*L+k)*B + b] = sum_{s, t in chunk} gy[s,t,b] * q[s,t-k,b]   (partial tap gradients)
// Workgroup (xcd_block: basins, then chunks) = 64 basins x one chunk of ROUTE_CHUNK_BWD days, four waves.  The chunk's rows of q (with the 14 days
// before it) and of gy (with the 14 days after it) are staged in LDS, every thread's share of the loads issued at
// once -- one round trip to memory per series instead of one per 8 days -- and each row is read from memory
// once.  The sums are independent of each other, so the four waves share them without changing one: wave p forms
// gq of the days 16 p .. 16 p + 15 of the chunk (all 15 taps each, ascending k) and the tap gradients 4 p .. 4 p + 3
// (all days of the chunk, series by series, ascending t; fma in double).  One thread per (basin, chunk) walked
// 64 days x 15 taps x (fp32 multiply-add + fp64 fma) on 1.2 waves per SIMD.
// gq has n_rows >= S rows of [T,B]: the rows S .. n_rows - 1 get zeros for the workgroup's own days and basins.
#define ROUTE_BWD_ROWS (ROUTE_CHUNK_BWD + HBVX_UH_MAXLEN - 1)
#define ROUTE_BWD_DAYS (ROUTE_CHUNK_BWD / 4)     // days of gq per wave
#define ROUTE_BWD_TAPS 4                         // tap gradients per wave (the last wave: 3)
static_assert(ROUTE_CHUNK_BWD % 4 == 0 && 4 * ROUTE_BWD_TAPS >= HBVX_UH_MAXLEN, "k_route_bwd: four waves share a chunk");
__global__ void __launch_bounds__(256) k_route_bwd(int T, int B, int S, int L, int n_rows,
                                                   const float *__restrict__ q,
                                                   const float *__restrict__ uh,
                                                   const float *__restrict__ gy,
                                                   float *__restrict__ gq, double *__restrict__ ws)
{
    __shared__ float sq[ROUTE_BWD_ROWS][64], sg[ROUTE_BWD_ROWS][64];   // q[t0 - 14 + r], gy[t0 + r]
    constexpr int NLOAD = (ROUTE_BWD_ROWS + 3) / 4;
    const int lane = threadIdx.x & 63, part = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (a scalar: row addresses are)
    const int nx = (B + 63) / 64;
    const int blk = xcd_block();
    if (blk >= nx * ((T + ROUTE_CHUNK_BWD - 1) / ROUTE_CHUNK_BWD)) return;      // (the whole workgroup)
    const int b = (blk % nx) * 64 + lane;
    const int chunk = blk / nx;
    const int t0 = chunk * ROUTE_CHUNK_BWD;
    const int t1 = min(T, t0 + ROUTE_CHUNK_BWD);
    const bool live = b < B;        // (no early return: the workgroup meets at barriers)
    const int d0 = part * ROUTE_BWD_DAYS, k0 = part * ROUTE_BWD_TAPS;
    // The tap gradients are summed in DOUBLE: what leaves this path is sum_k gw[k] w_k (ln t_k - <ln t>), whose weights
    // sum to zero (the hydrograph is normalised), so the common part of the gw[k] -- nearly all of them when the
    // inflow is smooth -- cancels and float32 sums (eps x ~1e+2) left 1e-6 where the result is 1e-4: 0.7 % off the
    // float64 value on hbv_ties' route_b, twenty times the reference's own error (round 5).
    float w[HBVX_UH_MAXLEN];
    double gw[ROUTE_BWD_TAPS];
    load_uh(uh, live ? b : B - 1, L, w);
#pragma unroll
    for (int j = 0; j < ROUTE_BWD_TAPS; j++) gw[j] = 0.0;
    for (int s = 0; s < S; s++) {
        const float *qs = q + (int64_t)s * T * B;      // rows are addressed as (uniform row pointer)[b]
        const float *gs = gy + (int64_t)s * T * B;
        float *gqs = gq + (int64_t)s * T * B;
        float vq[NLOAD], vg[NLOAD];
#pragma unroll
        for (int i = 0; i < NLOAD; i++) {
            const int r = part + 4 * i, tq = t0 - (HBVX_UH_MAXLEN - 1) + r, tg = t0 + r;
            const bool in = live && r < ROUTE_BWD_ROWS;
            vq[i] = (in && tq >= 0 && tq < t1) ? (qs + (int64_t)tq * B)[b] : 0.0f;
            vg[i] = (in && tg < T) ? (gs + (int64_t)tg * B)[b] : 0.0f;
        }
        if (s) __syncthreads();     // the previous series' tile has been read
#pragma unroll
        for (int i = 0; i < NLOAD; i++) {
            const int r = part + 4 * i;
            if (r < ROUTE_BWD_ROWS) {
                sq[r][lane] = vq[i];
                sg[r][lane] = vg[i];
            }
        }
        __syncthreads();
        if (s == 0 && live) {
            for (int z = S; z < n_rows; z++) {
                float *gz = gq + (int64_t)z * T * B;
#pragma unroll
                for (int d = 0; d < ROUTE_BWD_DAYS; d++)
                    if (t0 + d0 + d < t1) (gz + (int64_t)(t0 + d0 + d) * B)[b] = 0.0f;
            }
        }
        float g[ROUTE_BWD_DAYS + HBVX_UH_MAXLEN - 1];     // gy[t0 + d0 + i], zero from T on
#pragma unroll
        for (int i = 0; i < ROUTE_BWD_DAYS + HBVX_UH_MAXLEN - 1; i++) g[i] = sg[d0 + i][lane];
#pragma unroll
        for (int d = 0; d < ROUTE_BWD_DAYS; d++) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < HBVX_UH_MAXLEN; k++) acc += w[k] * g[d + k];
            if (live && t0 + d0 + d < t1) (gqs + (int64_t)(t0 + d0 + d) * B)[b] = acc;
        }
        // tap k0 + j of day t0 + i reads q[t0 + i - k0 - j] = sq[i + 14 - k0 - j]; the window slides through qw.  (The
        // last wave's fourth value is tap 15, which does not exist: its row index is kept in range and its sum dropped.)
        double qw[ROUTE_BWD_TAPS];
#pragma unroll
        for (int j = 1; j < ROUTE_BWD_TAPS; j++) qw[j] = (double)sq[max(HBVX_UH_MAXLEN - 1 - k0 - j, 0)][lane];
        const int nd = t1 - t0;
#pragma unroll 8
        for (int i = 0; i < nd; i++) {
            qw[0] = (double)sq[i + HBVX_UH_MAXLEN - 1 - k0][lane];
            const double g0 = (double)sg[i][lane];
#pragma unroll
            for (int j = 0; j < ROUTE_BWD_TAPS; j++) gw[j] = fma(g0, qw[j], gw[j]);
#pragma unroll
            for (int j = ROUTE_BWD_TAPS - 1; j > 0; j--) qw[j] = qw[j - 1];
        }
    }
    if (ws && live) {
#pragma unroll
        for (int j = 0; j < ROUTE_BWD_TAPS; j++)
            if (k0 + j < L) ws[((int64_t)chunk * L + k0 + j) * B + b] = gw[j];
    }
}

// Tangent of the routing: y_dot[s,t,b] = sum_k UH[b,k] q_dot[s,t-k,b] + UH_dot[b,k] q[s,t-k,b], with
//   UH_dot_k = w_k ((ln t_k - sum_j w_j ln t_j) aa_dot + (t_k - sum_j w_j t_j) / theta^2 theta_dot)
// (the derivatives k_route_bwd_params applies; the means in double, where their sum cancels).  The thread layout
// of k_route_fwd; every thread forms its basin's UH_dot itself (15 taps: cheaper than a second launch).
// blockIdx.z = direction * S + series: one launch for all directions (at 200 directions a launch each would cost more
// than the recurrence); hbvx_route_tangent is the launch with one direction.
__global__ void __launch_bounds__(256) k_route_tan_batch(const hbvx_route_desc r, const float *__restrict__ q,
                                                         const float *__restrict__ uh, const float *__restrict__ qd_all,
                                                         int64_t qd_ds, const float *__restrict__ rad_all,
                                                         const float *__restrict__ rbd_all, int64_t r_ds,
                                                         float *__restrict__ yd_all)
{
    const int T = r.T, B = r.B, L = r.L;
    const int b = blockIdx.x * 64 + (threadIdx.x & 63);
    const int chunk = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int t0 = chunk * ROUTE_CHUNK;
    if (b >= B || t0 >= T) return;
    const int t1 = min(T, t0 + ROUTE_CHUNK);
    const int dir = blockIdx.z / r.S, s = blockIdx.z - dir * r.S;
    const float *qd = qd_all ? qd_all + dir * qd_ds : nullptr;
    const float *rad = rad_all ? rad_all + dir * r_ds : nullptr, *rbd = rbd_all ? rbd_all + dir * r_ds : nullptr;
    float *yd = yd_all + (int64_t)dir * r.S * T * B;
    float ua, ub, a, bb;
    route_ab(r, b, ua, ub, a, bb);
    const float theta = fmaxf(bb, 0.0f) + 0.5f;
    float dua = rad ? rad[(int64_t)b * r.r_stride] : 0.0f, dub = rbd ? rbd[(int64_t)b * r.r_stride] : 0.0f;
    if (r.raw_sigmoid) {
        dua *= ua * (1.0f - ua);
        dub *= ub * (1.0f - ub);
    }
    const double daa = (a > 0.0f) ? (double)(dua * (r.a_hi - r.a_lo)) : 0.0;      // relu (uh_routing.py:11-14)
    const double dth = (bb > 0.0f) ? (double)(dub * (r.b_hi - r.b_lo)) : 0.0;
    float w[HBVX_UH_MAXLEN], dw[HBVX_UH_MAXLEN];
    load_uh(uh, b, L, w);
    double mlt = 0.0, mt = 0.0;
#pragma unroll
    for (int k = 0; k < HBVX_UH_MAXLEN; k++) {
        const double tk = (double)k + 0.5;
        mlt += (double)w[k] * log(tk);
        mt += (double)w[k] * tk;
    }
    const double th2 = (double)theta * (double)theta;
#pragma unroll
    for (int k = 0; k < HBVX_UH_MAXLEN; k++) {
        const double tk = (double)k + 0.5;
        dw[k] = (float)((double)w[k] * ((log(tk) - mlt) * daa + ((tk - mt) / th2) * dth));
    }
    const float *qs = q + (int64_t)s * T * B + b;
    const float *qds = qd ? qd + (int64_t)s * T * B + b : nullptr;
    float *ys = yd + (int64_t)s * T * B + b;
    float win[HBVX_UH_MAXLEN], dwin[HBVX_UH_MAXLEN];
#pragma unroll
    for (int k = 1; k < HBVX_UH_MAXLEN; k++) {
        win[k] = (t0 - k >= 0) ? qs[(int64_t)(t0 - k) * B] : 0.0f;
        dwin[k] = (qds && t0 - k >= 0) ? qds[(int64_t)(t0 - k) * B] : 0.0f;
    }
    for (int t = t0; t < t1; t++) {
        win[0] = qs[(int64_t)t * B];
        dwin[0] = qds ? qds[(int64_t)t * B] : 0.0f;
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < HBVX_UH_MAXLEN; k++) acc += w[k] * dwin[k] + dw[k] * win[k];
        ys[(int64_t)t * B] = acc;
#pragma unroll
        for (int k = HBVX_UH_MAXLEN - 1; k > 0; k--) {
            win[k] = win[k - 1];
            dwin[k] = dwin[k - 1];
        }
    }
}

// stage 2: reduce the chunks (fixed order: deterministic) and go through the normalised
// gamma UH to the routing inputs.  Block = 16 basins x 16 tap-threads x 4 parts: thread (bl, k, part) sums tap k over
// the chunks c = part (mod 4) in ascending order (part 0 also the last nchunk mod 4 ones), the parts are combined as
// (p0 + p1) + (p2 + p3) -- the association the one-thread-per-tap version used, on four times the threads and blocks
// (11 blocks of 1 024 at config 2 were a 35 us latency chain of 229 dependent loads; with one load in flight per thread
// the four parts took 15.7 us, with eight 12 us) -- then the k == 0 threads finish
// per basin.
// d w_k / d aa    = w_k (ln t_k - sum_j w_j ln t_j)      (Gamma(aa) and theta^aa cancel
// d w_k / d theta = w_k (t_k - sum_j w_j t_j) / theta^2    in the normalisation)
#define ROUTE_PB 16      // basins per block of k_route_bwd_params
__global__ void __launch_bounds__(1024) k_route_bwd_params(const hbvx_route_desc r, int nchunk,
                                                           const float *__restrict__ uh,
                                                           const double *__restrict__ ws,
                                                           float *grad_ra, float *grad_rb)
{
    __shared__ double prt[4][16][ROUTE_PB];
    __shared__ double red[16][ROUTE_PB];
    const int bl = threadIdx.x & (ROUTE_PB - 1), k = (threadIdx.x >> 4) & 15, part = threadIdx.x >> 8;
    const int b = blockIdx.x * ROUTE_PB + bl;
    const int B = r.B, L = r.L;
    double acc = 0.0;
    if (b < B && k < L) {
        const double *src = ws + (int64_t)k * B + b;
        const int64_t cs = (int64_t)L * B;
        const int n4 = nchunk & ~3;
        int c = part;
        // eight chunks' loads issued before the first add (one in flight made nchunk / 4 dependent round trips); the
        // adds keep their ascending order
        for (; c + 4 * 7 < n4; c += 4 * 8) {
            double v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = src[(int64_t)(c + 4 * j) * cs];
#pragma unroll
            for (int j = 0; j < 8; j++) acc += v[j];
        }
        for (; c < n4; c += 4) acc += src[(int64_t)c * cs];
        if (part == 0)
            for (int c = n4; c < nchunk; c++) acc += src[(int64_t)c * cs];
    }
    prt[part][k][bl] = acc;
    __syncthreads();
    if (part == 0) red[k][bl] = (prt[0][k][bl] + prt[1][k][bl]) + (prt[2][k][bl] + prt[3][k][bl]);
    __syncthreads();
    if (part != 0 || k != 0 || b >= B) return;
    float ua, ub, a, bb;
    route_ab(r, b, ua, ub, a, bb);
    const float theta = fmaxf(bb, 0.0f) + 0.5f;
    // the finish in double as well: the cancellation happens HERE (sum_j c_j = 0), on sums that are now exact to 1e-16
    double w[HBVX_UH_MAXLEN], gw[HBVX_UH_MAXLEN];
    double mlt = 0.0, mt = 0.0;
#pragma unroll
    for (int j = 0; j < HBVX_UH_MAXLEN; j++) {
        gw[j] = (j < L) ? red[j][bl] : 0.0;
        w[j] = (j < L) ? (double)uh[(int64_t)b * L + j] : 0.0;
        const double tk = (double)j + 0.5;
        mlt += w[j] * log(tk);
        mt += w[j] * tk;
    }
    double gaa = 0.0, gth = 0.0;
    const double th2 = (double)theta * (double)theta;
#pragma unroll
    for (int j = 0; j < HBVX_UH_MAXLEN; j++) {
        const double tk = (double)j + 0.5;
        gaa += gw[j] * w[j] * (log(tk) - mlt);
        gth += gw[j] * w[j] * ((tk - mt) / th2);
    }
    float ga = (a > 0.0f) ? (float)gaa : 0.0f;   // relu backward (uh_routing.py:11-14)
    float gb = (bb > 0.0f) ? (float)gth : 0.0f;
    float gua = ga * (r.a_hi - r.a_lo), gub = gb * (r.b_hi - r.b_lo);
    if (r.raw_sigmoid) {
        gua *= ua * (1.0f - ua);
        gub *= ub * (1.0f - ub);
    }
    if (grad_ra) grad_ra[(int64_t)b * r.r_stride] += gua;
    if (grad_rb) grad_rb[(int64_t)b * r.r_stride] += gub;
}

// ---------------------------------------------------------------------------
// host side of the C ABI
// ---------------------------------------------------------------------------
int hbvx_host::check_desc(const hbvx_desc *d)
{
    if (!d) return fail(HBVX_E_NULL, "desc is NULL");
    if (d->abi_version != HBVX_ABI_VERSION) return fail(HBVX_E_ABI, "abi_version mismatch");
    if (d->T < 0 || d->B <= 0 || d->M <= 0 || d->M > 64) return fail(HBVX_E_SHAPE, "bad T/B/M");
    bool ok = false;
    if (d->model == HBVX_MODEL_HBV10) ok = (d->n_param == 12 || d->n_param == 13);
    else if (d->model == HBVX_MODEL_HBV11P) ok = (d->n_param == 14);
    else if (d->model == HBVX_MODEL_HBV20) ok = (d->n_param == 16);
    else if (d->model == HBVX_MODEL_HBVADJ) ok = (d->n_param == 12 || d->n_param == 13);
    else if (d->model == HBVX_MODEL_HOURLY) ok = (d->n_param == 19);
    else return fail(HBVX_E_UNSUPPORTED, "unknown model");
    if (!ok) return fail(HBVX_E_SHAPE, "n_param does not match model");
    if (!d->x && d->T > 0) return fail(HBVX_E_NULL, "forcing pointer is NULL");   /* an empty record has no forcings */
    if (d->ch_prcp < 0 || d->ch_tmean < 0 || d->ch_pet < 0)
        return fail(HBVX_E_SHAPE, "negative forcing channel");
    if (!(d->nearzero >= 0.0f)) return fail(HBVX_E_SHAPE, "nearzero must be >= 0 (the storages' lower clamp, hbv.py:54)");
    if ((d->model == HBVX_MODEL_HBV20 || d->model == HBVX_MODEL_HOURLY) && (!d->ac || !d->elev))
        return fail(HBVX_E_NULL, "HBV 2.0 needs ac and elev");
    for (int i = 0; i < d->n_param; i++)
        if (!d->p[i].sta) return fail(HBVX_E_NULL, "static parameter pointer is NULL");
    // Bounds come from the caller (a model's parameter_bounds table may be edited).  Two short forms of the forward
    // equal the reference only inside the reference's own tables (hbv.py:88-101, hbv_2_hourly.py:97-119) and are
    // refused outside them instead of silently computing something else (hbv_step.h):
    //  * the evaporation factor is taken from the storage BEFORE the excess leaves it (fwd_soil, CHAIN): equal to
    //    hbv.py:474-477 iff LP <= 1 (with LP > 1 an excess day gives (1 / LP)**BETAET < 1 there, 1 here);
    //  * the powers run on 2^(y log2 x) without a lower clamp of the base (pow_unit_): x = 0 needs y > 0
    //    (0 * -inf is NaN where torch's 0**0 is 1), i.e. positive lower bounds of BETA, BETAET, ALPHA.
    if (d->model != HBVX_MODEL_HBVADJ) {
        if (!(d->p[P_LP].hi <= 1.0f && d->p[P_LP].lo <= 1.0f))
            return fail(HBVX_E_UNSUPPORTED, "parLP bounds above 1 are not supported (evaporation factor on an excess day, hbv.py:474-477)");
        if (!(d->p[P_BETA].lo > 0.0f && d->p[P_BETA].hi > 0.0f))
            return fail(HBVX_E_UNSUPPORTED, "parBETA bounds must be positive (soil wetness power, hbv.py:462)");
        if (d->n_param > P_BETAET && !(d->p[P_BETAET].lo > 0.0f && d->p[P_BETAET].hi > 0.0f))
            return fail(HBVX_E_UNSUPPORTED, "parBETAET bounds must be positive (evaporation factor power, hbv.py:476)");
        if (d->model == HBVX_MODEL_HOURLY && !(d->p[P_ALPHA].lo > 0.0f && d->p[P_ALPHA].hi > 0.0f))
            return fail(HBVX_E_UNSUPPORTED, "parALPHA bounds must be positive (infiltration power, hbv_2_hourly.py:590-600)");
    }
    return HBVX_OK;
}

int hbvx_host::lg_members(int M)
{
    int lg = 0;
    while ((1 << lg) < M) lg++;
    return lg;
}

int hbvx_host::env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

// HBVX_KERNEL=simple selects the one-wave kernels (kept as a cross-check); default is the
// wave-specialised / streaming / time-parallel families.
bool hbvx_host::use_tiled(const hbvx_desc *d)
{
    const char *v = getenv("HBVX_KERNEL");
    if (v && !strcmp(v, "simple")) return false;
    return d->T > 0;
}

hipError_t hbvx_host::set_dynamic_lds(const void *kern, int lds)
{
    struct Entry { const void *k; int dev, lds; };
    static std::mutex mu;
    static Entry seen[256];
    static int n_seen = 0;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    Entry *e = nullptr;
    for (int i = 0; i < n_seen && !e; i++)
        if (seen[i].k == kern && seen[i].dev == dev) e = &seen[i];
    if (e && lds <= e->lds) return hipSuccess;
    const hipError_t rc = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (rc != hipSuccess) return rc;
    if (e) e->lds = lds;
    else if (n_seen < 256) seen[n_seen++] = Entry{kern, dev, lds};
    // (a full table only costs the driver round trip again: the attribute is still raised before the launch)
    return hipSuccess;
}

int hbvx_host::count_dyn(const hbvx_desc *d)
{
    int nd = 0;
    for (int i = 0; i < d->n_param; i++) nd += d->p[i].dyn ? 1 : 0;
    return nd;
}

int hbvx_host::device_cu_count()
{
    static int n_cu[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (n_cu[dev] == 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        n_cu[dev] = v;
    }
    return n_cu[dev];
}

bool &hbvx_host::zero_taken()
{
    static thread_local bool taken = false;
    return taken;
}

static int forward_dispatch(const hbvx_desc *d, const hbvx_fwd_out *out, void *stream);

extern "C" int hbvx_forward(const hbvx_desc *d, const hbvx_fwd_out *out, void *stream)
{
    zero_taken() = false;
    if (out && out->zero_ptr && !out->zero_state) return fail(HBVX_E_NULL, "zero_ptr needs zero_state");
    return forward_dispatch(d, out, stream);
}

static int forward_dispatch(const hbvx_desc *d, const hbvx_fwd_out *out, void *stream)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (d->model == HBVX_MODEL_HBVADJ) return fail(HBVX_E_UNSUPPORTED, "use hbvx_adj_forward for HBVADJ");
    if (!out || !out->state_out) return fail(HBVX_E_NULL, "state_out is NULL");
    const int want_nf = (d->model == HBVX_MODEL_HBV10) ? 11 : 12;
    if (out->flux && out->n_flux != want_nf) return fail(HBVX_E_SHAPE, "n_flux does not match model");
    if (out->traj && out->traj_layout != HBVX_TRAJ_ROWS) {
        const int kind = HBVX_TRAJ_KIND(out->traj_layout);
        if (kind == HBVX_TRAJ_CKPT) {
            // K-day checkpoints: the streaming kernel where it has an instance, else the generic one
            const int K = HBVX_TRAJ_CKPT_DAYS(out->traj_layout);
            if (K != 4 && K != 8 && K != 16) return fail(HBVX_E_SHAPE, "checkpoint interval must be 4, 8 or 16");
            if (out->aux) return fail(HBVX_E_SHAPE, "checkpoints: aux must be NULL");
            if (try_fwd_stream(d, out, stream, &rc)) return rc;
            if (try_fwd_pipe(d, out, stream, &rc)) return rc;
            if (try_fwd_stream(d, out, stream, &rc, true)) return rc;
            FwdArgs ca;
            ca.d = *d;
            ca.o = *out;
            ca.lgMp = lg_members(d->M);
            const int bpw_c = 64 >> ca.lgMp;
            note_dispatch(0, "simple");
            const dim3 grid_c((d->B + bpw_c - 1) / bpw_c);
            hipError_t ec = with_model(d, [&](auto m, auto be) {
                hipLaunchKernelGGL((k_fwd<m, be>), grid_c, dim3(64), 0, (hipStream_t)stream, ca);
                return hipGetLastError();
            });
            return ec == hipSuccess ? HBVX_OK : hip_fail(ec, "hbvx_forward (checkpoints) launch");
        }
        // packed trajectory: the streaming family only (hbvx_preferred_traj_layout said so)
        if (out->traj_layout != HBVX_TRAJ_PACKED) return fail(HBVX_E_SHAPE, "unknown traj_layout");
        if (try_fwd_stream(d, out, stream, &rc, true)) return rc;
        return fail(HBVX_E_UNSUPPORTED, "packed trajectory: no forward kernel for this call");
    }
    // kernel families in order of preference ("Which kernel runs when"): the streaming
    // kernels take the grids above their measured cross-over, the pipelined forward the rest of what
    // it can hold, the tiled forward whatever is left
    if (try_fwd_stream(d, out, stream, &rc)) return rc;
    if (try_fwd_pipe(d, out, stream, &rc)) return rc;
    if (try_fwd_tiled(d, out, stream, &rc)) return rc;
    FwdArgs a;
    a.d = *d;
    a.o = *out;
    a.lgMp = lg_members(d->M);
    const int bpw = 64 >> a.lgMp;
    dim3 grid((d->B + bpw - 1) / bpw);
    note_dispatch(0, "simple");
    hipError_t e = with_model(d, [&](auto m, auto be) {
        hipLaunchKernelGGL((k_fwd<m, be>), grid, dim3(64), 0, (hipStream_t)stream, a);
        return hipGetLastError();
    });
    if (e != hipSuccess) return hip_fail(e, "hbvx_forward launch");
    return HBVX_OK;
}

// hbvx_backward (n_live = 4) and hbvx_backward_live: n_live = rows of io->grad_flux4 that exist.  Below 4 only the
// one-pass static adjoint may take the call -- every other family reads four rows -- and a refusal launches nothing
static int backward_impl(const hbvx_desc *d, const hbvx_bwd_io *io, void *stream, int n_live)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (d->model == HBVX_MODEL_HBVADJ) return fail(HBVX_E_UNSUPPORTED, "use hbvx_adj_backward for HBVADJ");
    if (!io || !io->traj) return fail(HBVX_E_NULL, "traj is NULL");
    const int want_nf = (d->model == HBVX_MODEL_HBV10) ? 11 : 12;
    if (io->n_flux != want_nf) return fail(HBVX_E_SHAPE, "n_flux does not match model");
    if (d->T == 0) return HBVX_OK;
    const bool live = n_live < 4;
    if (live && (io->traj_layout != HBVX_TRAJ_ROWS || !io->grad_flux4))
        return fail(HBVX_E_UNSUPPORTED, "live rows: row trajectory and grad_flux4 only");
    if (io->traj_layout != HBVX_TRAJ_ROWS) {
        if (HBVX_TRAJ_KIND(io->traj_layout) == HBVX_TRAJ_CKPT) {
            if (try_bwd_stream_ckpt(d, io, stream, &rc)) return rc;
            if (try_bwd_ckpt(d, io, stream, &rc)) return rc;
            return fail(HBVX_E_UNSUPPORTED, "checkpoints: no adjoint kernel for this call");
        }
        if (io->traj_layout != HBVX_TRAJ_PACKED) return fail(HBVX_E_SHAPE, "unknown traj_layout");
        if (try_bwd_stream(d, io, stream, &rc)) return rc;
        return fail(HBVX_E_UNSUPPORTED, "packed trajectory: no adjoint kernel for this call");
    }
    if (try_bwd_stream(d, io, stream, &rc, n_live)) return rc;
    if (try_bwd_chunked(d, io, stream, &rc, n_live)) return rc;
    if (live) return fail(HBVX_E_UNSUPPORTED, "live rows: the one-pass static adjoint does not take this call");
    if (try_bwd_tiled(d, io, stream, &rc)) return rc;
    BwdArgs a;
    a.d = *d;
    a.io = *io;
    a.lgMp = lg_members(d->M);
    const int bpw = 64 >> a.lgMp;
    dim3 grid((d->B + bpw - 1) / bpw);
    store_gate(io, (hipStream_t)stream);
    note_dispatch(1, "simple");
    hipError_t e = with_model(d, [&](auto m, auto be) {
        hipLaunchKernelGGL((k_bwd<m, be>), grid, dim3(64), 0, (hipStream_t)stream, a);
        return hipGetLastError();
    });
    if (e != hipSuccess) return hip_fail(e, "hbvx_backward launch");
    return HBVX_OK;
}

extern "C" int hbvx_backward(const hbvx_desc *d, const hbvx_bwd_io *io, void *stream)
{
    return backward_impl(d, io, stream, 4);
}

// include/hbvx_live_rows.h
extern "C" int hbvx_backward_live(const hbvx_desc *d, const hbvx_bwd_io *io, int32_t n_live4, void *stream)
{
    if (n_live4 < 1 || n_live4 > 4) return fail(HBVX_E_SHAPE, "n_live4 must be 1 .. 4");
    return backward_impl(d, io, stream, n_live4);
}

static int check_route(const hbvx_route_desc *r)
{
    if (!r) return fail(HBVX_E_NULL, "route desc is NULL");
    if (r->abi_version != HBVX_ABI_VERSION) return fail(HBVX_E_ABI, "abi_version mismatch");
    if (r->T <= 0 || r->B <= 0 || r->S <= 0) return fail(HBVX_E_SHAPE, "bad T/B/S");
    const int L = r->T < HBVX_UH_MAXLEN ? r->T : HBVX_UH_MAXLEN;
    if (r->L != L) return fail(HBVX_E_SHAPE, "L must be min(T, 15)");
    if (!r->ra || !r->rb) return fail(HBVX_E_NULL, "routing parameter pointer is NULL");
    return HBVX_OK;
}

extern "C" int hbvx_route_forward(const hbvx_route_desc *r, const float *q, float *uh,
                                  float *q_rout, void *stream)
{
    int rc = check_route(r);
    if (rc) return rc;
    if (!q || !uh || !q_rout) return fail(HBVX_E_NULL, "route buffer is NULL");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_uh_gamma, dim3((r->B + UH_PB - 1) / UH_PB), dim3(16 * UH_PB), 0, st, *r, uh);
    const int64_t nblk = (int64_t)((r->B + 63) / 64) * ((r->T + ROUTE_FWD_TILE - 1) / ROUTE_FWD_TILE) * r->S;
    if (nblk > INT32_MAX - 8) return fail(HBVX_E_SHAPE, "routing: too many (basin, day, series) tiles for one launch");
    hipLaunchKernelGGL(k_route_fwd, dim3(xcd_grid(nblk)), dim3(256), 0, st, r->T, r->B, r->S, r->L, q, uh, q_rout);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_route_forward launch");
    return HBVX_OK;
}

static int route_chunks(const hbvx_route_desc *r) { return (r->T + ROUTE_CHUNK_BWD - 1) / ROUTE_CHUNK_BWD; }   // the adjoint's

extern "C" uint64_t hbvx_route_workspace_bytes(const hbvx_route_desc *r)
{
    if (!r || r->T <= 0 || r->B <= 0) return 0;
    return (uint64_t)route_chunks(r) * (uint64_t)r->L * (uint64_t)r->B * sizeof(double);    // (8-byte aligned: torch's allocations are)
}

static int launch_route_bwd(const hbvx_route_desc *r, const float *q, const float *uh, const float *grad_q_rout,
                            float *grad_q, int n_rows, float *grad_ra, float *grad_rb, void *workspace,
                            uint64_t workspace_bytes, void *stream, const char *what)
{
    int rc = check_route(r);
    if (rc) return rc;
    if (!q || !uh || !grad_q_rout || !grad_q) return fail(HBVX_E_NULL, "route buffer is NULL");
    if (n_rows < r->S) return fail(HBVX_E_SHAPE, "grad_q has fewer rows than series");
    hipStream_t st = (hipStream_t)stream;
    const bool want_p = grad_ra || grad_rb;
    if (want_p && (!workspace || workspace_bytes < hbvx_route_workspace_bytes(r)))
        return fail(HBVX_E_NULL, "route workspace missing or too small");
    const int nchunk = route_chunks(r);
    const int64_t nblk = (int64_t)((r->B + 63) / 64) * nchunk;
    if (nblk > INT32_MAX - 8) return fail(HBVX_E_SHAPE, "routing adjoint: too many (basin, chunk) tiles for one launch");
    hipLaunchKernelGGL(k_route_bwd, dim3(xcd_grid(nblk)), dim3(256), 0, st, r->T, r->B, r->S, r->L, n_rows, q, uh,
                       grad_q_rout, grad_q, want_p ? (double *)workspace : nullptr);
    if (want_p)
        hipLaunchKernelGGL(k_route_bwd_params, dim3((r->B + ROUTE_PB - 1) / ROUTE_PB), dim3(1024), 0, st, *r, nchunk,
                           uh, (const double *)workspace, grad_ra, grad_rb);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return HBVX_OK;
}

extern "C" int hbvx_route_backward(const hbvx_route_desc *r, const float *q, const float *uh,
                                   const float *grad_q_rout, float *grad_q, float *grad_ra,
                                   float *grad_rb, void *workspace, uint64_t workspace_bytes,
                                   void *stream)
{
    return launch_route_bwd(r, q, uh, grad_q_rout, grad_q, r ? r->S : 0, grad_ra, grad_rb, workspace, workspace_bytes,
                            stream, "hbvx_route_backward launch");
}

extern "C" int hbvx_route_backward_rows(const hbvx_route_desc *r, const float *q, const float *uh,
                                        const float *grad_q_rout, float *grad_q, int32_t grad_q_rows, float *grad_ra,
                                        float *grad_rb, void *workspace, uint64_t workspace_bytes, void *stream)
{
    return launch_route_bwd(r, q, uh, grad_q_rout, grad_q, grad_q_rows, grad_ra, grad_rb, workspace, workspace_bytes,
                            stream, "hbvx_route_backward_rows launch");
}

// ---------------------------------------------------------------------------
// diagnostics: device-side accuracy probe of hbvx::pow_pos_ (tests only)
// ---------------------------------------------------------------------------
__global__ void k_selftest_pow(const float *x, const float *y, float *out, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pow_pos_(x[i], y[i]);
}

extern "C" int hbvx_selftest_pow(const float *x, const float *y, float *out, int n, void *stream)
{
    if (!x || !y || !out || n <= 0) return fail(HBVX_E_NULL, "selftest_pow: bad arguments");
    hipLaunchKernelGGL(k_selftest_pow, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, y,
                       out, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "selftest_pow launch");
    return HBVX_OK;
}

__global__ void k_selftest_div(const float *x, const float *y, float *out, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = div_(x[i], y[i]);
}

extern "C" int hbvx_selftest_div(const float *x, const float *y, float *out, int n, void *stream)
{
    if (!x || !y || !out || n <= 0) return fail(HBVX_E_NULL, "selftest_div: bad arguments");
    hipLaunchKernelGGL(k_selftest_div, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, y,
                       out, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "selftest_div launch");
    return HBVX_OK;
}

// ---------------------------------------------------------------------------
// baseflow index (hbv.py:562-567), fixed-order sums.  Per basin and series, 64 time slices sl with two chains each,
//   a over t = sl, sl + 128, ..   and   c over t = sl + 64, sl + 192, ..      (ascending, from 0)
// then a + c per slice, then the slices sl = 0..63 in sequence.  Block = PB basins x 64 slices (x the two chains
// where a thread owns one chain of both series), BFI_ROWS rows in flight before the first add; the blocks on the map
// of xcd_block.  Measured alone at config 2 (39 MB, 6 us at the copy rate): 16 basins x 64 slices with both chains
// on one thread, 42 blocks: 30 us, with or without eight rows in flight (not a latency chain); 8 basins on 84 blocks
// 30 us; the 16-basin form on the XCD map 28 us; 8 / 4 basins with a chain per thread on the XCD map 24 / 22 us; without
// the map 4 / 2 / 1 basins 44 / 58 / 66 us, 64-basin rows on 11 blocks 147 us.  What binds is the 128-byte lines a
// narrow piece of a 4-byte-aligned row shares with its neighbours, fetched by every L2 that holds one of them.
// k_bfi_tan_batch below keeps the 16 x 64 layout and its own order.
// ---------------------------------------------------------------------------
#define BFI_ROWS 8      // rows in flight per series and thread
// NH = 2: a chain per thread (narrow blocks for few basins); NH = 1: both chains of a slice on one thread
template <int PB, int NH>
__global__ void __launch_bounds__(PB * 64 * NH) k_bfi(int T, int B, const float *__restrict__ qs,
                                                      const float *__restrict__ q2, float nz,
                                                      float *__restrict__ bfi)
{
    constexpr int NC = 2 / NH, NR = BFI_ROWS / NC;      // chains per thread, rows of a chain in flight
    __shared__ float r0[2][64][PB], r2[2][64][PB];
    const int bl = threadIdx.x % PB, sl = (threadIdx.x / PB) & 63, half = threadIdx.x / (PB * 64);
    const int b = xcd_block() * PB + bl;        // (past B: the lanes idle, the barrier is still met)
    float a0[NC], a2[NC];
#pragma unroll
    for (int i = 0; i < NC; i++) a0[i] = a2[i] = 0.0f;
    if (b < B) {
        const int h0 = half * NC;               // this thread's chains are h0 .. h0 + NC - 1: rows t + 64 h
        int t = sl;
        for (; t + 64 * (h0 + NC - 1) + 128 * (NR - 1) < T; t += 128 * NR) {
            float v0[NC][NR], v2[NC][NR];
#pragma unroll
            for (int j = 0; j < NR; j++)
#pragma unroll
                for (int i = 0; i < NC; i++) {
                    v0[i][j] = qs[(int64_t)(t + 64 * (h0 + i) + 128 * j) * B + b];
                    v2[i][j] = q2[(int64_t)(t + 64 * (h0 + i) + 128 * j) * B + b];
                }
#pragma unroll
            for (int j = 0; j < NR; j++)
#pragma unroll
                for (int i = 0; i < NC; i++) {
                    a0[i] += v0[i][j];
                    a2[i] += v2[i][j];
                }
        }
#pragma unroll
        for (int i = 0; i < NC; i++)
            for (int tt = t + 64 * (h0 + i); tt < T; tt += 128) {
                a0[i] += qs[(int64_t)tt * B + b];
                a2[i] += q2[(int64_t)tt * B + b];
            }
    }
#pragma unroll
    for (int i = 0; i < NC; i++) {
        r0[half * NC + i][sl][bl] = a0[i];
        r2[half * NC + i][sl][bl] = a2[i];
    }
    __syncthreads();
    if (threadIdx.x < PB && b < B) {
        float s0 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int k = 0; k < 64; k++) {
            s0 += r0[0][k][bl] + r0[1][k][bl];
            s2 += r2[0][k][bl] + r2[1][k][bl];
        }
        bfi[b] = 100.0f * (s2 / (s0 + nz));
    }
}

// 16-basin blocks (64-byte pieces of a row, both chains on a thread) once they fill the chip on their own; below
// that 4-basin blocks with a chain per thread: four times the blocks (measured: the comment above; at 12 500 basins
// x 730 days the 4-basin form took 44 us against 34 us for 16-basin blocks).
#define BFI_WIDE_BLOCKS 256
extern "C" int hbvx_bfi(int32_t T, int32_t B, const float *qs, const float *q2, float nearzero,
                        float *bfi, void *stream)
{
    if (!qs || !q2 || !bfi || T <= 0 || B <= 0) return fail(HBVX_E_NULL, "hbvx_bfi: bad arguments");
    if ((B + 15) / 16 >= BFI_WIDE_BLOCKS)
        hipLaunchKernelGGL((k_bfi<16, 1>), dim3(xcd_grid((B + 15) / 16)), dim3(1024), 0, (hipStream_t)stream, T, B, qs, q2,
                           nearzero, bfi);
    else
        hipLaunchKernelGGL((k_bfi<4, 2>), dim3(xcd_grid((B + 3) / 4)), dim3(512), 0, (hipStream_t)stream, T, B, qs, q2,
                           nearzero, bfi);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_bfi launch");
    return HBVX_OK;
}

// Tangent of the baseflow index (quotient rule).  Block = 16 basins x 64 time slices; a slice's rows t = sl, sl + 64, ..
// are summed in ascending order, then the slices in sequence.
__device__ __forceinline__ void bfi_tan_body(int T, int B, const float *__restrict__ qs,
                                             const float *__restrict__ q2, const float *__restrict__ qsd,
                                             const float *__restrict__ q2d, float nz, float *__restrict__ bfid)
{
    __shared__ float r0[64][16], r2[64][16], d0[64][16], d2[64][16];
    const int bl = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int b = blockIdx.x * 16 + bl;
    float a0 = 0.0f, a2 = 0.0f, e0 = 0.0f, e2 = 0.0f;
    if (b < B) {
        for (int t = sl; t < T; t += 64) {
            a0 += qs[(int64_t)t * B + b];
            a2 += q2[(int64_t)t * B + b];
            e0 += qsd ? qsd[(int64_t)t * B + b] : 0.0f;
            e2 += q2d ? q2d[(int64_t)t * B + b] : 0.0f;
        }
    }
    r0[sl][bl] = a0;
    r2[sl][bl] = a2;
    d0[sl][bl] = e0;
    d2[sl][bl] = e2;
    __syncthreads();
    if (sl == 0 && b < B) {
        float s0 = 0.0f, s2 = 0.0f, t0 = 0.0f, t2 = 0.0f;
#pragma unroll
        for (int k = 0; k < 64; k++) {
            s0 += r0[k][bl];
            s2 += r2[k][bl];
            t0 += d0[k][bl];
            t2 += d2[k][bl];
        }
        const float den = s0 + nz;
        bfid[b] = 100.0f * ((t2 - s2 * (t0 / den)) / den);
    }
}

// blockIdx.y is the direction; hbvx_bfi_tangent is the launch with one.
__global__ void __launch_bounds__(1024) k_bfi_tan_batch(int T, int B, const float *__restrict__ qs,
                                                        const float *__restrict__ q2, const float *__restrict__ qsd,
                                                        const float *__restrict__ q2d, int64_t ds, float nz,
                                                        float *__restrict__ bfid)
{
    const int64_t dir = blockIdx.y;
    bfi_tan_body(T, B, qs, q2, qsd ? qsd + dir * ds : nullptr, q2d ? q2d + dir * ds : nullptr, nz, bfid + dir * B);
}

// ---------------------------------------------------------------------------
// tangent entry points.  hbvx_route_tangent and hbvx_bfi_tangent are the several-direction launches with n_dir = 1:
// their pointers go to the kernels as given (NULL: zero tangent), and the direction strides, which only ever multiply
// direction 0 there, are 0.  "A stride of 0 is a zero tangent" is a rule of the batch entry points alone, applied
// there before the shared launch.  The recurrence's entry points are in launch_tan.hip.
// ---------------------------------------------------------------------------
static int launch_bfi_tan(int T, int B, int n_dir, const float *qs, const float *q2, const float *qs_dot,
                          const float *q2_dot, int64_t dot_d_stride, float nearzero, float *bfi_dot, void *stream,
                          const char *what)
{
    hipLaunchKernelGGL(k_bfi_tan_batch, dim3((B + 15) / 16, n_dir), dim3(1024), 0, (hipStream_t)stream, T, B, qs, q2,
                       qs_dot, q2_dot, dot_d_stride, nearzero, bfi_dot);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return HBVX_OK;
}

extern "C" int hbvx_bfi_tangent(int32_t T, int32_t B, const float *qs, const float *q2, const float *qs_dot,
                                const float *q2_dot, float nearzero, float *bfi_dot, void *stream)
{
    if (!qs || !q2 || !bfi_dot || T <= 0 || B <= 0) return fail(HBVX_E_NULL, "hbvx_bfi_tangent: bad arguments");
    return launch_bfi_tan(T, B, 1, qs, q2, qs_dot, q2_dot, 0, nearzero, bfi_dot, stream, "hbvx_bfi_tangent launch");
}

extern "C" int hbvx_bfi_tangent_batch(int32_t T, int32_t B, int32_t n_dir, const float *qs, const float *q2,
                                      const float *qs_dot, const float *q2_dot, int64_t dot_d_stride, float nearzero,
                                      float *bfi_dot, void *stream)
{
    if (!qs || !q2 || !bfi_dot || T <= 0 || B <= 0) return fail(HBVX_E_NULL, "hbvx_bfi_tangent_batch: bad arguments");
    if (n_dir < 1 || n_dir > 65535) return fail(HBVX_E_SHAPE, "hbvx_bfi_tangent_batch: n_dir must be in 1..65535");
    if (!dot_d_stride) qs_dot = q2_dot = nullptr;
    return launch_bfi_tan(T, B, n_dir, qs, q2, qs_dot, q2_dot, dot_d_stride, nearzero, bfi_dot, stream,
                          "hbvx_bfi_tangent_batch launch");
}

static int launch_route_tan(const hbvx_route_desc *r, int n_dir, const float *q, const float *uh, const float *q_dot,
                            int64_t q_dot_d_stride, const float *ra_dot, const float *rb_dot, int64_t r_d_stride,
                            float *q_rout_dot, void *stream, const char *what)
{
    const int nchunk = (r->T + ROUTE_CHUNK - 1) / ROUTE_CHUNK;
    hipLaunchKernelGGL(k_route_tan_batch, dim3((r->B + 63) / 64, (nchunk + 3) / 4, n_dir * r->S), dim3(256), 0,
                       (hipStream_t)stream, *r, q, uh, q_dot, q_dot_d_stride, ra_dot, rb_dot, r_d_stride, q_rout_dot);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return HBVX_OK;
}

extern "C" int hbvx_route_tangent(const hbvx_route_desc *r, const float *q, const float *uh, const float *q_dot,
                                  const float *ra_dot, const float *rb_dot, float *q_rout_dot, void *stream)
{
    int rc = check_route(r);
    if (rc) return rc;
    if (!q || !uh || !q_rout_dot) return fail(HBVX_E_NULL, "route buffer is NULL");
    return launch_route_tan(r, 1, q, uh, q_dot, 0, ra_dot, rb_dot, 0, q_rout_dot, stream, "hbvx_route_tangent launch");
}

extern "C" int hbvx_route_tangent_batch(const hbvx_route_desc *r, int32_t n_dir, const float *q, const float *uh,
                                        const float *q_dot, int64_t q_dot_d_stride, const float *ra_dot,
                                        const float *rb_dot, int64_t r_d_stride, float *q_rout_dot, void *stream)
{
    int rc = check_route(r);
    if (rc) return rc;
    if (!q || !uh || !q_rout_dot) return fail(HBVX_E_NULL, "route buffer is NULL");
    if (n_dir < 1 || (int64_t)n_dir * r->S > 65535)
        return fail(HBVX_E_SHAPE, "hbvx_route_tangent_batch: n_dir must be >= 1 and n_dir * S <= 65535");
    if (!q_dot_d_stride) q_dot = nullptr;
    if (!r_d_stride) ra_dot = rb_dot = nullptr;
    return launch_route_tan(r, n_dir, q, uh, q_dot, q_dot_d_stride, ra_dot, rb_dot, r_d_stride, q_rout_dot, stream,
                            "hbvx_route_tangent_batch launch");
}

// ---------------------------------------------------------------------------
// gage routing (hbv_2_hourly.py:800-897)
// ---------------------------------------------------------------------------
static int check_gage(const hbvx_gage_desc *r)
{
    if (!r) return fail(HBVX_E_NULL, "gage desc is NULL");
    if (r->abi_version != HBVX_ABI_VERSION) return fail(HBVX_E_ABI, "abi_version mismatch");
    if (r->T <= 0 || r->U <= 0 || r->G <= 0 || r->NPAIR < 0) return fail(HBVX_E_SHAPE, "bad T/U/G/NPAIR");
    int L = r->T < HBVX_GAGE_MAXLEN ? r->T : HBVX_GAGE_MAXLEN;
    if (r->L != L) return fail(HBVX_E_SHAPE, "L must be min(T, 72)");
    if (r->U > 65535 || r->G > 65535) return fail(HBVX_E_SHAPE, "more than 65535 units or gages per call");
    if (!r->pair_unit || !r->gage_ptr || !r->pair_gage || !r->unit_ptr || !r->unit_pairs || !r->areas ||
        !r->denom || !r->dp)
        return fail(HBVX_E_NULL, "gage routing pointer is NULL");
    return HBVX_OK;
}

extern "C" uint64_t hbvx_gage_route_workspace_bytes(const hbvx_gage_desc *r)
{
    if (!r || r->T <= 0 || r->U <= 0 || r->G <= 0) return 0;
    // transposed runoff [U,T], transposed gradient [G,T], transposed input gradient [U,T],
    // per-pair series [NPAIR,T]
    return ((uint64_t)2 * r->U + r->G + r->NPAIR) * (uint64_t)r->T * sizeof(float);
}

static void launch_transpose(int R, int C, const float *in, float *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_transpose, dim3((C + 31) / 32, (R + 31) / 32), dim3(256), 0, st, R, C, in, out);
}

extern "C" int hbvx_gage_route_forward(const hbvx_gage_desc *r, const float *qs, float *uh, float *out,
                                       void *workspace, uint64_t workspace_bytes, void *stream)
{
    int rc = check_gage(r);
    if (rc) return rc;
    if (!qs || !uh || !out) return fail(HBVX_E_NULL, "gage routing buffer is NULL");
    if (!workspace || workspace_bytes < hbvx_gage_route_workspace_bytes(r))
        return fail(HBVX_E_NULL, "gage routing workspace missing or too small");
    hipStream_t st = (hipStream_t)stream;
    float *qsT = (float *)workspace;
    launch_transpose(r->T, r->U, qs, qsT, st);
    if (r->NPAIR > 0) hipLaunchKernelGGL(k_gage_uh, dim3(r->NPAIR), dim3(128), 0, st, *r, uh);
    float *lag = qsT + ((int64_t)2 * r->U + r->G) * r->T;
    if (r->NPAIR > 0)
        hipLaunchKernelGGL(k_gage_lag_fwd, dim3(r->NPAIR, (r->T + GAGE_TILE4 - 1) / GAGE_TILE4), dim3(GAGE_TILE), 0,
                           st, *r, qsT, uh, lag);
    hipLaunchKernelGGL(k_gage_sum_fwd, dim3((r->T + 255) / 256, r->G), dim3(256), 0, st, *r, lag, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_gage_route_forward launch");
    return HBVX_OK;
}

extern "C" int hbvx_gage_route_backward(const hbvx_gage_desc *r, const float *qs, const float *uh,
                                        const float *grad_out, float *grad_qs, float *grad_dp,
                                        void *workspace, uint64_t workspace_bytes, void *stream)
{
    int rc = check_gage(r);
    if (rc) return rc;
    if (!qs || !uh || !grad_out || !grad_qs || !grad_dp) return fail(HBVX_E_NULL, "gage routing buffer is NULL");
    if (!workspace || workspace_bytes < hbvx_gage_route_workspace_bytes(r))
        return fail(HBVX_E_NULL, "gage routing workspace missing or too small");
    hipStream_t st = (hipStream_t)stream;
    float *qsT = (float *)workspace;
    float *goT = qsT + (int64_t)r->U * r->T;
    float *gqsT = goT + (int64_t)r->G * r->T;
    launch_transpose(r->T, r->U, qs, qsT, st);
    launch_transpose(r->T, r->G, grad_out, goT, st);
    float *lag = gqsT + (int64_t)r->U * r->T;
    if (r->NPAIR > 0)
        hipLaunchKernelGGL(k_gage_lag_bwd, dim3(r->NPAIR, (r->T + GAGE_TILE4 - 1) / GAGE_TILE4), dim3(GAGE_TILE), 0,
                           st, *r, uh, goT, lag);
    hipLaunchKernelGGL(k_gage_sum_bwd, dim3((r->T + 255) / 256, r->U), dim3(256), 0, st, *r, lag, gqsT);
    launch_transpose(r->U, r->T, gqsT, grad_qs, st);
    if (r->NPAIR > 0)
        hipLaunchKernelGGL(k_gage_bwd_p, dim3(r->NPAIR), dim3(GAGE_TILE), 0, st, *r, qsT, goT, grad_dp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_gage_route_backward launch");
    return HBVX_OK;
}

// Tangent of the gage routing over n_dir directions.  Workspace: the transposed runoff [U,T] once, and per direction
// of a slab its transposed runoff tangent [U,T], its tap tangents [NPAIR,L] and its per-pair series [NPAIR,T].  The
// per-pair series dominate (104 MB per direction at 12 000 pairs x 2 160 hours), so the directions go through in
// slabs of at most GAGE_TAN_SLAB_BYTES of per-direction scratch; every direction's arithmetic is the same whatever the
// slab it falls in.
#define GAGE_TAN_SLAB_BYTES ((uint64_t)1 << 30)
static uint64_t gage_tan_dir_bytes(const hbvx_gage_desc *r)
{
    return ((uint64_t)r->U * r->T + (uint64_t)r->NPAIR * r->L + (uint64_t)r->NPAIR * r->T) * sizeof(float);
}
static int gage_tan_slab(const hbvx_gage_desc *r, int n_dir)
{
    uint64_t fit = GAGE_TAN_SLAB_BYTES / gage_tan_dir_bytes(r);
    if (fit < 1) fit = 1;
    if (fit > 65535) fit = 65535;           // the direction is a grid's z
    return (uint64_t)n_dir < fit ? n_dir : (int)fit;
}

extern "C" uint64_t hbvx_gage_route_tangent_workspace_bytes(const hbvx_gage_desc *r, int32_t n_dir)
{
    if (!r || r->T <= 0 || r->U <= 0 || r->G <= 0 || r->NPAIR < 0 || r->L <= 0 || n_dir < 1) return 0;
    return (uint64_t)r->U * r->T * sizeof(float) + (uint64_t)gage_tan_slab(r, n_dir) * gage_tan_dir_bytes(r);
}

extern "C" int hbvx_gage_route_tangent_batch(const hbvx_gage_desc *r, int32_t n_dir, const float *qs, const float *uh,
                                             const float *qs_dot, int64_t qs_dot_d_stride, const float *dp_dot,
                                             int64_t dp_dot_d_stride, float *out_dot, void *workspace,
                                             uint64_t workspace_bytes, void *stream)
{
    int rc = check_gage(r);
    if (rc) return rc;
    if (n_dir < 1 || n_dir > 65535) return fail(HBVX_E_SHAPE, "hbvx_gage_route_tangent_batch: n_dir must be in 1..65535");
    if (!qs || !uh || !out_dot) return fail(HBVX_E_NULL, "gage routing buffer is NULL");
    if (!workspace || workspace_bytes < hbvx_gage_route_tangent_workspace_bytes(r, n_dir))
        return fail(HBVX_E_NULL, "gage routing workspace missing or too small");
    // a stride of 0 is a zero tangent, like a NULL pointer
    if (!qs_dot_d_stride) qs_dot = nullptr;
    if (!dp_dot_d_stride) dp_dot = nullptr;
    hipStream_t st = (hipStream_t)stream;
    const int slab = gage_tan_slab(r, n_dir);
    const int64_t UT = (int64_t)r->U * r->T, PL = (int64_t)r->NPAIR * r->L;
    float *qsT = (float *)workspace;
    float *qdT = qsT + UT;
    float *uhd = qdT + slab * UT;
    float *lag = uhd + slab * PL;
    if (dp_dot) launch_transpose(r->T, r->U, qs, qsT, st);
    for (int d0 = 0; d0 < n_dir; d0 += slab) {
        const int nd = n_dir - d0 < slab ? n_dir - d0 : slab;
        if (qs_dot)
            for (int d = 0; d < nd; d++)
                launch_transpose(r->T, r->U, qs_dot + (int64_t)(d0 + d) * qs_dot_d_stride, qdT + d * UT, st);
        if (r->NPAIR > 0) {
            if (dp_dot)
                hipLaunchKernelGGL(k_gage_uh_tan, dim3(r->NPAIR), dim3(128), 0, st, *r, nd,
                                   dp_dot + (int64_t)d0 * dp_dot_d_stride, dp_dot_d_stride, uhd);
            hipLaunchKernelGGL(k_gage_lag_tan, dim3(r->NPAIR, (r->T + GAGE_TILE4 - 1) / GAGE_TILE4, nd), dim3(GAGE_TILE),
                               0, st, *r, qsT, uh, qs_dot ? qdT : nullptr, dp_dot ? uhd : nullptr, lag);
        }
        hipLaunchKernelGGL(k_gage_sum_tan, dim3((r->T + 255) / 256, r->G, nd), dim3(256), 0, st, *r, lag,
                           out_dot + (int64_t)d0 * r->T * r->G);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_gage_route_tangent_batch launch");
    return HBVX_OK;
}

// ---------------------------------------------------------------------------
// zero fill of the dense gradient buffers (the autograd contract wants grad tensors shaped like the raw
// parameter tensor [T,B,ny], of which static parameters touch one row): streaming 16-byte non-temporal
// stores, grid-stride, no read-for-ownership
// ---------------------------------------------------------------------------
typedef float zero_f4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) k_zero_nt(zero_f4 *__restrict__ p, uint64_t n16)
{
    const zero_f4 z = {0.f, 0.f, 0.f, 0.f};
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * 256)
        __builtin_nontemporal_store(z, &p[i]);
}

// Small and ragged pieces go through a kernel too, never hipMemsetAsync: captured into a HIP graph (graph=True), the
// memset node of a 1 944-byte static-parameter gradient replayed as a no-op on this stack -- the adjoint then added
// its sums to stale memory (round 5: tests/test_graphed.py, Hbv_2's [B, ws] gradient).  A kernel node replays.
__global__ void __launch_bounds__(256) k_zero_bytes(unsigned char *__restrict__ p, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}
static hipError_t zero_bytes(void *ptr, uint64_t n, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_zero_bytes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (unsigned char *)ptr, n);
    return hipGetLastError();
}

extern "C" int hbvx_zero(void *ptr, uint64_t bytes, void *stream)
{
    if (!ptr && bytes) return fail(HBVX_E_NULL, "hbvx_zero: buffer is NULL");
    hipStream_t st = (hipStream_t)stream;
    const uint64_t head = ((uintptr_t)ptr & 15) ? 16 - ((uintptr_t)ptr & 15) : 0;
    if (bytes < 4096 || head >= bytes) {
        hipError_t e = zero_bytes(ptr, bytes, st);
        return e == hipSuccess ? 0 : hip_fail(e, "hbvx_zero");
    }
    hipError_t e = hipSuccess;
    if (head) e = zero_bytes(ptr, head, st);
    const uint64_t n16 = (bytes - head) / 16, tail = (bytes - head) - n16 * 16;
    // one 16-byte store per thread: on MI355X 6.6 TB/s against 5.3 for a grid-stride loop on a few thousand
    // workgroups (3.8 GB: 0.58 ms against 0.72 ms for torch's fill)
    const uint64_t want = n16 / 256 + 1;
    const int blocks = (int)(want < 0x7fffffffull ? want : 0x7fffffffull);
    hipLaunchKernelGGL(k_zero_nt, dim3(blocks), dim3(256), 0, st, (zero_f4 *)((char *)ptr + head), n16);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess && tail) e = zero_bytes((char *)ptr + head + n16 * 16, tail, st);
    return e == hipSuccess ? 0 : hip_fail(e, "hbvx_zero");
}

// hbvx_zero_rest (include/hbvx.h): what the forward's fill workgroups left of hbvx_fwd_out.zero_ptr.  The first missing piece
// is a device-side number (zero_state[0]), so the grid covers the whole buffer and the threads in front of it leave: eight
// 16-byte stores per thread, a wave instruction = 1 KB contiguous.
__global__ void __launch_bounds__(256) k_zero_rest(zero_f4 *__restrict__ p, uint64_t n16, const unsigned *__restrict__ state)
{
    const uint64_t npiece = (n16 + HBVX_ZERO_PIECE / 16 - 1) / (HBVX_ZERO_PIECE / 16);
    const uint64_t claimed = state[0];
    const uint64_t start = (claimed < npiece ? claimed : npiece) * (HBVX_ZERO_PIECE / 16);
    const uint64_t i0 = (uint64_t)blockIdx.x * 2048 + threadIdx.x;
    if (i0 + 2048 <= start) return;
    const zero_f4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t i = i0 + (uint64_t)k * 256;
        if (i >= start && i < n16) __builtin_nontemporal_store(z, &p[i]);
    }
}

extern "C" int hbvx_zero_rest(void *ptr, uint64_t bytes, const void *zero_state, void *stream)
{
    if (!bytes) return HBVX_OK;
    if (!ptr || !zero_state) return fail(HBVX_E_NULL, "hbvx_zero_rest: buffer or state is NULL");
    if ((uintptr_t)ptr & 15) return fail(HBVX_E_SHAPE, "hbvx_zero_rest: buffer must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const uint64_t n16 = bytes / 16, tail = bytes - n16 * 16;
    hipError_t e = hipSuccess;
    if (n16) {
        const uint64_t blocks = (n16 + 2047) / 2048;
        if (blocks > 0x7fffffffull) return fail(HBVX_E_SHAPE, "hbvx_zero_rest: buffer too large");
        hipLaunchKernelGGL(k_zero_rest, dim3((unsigned)blocks), dim3(256), 0, st, (zero_f4 *)ptr, n16, (const unsigned *)zero_state);
        e = hipGetLastError();
    }
    if (e == hipSuccess && tail) e = zero_bytes((char *)ptr + n16 * 16, tail, st);
    return e == hipSuccess ? HBVX_OK : hip_fail(e, "hbvx_zero_rest");
}

// Zero fill that leaves out what the adjoint overwrites (include/hbvx.h: hbvx_zero_except).
// Rows outside [r0, r1) are contiguous memory: plain hbvx_zero.  Inside, only the gaps between
// the kept column groups are written: 16 lanes per row walk the (few, short) gap ranges.  When less
// than half of a row is kept the dense fill is cheaper than the gap walk and is used instead (the
// adjoint's stores then land on zeros).
struct ZeroGaps {
    int n;
    int start[34], len[34];
};

__global__ void __launch_bounds__(256) k_zero_gaps(float *__restrict__ p, int64_t r0, int64_t r1, int width,
                                                    const ZeroGaps G)
{
    const int64_t row = r0 + (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (row >= r1) return;
    float *q = p + row * width;
    const int lane = threadIdx.x & 15;
    for (int g = 0; g < G.n; g++)
        for (int c = lane; c < G.len[g]; c += 16) q[G.start[g] + c] = 0.0f;
}

extern "C" int hbvx_zero_except(float *ptr, int64_t rows, int32_t width, int64_t r0, int64_t r1, int32_t group_w,
                                uint32_t keep_groups, void *stream)
{
    if (rows < 0 || width <= 0 || group_w <= 0) return fail(HBVX_E_SHAPE, "hbvx_zero_except: bad shape");
    if (!ptr && rows) return fail(HBVX_E_NULL, "hbvx_zero_except: buffer is NULL");
    if (rows == 0) return 0;
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > rows ? rows : r1;
    // gap ranges = complement of the kept groups inside [0, width)
    ZeroGaps G;
    G.n = 0;
    int kept_cols = 0, c = 0;
    while (c < width) {
        const int g = c / group_w;
        const bool kept = g < 32 && ((keep_groups >> g) & 1u);
        int e = (g + 1) * group_w;
        e = e > width ? width : e;
        if (kept) kept_cols += e - c;
        else if (G.n > 0 && G.start[G.n - 1] + G.len[G.n - 1] == c) G.len[G.n - 1] += e - c;
        else if (G.n < 34) { G.start[G.n] = c; G.len[G.n] = e - c; G.n++; }
        c = e;
    }
    if (r1 <= r0 || 2 * kept_cols < width)
        return hbvx_zero(ptr, (uint64_t)rows * (uint64_t)width * sizeof(float), stream);
    int rc = 0;
    if (r0 > 0) rc = hbvx_zero(ptr, (uint64_t)r0 * (uint64_t)width * sizeof(float), stream);
    if (!rc && r1 < rows)
        rc = hbvx_zero(ptr + r1 * width, (uint64_t)(rows - r1) * (uint64_t)width * sizeof(float), stream);
    if (rc || G.n == 0) return rc;
    const int64_t nblk = (r1 - r0 + 15) / 16;
    if (nblk > 0x7fffffff) return hbvx_zero(ptr, (uint64_t)rows * (uint64_t)width * sizeof(float), stream);
    hipLaunchKernelGGL(k_zero_gaps, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, ptr, r0, r1, (int)width, G);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, "hbvx_zero_except");
}

