// hbv_pop.h -- population evaluation (hbvx_population_cost, include/hbvx.h): the weighted squared error of the routed
// ensemble-mean streamflow of P candidate static-parameter sets per basin, one number per (candidate, basin), from one
// launch that writes nothing else -- and (hbvx_population_stats) the same launch with three more chains per (candidate,
// basin), on the raw, the square-root or the log flow, from which NSE, KGE, correlation, variability and bias follow on
// the host: four [P,B] numbers instead of one, still no series -- and (hbvx_population_joint) that launch with the same
// four chains on a second series beside streamflow, the day's ensemble mean of one un-routed flux (AET, SWE, Q0, Q1, Q2):
// eight [P,B] numbers.
//
// What happens to a basin's ensemble mean after the day step -- the normalised gamma unit hydrograph, the 15-day
// window, the causal convolution and the residual chain -- is hbvx_popk::Basin below and compiles for the host as
// well (tests/hosttest/pop_host.cpp), so the CPU tier checks it without a GPU; the kernel maps lanes onto it.
// hbvx_popk::BasinStats is Basin plus the transform and the three moment chains (tests/hosttest/popstats_host.cpp).
// hbvx_popk::AuxStats is the aux term's four chains (tests/hosttest/popjoint_host.cpp).
// k_pop maps lanes onto the one struct, k_pop_stats<TR> onto the other, k_pop_joint<TR> onto a BasinStats and an AuxStats.
// hbvx_popk::PeriodMean is the mean over a period that hbvx_population_period (hbv_pop_period.h) puts between each of the
// two values and its chains (tests/hosttest/popperiod_host.cpp).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HBVX_POP_HD __host__ __device__ __forceinline__
#else
#define HBVX_POP_HD inline
#endif

namespace hbvx_popk {

constexpr int UH = 15;      // HBVX_UH_MAXLEN

// The normalised gamma unit hydrograph (uh_routing.py:5-22) of physical route_a = a, route_b = bb: taps 0..L-1 as
// k_uh_gamma stores them and k_route_fwd loads them back, zero from L on.  A restatement of k_uh_gamma's lines
// (hbvx.hip), operation for operation -- the sum runs over all 15 values, zeros included.  k_uh_gamma keeps its own
// text: calling this from it changed that kernel's instruction schedule (tools/compare_code.py), and the forward's
// kernels are pinned.  A change to either belongs in both.
HBVX_POP_HD void gamma_taps(float a, float bb, int L, float (&w)[UH])
{
    float aa = fmaxf(a, 0.0f) + 0.1f;
    float theta = fmaxf(bb, 0.0f) + 0.5f;
    float denom = expf(lgammaf(aa)) * powf(theta, aa);
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < UH; k++) {
        float t = (float)k + 0.5f;
        float mid = powf(t, aa - 1.0f);
        float right = expf(-t / theta);
        w[k] = (k < L) ? 1.0f / denom * mid * right : 0.0f;
        sum += w[k];
    }
#pragma unroll
    for (int k = 0; k < UH; k++) w[k] = (k < L) ? w[k] / sum : 0.0f;
}

// One (candidate, basin).  push() takes the days in ascending order:
//   routed:  win[0] = q;  y = chain over ascending k = 0..14:  acc += uh[k] * win[k]  from 0 (the product rounded, then
//            the sum: k_route_fwd's line under -ffp-contract=off), zero history before the first day; else y = q;
//   counted: r = y - target;  cost = fmaf(w * r, r, cost)  (w * r rounded once).  Without weights the caller passes
//            w = 1, which gives fmaf(r, r, cost) bit for bit (1 * r is exact).
// A day that is not counted moves the window and leaves the cost alone.
struct Basin {
    float uh[UH], win[UH];
    float cost;
    bool routed;

    HBVX_POP_HD void start(bool with_routing)
    {
#pragma unroll
        for (int k = 0; k < UH; k++) uh[k] = win[k] = 0.0f;
        cost = 0.0f;
        routed = with_routing;
    }

    HBVX_POP_HD float push(float q, float target, float w, bool counted)
    {
        float y = q;
        if (routed) {
            win[0] = q;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < UH; k++) acc += uh[k] * win[k];
#pragma unroll
            for (int k = UH - 1; k > 0; k--) win[k] = win[k - 1];
            y = acc;
        }
        if (counted) {
            const float r = y - target;
            cost = __builtin_fmaf(w * r, r, cost);
        }
        return y;
    }
};

constexpr int T_NONE = 0, T_SQRT = 1, T_LOG = 2;      // HBVX_POP_T_*

// Basin with the sums a score other than the squared error needs.  The window and the routed value y are Basin's own
// lines (its push with counted = false), so y is the same in every transform; a counted day then takes
//   y' = y | sqrtf(y) | logf(y + eps)          r = y' - o'      d = y' - m      e = o' - m
//   cost = fmaf(w * r, r, cost)                (Basin's line: under T_NONE the same operations on the same values)
//   s1 = fmaf(w, d, s1)    s2 = fmaf(w * d, d, s2)    s3 = fmaf(w * d, e, s3)      (w * r, w * d rounded once)
// with o' the target ALREADY transformed and m the caller's shift, the weighted mean of o': the moments are taken about
// m because raw float32 sums of y'^2 and y' o' over twenty years cancel to nothing when the flow varies little about a
// large mean (the population kernel).  eps is read under T_LOG only.
struct BasinStats : Basin {
    float m, eps;
    float s1, s2, s3;

    HBVX_POP_HD void start(bool with_routing, float shift, float log_eps)
    {
        Basin::start(with_routing);
        m = shift;
        eps = log_eps;
        s1 = s2 = s3 = 0.0f;
    }

    template <int TR>
    HBVX_POP_HD float transform(float y) const
    {
        return TR == T_SQRT ? sqrtf(y) : TR == T_LOG ? logf(y + eps) : y;
    }

    template <int TR>
    HBVX_POP_HD float push(float q, float target, float w, bool counted)
    {
        const float y = Basin::push(q, 0.0f, 0.0f, false);
        if (counted) {
            const float yt = transform<TR>(y);
            const float r = yt - target;
            cost = __builtin_fmaf(w * r, r, cost);
            const float dd = yt - m, e = target - m;
            s1 = __builtin_fmaf(w, dd, s1);
            s2 = __builtin_fmaf(w * dd, dd, s2);
            s3 = __builtin_fmaf(w * dd, e, s3);
        }
        return y;
    }

    // The lines of a counted day of push() on a value that is already there -- hbvx_population_period's period mean of
    // y: v' = transform(v), then r, d, e and the four chains against `target` (already transformed) and w.  A
    // restatement: push() keeps its text (k_pop_stats and k_pop_joint are pinned).  A change belongs in both.
    template <int TR>
    HBVX_POP_HD void score(float v, float target, float w)
    {
        const float yt = transform<TR>(v);
        const float r = yt - target;
        cost = __builtin_fmaf(w * r, r, cost);
        const float dd = yt - m, e = target - m;
        s1 = __builtin_fmaf(w, dd, s1);
        s2 = __builtin_fmaf(w * dd, dd, s2);
        s3 = __builtin_fmaf(w * dd, e, s3);
    }
};

// The mean of a series over one period of hbvx_population_period: add() takes the period's days in ascending order, the
// first one ASSIGNS (so a one-day period is y / 1.0f = y bit for bit, negative zero included, and nothing of the period
// before is left), close(n) is the one division by the period's day count:
//   acc = y (first day) | acc + y (later days)        mean = acc / (float)n
struct PeriodMean {
    float acc;

    HBVX_POP_HD void add(float y, bool first) { acc = first ? y : acc + y; }

    HBVX_POP_HD float close(int n) const { return acc / (float)n; }
};

// The aux term of hbvx_population_joint: the four chains of BasinStats on a value that is neither routed nor
// transformed.  push() takes the COUNTED days in ascending order:
//   r = v - o      d = v - m      e = o - m
//   sse = fmaf(w * r, r, sse)    s1 = fmaf(w, d, s1)    s2 = fmaf(w * d, d, s2)    s3 = fmaf(w * d, e, s3)
// with o the aux target, m the caller's shift (the weighted mean of o) and w * r, w * d each rounded once: BasinStats'
// lines under T_NONE on another value, so a test that feeds both the same numbers gets the same bits.
struct AuxStats {
    float m;
    float sse, s1, s2, s3;

    HBVX_POP_HD void start(float shift)
    {
        m = shift;
        sse = s1 = s2 = s3 = 0.0f;
    }

    HBVX_POP_HD void push(float v, float target, float w)
    {
        const float r = v - target;
        sse = __builtin_fmaf(w * r, r, sse);
        const float dd = v - m, e = target - m;
        s1 = __builtin_fmaf(w, dd, s1);
        s2 = __builtin_fmaf(w * dd, dd, s2);
        s3 = __builtin_fmaf(w * dd, e, s3);
    }
};

} // namespace hbvx_popk

#if defined(__HIPCC__)

#include "hbv_lane.h"

namespace hbvx {

struct PopArgs {
    hbvx_desc d;
    hbvx_pop pop;
    hbvx_route_desc r;      // *pop.route (the pointer is the host's); read only with has_route
    int has_route;
    int lgMp;
};

struct PopStatsArgs {
    PopArgs a;
    const float *shift, *eps;   // hbvx_pop_stats': [B] each
    float *s1, *s2, *s3;        // [P,B] each
};

struct PopJointArgs {
    PopStatsArgs s;             // the flow term: hbvx_population_stats' arguments
    int aux_series;             // HBVX_F_Q0 .. HBVX_F_SWE
    const float *aux_target, *aux_w, *aux_shift;    // hbvx_pop_joint's: [T - t_first, B], the same or NULL, [B]
    float *aux_sse, *aux_s1, *aux_s2, *aux_s3;      // [P,B] each
    float *aux_sim;             // [P, T - t_first, B] or NULL
};

// ---------------------------------------------------------------------------
// k_pop<MODEL, BETAET>: k_fwd's day loop (the same Step::fwd instance, the same one-day-ahead register prefetch of the
// forcings and the dynamic rows, the same ensemble sum and weights) with the lane mapping of k_tan's several-direction
// form: one wave per workgroup, blockIdx.x the wave's group of basins, blockIdx.y the CANDIDATE, one lane per (basin,
// member).  A candidate is a wave of its own that reads the forcings itself -- they come out of the L2 / Infinity
// Cache after the first candidate's pass -- and nothing is shared between candidates inside the kernel: what many
// candidates in one launch gain over a forward each is that their waves fill the SIMDs one forward leaves idle, and
// that nothing but [P,B] costs is written.  The candidate index is uniform over the wave, so a candidate's base
// address is scalar.  Several candidates per lane are not tried: k_tan measured that form and lost at every size
// (hbv_tan.h), for a reason that holds here too (the loop is bound by instruction issue, registers cost resident waves).
//
// After ens_sum every lane of a basin holds the mean, so every lane carries the basin's window and cost chain (the
// same values: no shuffle, no divergence) and the leader stores.  The bits of cost[c,b] and sim[c,:,b] depend on
// candidate c's values alone: c enters addresses only.
// ---------------------------------------------------------------------------
template <int MODEL, bool BETAET>
__global__ void __launch_bounds__(64) k_pop(const PopArgs A)
{
    constexpr int NP = NParam<MODEL, BETAET>::value;
    const hbvx_desc &d = A.d;
    const hbvx_pop &pp = A.pop;
    const int lgMp = A.lgMp;
    const LaneId L = lane_id(d, lgMp);
    const int T = d.T;
    const int t_first = pp.t_first;
    const int64_t N = (int64_t)d.B * d.M;
    const int64_t c = blockIdx.y;
    const bool raw = d.raw_sigmoid != 0;
    const float nz = d.nearzero;
    const float ac = (MODEL == MODEL_HBV20) ? d.ac[L.b] : 0.0f;
    const float elev = (MODEL == MODEL_HBV20) ? d.elev[L.b] : 0.0f;

    float p[NPARAM_MAX];
    const float *dynp[NP];
    bool use_dyn[NP];
    unsigned dmask = 0;
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const hbvx_param_src &s = d.p[i];
        const hbvx_pop_src &cs = pp.p[i];
        float v = cs.sta ? cs.sta[c * cs.c_stride + (int64_t)L.b * cs.b_stride + L.j]
                         : s.sta[(int64_t)L.b * s.sta_b_stride + L.j];
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

    hbvx_popk::Basin bs;
    bs.start(A.has_route != 0);
    if (A.has_route) {      // route_ab's lines (hbvx.hip) on the candidate's routing inputs
        const hbvx_route_desc &r = A.r;
        const float va = pp.ra ? pp.ra[c * pp.r_c_stride + (int64_t)L.b * pp.r_b_stride] : r.ra[(int64_t)L.b * r.r_stride];
        const float vb = pp.rb ? pp.rb[c * pp.r_c_stride + (int64_t)L.b * pp.r_b_stride] : r.rb[(int64_t)L.b * r.r_stride];
        const float ua = r.raw_sigmoid ? sigmoid_(va) : va;
        const float ub = r.raw_sigmoid ? sigmoid_(vb) : vb;
        hbvx_popk::gamma_taps(descale_(ua, r.a_lo, r.a_hi), descale_(ub, r.b_lo, r.b_hi), r.L, bs.uh);
    }

    const float *xb = d.x + (int64_t)L.b * d.x_b_stride;
    const float *mu = d.muwts ? d.muwts + (int64_t)L.b * d.mu_b_stride + L.j : nullptr;
    const float invM = 1.0f / (float)d.M;
    const float act = L.active ? 1.0f : 0.0f;
    const float *tg = pp.target + L.b;              // row t - t_first of [T - t_first, B]
    const float *wt = pp.w ? pp.w + L.b : nullptr;
    float *sim = pp.sim ? pp.sim + c * (int64_t)(T - t_first) * d.B + L.b : nullptr;

    // one-step-ahead register prefetch of the per-step inputs (k_fwd's), the observation and its weight with them
    float nxf[3], nxd[NP], nxo = 0.0f, nxw = 1.0f;
    {
        const float *xr = xb;
        nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
#pragma unroll
        for (int i = 0; i < NP; i++) nxd[i] = ((dmask >> i) & 1) ? dynp[i][0] : 0.f;
        if (t_first == 0) {
            nxo = tg[0];
            if (wt) nxw = wt[0];
        }
    }

    for (int t = 0; t < T; t++) {
        Step<MODEL, BETAET> s;
        s.P = nxf[0]; s.Tf = nxf[1]; s.PET = nxf[2];
        float cur[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) cur[i] = nxd[i];
        const float obs = nxo, wobs = nxw;
        {
            const int tn = t + 1 < T ? t + 1 : t;
            const float *xr = xb + (int64_t)tn * d.x_t_stride;
            nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
#pragma unroll
            for (int i = 0; i < NP; i++)
                if ((dmask >> i) & 1) nxd[i] = dynp[i][(int64_t)tn * d.p[i].dyn_t_stride];
            if (tn >= t_first) {
                const int64_t row = (int64_t)(tn - t_first) * d.B;
                nxo = tg[row];
                if (wt) nxw = wt[row];
            }
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
        st[0] = s.SP3; st[1] = s.MW3; st[2] = s.SM4; st[3] = s.SUZ4; st[4] = s.SLZ2;

        // the ensemble mean of Q as k_fwd forms series HBVX_F_QSIM
        const float wq = mu ? mu[(int64_t)t * d.mu_t_stride] : 1.0f;
        float q = ens_sum((mu ? s.Q * wq : s.Q) * act, lgMp);
        if (!mu) q = q * invM;
        const bool counted = t >= t_first;
        const float y = bs.push(q, obs, wobs, counted);
        if (counted && sim && L.leader) sim[(int64_t)(t - t_first) * d.B] = y;
    }
    if (L.leader) pp.cost[c * d.B + L.b] = bs.cost;
}

// ---------------------------------------------------------------------------
// k_pop_stats<MODEL, BETAET, TR>: k_pop on a BasinStats -- the same lanes, the same day loop, the same y; the shift
// and eps of the lane's basin are two more registers, the three chains three more, and the leader stores four numbers.
// TR is a template parameter: a wave-uniform switch inside the day loop would keep the log's registers live in every
// transform.
//
// A restatement of k_pop's lines, not a shared body: one body for both (an inlined function template on the struct,
// with overloads or `if constexpr` at the three places that differ) was built, and every form of it changed k_pop's
// registers (138 -> 140 for HBV 1.0) and schedule (tools/compare_code.py), which are pinned; so k_pop keeps its text, as
// k_uh_gamma does above.  A change to either belongs in both: tests/test_population_stats_gpu.py holds the two to the
// same bits of the squared error and of the series.
// ---------------------------------------------------------------------------
template <int MODEL, bool BETAET, int TR>
__global__ void __launch_bounds__(64) k_pop_stats(const PopStatsArgs S)
{
    constexpr int NP = NParam<MODEL, BETAET>::value;
    const PopArgs &A = S.a;
    const hbvx_desc &d = A.d;
    const hbvx_pop &pp = A.pop;
    const int lgMp = A.lgMp;
    const LaneId L = lane_id(d, lgMp);
    const int T = d.T;
    const int t_first = pp.t_first;
    const int64_t N = (int64_t)d.B * d.M;
    const int64_t c = blockIdx.y;
    const bool raw = d.raw_sigmoid != 0;
    const float nz = d.nearzero;
    const float ac = (MODEL == MODEL_HBV20) ? d.ac[L.b] : 0.0f;
    const float elev = (MODEL == MODEL_HBV20) ? d.elev[L.b] : 0.0f;

    float p[NPARAM_MAX];
    const float *dynp[NP];
    bool use_dyn[NP];
    unsigned dmask = 0;
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const hbvx_param_src &s = d.p[i];
        const hbvx_pop_src &cs = pp.p[i];
        float v = cs.sta ? cs.sta[c * cs.c_stride + (int64_t)L.b * cs.b_stride + L.j]
                         : s.sta[(int64_t)L.b * s.sta_b_stride + L.j];
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

    hbvx_popk::BasinStats bs;
    bs.start(A.has_route != 0, S.shift[L.b], TR == hbvx_popk::T_LOG ? S.eps[L.b] : 0.0f);
    if (A.has_route) {      // route_ab's lines (hbvx.hip) on the candidate's routing inputs
        const hbvx_route_desc &r = A.r;
        const float va = pp.ra ? pp.ra[c * pp.r_c_stride + (int64_t)L.b * pp.r_b_stride] : r.ra[(int64_t)L.b * r.r_stride];
        const float vb = pp.rb ? pp.rb[c * pp.r_c_stride + (int64_t)L.b * pp.r_b_stride] : r.rb[(int64_t)L.b * r.r_stride];
        const float ua = r.raw_sigmoid ? sigmoid_(va) : va;
        const float ub = r.raw_sigmoid ? sigmoid_(vb) : vb;
        hbvx_popk::gamma_taps(descale_(ua, r.a_lo, r.a_hi), descale_(ub, r.b_lo, r.b_hi), r.L, bs.uh);
    }

    const float *xb = d.x + (int64_t)L.b * d.x_b_stride;
    const float *mu = d.muwts ? d.muwts + (int64_t)L.b * d.mu_b_stride + L.j : nullptr;
    const float invM = 1.0f / (float)d.M;
    const float act = L.active ? 1.0f : 0.0f;
    const float *tg = pp.target + L.b;              // row t - t_first of [T - t_first, B]: the TRANSFORMED target
    const float *wt = pp.w ? pp.w + L.b : nullptr;
    float *sim = pp.sim ? pp.sim + c * (int64_t)(T - t_first) * d.B + L.b : nullptr;

    // one-step-ahead register prefetch of the per-step inputs (k_fwd's), the observation and its weight with them
    float nxf[3], nxd[NP], nxo = 0.0f, nxw = 1.0f;
    {
        const float *xr = xb;
        nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
#pragma unroll
        for (int i = 0; i < NP; i++) nxd[i] = ((dmask >> i) & 1) ? dynp[i][0] : 0.f;
        if (t_first == 0) {
            nxo = tg[0];
            if (wt) nxw = wt[0];
        }
    }

    for (int t = 0; t < T; t++) {
        Step<MODEL, BETAET> s;
        s.P = nxf[0]; s.Tf = nxf[1]; s.PET = nxf[2];
        float cur[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) cur[i] = nxd[i];
        const float obs = nxo, wobs = nxw;
        {
            const int tn = t + 1 < T ? t + 1 : t;
            const float *xr = xb + (int64_t)tn * d.x_t_stride;
            nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
#pragma unroll
            for (int i = 0; i < NP; i++)
                if ((dmask >> i) & 1) nxd[i] = dynp[i][(int64_t)tn * d.p[i].dyn_t_stride];
            if (tn >= t_first) {
                const int64_t row = (int64_t)(tn - t_first) * d.B;
                nxo = tg[row];
                if (wt) nxw = wt[row];
            }
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
        st[0] = s.SP3; st[1] = s.MW3; st[2] = s.SM4; st[3] = s.SUZ4; st[4] = s.SLZ2;

        // the ensemble mean of Q as k_fwd forms series HBVX_F_QSIM
        const float wq = mu ? mu[(int64_t)t * d.mu_t_stride] : 1.0f;
        float q = ens_sum((mu ? s.Q * wq : s.Q) * act, lgMp);
        if (!mu) q = q * invM;
        const bool counted = t >= t_first;
        const float y = bs.template push<TR>(q, obs, wobs, counted);
        if (counted && sim && L.leader) sim[(int64_t)(t - t_first) * d.B] = y;      // y, not y'
    }
    if (L.leader) {
        const int64_t at = c * d.B + L.b;
        pp.cost[at] = bs.cost;
        S.s1[at] = bs.s1;
        S.s2[at] = bs.s2;
        S.s3[at] = bs.s3;
    }
}

// ---------------------------------------------------------------------------
// k_pop_joint<MODEL, BETAET, TR>: k_pop_stats with an AuxStats beside the BasinStats -- the same lanes, grid, candidate
// axis and day loop, the same y and the same four flow chains (tests/test_population_joint_gpu.py holds them to
// k_pop_stats' bits); per day one more ensemble sum, of the flux the aux term scores -- in the same butterfly loop as the
// flow's --, and four more chains on it.  The aux target and weight join the one-day-ahead prefetch.
//
// Again a restatement, for the reason given above k_pop_stats: k_pop and k_pop_stats keep their text, registers and
// schedule.  A change to the day loop belongs in all three.
//
// Which flux is taken is a run-time select on J.aux_series, uniform over the launch, not a template parameter: the five
// values are all live at the end of Step::fwd anyway (Q is their sum, SP3 is the next state, ET has just closed the soil
// balance), so the select keeps little alive that a fixed choice would free -- built both ways, a fixed AET or SWE came
// out one VGPR below the select (three in one HBV 1.1p instance; DESIGN.md has the table), never across an occupancy
// step of the final kernel, at five times the instantiations.
// ---------------------------------------------------------------------------
template <int MODEL, bool BETAET, int TR>
__global__ void __launch_bounds__(64) k_pop_joint(const PopJointArgs J)
{
    constexpr int NP = NParam<MODEL, BETAET>::value;
    const PopStatsArgs &S = J.s;
    const PopArgs &A = S.a;
    const hbvx_desc &d = A.d;
    const hbvx_pop &pp = A.pop;
    const int lgMp = A.lgMp;
    const LaneId L = lane_id(d, lgMp);
    const int T = d.T;
    const int t_first = pp.t_first;
    const int64_t N = (int64_t)d.B * d.M;
    const int64_t c = blockIdx.y;
    const bool raw = d.raw_sigmoid != 0;
    const float nz = d.nearzero;
    const float ac = (MODEL == MODEL_HBV20) ? d.ac[L.b] : 0.0f;
    const float elev = (MODEL == MODEL_HBV20) ? d.elev[L.b] : 0.0f;

    float p[NPARAM_MAX];
    const float *dynp[NP];
    bool use_dyn[NP];
    unsigned dmask = 0;
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const hbvx_param_src &s = d.p[i];
        const hbvx_pop_src &cs = pp.p[i];
        float v = cs.sta ? cs.sta[c * cs.c_stride + (int64_t)L.b * cs.b_stride + L.j]
                         : s.sta[(int64_t)L.b * s.sta_b_stride + L.j];
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

    hbvx_popk::BasinStats bs;
    bs.start(A.has_route != 0, S.shift[L.b], TR == hbvx_popk::T_LOG ? S.eps[L.b] : 0.0f);
    if (A.has_route) {      // route_ab's lines (hbvx.hip) on the candidate's routing inputs
        const hbvx_route_desc &r = A.r;
        const float va = pp.ra ? pp.ra[c * pp.r_c_stride + (int64_t)L.b * pp.r_b_stride] : r.ra[(int64_t)L.b * r.r_stride];
        const float vb = pp.rb ? pp.rb[c * pp.r_c_stride + (int64_t)L.b * pp.r_b_stride] : r.rb[(int64_t)L.b * r.r_stride];
        const float ua = r.raw_sigmoid ? sigmoid_(va) : va;
        const float ub = r.raw_sigmoid ? sigmoid_(vb) : vb;
        hbvx_popk::gamma_taps(descale_(ua, r.a_lo, r.a_hi), descale_(ub, r.b_lo, r.b_hi), r.L, bs.uh);
    }

    hbvx_popk::AuxStats ax;
    ax.start(J.aux_shift[L.b]);
    const int aux_series = J.aux_series;        // uniform over the launch

    const float *xb = d.x + (int64_t)L.b * d.x_b_stride;
    const float *mu = d.muwts ? d.muwts + (int64_t)L.b * d.mu_b_stride + L.j : nullptr;
    const float invM = 1.0f / (float)d.M;
    const float act = L.active ? 1.0f : 0.0f;
    const float *tg = pp.target + L.b;              // row t - t_first of [T - t_first, B]: the TRANSFORMED target
    const float *wt = pp.w ? pp.w + L.b : nullptr;
    float *sim = pp.sim ? pp.sim + c * (int64_t)(T - t_first) * d.B + L.b : nullptr;
    // the same rows of the aux target and its weights, addressed from the (scalar) bases with the lane's basin added per
    // load: three per-lane pointers less, which is what keeps HBV 1.1p at three waves (DESIGN.md has the table)
    const float *atg = J.aux_target;
    const float *awt = J.aux_w;
    float *asim = J.aux_sim ? J.aux_sim + c * (int64_t)(T - t_first) * d.B : nullptr;

    // one-step-ahead register prefetch of the per-step inputs (k_fwd's), both observations and their weights with them
    float nxf[3], nxd[NP], nxo = 0.0f, nxw = 1.0f, nxa = 0.0f, nxaw = 1.0f;
    {
        const float *xr = xb;
        nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
#pragma unroll
        for (int i = 0; i < NP; i++) nxd[i] = ((dmask >> i) & 1) ? dynp[i][0] : 0.f;
        if (t_first == 0) {
            nxo = tg[0];
            if (wt) nxw = wt[0];
            nxa = atg[L.b];
            if (awt) nxaw = awt[L.b];
        }
    }

    for (int t = 0; t < T; t++) {
        Step<MODEL, BETAET> s;
        s.P = nxf[0]; s.Tf = nxf[1]; s.PET = nxf[2];
        float cur[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) cur[i] = nxd[i];
        const float obs = nxo, wobs = nxw, aobs = nxa, awobs = nxaw;
        {
            const int tn = t + 1 < T ? t + 1 : t;
            const float *xr = xb + (int64_t)tn * d.x_t_stride;
            nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
#pragma unroll
            for (int i = 0; i < NP; i++)
                if ((dmask >> i) & 1) nxd[i] = dynp[i][(int64_t)tn * d.p[i].dyn_t_stride];
            if (tn >= t_first) {
                const int64_t row = (int64_t)(tn - t_first) * d.B;
                nxo = tg[row];
                if (wt) nxw = wt[row];
                nxa = atg[row + L.b];
                if (awt) nxaw = awt[row + L.b];
            }
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
        st[0] = s.SP3; st[1] = s.MW3; st[2] = s.SM4; st[3] = s.SUZ4; st[4] = s.SLZ2;

        // the ensemble mean of Q as k_fwd forms series HBVX_F_QSIM, and the aux value as it forms that flux series: the
        // plain ensemble mean (invM with muwts too), never routed.  The two xor butterflies run in ONE loop, each value's
        // additions in ens_sum's order (so q has k_pop_stats' bits): as two loops the second waits out the first's
        // cross-lane latency on every day of a serial loop.
        const float wq = mu ? mu[(int64_t)t * d.mu_t_stride] : 1.0f;
        const float av = aux_series == HBVX_F_AET ? s.ET : aux_series == HBVX_F_SWE ? s.SP3
                       : aux_series == HBVX_F_Q0 ? s.Q0 : aux_series == HBVX_F_Q1 ? s.Q1 : s.Q2;
        float q = (mu ? s.Q * wq : s.Q) * act, v = av * act;
        for (int k = 0; k < lgMp; k++) {
            const float qo = __shfl_xor(q, 1 << k, 64), vo = __shfl_xor(v, 1 << k, 64);
            q += qo;
            v += vo;
        }
        if (!mu) q = q * invM;
        v = v * invM;
        const bool counted = t >= t_first;
        const float y = bs.template push<TR>(q, obs, wobs, counted);
        if (counted && sim && L.leader) sim[(int64_t)(t - t_first) * d.B] = y;      // y, not y'
        if (counted) {
            ax.push(v, aobs, awobs);
            if (asim && L.leader) asim[(int64_t)(t - t_first) * d.B + L.b] = v;
        }
    }
    if (L.leader) {
        const int64_t at = c * d.B + L.b;
        pp.cost[at] = bs.cost;
        S.s1[at] = bs.s1;
        S.s2[at] = bs.s2;
        S.s3[at] = bs.s3;
        J.aux_sse[at] = ax.sse;
        J.aux_s1[at] = ax.s1;
        J.aux_s2[at] = ax.s2;
        J.aux_s3[at] = ax.s3;
    }
}


} // namespace hbvx

#endif // __HIPCC__
