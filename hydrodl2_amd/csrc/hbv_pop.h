// hbv_pop.h -- population evaluation of the explicit models (include/hbvx.h): for P candidate static-parameter sets per
// basin, from one launch that writes no series it is not asked for,
//   hbvx_population_cost    the weighted squared error of the routed ensemble-mean streamflow: one [P,B] number;
//   hbvx_population_stats   that and three more chains per (candidate, basin), on the raw, the square-root or the log
//                           flow, from which NSE, KGE, correlation, variability and bias follow on the host: four;
//   hbvx_population_joint   the same four chains on a second series beside streamflow, the day's ensemble mean of one
//                           un-routed flux (AET, SWE, Q0, Q1, Q2): eight;
//   hbvx_population_period  the eight with the routed flow and the aux flux averaged over the periods of two calendars
//                           -- 8-day composites, months -- before they meet their targets: the sums run once per period
//                           instead of once per day, and the optional series are [P,K,B] period means.
// One kernel template, k_pop below, is the day loop of all four; launch_pop.hip has the entry points.  A fifth form of
// it, the runoff form, is stage 1 of the hourly model's population evaluation (hbvx_hourly_population_runoff,
// include/hbvx_gage_pop.h; launch_gage_pop.hip): the candidate loop alone, storing each candidate's unit runoff.  A
// sixth, the FDC form (hbvx_population_fdc, include/hbvx_pop_fdc.h; launch_pop.hip), is the daily stats form with
// exceedance counts and volumes above per-basin thresholds: the simulated flow-duration curve sampled at K points.  A
// seventh, the event form (hbvx_population_events, include/hbvx_pop_events.h; launch_pop.hip), is the daily stats form
// with the peak, the day of the peak and the volume inside per-basin event windows of scored days.  An eighth, the
// ensemble form (hbvx_population_ensemble, include/hbvx_pop_ens.h; launch_pop.hip), is the daily stats form over a window
// of the days with storages, routing history and forcing noise per particle, handed back for the next window.
//
// What happens to a basin's ensemble mean after the day step -- the normalised gamma unit hydrograph, the 15-day
// window, the causal convolution and the residual chain -- is hbvx_popk::Basin below and compiles for the host as
// well (tests/hosttest/pop_host.cpp), so the CPU tier checks it without a GPU; the kernel maps lanes onto it.
// hbvx_popk::BasinStats is Basin plus the transform and the three moment chains (tests/hosttest/popstats_host.cpp).
// hbvx_popk::AuxStats is the aux term's four chains (tests/hosttest/popjoint_host.cpp).
// hbvx_popk::PeriodMean is the mean over a period that hbvx_population_period puts between each of the two values and
// its chains (tests/hosttest/popperiod_host.cpp).
// hbvx_popk::FdcSlot is one threshold's exceedance count and volume (tests/hosttest/popfdc_host.cpp); k_gp_fdc
// (hbv_gage_pop.h, include/hbvx_gage_fdc.h) feeds the same slot the hours of a gage, and hbvx_popk::quant_key is the
// sortable image of a flow in that header's quantile call (tests/hosttest/gagefdc_host.cpp has both).
// hbvx_popk::EventSlot is one flood event's peak, hour of the peak and volume (hbvx_gage_population_events,
// include/hbvx_gage_events.h; tests/hosttest/gageevents_host.cpp); the event form of k_pop feeds the same slot days.
// hbvx_popk::EventCursor is that form's walk over a basin's window rows (tests/hosttest/popevents_host.cpp).
// Basin::load_history / save_history hand the routing window from one call of the ensemble form to the next
// (tests/hosttest/popens_host.cpp).
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

// The gamma unit hydrograph's arithmetic per tap (uh_routing.py:5-22), aa = relu(route_a) + 0.1, theta = relu(route_b)
// + 0.5: tap k before normalisation is 1 / denom * mid * right, in that order.  k_uh_gamma (hbvx.hip) runs one thread
// per (basin, tap) on these two, sums the 15 values of a basin in ascending k, zeros from L on included, and divides
// each by the sum.
HBVX_POP_HD float gamma_denom(float aa, float theta) { return expf(lgammaf(aa)) * powf(theta, aa); }
HBVX_POP_HD float gamma_tap(float denom, float aa, float theta, int k)
{
    float t = (float)k + 0.5f;
    float mid = powf(t, aa - 1.0f);
    float right = expf(-t / theta);
    return 1.0f / denom * mid * right;
}

// The normalised gamma unit hydrograph of physical route_a = a, route_b = bb: taps 0..L-1 as k_uh_gamma stores them and
// k_route_fwd loads them back, zero from L on.  A restatement of gamma_denom / gamma_tap and of k_uh_gamma's sum and
// divide, operation for operation (tests/test_uh_tap_host.py holds the two texts to each other).  It keeps its own
// text: calling the two helpers from it changed the instruction schedule of the population kernels
// (tools/compare_code.py), and those are pinned.  A change to either belongs in both.
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

    // The window across calls (hbvx_population_ensemble, include/hbvx_pop_ens.h): after a push, win[1 + k] is the value
    // pushed k + 1 pushes ago, so entry k of a history taken at day t is the un-routed value of day t - 1 - k, k = 0..13,
    // `stride` floats apart.  load_history before the first push of a call (h NULL: zeros, start()'s own) and
    // save_history after its last hand the 14 values over bit for bit; win[0] is overwritten by the next push.
    HBVX_POP_HD void load_history(const float *h, int64_t stride)
    {
#pragma unroll
        for (int k = 0; k < UH - 1; k++) win[k + 1] = h ? h[k * stride] : 0.0f;
    }

    HBVX_POP_HD void save_history(float *h, int64_t stride) const
    {
#pragma unroll
        for (int k = 0; k < UH - 1; k++) h[k * stride] = win[k + 1];
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
        if (counted) score<TR>(y, target, w);
        return y;
    }

    // A counted day of push() on a value that is already there -- also hbvx_population_period's period mean of y:
    // v' = transform(v), then r, d, e and the four chains against `target` (already transformed) and w.
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

// One threshold of hbvx_population_fdc for one (candidate, basin).  push() takes the days that enter the flow-duration
// curve in ascending order, with the raw routed flow y (never its transform):
//   y > thr:   n = n + 1      vol = vol + y          (one float32 addition, in day order)
// A day at the threshold is not above it; a NaN flow is above nothing; -0 is not above +0.
struct FdcSlot {
    uint32_t n;
    float vol;

    HBVX_POP_HD void start()
    {
        n = 0;
        vol = 0.0f;
    }

    HBVX_POP_HD void push(float y, float thr)
    {
        if (y > thr) {
            n += 1;
            vol = vol + y;
        }
    }
};

constexpr int FDC_MAX_THR = 32;     // HBVX_POP_FDC_MAX_THR

// The sortable image of a flow for hbvx_gage_population_quantiles (include/hbvx_gage_fdc.h): an unsigned key whose
// integer order is float32's total order on the values that are not NaN, -0 below +0 (a set sign bit flips every bit, a
// clear one sets it), every NaN QUANT_NAN above all of them, and QUANT_NONE, which no flow maps to (-inf is 0x007FFFFF),
// below all of them: the key of an hour that is not scored and of the padding.  quant_value undoes quant_key bit for bit.
constexpr uint32_t QUANT_NONE = 0u, QUANT_NAN = 0xFFFFFFFFu;

HBVX_POP_HD uint32_t quant_key(float y)
{
    const uint32_t b = __builtin_bit_cast(uint32_t, y);
    if (y != y) return QUANT_NAN;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

HBVX_POP_HD float quant_value(uint32_t key)
{
    return __builtin_bit_cast(float, (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// One event window of hbvx_gage_population_events for one (candidate, gage).  push() takes the hours of the window in
// ascending order, with the hourly gage flow y and the hour t:
//   y > peak:  peak = y, hour = t          vol = vol + y   (one float32 addition per hour, in hour order)
// A plateau keeps its first hour; a NaN flow is above nothing (it leaves peak and hour alone and poisons vol); -0 is not
// above +0.  A slot that is pushed nothing stays at -inf, -1, +0: the absent event.
struct EventSlot {
    float peak;
    int32_t hour;
    float vol;

    HBVX_POP_HD void start()
    {
        peak = -INFINITY;
        hour = -1;
        vol = 0.0f;
    }

    HBVX_POP_HD void push(float y, int32_t t)
    {
        if (y > peak) {
            peak = y;
            hour = t;
        }
        vol = vol + y;
    }
};

// The walk of hbvx_population_events over one basin's E window rows (include/hbvx_pop_events.h states the rule): rows are
// offered in order e = 0, 1, ... through admit(); [ws, we] is the live window in scored days, and `we` doubles as the last
// day any live window took (-1 before the first), so a row is live iff its start is beyond it and its clamped end is not
// before its start.  Between live windows, and after the last, ws is INT32_MAX: inside() is false on every day.
//   admit(s, f, T_out):  f = min(f, T_out - 1);  live = s > we && f >= s;  live: ws = s, we = f
// The caller steps e past every row it offers, live (when the window closes) or absent (at once), so a basin takes E
// steps whatever the rows hold, and no day outside 0 .. T_out - 1 is ever inside.
struct EventCursor {
    int32_t e, ws, we;

    HBVX_POP_HD void start()
    {
        e = 0;
        ws = INT32_MAX;
        we = -1;
    }

    HBVX_POP_HD bool admit(int32_t s, int32_t f, int32_t T_out)
    {
        f = f < T_out - 1 ? f : T_out - 1;
        const bool live = s > we && f >= s;
        if (live) {
            ws = s;
            we = f;
        }
        return live;
    }

    HBVX_POP_HD void rest() { ws = INT32_MAX; }         // no live window: between two, and behind the last row

    HBVX_POP_HD bool inside(int32_t rel) const { return rel >= ws && rel <= we; }

    HBVX_POP_HD bool closes(int32_t rel) const { return rel == we; }      // (asked on a day that is inside)
};

} // namespace hbvx_popk

#if defined(__HIPCC__)

#include <type_traits>

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

// hbvx_hourly_population_runoff (include/hbvx_gage_pop.h): the candidate loop alone.  `a` carries the descriptor and the
// candidates' sources (a.pop.p); nothing else of a.pop is read.
struct PopRunoffArgs {
    PopArgs a;
    float *runoff;              // [P,T,B]: each candidate's hourly unit runoff, the module's Qs
};

struct PopPeriodArgs {
    PopJointArgs j;             // the two terms: hbvx_population_joint's arguments, targets / weights / series per PERIOD
    int has_aux;                // 0: aux_series == HBVX_POP_NO_AUX, nothing of j's aux part is read or written
    int n_flow, n_aux;          // KF, KA
    const int *flow_end, *aux_end;      // [KF], [KA]: closing days relative to t_first, ascending
};

// hbvx_population_fdc (include/hbvx_pop_fdc.h): the daily stats form, and per (candidate, threshold, basin) a count and a
// volume.
struct PopFdcArgs {
    PopStatsArgs s;             // hbvx_population_stats' arguments
    int n_thr;                  // K, 1..hbvx_popk::FDC_MAX_THR
    const float *thr;           // [K,B]
    int32_t *count;             // [P,K,B]
    float *volume;              // [P,K,B]
};

// hbvx_population_events (include/hbvx_pop_events.h): the daily stats form, and per (candidate, event, basin) a peak, its
// day and a volume.
struct PopEventArgs {
    PopStatsArgs s;             // hbvx_population_stats' arguments
    int n_events;               // E, 1..T - t_first
    const int32_t *start, *end; // [E,B] inclusive scored days
    float *peak;                // [P,E,B]
    int32_t *peak_day;          // [P,E,B]
    float *volume;              // [P,E,B]
};

// hbvx_population_ensemble (include/hbvx_pop_ens.h): the daily stats form over days t_begin .. t_end-1, each particle
// (candidate) with storages, routing history and forcing noise of its own.
struct PopEnsArgs {
    PopStatsArgs s;             // hbvx_population_stats' arguments; target / w / sim are window-relative
    int t_begin, t_end;         // 0 <= t_begin < t_end <= d.T
    int n_src, src_first;       // particles of state_in / hist_in (>= 1), the identity ancestor's offset
    const float *state_in;      // [n_src,5,B,M] or NULL (the descriptor's, or 0.001)
    float *state_out;           // [P,5,B,M]
    const float *hist_in;       // [n_src,14,B] or NULL (zeros)
    float *hist_out;            // [P,14,B]; written when the call routes
    const int32_t *ancestor;    // [P,B] or NULL (src_first + c)
    const float *p_mul, *t_add; // each NULL (no operation) or [c * c_stride + (t - t_begin) * t_stride + b]
    int64_t pm_c_stride, pm_t_stride, ta_c_stride, ta_t_stride;
};

// The event form addresses a basin's rows of start / end and of a candidate's [E,B] outputs with a 32-bit element index,
// e * B + b (the launcher refuses E * B beyond this): a scalar base and a per-lane 32-bit offset.  With 64-bit per-lane
// addresses the compiler hoists five of them out of the day loop, ten VGPRs, and HBV 1.1p drops to two waves per SIMD.
constexpr int64_t EVENT_MAX_CELLS = (int64_t)1 << 30;

// The slots of the FDC form per lane, R = ceil(K / Mp), and the dynamic LDS of a launch: [R][threshold, count,
// volume][64 lanes] of four bytes each.
__host__ __device__ __forceinline__ int fdc_slots(int n_thr, int lgMp) { return (n_thr + (1 << lgMp) - 1) >> lgMp; }
__host__ __device__ __forceinline__ unsigned fdc_lds_bytes(int n_thr, int lgMp) { return (unsigned)fdc_slots(n_thr, lgMp) * 64u * 12u; }

// each struct's view of the ones nested in it
__host__ __device__ __forceinline__ const PopArgs &pop_args(const PopArgs &A) { return A; }
__host__ __device__ __forceinline__ const PopArgs &pop_args(const PopStatsArgs &A) { return A.a; }
__host__ __device__ __forceinline__ const PopArgs &pop_args(const PopJointArgs &A) { return A.s.a; }
__host__ __device__ __forceinline__ const PopArgs &pop_args(const PopPeriodArgs &A) { return A.j.s.a; }
__host__ __device__ __forceinline__ const PopArgs &pop_args(const PopRunoffArgs &A) { return A.a; }
__host__ __device__ __forceinline__ const PopArgs &pop_args(const PopFdcArgs &A) { return A.s.a; }
__host__ __device__ __forceinline__ const PopArgs &pop_args(const PopEventArgs &A) { return A.s.a; }
__host__ __device__ __forceinline__ const PopArgs &pop_args(const PopEnsArgs &A) { return A.s.a; }
__host__ __device__ __forceinline__ const PopStatsArgs &stats_args(const PopEnsArgs &A) { return A.s; }
__host__ __device__ __forceinline__ const PopStatsArgs &stats_args(const PopStatsArgs &A) { return A; }
__host__ __device__ __forceinline__ const PopStatsArgs &stats_args(const PopJointArgs &A) { return A.s; }
__host__ __device__ __forceinline__ const PopStatsArgs &stats_args(const PopPeriodArgs &A) { return A.j.s; }
__host__ __device__ __forceinline__ const PopStatsArgs &stats_args(const PopFdcArgs &A) { return A.s; }
__host__ __device__ __forceinline__ const PopStatsArgs &stats_args(const PopEventArgs &A) { return A.s; }
__host__ __device__ __forceinline__ const PopJointArgs &joint_args(const PopJointArgs &A) { return A; }
__host__ __device__ __forceinline__ const PopJointArgs &joint_args(const PopPeriodArgs &A) { return A.j; }

constexpr int T_COST = -1;      // TR of the cost-only instances (the others are hbvx_popk::T_*)

// The FDC form's dynamic LDS (fdc_lds_bytes): only its instances name it.
__device__ __forceinline__ float *fdc_lds()
{
    extern __shared__ float fdc_lds_base[];
    return fdc_lds_base;
}

template <int TR> struct PopBasin { using type = hbvx_popk::BasinStats; };
template <> struct PopBasin<T_COST> { using type = hbvx_popk::Basin; };

// ---------------------------------------------------------------------------
// k_pop<MODEL, BETAET, TR, Args>: the one day loop of the explicit models' population entry points.  It is k_fwd's day
// loop (the same Step::fwd instance, the same one-day-ahead register prefetch of the forcings and the dynamic rows, the
// same ensemble sum and weights) with the lane mapping of k_tan's several-direction form: one wave per workgroup,
// blockIdx.x the wave's group of basins, blockIdx.y the CANDIDATE, one lane per (basin, member).  A candidate is a wave
// of its own that reads the forcings itself -- they come out of the L2 / Infinity Cache after the first candidate's
// pass -- and nothing is shared between candidates inside the kernel: what many candidates in one launch gain over a
// forward each is that their waves fill the SIMDs one forward leaves idle, and that nothing but [P,B] sums is written.
// The candidate index is uniform over the wave, so a candidate's base address is scalar.  Several candidates per lane
// are not tried: k_tan measured that form and lost at every size (hbv_tan.h), for a reason that holds here too (the
// loop is bound by instruction issue, registers cost resident waves).
//
// After the ensemble sum every lane of a basin holds the mean, so every lane carries the basin's window and chains (the
// same values: no shuffle, no divergence) and the leader stores.  The bits of what candidate c gets depend on c's values
// alone: c enters addresses only.
//
// Args is the form, each one the form before it and something more:
//   PopArgs        TR = T_COST; lanes map onto hbvx_popk::Basin: the squared error of the routed mean flow.
//   PopStatsArgs   TR = T_NONE / T_SQRT / T_LOG; lanes map onto BasinStats: the shift and eps of the lane's basin are two
//                  more registers, the three moment chains three more, the leader stores four numbers.  TR is a template
//                  parameter: a wave-uniform switch inside the day loop would keep the log's registers live in every
//                  transform.
//   PopJointArgs   an AuxStats beside the BasinStats: per day one more ensemble sum, of the flux the aux term scores, and
//                  four more chains on it.  The aux target and weight join the one-day-ahead prefetch.  Which flux is
//                  taken is a run-time select on aux_series, uniform over the launch, not a template parameter: the five
//                  values are all live at the end of Step::fwd anyway (Q is their sum, SP3 is the next state, ET has just
//                  closed the soil balance), so the select keeps little alive that a fixed choice would free -- built
//                  both ways, a fixed AET or SWE came out one VGPR below the select (three in one HBV 1.1p instance;
//                  DESIGN.md has the table), never across an occupancy step, at five times the instantiations.
//   PopPeriodArgs  (PERIOD) a PeriodMean between each of the two values and its chains.  Each calendar has a cursor k, the
//                  day its period opened and the day it closes, all relative to t_first and uniform over the wave (they
//                  come from kernel arguments and scalar loads).  A scored day adds to the period's accumulator; a day
//                  that closes a period divides once, runs the four chains against row k of the target, lets the leader
//                  store the mean, moves the cursor and loads the next closing day and the next period's target row and
//                  weight -- at the OPENING of the period that needs them, so that its close does not wait on memory;
//                  they are not in the per-day prefetch.  A cursor stops at its count: no closing day and no target row
//                  beyond K is read, whatever the calendar holds.  A closing day that is not ahead of the cursor's day (a
//                  calendar that does not ascend) is never met: the periods from there on stay open, nothing else
//                  happens.  Days after the last closing day are simulated and scored nowhere.  Without an aux term
//                  (has_aux == 0, uniform over the launch; a run-time flag in this form only) the aux value is zero
//                  through the butterfly and nothing aux is accumulated, loaded or stored.
//   PopRunoffArgs  (RUNOFF) TR = T_COST; Step<MODEL_HOURLY> only: the candidate loop with none of the window or chains.  The
//                  hour's ensemble mean times 1/24 is the module's Qs, and the unit's leader stores it to [P,T,B]: the score
//                  of the hourly model lives at the gages, after a sum over units (hbv_gage_pop.h takes it from there).
//   PopFdcArgs     (FDC) the daily stats form, and K exceedance counters and volumes per basin (hbvx_popk::FdcSlot).  After
//                  the butterfly all Mp lanes of a basin hold the same y, so the lanes share the thresholds out: lane jm
//                  owns k = jm, jm + Mp, ... below K -- padded member lanes too, they hold y as well -- which is R =
//                  ceil(K / Mp) slots per lane, uniform over the launch.  R is a run-time number, so the slots live in
//                  dynamic LDS, slot-major [R][thr, n, vol][64 lanes]: a lane touches its own column only (no atomics, no
//                  barrier, no bank conflict; the three planes of a slot are one address and three immediate offsets).  A
//                  slot beyond K holds thr = +inf and is never stored.  The thresholds are in LDS beside the sums, not
//                  re-read from memory: a global load per slot and day would put R more vector loads on a loop that
//                  issue binds, behind the same address arithmetic the LDS column needs once.  A day enters when it is
//                  counted and its weight is > 0 (the weight is a mask here); the comparison is on y, not its transform.
//                  Everything of it is behind `if constexpr (FDC)`: the other instances are untouched
//                  (profiles/r24_population_fdc.md has the comparison).
//   PopEventArgs   (EVENTS) the daily stats form, and E event windows per basin (hbvx_popk::EventCursor, EventSlot).  After
//                  the butterfly every lane of a basin holds the same y, so every lane carries its basin's cursor and slot
//                  -- six registers: the row, the live window, the peak, its day, the volume -- and the leader stores.
//                  One slot is live at a time, so unlike the FDC form's K slots it stays in registers: parked in LDS it
//                  came out one VGPR higher, not lower (the column's address is a register too).  A scored day inside
//                  the live window pushes the raw y (not its transform, and whatever the day's weight: the window is
//                  the mask); the day that closes it stores the row, restarts the slot and
//                  seeks the next live row, storing -inf, -1, +0 for every absent row it passes.  Windows differ per
//                  basin, so the lanes of different basins diverge there under the execution mask: no atomics, no
//                  barrier.  The seek reads two int32 per row and runs E steps per lane over the whole launch; no row
//                  beyond E and no day outside the scored days is touched whatever the rows hold.  Everything of it is
//                  behind `if constexpr (EVENTS)` (profiles/r26_population_events.md has the comparison).
//   PopEnsArgs     (ENS) the daily stats form over the window t_begin .. t_end-1 of the descriptor's days, the candidate a
//                  PARTICLE.  One int32 load per lane before the day loop names the particle's ancestor (clamped to
//                  0 .. n_src-1: memory-safe for any content); the five storages and, when the call routes, the 14 values
//                  of the window's history come from the ancestor's slot (Basin::load_history).  p_mul / t_add join the
//                  one-day-ahead prefetch like nxo / nxw and are applied between the prefetch and Step::fwd, one multiply
//                  and one add; a NULL pointer (uniform over the launch) is the absent operation.  Scored days are those
//                  >= t0 = max(t_begin, t_first), and target / w / sim rows count from t0.  After the last day every
//                  active lane stores its five storages (k_fwd's state_out convention: the lanes of padded members
//                  store nothing) and the leader the history (save_history).  The loop bounds, t0 and the prefetch's
//                  last-row clamp are this form's own variables (ens_tb, ens_te, ens_t0); the other forms keep theirs.
//                  Everything of it is behind `if constexpr (ENS)` (profiles/r30_population_ensemble.md has the comparison).
// The flow's operations are the same ones on the same values in every form, and the aux term's in both of its forms:
// tests/test_population_stats_gpu.py, test_population_joint_gpu.py and test_population_period_gpu.py (daily calendars)
// hold each form to the bits of the one before it.
//
// Every instance is instruction for instruction the kernel it had when the four forms were four texts (profiles/
// r21_population_one_source.md), so what was measured on those holds for these.  The compiler's schedule follows the
// order and shape of the statements, and four things keep it:
//   - the day's observations are loop-local constants (`obs = nxo` at the top of the iteration) in the daily forms; the
//     period form's are variables of their own that live across days (`pobs`), not the prefetched ones reused;
//   - the day count in the base address of `sim` / `aux_sim` is the inline expression `(T - t_first)` in the daily
//     forms, not a variable shared with the period form's KF / KA;
//   - `has_aux` is the constant true in the joint form;
//   - the cost form's one store indexes `pp.cost[c * d.B + L.b]` in place; the other forms share `at` between their
//     stores (the cost form through `at` computes the index before it loads the pointer).
// A fix to the day's arithmetic belongs in Step::fwd, a fix to the loop around it here, once.
// ---------------------------------------------------------------------------
template <int MODEL, bool BETAET, int TR, typename Args>
__global__ void __launch_bounds__(64) k_pop(const Args Q)
{
    constexpr bool RUNOFF = std::is_same<Args, PopRunoffArgs>::value;
    constexpr bool STATS = !RUNOFF && !std::is_same<Args, PopArgs>::value;
    constexpr bool PERIOD = std::is_same<Args, PopPeriodArgs>::value;
    constexpr bool JOINT = PERIOD || std::is_same<Args, PopJointArgs>::value;      // the forms with an aux term
    constexpr bool FDC = std::is_same<Args, PopFdcArgs>::value;
    constexpr bool EVENTS = std::is_same<Args, PopEventArgs>::value;
    constexpr bool ENS = std::is_same<Args, PopEnsArgs>::value;
    static_assert(STATS == (TR != T_COST), "TR = T_COST is the cost form's, and its alone");
    constexpr int NP = NParam<MODEL, BETAET>::value;
    const PopArgs &A = pop_args(Q);
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
    const float ac = (MODEL == MODEL_HBV20 || MODEL == MODEL_HOURLY) ? d.ac[L.b] : 0.0f;
    const float elev = (MODEL == MODEL_HBV20 || MODEL == MODEL_HOURLY) ? d.elev[L.b] : 0.0f;

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
    // ENS: the window and its first scored day (uniform), and the slot the particle starts from: one index load per lane,
    // clamped to the sources that exist
    int ens_tb = 0, ens_te = 0, ens_t0 = 0;
    int64_t anc = 0;
    if constexpr (ENS) {
        ens_tb = Q.t_begin, ens_te = Q.t_end;
        ens_t0 = ens_tb > t_first ? ens_tb : t_first;
        int a = Q.ancestor ? Q.ancestor[c * d.B + L.b] : Q.src_first + (int)c;
        a = a < 0 ? 0 : a;
        a = a > Q.n_src - 1 ? Q.n_src - 1 : a;
        anc = a;
        const float *sp = Q.state_in ? Q.state_in + anc * 5 * N : d.state_in;
#pragma unroll
        for (int k = 0; k < 5; k++) st[k] = sp ? sp[k * N + L.n] : 0.001f;
    } else {
#pragma unroll
        for (int k = 0; k < 5; k++) st[k] = d.state_in ? d.state_in[k * N + L.n] : 0.001f;
    }

    typename PopBasin<TR>::type bs;
    if constexpr (RUNOFF) ;     // no window, no chains: the runoff form scores nothing
    else if constexpr (STATS)
        bs.start(A.has_route != 0, stats_args(Q).shift[L.b], TR == hbvx_popk::T_LOG ? stats_args(Q).eps[L.b] : 0.0f);
    else bs.start(A.has_route != 0);
    if (!RUNOFF && A.has_route) {      // route_ab's lines (hbvx.hip) on the candidate's routing inputs
        const hbvx_route_desc &r = A.r;
        const float va = pp.ra ? pp.ra[c * pp.r_c_stride + (int64_t)L.b * pp.r_b_stride] : r.ra[(int64_t)L.b * r.r_stride];
        const float vb = pp.rb ? pp.rb[c * pp.r_c_stride + (int64_t)L.b * pp.r_b_stride] : r.rb[(int64_t)L.b * r.r_stride];
        const float ua = r.raw_sigmoid ? sigmoid_(va) : va;
        const float ub = r.raw_sigmoid ? sigmoid_(vb) : vb;
        hbvx_popk::gamma_taps(descale_(ua, r.a_lo, r.a_hi), descale_(ub, r.b_lo, r.b_hi), r.L, bs.uh);
        if constexpr (ENS) bs.load_history(Q.hist_in ? Q.hist_in + anc * (hbvx_popk::UH - 1) * d.B + L.b : nullptr, d.B);
    }

    bool has_aux = JOINT;       // uniform over the launch
    hbvx_popk::AuxStats ax;
    int aux_series = 0;
    if constexpr (PERIOD) has_aux = Q.has_aux != 0;
    if constexpr (JOINT) {
        ax.start(has_aux ? joint_args(Q).aux_shift[L.b] : 0.0f);
        aux_series = joint_args(Q).aux_series;
    }

    const float *xb = d.x + (int64_t)L.b * d.x_b_stride;
    const float *mu = d.muwts ? d.muwts + (int64_t)L.b * d.mu_b_stride + L.j : nullptr;
    const float invM = 1.0f / (float)d.M;
    const float act = L.active ? 1.0f : 0.0f;
    int KF = 0, KA = 0;                             // PERIOD: the calendars' lengths and closing days
    const int *fend = nullptr, *aend = nullptr;
    if constexpr (PERIOD) {
        KF = Q.n_flow, KA = has_aux ? Q.n_aux : 0;
        fend = Q.flow_end, aend = Q.aux_end;
    }
    // row t - t_first of [T - t_first, B], PERIOD: row k of [KF, B]; with STATS the TRANSFORMED target
    const float *tg = pp.target + L.b;
    const float *wt = pp.w ? pp.w + L.b : nullptr;
    float *sim;
    if constexpr (PERIOD) sim = pp.sim ? pp.sim + c * (int64_t)KF * d.B + L.b : nullptr;
    else if constexpr (ENS) sim = pp.sim && ens_te > ens_t0 ? pp.sim + c * (int64_t)(ens_te - ens_t0) * d.B + L.b : nullptr;
    else sim = pp.sim ? pp.sim + c * (int64_t)(T - t_first) * d.B + L.b : nullptr;
    // the same rows of the aux target and its weights, addressed from the (scalar) bases with the lane's basin added per
    // load: three per-lane pointers less, which is what keeps HBV 1.1p at three waves (DESIGN.md has the table)
    const float *atg = nullptr, *awt = nullptr;
    float *asim = nullptr;
    if constexpr (JOINT) {
        atg = joint_args(Q).aux_target;
        awt = joint_args(Q).aux_w;
        if constexpr (PERIOD) asim = has_aux && joint_args(Q).aux_sim ? joint_args(Q).aux_sim + c * (int64_t)KA * d.B : nullptr;
        else asim = joint_args(Q).aux_sim ? joint_args(Q).aux_sim + c * (int64_t)(T - t_first) * d.B : nullptr;
    }

    // PERIOD: the calendars' cursors (uniform): period kf of the flow runs from day sf to day ef of the scored days, ka /
    // sa / ea the same for the aux series; and the open periods' target rows and weights
    int kf = 0, sf = 0, ef = KF > 0 ? fend[0] : -1;
    int ka = 0, sa = 0, ea = KA > 0 ? aend[0] : -1;
    float pobs = 0.0f, pwobs = 1.0f, paobs = 0.0f, pawobs = 1.0f;
    hbvx_popk::PeriodMean pf, pa;
    if constexpr (PERIOD) {
        if (KF > 0) {
            pobs = tg[0];
            if (wt) pwobs = wt[0];
        }
        if (KA > 0) {
            paobs = atg[L.b];
            if (awt) pawobs = awt[L.b];
        }
        pf.acc = pa.acc = 0.0f;
    }

    // FDC: the lane's column of the slots, R of them; slot r is threshold k = jm + r * Mp, +inf from K on
    float *slot = nullptr;
    int R = 0;
    if constexpr (FDC) {
        R = fdc_slots(Q.n_thr, lgMp);
        slot = fdc_lds() + (threadIdx.x & 63);
        for (int r = 0; r < R; r++) {
            const int k = L.jm + (r << lgMp);
            slot[r * 192] = k < Q.n_thr ? Q.thr[(int64_t)k * d.B + L.b] : INFINITY;
            slot[r * 192 + 64] = __uint_as_float(0u);
            slot[r * 192 + 128] = 0.0f;
        }
    }

    // EVENTS: the basin's cursor and slot (the same in all of its lanes), six registers.  ev_seek() offers the rows from
    // ec.e on until one is live, the leader storing the absent ones on the way; the row index only rises, so all seeks of
    // a lane together take n_events steps.  The element index of a row is 32-bit (EVENT_MAX_CELLS).
    hbvx_popk::EventCursor ec;
    hbvx_popk::EventSlot evs;
    auto ev_store = [&](int e) {
        if constexpr (EVENTS) {
            if (L.leader) {
                const int64_t cat = c * Q.n_events * d.B;       // (uniform: the candidate's [E,B] block)
                const uint32_t at = (uint32_t)e * (uint32_t)d.B + (uint32_t)L.b;
                (Q.peak + cat)[at] = evs.peak;
                (Q.peak_day + cat)[at] = evs.hour;
                (Q.volume + cat)[at] = evs.vol;
            }
        }
    };
    auto ev_seek = [&]() {
        if constexpr (EVENTS) {
            ec.rest();
            for (; ec.e < Q.n_events; ec.e++) {
                const uint32_t row = (uint32_t)ec.e * (uint32_t)d.B + (uint32_t)L.b;
                if (ec.admit(Q.start[row], Q.end[row], T - t_first)) break;
                ev_store(ec.e);         // (evs is at its start: the absent event)
            }
        }
    };
    if constexpr (EVENTS) {
        ec.start();
        evs.start();
        ev_seek();
    }

    // one-step-ahead register prefetch of the per-step inputs (k_fwd's); in the daily forms the observations and their
    // weights with them
    float nxf[3], nxd[NP], nxo = 0.0f, nxw = 1.0f, nxa = 0.0f, nxaw = 1.0f;
    // ENS: the particle's rows of the two perturbations (row 0 is day t_begin), and their prefetched values
    const float *pmul = nullptr, *tadd = nullptr;
    float nxpm = 1.0f, nxta = 0.0f;
    if constexpr (ENS) {
        pmul = Q.p_mul ? Q.p_mul + c * Q.pm_c_stride + L.b : nullptr;
        tadd = Q.t_add ? Q.t_add + c * Q.ta_c_stride + L.b : nullptr;
        const float *xr = xb + (int64_t)ens_tb * d.x_t_stride;
        nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
#pragma unroll
        for (int i = 0; i < NP; i++) nxd[i] = ((dmask >> i) & 1) ? dynp[i][(int64_t)ens_tb * d.p[i].dyn_t_stride] : 0.f;
        if (ens_tb >= t_first) {
            nxo = tg[0];
            if (wt) nxw = wt[0];
        }
        if (pmul) nxpm = pmul[0];
        if (tadd) nxta = tadd[0];
    } else {
        const float *xr = xb;
        nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
#pragma unroll
        for (int i = 0; i < NP; i++) nxd[i] = ((dmask >> i) & 1) ? dynp[i][0] : 0.f;
        if constexpr (!PERIOD && !RUNOFF) {
            if (t_first == 0) {
                nxo = tg[0];
                if (wt) nxw = wt[0];
                if constexpr (JOINT) {
                    nxa = atg[L.b];
                    if (awt) nxaw = awt[L.b];
                }
            }
        }
    }

    // (ENS ? a : b is folded where it stands: each instance names its own bounds)
    for (int t = ENS ? ens_tb : 0; t < (ENS ? ens_te : T); t++) {
        Step<MODEL, BETAET> s;
        s.P = nxf[0]; s.Tf = nxf[1]; s.PET = nxf[2];
        const float cpm = nxpm, cta = nxta;     // (ENS: the day's perturbations, applied below, after the prefetch)
        float cur[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) cur[i] = nxd[i];
        const float obs = nxo, wobs = nxw, aobs = nxa, awobs = nxaw;
        {
            const int tn = t + 1 < (ENS ? ens_te : T) ? t + 1 : t;
            const float *xr = xb + (int64_t)tn * d.x_t_stride;
            nxf[0] = xr[d.ch_prcp]; nxf[1] = xr[d.ch_tmean]; nxf[2] = xr[d.ch_pet];
#pragma unroll
            for (int i = 0; i < NP; i++)
                if ((dmask >> i) & 1) nxd[i] = dynp[i][(int64_t)tn * d.p[i].dyn_t_stride];
            if constexpr (ENS) {
                if (tn >= ens_t0) {
                    const int64_t row = (int64_t)(tn - ens_t0) * d.B;
                    nxo = tg[row];
                    if (wt) nxw = wt[row];
                }
                if (pmul) nxpm = pmul[(int64_t)(tn - ens_tb) * Q.pm_t_stride];
                if (tadd) nxta = tadd[(int64_t)(tn - ens_tb) * Q.ta_t_stride];
            } else if constexpr (!PERIOD && !RUNOFF) {
                if (tn >= t_first) {
                    const int64_t row = (int64_t)(tn - t_first) * d.B;
                    nxo = tg[row];
                    if (wt) nxw = wt[row];
                    if constexpr (JOINT) {
                        nxa = atg[row + L.b];
                        if (awt) nxaw = awt[row + L.b];
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NP; i++)
            if ((dmask >> i) & 1) {
                float v = raw ? sigmoid_dyn_(cur[i]) : cur[i];
                float pv = descale_(v, d.p[i].lo, d.p[i].hi);
                if (use_dyn[i]) p[i] = pv;
            }
        if constexpr (ENS) {
            if (pmul) s.P = s.P * cpm;          // one multiply, one add; a NULL pointer is no operation at all
            if (tadd) s.Tf = s.Tf + cta;
        }
        s.SP = st[0]; s.MW = st[1]; s.SM = st[2]; s.SUZ = st[3]; s.SLZ = st[4];
        s.template fwd<false, true>(p, nz, ac, elev, 0.f, 0.f);
        st[0] = s.SP3; st[1] = s.MW3; st[2] = s.SM4; st[3] = s.SUZ4; st[4] = s.SLZ2;

        // the ensemble mean of Q as k_fwd forms series HBVX_F_QSIM, and the aux value as it forms that flux series: the
        // plain ensemble mean (invM with muwts too), never routed.  The two xor butterflies run in ONE loop, each value's
        // additions in ens_sum's order (so q has the bits of the forms without an aux term): as two loops the second
        // waits out the first's cross-lane latency on every day of a serial loop.
        const float wq = mu ? mu[(int64_t)t * d.mu_t_stride] : 1.0f;
        float q, v = 0.0f;
        if constexpr (JOINT) {
            const float av = !has_aux ? 0.0f
                           : aux_series == HBVX_F_AET ? s.ET : aux_series == HBVX_F_SWE ? s.SP3
                           : aux_series == HBVX_F_Q0 ? s.Q0 : aux_series == HBVX_F_Q1 ? s.Q1 : s.Q2;
            q = (mu ? s.Q * wq : s.Q) * act, v = av * act;
            for (int k = 0; k < lgMp; k++) {
                const float qo = __shfl_xor(q, 1 << k, 64), vo = __shfl_xor(v, 1 << k, 64);
                q += qo;
                v += vo;
            }
            if (!mu) q = q * invM;
            v = v * invM;
        } else {
            q = ens_sum((mu ? s.Q * wq : s.Q) * act, lgMp);
            if (!mu) q = q * invM;
        }
        if constexpr (RUNOFF) {
            // the module's Qs: the ensemble mean times dt = 1/24, one float32 multiply (hbv_2_hourly.py:741)
            if (L.leader) Q.runoff[(c * T + t) * d.B + L.b] = q * (float)(1.0 / 24.0);
        } else if constexpr (PERIOD) {
            const float y = bs.Basin::push(q, 0.0f, 0.0f, false);       // the routing runs every day
            const int rel = t - t_first;                                // the day among the scored days
            if (rel >= 0 && kf < KF) {
                pf.add(y, rel == sf);
                if (rel == ef) {
                    const int n = ef - sf + 1;
                    const float mean = n == 1 ? pf.acc : pf.close(n);       // (x / 1.0f is x: the same bits, no division)
                    bs.template score<TR>(mean, pobs, pwobs);
                    if (sim && L.leader) sim[(int64_t)kf * d.B] = mean;     // the mean, not its transform
                    kf++;
                    sf = rel + 1;
                    if (kf < KF) {
                        ef = fend[kf];
                        pobs = tg[(int64_t)kf * d.B];
                        if (wt) pwobs = wt[(int64_t)kf * d.B];
                    }
                }
            }
            if (rel >= 0 && ka < KA) {
                pa.add(v, rel == sa);
                if (rel == ea) {
                    const int n = ea - sa + 1;
                    const float mean = n == 1 ? pa.acc : pa.close(n);
                    ax.push(mean, paobs, pawobs);
                    if (asim && L.leader) asim[(int64_t)ka * d.B + L.b] = mean;
                    ka++;
                    sa = rel + 1;
                    if (ka < KA) {
                        ea = aend[ka];
                        paobs = atg[(int64_t)ka * d.B + L.b];
                        if (awt) pawobs = awt[(int64_t)ka * d.B + L.b];
                    }
                }
            }
        } else {
            const bool counted = t >= t_first;
            float y;
            if constexpr (STATS) y = bs.template push<TR>(q, obs, wobs, counted);
            else y = bs.push(q, obs, wobs, counted);
            if constexpr (ENS) {
                if (counted && sim && L.leader) sim[(int64_t)(t - ens_t0) * d.B] = y;
            } else if (counted && sim && L.leader) sim[(int64_t)(t - t_first) * d.B] = y;      // y, not its transform
            if constexpr (FDC) {
                if (counted && wobs > 0.0f) {
                    for (int r = 0; r < R; r++) {
                        hbvx_popk::FdcSlot f;
                        f.n = __float_as_uint(slot[r * 192 + 64]);
                        f.vol = slot[r * 192 + 128];
                        f.push(y, slot[r * 192]);
                        slot[r * 192 + 64] = __uint_as_float(f.n);
                        slot[r * 192 + 128] = f.vol;
                    }
                }
            }
            if constexpr (EVENTS) {
                const int rel = t - t_first;            // the day among the scored days; negative days are inside nothing
                if (ec.inside(rel)) {
                    evs.push(y, rel);
                    if (ec.closes(rel)) {
                        ev_store(ec.e);
                        evs.start();
                        ec.e++;
                        ev_seek();
                    }
                }
            }
            if constexpr (JOINT) {
                if (counted) {
                    ax.push(v, aobs, awobs);
                    if (asim && L.leader) asim[(int64_t)(t - t_first) * d.B + L.b] = v;
                }
            }
        }
    }
    if constexpr (RUNOFF) return;
    if constexpr (ENS) {
        // the storages after day t_end - 1, as k_fwd stores state_out: the lanes of real (basin, member) pairs; and the
        // window's history, the same in every lane of a basin, from its leader
        if (L.active) {
            float *so = Q.state_out + c * 5 * N;
#pragma unroll
            for (int k = 0; k < 5; k++) so[k * N + L.n] = st[k];
        }
        if (A.has_route && L.leader) bs.save_history(Q.hist_out + c * (hbvx_popk::UH - 1) * d.B + L.b, d.B);
    }
    if constexpr (FDC) {
        // every lane of a real basin stores the slots it owns (L.b is clamped: the lanes of basins beyond B store nothing)
        const bool real = (int)blockIdx.x * (64 >> lgMp) + ((int)(threadIdx.x & 63) >> lgMp) < d.B;
        if (real) {
            for (int r = 0; r < R; r++) {
                const int k = L.jm + (r << lgMp);
                if (k < Q.n_thr) {
                    const int64_t at = (c * Q.n_thr + k) * d.B + L.b;
                    Q.count[at] = (int32_t)__float_as_uint(slot[r * 192 + 64]);
                    Q.volume[at] = slot[r * 192 + 128];
                }
            }
        }
    }
    if (L.leader) {
        if constexpr (STATS) {
            const int64_t at = c * d.B + L.b;
            const PopStatsArgs &S = stats_args(Q);
            pp.cost[at] = bs.cost;
            S.s1[at] = bs.s1;
            S.s2[at] = bs.s2;
            S.s3[at] = bs.s3;
            if constexpr (JOINT) {
                if (has_aux) {
                    const PopJointArgs &J = joint_args(Q);
                    J.aux_sse[at] = ax.sse;
                    J.aux_s1[at] = ax.s1;
                    J.aux_s2[at] = ax.s2;
                    J.aux_s3[at] = ax.s3;
                }
            }
        } else pp.cost[c * d.B + L.b] = bs.cost;
    }
}

} // namespace hbvx

#endif // __HIPCC__
