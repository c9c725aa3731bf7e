// launch_pop.hip -- the entry points of the population evaluation: hbvx_population_cost, hbvx_population_stats,
// hbvx_population_joint and hbvx_population_period (hbv_pop.h), the flow-duration call hbvx_population_fdc
// (include/hbvx_pop_fdc.h; k_pop's FDC form), the flood-event call hbvx_population_events (include/hbvx_pop_events.h;
// k_pop's event form), the ensemble call hbvx_population_ensemble (include/hbvx_pop_ens.h; k_pop's ensemble form), and the
// implicit scheme's hbvx_adj_population_cost,
// hbvx_adj_population_stats and hbvx_adj_population_period (hbv_adj_pop.h).
#include "hbvx_host.h"
#include "../../include/hbvx_pop_fdc.h"
#include "../../include/hbvx_pop_events.h"
#include "../../include/hbvx_pop_ens.h"
#include "hbv_pop.h"
#define HBVX_CHUNK_NO_SHARED_KERNELS
#include "hbv_chunked.h"        // (first: hbv_adj_kernels.h uses its XCD-aware block map)
#include "hbv_adj_pop.h"

using namespace hbvx;
using namespace hbvx_host;

namespace {

int fail_as(const char *who, int code, const char *msg)
{
    char text[160];
    snprintf(text, sizeof text, "%s: %s", who, msg);
    return fail(code, text);
}

// The argument checks all entry points share, and the kernel's arguments; `who` names the entry point in the messages.
// adj: the implicit scheme's entry points -- the model test, and what check_adj (launch_adj.hip) asks of the Newton policy.
// need_target: false where the call scores no day (a window of the ensemble form before t_first) and reads no target.
int prepare(const char *who, const hbvx_desc *d, const hbvx_pop *pop, PopArgs &a, bool adj = false, bool need_target = true)
{
    if (adj) {
        if (d->model != HBVX_MODEL_HBVADJ) return fail_as(who, HBVX_E_UNSUPPORTED, "the implicit scheme (HBVADJ) only");
        if (!(d->adj_gtol >= 0.0f) || d->adj_max_iter < 0 || d->adj_max_iter > 64)
            return fail_as(who, HBVX_E_SHAPE, "bad Newton policy (adj_gtol / adj_max_iter)");
        if (d->adj_stop < 0 || d->adj_stop > 2) return fail_as(who, HBVX_E_SHAPE, "adj_stop must be 0, 1 or 2");
        if (d->adj_stop == 1)
            return fail_as(who, HBVX_E_UNSUPPORTED, "adj_stop = 1 (the batch-wide stopping rule) would make a candidate's "
                                                    "cost depend on the lanes that share its wave");
        if (d->muwts) return fail_as(who, HBVX_E_UNSUPPORTED, "muwts must be NULL (the implicit scheme has no ensemble weights)");
    } else if (d->model != HBVX_MODEL_HBV10 && d->model != HBVX_MODEL_HBV11P && d->model != HBVX_MODEL_HBV20)
        return fail_as(who, HBVX_E_UNSUPPORTED, "HBV 1.0 / 1.1p / 2.0 only");
    if (!pop->target && need_target) return fail_as(who, HBVX_E_NULL, "target is NULL");
    if (!pop->cost) return fail_as(who, HBVX_E_NULL, "cost is NULL");
    if (pop->n_cand < 1 || pop->n_cand > 65535) return fail_as(who, HBVX_E_SHAPE, "n_cand must be in 1..65535");
    if (pop->t_first < 0 || pop->t_first >= d->T) return fail_as(who, HBVX_E_SHAPE, "t_first outside the call's days");
    for (int i = d->n_param; i < HBVX_MAX_PARAM; i++)
        if (pop->p[i].sta) return fail_as(who, HBVX_E_SHAPE, "candidate values for a parameter slot the model lacks");
    memset(&a.r, 0, sizeof a.r);
    a.has_route = 0;
    if (const hbvx_route_desc *r = pop->route) {
        if (r->abi_version != HBVX_ABI_VERSION) return fail_as(who, HBVX_E_ABI, "route abi_version mismatch");
        if (r->L != (d->T < HBVX_UH_MAXLEN ? d->T : HBVX_UH_MAXLEN)) return fail_as(who, HBVX_E_SHAPE, "route L must be min(T, 15)");
        if (r->T != d->T || r->B != d->B) return fail_as(who, HBVX_E_SHAPE, "route T / B differ from the descriptor's");
        if ((!pop->ra && !r->ra) || (!pop->rb && !r->rb))
            return fail_as(who, HBVX_E_NULL, "a routing input is neither in pop nor in route");
        a.r = *r;
        a.has_route = 1;
    }
    a.d = *d;
    a.pop = *pop;
    a.pop.route = nullptr;      // a host pointer: the kernel reads its copy in a.r
    a.lgMp = lg_members(d->M);
    return HBVX_OK;
}

// The stats entry points' own checks and arguments, after prepare.
int prepare_stats(const char *who, const hbvx_pop_stats *ps, PopStatsArgs &s)
{
    if (ps->transform != HBVX_POP_T_NONE && ps->transform != HBVX_POP_T_SQRT && ps->transform != HBVX_POP_T_LOG)
        return fail_as(who, HBVX_E_UNSUPPORTED, "transform must be HBVX_POP_T_NONE, _SQRT or _LOG");
    if (!ps->shift) return fail_as(who, HBVX_E_NULL, "shift is NULL");
    if (ps->transform == HBVX_POP_T_LOG && !ps->eps) return fail_as(who, HBVX_E_NULL, "eps is NULL under HBVX_POP_T_LOG");
    if (!ps->s1 || !ps->s2 || !ps->s3) return fail_as(who, HBVX_E_NULL, "s1 / s2 / s3 is NULL");
    s.shift = ps->shift;
    s.eps = ps->eps;
    s.s1 = ps->s1;
    s.s2 = ps->s2;
    s.s3 = ps->s3;
    return HBVX_OK;
}

// The aux term's checks and arguments, after prepare_stats.  series_ok: whether the entry point scores pj->aux_series
// (the explicit models a flux, the implicit scheme a storage); series_msg: what it says when not.
int prepare_aux(const char *who, const hbvx_pop_joint *pj, bool series_ok, const char *series_msg, PopJointArgs &j)
{
    if (!series_ok) return fail_as(who, HBVX_E_UNSUPPORTED, series_msg);
    if (!pj->aux_target) return fail_as(who, HBVX_E_NULL, "aux_target is NULL");
    if (!pj->aux_shift) return fail_as(who, HBVX_E_NULL, "aux_shift is NULL");
    if (!pj->aux_sse || !pj->aux_s1 || !pj->aux_s2 || !pj->aux_s3)
        return fail_as(who, HBVX_E_NULL, "aux_sse / aux_s1 / aux_s2 / aux_s3 is NULL");
    j.aux_series = pj->aux_series;
    j.aux_target = pj->aux_target;
    j.aux_w = pj->aux_w;
    j.aux_shift = pj->aux_shift;
    j.aux_sse = pj->aux_sse;
    j.aux_s1 = pj->aux_s1;
    j.aux_s2 = pj->aux_s2;
    j.aux_s3 = pj->aux_s3;
    j.aux_sim = pj->aux_sim;
    return HBVX_OK;
}

bool is_aux_flux(int series)        // the fluxes the explicit models score as an aux term
{
    switch (series) {
    case HBVX_F_Q0: case HBVX_F_Q1: case HBVX_F_Q2: case HBVX_F_AET: case HBVX_F_SWE: return true;
    default: return false;
    }
}

// Everything the period entry points check after `pq`, and the kernel's arguments.
int prepare_period(const char *who, const hbvx_desc *d, const hbvx_pop_period *pq, PopPeriodArgs &q, bool adj)
{
    const hbvx_pop_joint *pj = &pq->joint;
    PopJointArgs &j = q.j;
    int rc = prepare(who, d, &pj->flow.pop, j.s.a, adj);
    if (rc) return rc;
    rc = prepare_stats(who, &pj->flow, j.s);
    if (rc) return rc;
    const int t_out = d->T - pj->flow.pop.t_first;
    if (!pq->flow_end) return fail_as(who, HBVX_E_NULL, "flow_end is NULL");
    if (pq->n_flow_periods < 1 || pq->n_flow_periods > t_out)
        return fail_as(who, HBVX_E_SHAPE, "n_flow_periods must be in 1..T - t_first");
    q.has_aux = pj->aux_series != HBVX_POP_NO_AUX;
    j = PopJointArgs{j.s, pj->aux_series, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    q.n_flow = pq->n_flow_periods;
    q.flow_end = pq->flow_end;
    q.n_aux = 0;
    q.aux_end = nullptr;
    if (q.has_aux) {
        if (adj)
            rc = prepare_aux(who, pj, pj->aux_series >= HBVX_ADJ_AUX_SNOWPACK && pj->aux_series <= HBVX_ADJ_AUX_SLZ,
                             "aux_series must be HBVX_POP_NO_AUX or HBVX_ADJ_AUX_SNOWPACK .. _SLZ (a storage index 0..4)", j);
        else
            rc = prepare_aux(who, pj, is_aux_flux(pj->aux_series),
                             "aux_series must be HBVX_POP_NO_AUX or HBVX_F_Q0, _Q1, _Q2, _AET or _SWE", j);
        if (rc) return rc;
        if (!pq->aux_end) return fail_as(who, HBVX_E_NULL, "aux_end is NULL");
        if (pq->n_aux_periods < 1 || pq->n_aux_periods > t_out)
            return fail_as(who, HBVX_E_SHAPE, "n_aux_periods must be in 1..T - t_first");
        q.n_aux = pq->n_aux_periods;
        q.aux_end = pq->aux_end;
    }
    return HBVX_OK;
}

// The template instance of a transform: f(TR) with TR one of hbvx_popk::T_* as std::integral_constant, as with_model
// (hbvx_host.h).  prepare_stats has checked the value.
template <typename F>
auto with_transform(int transform, F &&f)
{
    switch (transform) {
    case HBVX_POP_T_SQRT: return f(std::integral_constant<int, hbvx_popk::T_SQRT>{});
    case HBVX_POP_T_LOG: return f(std::integral_constant<int, hbvx_popk::T_LOG>{});
    default: return f(std::integral_constant<int, hbvx_popk::T_NONE>{});
    }
}

dim3 pop_grid(const PopArgs &a)
{
    const int bpw = 64 >> a.lgMp;
    return dim3((a.d.B + bpw - 1) / bpw, a.pop.n_cand);
}

int launched(const char *who)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) return HBVX_OK;
    char what[64];
    snprintf(what, sizeof what, "%s launch", who);
    return hip_fail(e, what);
}

// The explicit models: k_pop's instance for the descriptor's model, TR (T_COST for PopArgs) and the form Args.  lds: the
// launch's dynamic LDS in bytes (the FDC form's slots; nothing in the others).
template <int TR, typename Args>
int launch_pop(const char *who, const Args &args, void *stream, unsigned lds = 0)
{
    const PopArgs &a = pop_args(args);
    const dim3 grid = pop_grid(a);
    with_model(&a.d, [&](auto m, auto be) {
        if constexpr (m != MODEL_HOURLY)
            hipLaunchKernelGGL((k_pop<m, be, TR, Args>), grid, dim3(64), lds, (hipStream_t)stream, args);
    });
    return launched(who);
}

// The implicit scheme: k_adj_pop's instance for the descriptor's parameter count and "few" mode (hbv_adj_kernels.h:
// whether the call has at most ADJ_FEW dynamic parameters, and then their slot list), TR, AUX and the form Args.
template <int TR, bool AUX, typename Args>
int launch_adj_pop(const char *who, const Args &args, void *stream)
{
    const PopArgs &a = pop_args(args);
    AdjFew few{};
    const bool is_few = count_dyn(&a.d) <= ADJ_FEW;
    if (is_few)
        for (int i = 0; i < a.d.n_param; i++)
            if (a.d.p[i].dyn) few.slot[few.nd++] = i;
    const dim3 grid = pop_grid(a);
    with_adj(&a.d, is_few, [&](auto be, auto fw) {
        hipLaunchKernelGGL((k_adj_pop<be, fw, TR, AUX, Args>), grid, dim3(64), 0, (hipStream_t)stream, args, few);
    });
    return launched(who);
}

} // namespace

extern "C" int hbvx_population_cost(const hbvx_desc *d, const hbvx_pop *pop, void *stream)
{
    const char *who = "hbvx_population_cost";
    int rc = check_desc(d);
    if (rc) return rc;
    if (!pop) return fail_as(who, HBVX_E_NULL, "pop is NULL");
    PopArgs a;
    rc = prepare(who, d, pop, a);
    if (rc) return rc;
    return launch_pop<T_COST>(who, a, stream);
}

extern "C" int hbvx_population_stats(const hbvx_desc *d, const hbvx_pop_stats *ps, void *stream)
{
    const char *who = "hbvx_population_stats";
    int rc = check_desc(d);
    if (rc) return rc;
    if (!ps) return fail_as(who, HBVX_E_NULL, "ps is NULL");
    PopStatsArgs s;
    rc = prepare(who, d, &ps->pop, s.a);
    if (rc) return rc;
    rc = prepare_stats(who, ps, s);
    if (rc) return rc;
    return with_transform(ps->transform, [&](auto tr) { return launch_pop<tr>(who, s, stream); });
}

extern "C" int hbvx_population_joint(const hbvx_desc *d, const hbvx_pop_joint *pj, void *stream)
{
    const char *who = "hbvx_population_joint";
    int rc = check_desc(d);
    if (rc) return rc;
    if (!pj) return fail_as(who, HBVX_E_NULL, "pj is NULL");
    PopJointArgs j;
    rc = prepare(who, d, &pj->flow.pop, j.s.a);
    if (rc) return rc;
    rc = prepare_stats(who, &pj->flow, j.s);
    if (rc) return rc;
    rc = prepare_aux(who, pj, is_aux_flux(pj->aux_series), "aux_series must be HBVX_F_Q0, _Q1, _Q2, _AET or _SWE", j);
    if (rc) return rc;
    return with_transform(pj->flow.transform, [&](auto tr) { return launch_pop<tr>(who, j, stream); });
}

extern "C" int hbvx_population_period(const hbvx_desc *d, const hbvx_pop_period *pq, void *stream)
{
    const char *who = "hbvx_population_period";
    int rc = check_desc(d);
    if (rc) return rc;
    if (!pq) return fail_as(who, HBVX_E_NULL, "pq is NULL");
    PopPeriodArgs q;
    rc = prepare_period(who, d, pq, q, false);
    if (rc) return rc;
    return with_transform(pq->joint.flow.transform, [&](auto tr) { return launch_pop<tr>(who, q, stream); });
}

static_assert(HBVX_POP_FDC_MAX_THR == hbvx_popk::FDC_MAX_THR, "the header's limit and the kernel's");

extern "C" uint64_t hbvx_pop_fdc_sizeof(int which) { return which == 0 ? sizeof(hbvx_pop_fdc) : 0; }

extern "C" int hbvx_population_fdc(const hbvx_desc *d, const hbvx_pop_fdc *pf, void *stream)
{
    const char *who = "hbvx_population_fdc";
    int rc = check_desc(d);
    if (rc) return rc;
    if (!pf) return fail_as(who, HBVX_E_NULL, "pf is NULL");
    if (pf->abi_version != HBVX_POP_FDC_ABI_VERSION) return fail_as(who, HBVX_E_ABI, "pf abi_version mismatch");
    PopFdcArgs f;
    rc = prepare(who, d, &pf->flow.pop, f.s.a);        // (refuses HBVX_MODEL_HBVADJ and HBVX_MODEL_HOURLY)
    if (rc) return rc;
    rc = prepare_stats(who, &pf->flow, f.s);
    if (rc) return rc;
    if (pf->n_thr < 1 || pf->n_thr > HBVX_POP_FDC_MAX_THR) return fail_as(who, HBVX_E_SHAPE, "n_thr must be in 1..32");
    if (!pf->thr) return fail_as(who, HBVX_E_NULL, "thr is NULL");
    if (!pf->count || !pf->volume) return fail_as(who, HBVX_E_NULL, "count / volume is NULL");
    f.n_thr = pf->n_thr;
    f.thr = pf->thr;
    f.count = pf->count;
    f.volume = pf->volume;
    // at most 32 slots of 768 bytes: 24 KB, under the 64 KB a launch may ask for without an attribute
    const unsigned lds = fdc_lds_bytes(f.n_thr, f.s.a.lgMp);
    return with_transform(pf->flow.transform, [&](auto tr) { return launch_pop<tr>(who, f, stream, lds); });
}

extern "C" uint64_t hbvx_pop_events_sizeof(int which) { return which == 0 ? sizeof(hbvx_pop_events) : 0; }

extern "C" int hbvx_population_events(const hbvx_desc *d, const hbvx_pop_events *pe, void *stream)
{
    const char *who = "hbvx_population_events";
    int rc = check_desc(d);
    if (rc) return rc;
    if (!pe) return fail_as(who, HBVX_E_NULL, "pe is NULL");
    if (pe->abi_version != HBVX_POP_EVENTS_ABI_VERSION) return fail_as(who, HBVX_E_ABI, "pe abi_version mismatch");
    PopEventArgs ev;
    rc = prepare(who, d, &pe->flow.pop, ev.s.a);        // (refuses HBVX_MODEL_HBVADJ and HBVX_MODEL_HOURLY)
    if (rc) return rc;
    rc = prepare_stats(who, &pe->flow, ev.s);
    if (rc) return rc;
    if (pe->n_events < 1 || pe->n_events > d->T - pe->flow.pop.t_first)
        return fail_as(who, HBVX_E_SHAPE, "n_events must be in 1..T - t_first");
    if ((int64_t)pe->n_events * d->B > EVENT_MAX_CELLS) return fail_as(who, HBVX_E_SHAPE, "n_events * B must not exceed 2^30");
    if (!pe->start || !pe->end) return fail_as(who, HBVX_E_NULL, "start / end is NULL");
    if (!pe->peak || !pe->peak_day || !pe->volume) return fail_as(who, HBVX_E_NULL, "peak / peak_day / volume is NULL");
    ev.n_events = pe->n_events;
    ev.start = pe->start;
    ev.end = pe->end;
    ev.peak = pe->peak;
    ev.peak_day = pe->peak_day;
    ev.volume = pe->volume;
    return with_transform(pe->flow.transform, [&](auto tr) { return launch_pop<tr>(who, ev, stream); });
}

static_assert(HBVX_POP_ENS_HIST == hbvx_popk::UH - 1, "the header's history length and the kernel's");

// whether [a, a + na) and [b, b + nb) floats share an address (NULL shares nothing)
static bool ranges_overlap(const float *a, int64_t na, const float *b, int64_t nb)
{
    if (!a || !b) return false;
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + 4 * (uintptr_t)na, b0 = (uintptr_t)b, b1 = b0 + 4 * (uintptr_t)nb;
    return a0 < b1 && b0 < a1;
}

extern "C" int hbvx_population_ensemble(const hbvx_desc *d, const hbvx_pop_ens *pe, void *stream)
{
    const char *who = "hbvx_population_ensemble";
    int rc = check_desc(d);
    if (rc) return rc;
    if (!pe) return fail_as(who, HBVX_E_NULL, "pe is NULL");
    if (pe->t_begin < 0 || pe->t_begin >= pe->t_end || pe->t_end > d->T)
        return fail_as(who, HBVX_E_SHAPE, "the window must satisfy 0 <= t_begin < t_end <= T");
    const hbvx_pop *pop = &pe->s.pop;
    PopEnsArgs e;
    // a window that ends at or before t_first scores no day: no row of target / w / sim exists, the chains are +0
    rc = prepare(who, d, pop, e.s.a, false, pop->t_first < pe->t_end);     // (refuses HBVX_MODEL_HBVADJ and HBVX_MODEL_HOURLY)
    if (rc) return rc;
    rc = prepare_stats(who, &pe->s, e.s);
    if (rc) return rc;
    const int n_src = pe->n_src ? pe->n_src : pop->n_cand;
    if (n_src < 1 || pe->src_first < 0 || (!pe->ancestor && (int64_t)pe->src_first + pop->n_cand > n_src))
        return fail_as(who, HBVX_E_SHAPE, "n_src / src_first leave an identity ancestor outside 0..n_src-1");
    if (!pe->state_out) return fail_as(who, HBVX_E_NULL, "state_out is NULL");
    if (e.s.a.has_route && !pe->hist_out) return fail_as(who, HBVX_E_NULL, "hist_out is NULL in a call that routes");
    const int64_t N5 = 5 * (int64_t)d->B * d->M, H = (int64_t)HBVX_POP_ENS_HIST * d->B;
    if (ranges_overlap(pe->state_out, pop->n_cand * N5, pe->state_in, n_src * N5))
        return fail_as(who, HBVX_E_SHAPE, "state_out overlaps state_in");
    if (e.s.a.has_route && ranges_overlap(pe->hist_out, pop->n_cand * H, pe->hist_in, n_src * H))
        return fail_as(who, HBVX_E_SHAPE, "hist_out overlaps hist_in");
    e.t_begin = pe->t_begin;
    e.t_end = pe->t_end;
    e.n_src = n_src;
    e.src_first = pe->src_first;
    e.state_in = pe->state_in;
    e.state_out = pe->state_out;
    e.hist_in = pe->hist_in;
    e.hist_out = pe->hist_out;
    e.ancestor = pe->ancestor;
    e.p_mul = pe->p_mul;
    e.t_add = pe->t_add;
    e.pm_c_stride = pe->pm_c_stride;
    e.pm_t_stride = pe->pm_t_stride;
    e.ta_c_stride = pe->ta_c_stride;
    e.ta_t_stride = pe->ta_t_stride;
    return with_transform(pe->s.transform, [&](auto tr) { return launch_pop<tr>(who, e, stream); });
}

extern "C" int hbvx_adj_population_cost(const hbvx_desc *d, const hbvx_pop *pop, void *stream)
{
    const char *who = "hbvx_adj_population_cost";
    int rc = check_desc(d);
    if (rc) return rc;
    if (!pop) return fail_as(who, HBVX_E_NULL, "pop is NULL");
    PopStatsArgs s;
    rc = prepare(who, d, pop, s.a, true);
    if (rc) return rc;
    s.shift = s.eps = nullptr;
    s.s1 = s.s2 = s.s3 = nullptr;
    return launch_adj_pop<T_COST, false>(who, s, stream);
}

extern "C" int hbvx_adj_population_stats(const hbvx_desc *d, const hbvx_pop_stats *ps, void *stream)
{
    const char *who = "hbvx_adj_population_stats";
    int rc = check_desc(d);
    if (rc) return rc;
    if (!ps) return fail_as(who, HBVX_E_NULL, "ps is NULL");
    PopStatsArgs s;
    rc = prepare(who, d, &ps->pop, s.a, true);
    if (rc) return rc;
    rc = prepare_stats(who, ps, s);
    if (rc) return rc;
    return with_transform(ps->transform, [&](auto tr) { return launch_adj_pop<tr, false>(who, s, stream); });
}

extern "C" int hbvx_adj_population_period(const hbvx_desc *d, const hbvx_pop_period *pq, void *stream)
{
    const char *who = "hbvx_adj_population_period";
    int rc = check_desc(d);
    if (rc) return rc;
    if (!pq) return fail_as(who, HBVX_E_NULL, "pq is NULL");
    PopPeriodArgs q;
    rc = prepare_period(who, d, pq, q, true);
    if (rc) return rc;
    return with_transform(pq->joint.flow.transform, [&](auto tr) {
        return q.has_aux ? launch_adj_pop<tr, true>(who, q, stream) : launch_adj_pop<tr, false>(who, q, stream);
    });
}

// Diagnostics (tests only): the transform as the kernel applies it -- BasinStats::transform on the device.
template <int TR>
__global__ void k_selftest_pop_transform(const float *y, const float *eps, float *out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    hbvx_popk::BasinStats bs;
    bs.start(false, 0.0f, TR == hbvx_popk::T_LOG ? eps[i] : 0.0f);
    out[i] = bs.transform<TR>(y[i]);
}

extern "C" int hbvx_selftest_pop_transform(const float *y, const float *eps, float *out, int n, int transform, void *stream)
{
    if (!y || !out || n <= 0 || transform < HBVX_POP_T_NONE || transform > HBVX_POP_T_LOG || (transform == HBVX_POP_T_LOG && !eps))
        return fail(HBVX_E_NULL, "selftest_pop_transform: bad arguments");
    const dim3 grid((n + 255) / 256), block(256);
    with_transform(transform, [&](auto tr) {
        hipLaunchKernelGGL(k_selftest_pop_transform<tr>, grid, block, 0, (hipStream_t)stream, y, eps, out, n);
    });
    return launched("selftest_pop_transform");
}
