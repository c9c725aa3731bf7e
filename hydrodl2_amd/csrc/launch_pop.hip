// launch_pop.hip -- the entry points of the population evaluation: hbvx_population_cost, hbvx_population_stats and
// hbvx_population_joint (hbv_pop.h), hbvx_population_period (hbv_pop_period.h), and the first two's twins for the implicit scheme, hbvx_adj_population_cost and hbvx_adj_population_stats
// (hbv_adj_pop.h), and hbvx_adj_population_period (hbv_adj_pop_period.h).
#include "hbvx_host.h"
#include "hbv_pop.h"
#include "hbv_pop_period.h"
#define HBVX_CHUNK_NO_SHARED_KERNELS
#include "hbv_chunked.h"        // (first: hbv_adj_kernels.h uses its XCD-aware block map)
#include "hbv_adj_pop.h"
#include "hbv_adj_pop_period.h"

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
int prepare(const char *who, const hbvx_desc *d, const hbvx_pop *pop, PopArgs &a, bool adj = false)
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
    if (!pop->target) return fail_as(who, HBVX_E_NULL, "target is NULL");
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

dim3 pop_grid(const PopArgs &a)
{
    const int bpw = 64 >> a.lgMp;
    return dim3((a.d.B + bpw - 1) / bpw, a.pop.n_cand);
}

} // namespace

extern "C" int hbvx_population_cost(const hbvx_desc *d, const hbvx_pop *pop, void *stream)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (!pop) return fail(HBVX_E_NULL, "hbvx_population_cost: pop is NULL");
    PopArgs a;
    rc = prepare("hbvx_population_cost", d, pop, a);
    if (rc) return rc;
    const dim3 grid = pop_grid(a);
    with_model(d, [&](auto m, auto be) {
        if constexpr (m != MODEL_HOURLY)
            hipLaunchKernelGGL((k_pop<m, be>), grid, dim3(64), 0, (hipStream_t)stream, a);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_population_cost launch");
    return HBVX_OK;
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
    const dim3 grid = pop_grid(s.a);
    with_model(d, [&](auto m, auto be) {
        if constexpr (m != MODEL_HOURLY) {
            switch (ps->transform) {
            case HBVX_POP_T_SQRT:
                hipLaunchKernelGGL((k_pop_stats<m, be, hbvx_popk::T_SQRT>), grid, dim3(64), 0, (hipStream_t)stream, s);
                break;
            case HBVX_POP_T_LOG:
                hipLaunchKernelGGL((k_pop_stats<m, be, hbvx_popk::T_LOG>), grid, dim3(64), 0, (hipStream_t)stream, s);
                break;
            default:
                hipLaunchKernelGGL((k_pop_stats<m, be, hbvx_popk::T_NONE>), grid, dim3(64), 0, (hipStream_t)stream, s);
            }
        }
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_population_stats launch");
    return HBVX_OK;
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
    switch (pj->aux_series) {
    case HBVX_F_Q0: case HBVX_F_Q1: case HBVX_F_Q2: case HBVX_F_AET: case HBVX_F_SWE: break;
    default: return fail_as(who, HBVX_E_UNSUPPORTED, "aux_series must be HBVX_F_Q0, _Q1, _Q2, _AET or _SWE");
    }
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
    const dim3 grid = pop_grid(j.s.a);
    with_model(d, [&](auto m, auto be) {
        if constexpr (m != MODEL_HOURLY) {
            switch (pj->flow.transform) {
            case HBVX_POP_T_SQRT:
                hipLaunchKernelGGL((k_pop_joint<m, be, hbvx_popk::T_SQRT>), grid, dim3(64), 0, (hipStream_t)stream, j);
                break;
            case HBVX_POP_T_LOG:
                hipLaunchKernelGGL((k_pop_joint<m, be, hbvx_popk::T_LOG>), grid, dim3(64), 0, (hipStream_t)stream, j);
                break;
            default:
                hipLaunchKernelGGL((k_pop_joint<m, be, hbvx_popk::T_NONE>), grid, dim3(64), 0, (hipStream_t)stream, j);
            }
        }
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_population_joint launch");
    return HBVX_OK;
}

extern "C" int hbvx_population_period(const hbvx_desc *d, const hbvx_pop_period *pq, void *stream)
{
    const char *who = "hbvx_population_period";
    int rc = check_desc(d);
    if (rc) return rc;
    if (!pq) return fail_as(who, HBVX_E_NULL, "pq is NULL");
    const hbvx_pop_joint *pj = &pq->joint;
    PopPeriodArgs q;
    PopJointArgs &j = q.j;
    rc = prepare(who, d, &pj->flow.pop, j.s.a);
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
        switch (pj->aux_series) {
        case HBVX_F_Q0: case HBVX_F_Q1: case HBVX_F_Q2: case HBVX_F_AET: case HBVX_F_SWE: break;
        default:
            return fail_as(who, HBVX_E_UNSUPPORTED, "aux_series must be HBVX_POP_NO_AUX or HBVX_F_Q0, _Q1, _Q2, _AET or _SWE");
        }
        if (!pj->aux_target) return fail_as(who, HBVX_E_NULL, "aux_target is NULL");
        if (!pj->aux_shift) return fail_as(who, HBVX_E_NULL, "aux_shift is NULL");
        if (!pj->aux_sse || !pj->aux_s1 || !pj->aux_s2 || !pj->aux_s3)
            return fail_as(who, HBVX_E_NULL, "aux_sse / aux_s1 / aux_s2 / aux_s3 is NULL");
        if (!pq->aux_end) return fail_as(who, HBVX_E_NULL, "aux_end is NULL");
        if (pq->n_aux_periods < 1 || pq->n_aux_periods > t_out)
            return fail_as(who, HBVX_E_SHAPE, "n_aux_periods must be in 1..T - t_first");
        j.aux_target = pj->aux_target;
        j.aux_w = pj->aux_w;
        j.aux_shift = pj->aux_shift;
        j.aux_sse = pj->aux_sse;
        j.aux_s1 = pj->aux_s1;
        j.aux_s2 = pj->aux_s2;
        j.aux_s3 = pj->aux_s3;
        j.aux_sim = pj->aux_sim;
        q.n_aux = pq->n_aux_periods;
        q.aux_end = pq->aux_end;
    }
    const dim3 grid = pop_grid(j.s.a);
    with_model(d, [&](auto m, auto be) {
        if constexpr (m != MODEL_HOURLY) {
            switch (pj->flow.transform) {
            case HBVX_POP_T_SQRT:
                hipLaunchKernelGGL((k_pop_period<m, be, hbvx_popk::T_SQRT>), grid, dim3(64), 0, (hipStream_t)stream, q);
                break;
            case HBVX_POP_T_LOG:
                hipLaunchKernelGGL((k_pop_period<m, be, hbvx_popk::T_LOG>), grid, dim3(64), 0, (hipStream_t)stream, q);
                break;
            default:
                hipLaunchKernelGGL((k_pop_period<m, be, hbvx_popk::T_NONE>), grid, dim3(64), 0, (hipStream_t)stream, q);
            }
        }
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_population_period launch");
    return HBVX_OK;
}

// "Few" mode (hbv_adj_kernels.h): whether the call has at most ADJ_FEW dynamic parameters, and then their slot list
static bool adj_pop_few(const hbvx_desc *d, AdjFew &few)
{
    few = AdjFew{};
    if (count_dyn(d) > ADJ_FEW) return false;
    for (int i = 0; i < d->n_param; i++)
        if (d->p[i].dyn) few.slot[few.nd++] = i;
    return true;
}

template <int TR>
static void launch_adj_pop(const PopStatsArgs &s, void *stream)
{
    AdjFew few;
    const bool is_few = adj_pop_few(&s.a.d, few);
    const dim3 grid = pop_grid(s.a);
    with_adj(&s.a.d, is_few, [&](auto be, auto fw) {
        hipLaunchKernelGGL((k_adj_pop<be, fw, TR>), grid, dim3(64), 0, (hipStream_t)stream, s, few);
    });
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
    launch_adj_pop<T_COST>(s, stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_adj_population_cost launch");
    return HBVX_OK;
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
    switch (ps->transform) {
    case HBVX_POP_T_SQRT: launch_adj_pop<hbvx_popk::T_SQRT>(s, stream); break;
    case HBVX_POP_T_LOG: launch_adj_pop<hbvx_popk::T_LOG>(s, stream); break;
    default: launch_adj_pop<hbvx_popk::T_NONE>(s, stream);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_adj_population_stats launch");
    return HBVX_OK;
}

template <int TR, bool AUX>
static void launch_adj_pop_period(const PopPeriodArgs &q, void *stream)
{
    const PopArgs &a = q.j.s.a;
    AdjFew few;
    const bool is_few = adj_pop_few(&a.d, few);
    const dim3 grid = pop_grid(a);
    with_adj(&a.d, is_few, [&](auto be, auto fw) {
        hipLaunchKernelGGL((k_adj_pop_period<be, fw, TR, AUX>), grid, dim3(64), 0, (hipStream_t)stream, q, few);
    });
}

template <int TR>
static void launch_adj_pop_period(const PopPeriodArgs &q, void *stream)
{
    if (q.has_aux) launch_adj_pop_period<TR, true>(q, stream);
    else launch_adj_pop_period<TR, false>(q, stream);
}

extern "C" int hbvx_adj_population_period(const hbvx_desc *d, const hbvx_pop_period *pq, void *stream)
{
    const char *who = "hbvx_adj_population_period";
    int rc = check_desc(d);
    if (rc) return rc;
    if (!pq) return fail_as(who, HBVX_E_NULL, "pq is NULL");
    const hbvx_pop_joint *pj = &pq->joint;
    PopPeriodArgs q;
    PopJointArgs &j = q.j;
    rc = prepare(who, d, &pj->flow.pop, j.s.a, true);
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
        if (pj->aux_series < HBVX_ADJ_AUX_SNOWPACK || pj->aux_series > HBVX_ADJ_AUX_SLZ)
            return fail_as(who, HBVX_E_UNSUPPORTED, "aux_series must be HBVX_POP_NO_AUX or HBVX_ADJ_AUX_SNOWPACK .. _SLZ "
                                                    "(a storage index 0..4)");
        if (!pj->aux_target) return fail_as(who, HBVX_E_NULL, "aux_target is NULL");
        if (!pj->aux_shift) return fail_as(who, HBVX_E_NULL, "aux_shift is NULL");
        if (!pj->aux_sse || !pj->aux_s1 || !pj->aux_s2 || !pj->aux_s3)
            return fail_as(who, HBVX_E_NULL, "aux_sse / aux_s1 / aux_s2 / aux_s3 is NULL");
        if (!pq->aux_end) return fail_as(who, HBVX_E_NULL, "aux_end is NULL");
        if (pq->n_aux_periods < 1 || pq->n_aux_periods > t_out)
            return fail_as(who, HBVX_E_SHAPE, "n_aux_periods must be in 1..T - t_first");
        j.aux_target = pj->aux_target;
        j.aux_w = pj->aux_w;
        j.aux_shift = pj->aux_shift;
        j.aux_sse = pj->aux_sse;
        j.aux_s1 = pj->aux_s1;
        j.aux_s2 = pj->aux_s2;
        j.aux_s3 = pj->aux_s3;
        j.aux_sim = pj->aux_sim;
        q.n_aux = pq->n_aux_periods;
        q.aux_end = pq->aux_end;
    }
    switch (pj->flow.transform) {
    case HBVX_POP_T_SQRT: launch_adj_pop_period<hbvx_popk::T_SQRT>(q, stream); break;
    case HBVX_POP_T_LOG: launch_adj_pop_period<hbvx_popk::T_LOG>(q, stream); break;
    default: launch_adj_pop_period<hbvx_popk::T_NONE>(q, stream);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_adj_population_period launch");
    return HBVX_OK;
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
    if (transform == HBVX_POP_T_SQRT)
        hipLaunchKernelGGL(k_selftest_pop_transform<hbvx_popk::T_SQRT>, grid, block, 0, (hipStream_t)stream, y, eps, out, n);
    else if (transform == HBVX_POP_T_LOG)
        hipLaunchKernelGGL(k_selftest_pop_transform<hbvx_popk::T_LOG>, grid, block, 0, (hipStream_t)stream, y, eps, out, n);
    else
        hipLaunchKernelGGL(k_selftest_pop_transform<hbvx_popk::T_NONE>, grid, block, 0, (hipStream_t)stream, y, eps, out, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "selftest_pop_transform launch");
    return HBVX_OK;
}
