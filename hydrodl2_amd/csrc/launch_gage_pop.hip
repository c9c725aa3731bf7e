// launch_gage_pop.hip -- the entry points of the hourly model's population evaluation (include/hbvx_gage_pop.h):
// hbvx_hourly_population_runoff (k_pop's runoff form, hbv_pop.h) and hbvx_gage_population_stats (hbv_gage_pop.h), and of
// the event statistics on the latter's series (include/hbvx_gage_events.h): hbvx_gage_population_events (k_gp_events),
// and of the flow-duration statistics on it (include/hbvx_gage_fdc.h): hbvx_gage_population_fdc (k_gp_fdc) and
// hbvx_gage_population_quantiles (k_gp_keys, k_gp_quant).
#include "hbvx_host.h"
#include "hbv_gage_pop.h"

using namespace hbvx;
using namespace hbvx_host;

namespace {

int fail_as(const char *who, int code, const char *msg)
{
    char text[160];
    snprintf(text, sizeof text, "%s: %s", who, msg);
    return fail(code, text);
}

int launched(const char *who)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) return HBVX_OK;
    char what[64];
    snprintf(what, sizeof what, "%s launch", who);
    return hip_fail(e, what);
}

// What hbvx_gage_route_forward checks of its descriptor (hbvx.hip), without r->dp: the candidates bring their own.
int check_gage(const char *who, const hbvx_gage_desc *r)
{
    if (!r) return fail_as(who, HBVX_E_NULL, "gage desc is NULL");
    if (r->abi_version != HBVX_ABI_VERSION) return fail_as(who, HBVX_E_ABI, "abi_version mismatch");
    if (r->T <= 0 || r->U <= 0 || r->G <= 0 || r->NPAIR < 0) return fail_as(who, HBVX_E_SHAPE, "bad T/U/G/NPAIR");
    const int L = r->T < HBVX_GAGE_MAXLEN ? r->T : HBVX_GAGE_MAXLEN;
    if (r->L != L) return fail_as(who, HBVX_E_SHAPE, "L must be min(T, 72)");
    if (r->U > 65535 || r->G > 65535) return fail_as(who, HBVX_E_SHAPE, "more than 65535 units or gages per call");
    if (!r->pair_unit || !r->gage_ptr || !r->areas || !r->denom)
        return fail_as(who, HBVX_E_NULL, "gage routing pointer is NULL");
    return HBVX_OK;
}

int check_gage_pop(const char *who, const hbvx_gage_desc *r, const hbvx_gage_pop *gp)
{
    int rc = check_gage(who, r);
    if (rc) return rc;
    if (!gp) return fail_as(who, HBVX_E_NULL, "gp is NULL");
    if (gp->abi_version != HBVX_GAGE_POP_ABI_VERSION) return fail_as(who, HBVX_E_ABI, "gp abi_version mismatch");
    if (gp->n_cand < 1 || gp->n_cand > 65535) return fail_as(who, HBVX_E_SHAPE, "n_cand must be in 1..65535");
    if (!gp->runoff) return fail_as(who, HBVX_E_NULL, "runoff is NULL");
    if (gp->runoff_c_stride < 0) return fail_as(who, HBVX_E_SHAPE, "runoff_c_stride is negative");
    if (!gp->dp && !gp->uh && r->NPAIR > 0) return fail_as(who, HBVX_E_NULL, "neither dp nor uh is given");
    if (gp->transform != HBVX_POP_T_NONE && gp->transform != HBVX_POP_T_SQRT && gp->transform != HBVX_POP_T_LOG)
        return fail_as(who, HBVX_E_UNSUPPORTED, "transform must be HBVX_POP_T_NONE, _SQRT or _LOG");
    if (gp->n_periods < 1 || gp->n_periods > r->T) return fail_as(who, HBVX_E_SHAPE, "n_periods must be in 1..T");
    if (!gp->period_end) return fail_as(who, HBVX_E_NULL, "period_end is NULL");
    if (!gp->target) return fail_as(who, HBVX_E_NULL, "target is NULL");
    if (!gp->shift) return fail_as(who, HBVX_E_NULL, "shift is NULL");
    if (gp->transform == HBVX_POP_T_LOG && !gp->eps) return fail_as(who, HBVX_E_NULL, "eps is NULL under HBVX_POP_T_LOG");
    if (!gp->sse || !gp->s1 || !gp->s2 || !gp->s3) return fail_as(who, HBVX_E_NULL, "sse / s1 / s2 / s3 is NULL");
    return HBVX_OK;
}

int check_gage_events(const char *who, const hbvx_gage_events *ev)
{
    if (!ev) return fail_as(who, HBVX_E_NULL, "ev is NULL");
    if (ev->abi_version != HBVX_GAGE_EVENTS_ABI_VERSION) return fail_as(who, HBVX_E_ABI, "ev abi_version mismatch");
    if (ev->n_cand < 1 || ev->n_cand > 65535) return fail_as(who, HBVX_E_SHAPE, "n_cand must be in 1..65535");
    if (ev->T < 1 || ev->G < 1) return fail_as(who, HBVX_E_SHAPE, "bad T/G");
    if (ev->n_events < 1 || ev->n_events > ev->T) return fail_as(who, HBVX_E_SHAPE, "n_events must be in 1..T");
    if (!ev->series) return fail_as(who, HBVX_E_NULL, "series is NULL");
    if (!ev->start || !ev->end) return fail_as(who, HBVX_E_NULL, "start / end is NULL");
    if (!ev->peak || !ev->peak_hour || !ev->volume) return fail_as(who, HBVX_E_NULL, "peak / peak_hour / volume is NULL");
    return HBVX_OK;
}

static_assert(HBVX_GAGE_FDC_MAX_LEV == hbvx_popk::FDC_MAX_THR && HBVX_GAGE_FDC_MAX_LEV == HBVX_POP_FDC_MAX_THR,
              "the gage FDC call and the daily one share one limit on the levels");
static_assert(HBVX_GAGE_FDC_MAX_LEV <= gagepop::QUANT_THREADS, "k_gp_quant gathers one rank per thread");
static_assert((uint64_t)HBVX_GAGE_QUANT_MAX_T * sizeof(uint32_t) <= 65536, "the padded column must fit 64 KB of LDS");

// What both exports of include/hbvx_gage_fdc.h check of the struct they share.
int check_gage_fdc(const char *who, const hbvx_gage_fdc *gf)
{
    if (!gf) return fail_as(who, HBVX_E_NULL, "gf is NULL");
    if (gf->abi_version != HBVX_GAGE_FDC_ABI_VERSION) return fail_as(who, HBVX_E_ABI, "gf abi_version mismatch");
    if (gf->n_cand < 1 || gf->n_cand > 65535) return fail_as(who, HBVX_E_SHAPE, "n_cand must be in 1..65535");
    if (gf->T < 1 || gf->G < 1) return fail_as(who, HBVX_E_SHAPE, "bad T/G");
    if (gf->n_lev < 1 || gf->n_lev > HBVX_GAGE_FDC_MAX_LEV) return fail_as(who, HBVX_E_SHAPE, "n_lev must be in 1..32");
    if (!gf->series) return fail_as(who, HBVX_E_NULL, "series is NULL");
    if (!gf->scored) return fail_as(who, HBVX_E_NULL, "scored is NULL");
    return HBVX_OK;
}

// The candidates of one launch whose grid has `blocks` workgroups of `threads` threads per candidate: as many as keep the
// launch below 2^32 threads (and a grid dimension); 0 if one candidate alone does not fit.
int cands_per_launch(uint64_t blocks, uint64_t threads, int n_cand)
{
    const uint64_t budget = 0xFFFFFFFFull / (blocks * threads);
    return budget < (uint64_t)n_cand ? (int)budget : n_cand;
}

// the workspace's three parts, in floats
struct Plan {
    uint64_t qsT, uh, series;
};

Plan plan(const hbvx_gage_desc *r, const hbvx_gage_pop *gp)
{
    const uint64_t P = (uint64_t)gp->n_cand;
    Plan pl;
    pl.qsT = (gp->runoff_c_stride ? P : 1) * (uint64_t)r->U * r->T;
    pl.uh = gp->dp ? P * (uint64_t)r->NPAIR * r->L : 0;
    pl.series = gp->series ? 0 : P * (uint64_t)r->T * r->G;
    return pl;
}

} // namespace

extern "C" uint64_t hbvx_gage_pop_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(hbvx_pop_runoff);
    case 1: return sizeof(hbvx_gage_pop);
    default: return 0;
    }
}

extern "C" int hbvx_hourly_population_runoff(const hbvx_desc *d, const hbvx_pop_runoff *pr, void *stream)
{
    const char *who = "hbvx_hourly_population_runoff";
    int rc = check_desc(d);
    if (rc) return rc;
    if (d->model != HBVX_MODEL_HOURLY) return fail_as(who, HBVX_E_UNSUPPORTED, "the hourly model (HBVX_MODEL_HOURLY) only");
    if (!pr) return fail_as(who, HBVX_E_NULL, "pr is NULL");
    if (pr->abi_version != HBVX_GAGE_POP_ABI_VERSION) return fail_as(who, HBVX_E_ABI, "pr abi_version mismatch");
    if (pr->n_cand < 1 || pr->n_cand > 65535) return fail_as(who, HBVX_E_SHAPE, "n_cand must be in 1..65535");
    if (!pr->runoff) return fail_as(who, HBVX_E_NULL, "runoff is NULL");
    for (int i = d->n_param; i < HBVX_MAX_PARAM; i++)
        if (pr->p[i].sta) return fail_as(who, HBVX_E_SHAPE, "candidate values for a parameter slot the model lacks");
    PopRunoffArgs q;
    memset(&q, 0, sizeof q);
    q.a.d = *d;
    q.a.pop.n_cand = pr->n_cand;
    for (int i = 0; i < HBVX_MAX_PARAM; i++) q.a.pop.p[i] = pr->p[i];
    q.a.lgMp = lg_members(d->M);
    q.runoff = pr->runoff;
    const int bpw = 64 >> q.a.lgMp;
    const dim3 grid((d->B + bpw - 1) / bpw, pr->n_cand);
    hipLaunchKernelGGL((k_pop<MODEL_HOURLY, true, T_COST, PopRunoffArgs>), grid, dim3(64), 0, (hipStream_t)stream, q);
    return launched(who);
}

extern "C" uint64_t hbvx_gage_population_workspace_bytes(const hbvx_gage_desc *r, const hbvx_gage_pop *gp)
{
    if (!r || !gp || r->T <= 0 || r->U <= 0 || r->G <= 0 || r->NPAIR < 0 || r->L <= 0 || gp->n_cand < 1 || gp->n_cand > 65535)
        return 0;
    const Plan pl = plan(r, gp);
    return (pl.qsT + pl.uh + pl.series) * sizeof(float);
}

extern "C" int hbvx_gage_population_stats(const hbvx_gage_desc *r, const hbvx_gage_pop *gp, void *workspace,
                                          uint64_t workspace_bytes, void *stream)
{
    const char *who = "hbvx_gage_population_stats";
    int rc = check_gage_pop(who, r, gp);
    if (rc) return rc;
    if (!workspace || workspace_bytes < hbvx_gage_population_workspace_bytes(r, gp))
        return fail_as(who, HBVX_E_NULL, "workspace missing or too small");
    const Plan pl = plan(r, gp);
    hipStream_t st = (hipStream_t)stream;
    const int P = gp->n_cand;
    gagepop::Args a;
    a.r = *r;
    a.gp = *gp;
    a.qsT = (float *)workspace;
    a.qsT_c_stride = gp->runoff_c_stride ? (int64_t)r->U * r->T : 0;
    a.uh = gp->dp ? a.qsT + pl.qsT : const_cast<float *>(gp->uh);
    a.uh_c_stride = gp->dp ? (int64_t)r->NPAIR * r->L : 0;
    a.series = gp->series ? gp->series : a.qsT + pl.qsT + pl.uh;
    hipLaunchKernelGGL(gagepop::k_gp_transpose, dim3((r->U + 31) / 32, (r->T + 31) / 32, gp->runoff_c_stride ? P : 1),
                       dim3(256), 0, st, r->T, r->U, gp->runoff, gp->runoff_c_stride, a.qsT);
    if (gp->dp && r->NPAIR > 0) hipLaunchKernelGGL(gagepop::k_gp_uh, dim3(r->NPAIR, P), dim3(128), 0, st, a);
    hipLaunchKernelGGL(gagepop::k_gp_route, dim3((r->T + gagepop::TILE4 - 1) / gagepop::TILE4, r->G, P),
                       dim3(gagepop::TILE), 0, st, a);
    const dim3 sgrid((r->G + 63) / 64, P);
    switch (gp->transform) {
    case HBVX_POP_T_SQRT: hipLaunchKernelGGL(gagepop::k_gp_score<hbvx_popk::T_SQRT>, sgrid, dim3(64), 0, st, a); break;
    case HBVX_POP_T_LOG: hipLaunchKernelGGL(gagepop::k_gp_score<hbvx_popk::T_LOG>, sgrid, dim3(64), 0, st, a); break;
    default: hipLaunchKernelGGL(gagepop::k_gp_score<hbvx_popk::T_NONE>, sgrid, dim3(64), 0, st, a); break;
    }
    return launched(who);
}

extern "C" uint64_t hbvx_gage_events_sizeof(int which)
{
    return which == 0 ? sizeof(hbvx_gage_events) : 0;
}

extern "C" int hbvx_gage_population_events(const hbvx_gage_events *ev, void *stream)
{
    const char *who = "hbvx_gage_population_events";
    int rc = check_gage_events(who, ev);
    if (rc) return rc;
    gagepop::EventArgs a;
    a.ev = *ev;
    // A launch holds at most 65535 candidates and events (grid dimensions) and fewer than 2^32 threads: (candidates x
    // events) of one launch are bounded by what the gage groups leave of that, and the call is split on both axes.
    const uint64_t gx = ((uint64_t)ev->G + 63) / 64;
    const uint64_t budget = 0xFFFFFFFFull / (gx * 64);          // >= 1: G is an int32
    const int pc = (uint64_t)ev->n_cand < budget ? ev->n_cand : (int)budget;
    const uint64_t per = budget / (uint64_t)pc;
    const int ec = per < 65535 ? (int)per : 65535;              // >= 1
    for (a.c0 = 0; a.c0 < ev->n_cand; a.c0 += pc)
        for (a.e0 = 0; a.e0 < ev->n_events; a.e0 += ec) {
            const int np = ev->n_cand - a.c0 < pc ? ev->n_cand - a.c0 : pc;
            const int ne = ev->n_events - a.e0 < ec ? ev->n_events - a.e0 : ec;
            hipLaunchKernelGGL(gagepop::k_gp_events, dim3((unsigned)gx, np, ne), dim3(64), 0, (hipStream_t)stream, a);
        }
    return launched(who);
}

extern "C" uint64_t hbvx_gage_fdc_sizeof(int which)
{
    return which == 0 ? sizeof(hbvx_gage_fdc) : 0;
}

extern "C" int hbvx_gage_population_fdc(const hbvx_gage_fdc *gf, void *stream)
{
    const char *who = "hbvx_gage_population_fdc";
    int rc = check_gage_fdc(who, gf);
    if (rc) return rc;
    if (!gf->thr) return fail_as(who, HBVX_E_NULL, "thr is NULL");
    if (!gf->count || !gf->volume) return fail_as(who, HBVX_E_NULL, "count / volume is NULL");
    gagepop::FdcArgs a;
    a.gf = *gf;
    // (gage groups x candidates x blocks of levels) workgroups of 64; the call is split on the candidates so that no
    // launch reaches 2^32 threads.  One candidate alone exceeds that from 2^30 gages on: refused, not split further.
    const uint64_t gx = ((uint64_t)gf->G + 63) / 64;
    const unsigned gz = (unsigned)((gf->n_lev + gagepop::FDC_LEVELS - 1) / gagepop::FDC_LEVELS);
    const int pc = cands_per_launch(gx * gz, 64, gf->n_cand);
    if (pc < 1) return fail_as(who, HBVX_E_SHAPE, "G too large for one launch per candidate");
    for (a.c0 = 0; a.c0 < gf->n_cand; a.c0 += pc) {
        const int np = gf->n_cand - a.c0 < pc ? gf->n_cand - a.c0 : pc;
        hipLaunchKernelGGL(gagepop::k_gp_fdc, dim3((unsigned)gx, np, gz), dim3(64), 0, (hipStream_t)stream, a);
    }
    return launched(who);
}

extern "C" uint64_t hbvx_gage_quantiles_workspace_bytes(int32_t n_cand, int32_t T, int32_t G)
{
    if (n_cand < 1 || n_cand > 65535 || T < 1 || T > HBVX_GAGE_QUANT_MAX_T || G < 1) return 0;
    return (uint64_t)n_cand * (uint64_t)T * (uint64_t)G * sizeof(uint32_t);
}

extern "C" int hbvx_gage_population_quantiles(const hbvx_gage_fdc *gf, float *workspace, uint64_t workspace_bytes,
                                              void *stream)
{
    const char *who = "hbvx_gage_population_quantiles";
    int rc = check_gage_fdc(who, gf);
    if (rc) return rc;
    if (!gf->rank) return fail_as(who, HBVX_E_NULL, "rank is NULL");
    if (!gf->quantile) return fail_as(who, HBVX_E_NULL, "quantile is NULL");
    if (gf->T > HBVX_GAGE_QUANT_MAX_T) return fail_as(who, HBVX_E_UNSUPPORTED, "more than 16384 hours per column");
    if (!workspace || workspace_bytes < hbvx_gage_quantiles_workspace_bytes(gf->n_cand, gf->T, gf->G))
        return fail_as(who, HBVX_E_NULL, "workspace missing or too small");
    hipStream_t st = (hipStream_t)stream;
    gagepop::QuantArgs a;
    a.gf = *gf;
    a.keys = reinterpret_cast<uint32_t *>(workspace);
    a.g0 = 0;
    a.N = 1;
    while (a.N < gf->T) a.N <<= 1;                                  // <= 16384
    // the keys: (G / 32) x (T / 32) tiles of 256 threads per candidate.  Both kernels are split on the candidates so
    // that no launch reaches 2^32 threads; a G x T at which one candidate alone does (2^24 gages at 2^8 hours) is
    // refused, not split further.
    const uint64_t kx = ((uint64_t)gf->G + 31) / 32, ky = ((uint64_t)gf->T + 31) / 32;
    const int kc = cands_per_launch(kx * ky, 256, gf->n_cand);
    // the sort: G workgroups of QUANT_THREADS per candidate
    const int qc = cands_per_launch((uint64_t)gf->G, gagepop::QUANT_THREADS, gf->n_cand);
    if (kc < 1 || qc < 1) return fail_as(who, HBVX_E_SHAPE, "G x T too large for one launch per candidate");
    for (a.c0 = 0; a.c0 < gf->n_cand; a.c0 += kc) {
        const int np = gf->n_cand - a.c0 < kc ? gf->n_cand - a.c0 : kc;
        hipLaunchKernelGGL(gagepop::k_gp_keys, dim3((unsigned)kx, (unsigned)ky, np), dim3(256), 0, st, a);
    }
    for (a.c0 = 0; a.c0 < gf->n_cand; a.c0 += qc) {
        const int np = gf->n_cand - a.c0 < qc ? gf->n_cand - a.c0 : qc;
        hipLaunchKernelGGL(gagepop::k_gp_quant, dim3((unsigned)gf->G, np), dim3(gagepop::QUANT_THREADS),
                           (size_t)a.N * sizeof(uint32_t), st, a);
    }
    return launched(who);
}
