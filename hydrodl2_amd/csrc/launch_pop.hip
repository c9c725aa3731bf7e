// launch_pop.hip -- the entry point of the population evaluation (hbv_pop.h): hbvx_population_cost.
#include "hbvx_host.h"
#include "hbv_pop.h"

using namespace hbvx;
using namespace hbvx_host;

extern "C" int hbvx_population_cost(const hbvx_desc *d, const hbvx_pop *pop, void *stream)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (d->model != HBVX_MODEL_HBV10 && d->model != HBVX_MODEL_HBV11P && d->model != HBVX_MODEL_HBV20)
        return fail(HBVX_E_UNSUPPORTED, "hbvx_population_cost: HBV 1.0 / 1.1p / 2.0 only");
    if (!pop) return fail(HBVX_E_NULL, "hbvx_population_cost: pop is NULL");
    if (!pop->target) return fail(HBVX_E_NULL, "hbvx_population_cost: target is NULL");
    if (!pop->cost) return fail(HBVX_E_NULL, "hbvx_population_cost: cost is NULL");
    if (pop->n_cand < 1 || pop->n_cand > 65535) return fail(HBVX_E_SHAPE, "hbvx_population_cost: n_cand must be in 1..65535");
    if (pop->t_first < 0 || pop->t_first >= d->T) return fail(HBVX_E_SHAPE, "hbvx_population_cost: t_first outside the call's days");
    for (int i = d->n_param; i < HBVX_MAX_PARAM; i++)
        if (pop->p[i].sta) return fail(HBVX_E_SHAPE, "hbvx_population_cost: candidate values for a parameter slot the model lacks");
    PopArgs a;
    memset(&a.r, 0, sizeof a.r);
    a.has_route = 0;
    if (const hbvx_route_desc *r = pop->route) {
        if (r->abi_version != HBVX_ABI_VERSION) return fail(HBVX_E_ABI, "hbvx_population_cost: route abi_version mismatch");
        if (r->L != (d->T < HBVX_UH_MAXLEN ? d->T : HBVX_UH_MAXLEN)) return fail(HBVX_E_SHAPE, "hbvx_population_cost: route L must be min(T, 15)");
        if (r->T != d->T || r->B != d->B) return fail(HBVX_E_SHAPE, "hbvx_population_cost: route T / B differ from the descriptor's");
        if ((!pop->ra && !r->ra) || (!pop->rb && !r->rb))
            return fail(HBVX_E_NULL, "hbvx_population_cost: a routing input is neither in pop nor in route");
        a.r = *r;
        a.has_route = 1;
    }
    a.d = *d;
    a.pop = *pop;
    a.pop.route = nullptr;      // a host pointer: the kernel reads its copy in a.r
    a.lgMp = lg_members(d->M);
    const int bpw = 64 >> a.lgMp;
    const dim3 grid((d->B + bpw - 1) / bpw, pop->n_cand);
    with_model(d, [&](auto m, auto be) {
        if constexpr (m != MODEL_HOURLY)
            hipLaunchKernelGGL((k_pop<m, be>), grid, dim3(64), 0, (hipStream_t)stream, a);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_population_cost launch");
    return HBVX_OK;
}
