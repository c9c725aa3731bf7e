// launch_tan.hip -- the entry points of the tangent-linear recurrence (hbv_tan.h): hbvx_forward_tangent (one
// direction), hbvx_forward_tangent_batch (several) and hbvx_hourly_tangent_batch (the hourly model's).  The tangents
// of routing, BFI and gage routing are in hbvx.hip.
#include "hbvx_host.h"
#include "hbv_tan.h"

using namespace hbvx;
using namespace hbvx_host;

// What the two daily entry points check alike.  `unsupported`: the caller's own message for a model without
// a tangent kernel.
static int check_tan_model(const hbvx_desc *d, const char *unsupported)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (d->model != HBVX_MODEL_HBV10 && d->model != HBVX_MODEL_HBV11P && d->model != HBVX_MODEL_HBV20)
        return fail(HBVX_E_UNSUPPORTED, unsupported);
    return HBVX_OK;
}

// k_tan<model, BETAET, Args> of the descriptor's model, one wave per workgroup.  The entry points have refused the
// models they do not serve; the hourly model has no one-direction instance.
template <typename Args>
static int launch_tan(const hbvx_desc *d, const Args &a, dim3 grid, void *stream, const char *what)
{
    with_model(d, [&](auto m, auto be) {
        if constexpr (m != MODEL_HOURLY || std::is_same<Args, TanBatchArgs>::value)
            hipLaunchKernelGGL((k_tan<m, be, Args>), grid, dim3(64), 0, (hipStream_t)stream, a);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return HBVX_OK;
}

extern "C" int hbvx_forward_tangent(const hbvx_desc *d, const hbvx_tan_io *io, void *stream)
{
    int rc = check_tan_model(d, "hbvx_forward_tangent: HBV 1.0 / 1.1p / 2.0 only");
    if (rc) return rc;
    if (!io || !io->tan_state_out) return fail(HBVX_E_NULL, "tan_state_out is NULL");
    const int want_nf = (d->model == HBVX_MODEL_HBV10) ? 11 : 12;
    if (io->tan_flux && io->n_flux != want_nf) return fail(HBVX_E_SHAPE, "n_flux does not match model");
    rc = check_tan_params(d, io->p);
    if (rc) return rc;
    TanArgs a;
    a.d = *d;
    a.io = *io;
    a.lgMp = lg_members(d->M);
    const int bpw = 64 >> a.lgMp;
    return launch_tan(d, a, dim3((d->B + bpw - 1) / bpw), stream, "hbvx_forward_tangent launch");
}

// What the two several-direction recurrence entry points do alike once the model is accepted: the checks of the
// batch struct, and the kernel arguments with "a stride of 0 is a zero tangent" applied.  `who` names the entry point
// in the messages about n_dir.
static int prep_tan_batch(const hbvx_desc *d, const hbvx_tan_batch *tb, int want_nf, const char *who, TanBatchArgs &a)
{
    char msg[128];
    if (!tb) return fail(HBVX_E_NULL, "tan_batch is NULL");
    if (tb->n_dir < 1) {
        snprintf(msg, sizeof msg, "%s: n_dir must be >= 1", who);
        return fail(HBVX_E_SHAPE, msg);
    }
    if (!tb->tan_state_out) return fail(HBVX_E_NULL, "tan_state_out is NULL");
    if (tb->n_flux != want_nf) return fail(HBVX_E_SHAPE, "n_flux does not match model");
    if (tb->flux_mask >> tb->n_flux) return fail(HBVX_E_SHAPE, "flux_mask selects a series at or above n_flux");
    if (tb->flux_mask && !tb->tan_flux) return fail(HBVX_E_NULL, "tan_flux is NULL although flux_mask selects series");
    if (tb->dyn_t0 < 0 || tb->dyn_t0 > (d->T > 0 ? d->T - 1 : 0)) return fail(HBVX_E_SHAPE, "dyn_t0 outside the call's days");
    int rc = check_tan_params(d, tb->p);
    if (rc) return rc;
    if (tb->n_dir > 65535) {
        snprintf(msg, sizeof msg, "%s: too many directions for one launch", who);
        return fail(HBVX_E_SHAPE, msg);
    }
    a.d = *d;
    a.tb = *tb;
    a.lgMp = lg_members(d->M);
    zero_stride_tangents(a.tb, d->n_param);
    return HBVX_OK;
}

extern "C" int hbvx_forward_tangent_batch(const hbvx_desc *d, const hbvx_tan_batch *tb, void *stream)
{
    int rc = check_tan_model(d, "hbvx_forward_tangent_batch: HBV 1.0 / 1.1p / 2.0 only");
    if (rc) return rc;
    TanBatchArgs a;
    rc = prep_tan_batch(d, tb, (d->model == HBVX_MODEL_HBV10) ? 11 : 12, "hbvx_forward_tangent_batch", a);
    if (rc) return rc;
    const int bpw = 64 >> a.lgMp;
    return launch_tan(d, a, dim3((d->B + bpw - 1) / bpw, tb->n_dir), stream, "hbvx_forward_tangent_batch launch");
}

// The hourly model's tangent-linear recurrence: hbvx_forward_tangent_batch's checks, for HBVX_MODEL_HOURLY alone.
extern "C" int hbvx_hourly_tangent_batch(const hbvx_desc *d, const hbvx_tan_batch *tb, void *stream)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (d->model != HBVX_MODEL_HOURLY)
        return fail(HBVX_E_UNSUPPORTED, "hbvx_hourly_tangent_batch: the hourly model only (the daily models: hbvx_forward_tangent_batch)");
    TanBatchArgs a;
    rc = prep_tan_batch(d, tb, 12, "hbvx_hourly_tangent_batch", a);
    if (rc) return rc;
    const int bpw = 64 >> a.lgMp;
    return launch_tan(d, a, dim3((d->B + bpw - 1) / bpw, tb->n_dir), stream, "hbvx_hourly_tangent_batch launch");
}
