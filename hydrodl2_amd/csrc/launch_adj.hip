// launch_adj.hip -- the entry points of the implicit scheme ("HBV adjoint", hbv_adj.py; kernels in hbv_adj_kernels.h):
// hbvx_adj_forward, hbvx_adj_backward and hbvx_adj_tangent_batch.  The forward's tiled stepper is launched by
// launch_tiled.hip, its staged pipeline by launch_pipe.hip, the scan / reduce kernels of the time-parallel adjoint by
// launch_chunked.hip.
#include "hbvx_host.h"
#define HBVX_CHUNK_NO_SHARED_KERNELS
#include "hbv_chunked.h"        // (first: hbv_adj_kernels.h uses its XCD-aware block map)
#include "hbv_adj_kernels.h"

using namespace hbvx;
using namespace hbvx_host;

namespace hbvx_host {
// launch_chunked.hip: the scan / reduce kernels of the time-parallel scheme (shared with the implicit one)
void launch_chunk_scan(const hbvx::ChunkArgs &a, hipStream_t st);
void launch_chunk_reduce(const hbvx::ChunkArgs &a, int n_param, hipStream_t st);
}

static int check_adj(const hbvx_desc *d)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (d->model != HBVX_MODEL_HBVADJ) return fail(HBVX_E_UNSUPPORTED, "hbvx_adj_* needs model HBVADJ");
    if (!(d->adj_gtol >= 0.0f) || d->adj_max_iter < 0 || d->adj_max_iter > 64)
        return fail(HBVX_E_SHAPE, "bad Newton policy (adj_gtol / adj_max_iter)");
    return HBVX_OK;
}

// "Few" mode (hbv_adj_kernels.h): whether the call has at most ADJ_FEW dynamic parameters, and then their slot list
static bool adj_few(const hbvx_desc *d, AdjFew &few)
{
    few = AdjFew{};
    if (count_dyn(d) > ADJ_FEW) return false;
    for (int i = 0; i < d->n_param; i++)
        if (d->p[i].dyn) few.slot[few.nd++] = i;
    return true;
}

static int adj_forward_dispatch(const hbvx_desc *d, const hbvx_fwd_out *out, void *stream)
{
    int rc = check_adj(d);
    if (rc) return rc;
    if (!out || !out->state_out) return fail(HBVX_E_NULL, "state_out is NULL");
    if (out->flux && out->n_flux != 1) return fail(HBVX_E_SHAPE, "hbvx_adj_forward writes n_flux = 1");
    if (d->adj_stop < 0 || d->adj_stop > 2) return fail(HBVX_E_SHAPE, "adj_stop must be 0, 1 or 2");
    if (d->adj_stop == 2 && try_fwd_pipe(d, out, stream, &rc)) return rc;   // staged solve: three-wave pipeline
    if (try_fwd_tiled(d, out, stream, &rc)) return rc;
    AdjFwdArgs a;
    a.d = *d;
    a.o = *out;
    a.lgMp = lg_members(d->M);
    const int bpw = 64 >> a.lgMp;
    dim3 grid((d->B + bpw - 1) / bpw);
    with_adj(d, false, [&](auto be, auto) { hipLaunchKernelGGL(k_adj_fwd<be>, grid, dim3(64), 0, (hipStream_t)stream, a); });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_adj_forward launch");
    return HBVX_OK;
}

extern "C" int hbvx_adj_forward(const hbvx_desc *d, const hbvx_fwd_out *out, void *stream)
{
    zero_taken() = false;
    if (out && out->zero_ptr && !out->zero_state) return fail(HBVX_E_NULL, "zero_ptr needs zero_state");
    return adj_forward_dispatch(d, out, stream);
}

extern "C" int hbvx_adj_backward(const hbvx_desc *d, const hbvx_bwd_io *io, void *stream)
{
    int rc = check_adj(d);
    if (rc) return rc;
    if (!io || !io->traj) return fail(HBVX_E_NULL, "traj is NULL");
    if (io->n_flux != 1) return fail(HBVX_E_SHAPE, "hbvx_adj_backward expects n_flux = 1");
    if (d->T == 0) return HBVX_OK;
    hipStream_t st = (hipStream_t)stream;
    if (io->workspace && chunked_applicable(d) && io->workspace_bytes >= hbvx_backward_workspace_bytes(d)) {
        // time-parallel adjoint (hbv_adj_kernels.h + the scan / reduce kernels of hbv_chunked.h)
        ChunkArgs ca;
        ca.d = *d;
        ca.io = *io;
        ca.lgMp = lg_members(d->M);
        ca.C = chunk_days();
        ca.nchunk = (d->T + ca.C - 1) / ca.C;
        const int64_t N = (int64_t)d->B * d->M;
        ca.phi = (float *)io->workspace;
        ca.abnd = ca.phi + (int64_t)ca.nchunk * 30 * N;
        ca.gpart = ca.abnd + (int64_t)ca.nchunk * 5 * N;
        ca.per_xcd = chunk_per_xcd(d->B, ca.lgMp);
        ca.group = 1;
        dim3 g2((unsigned)(8 * ca.per_xcd * ca.nchunk));      // XCD-aware 1-D block map (hbv_chunked.h::chunk_block)
        AdjFew few;
        const bool is_few = adj_few(d, few);
        with_adj(d, is_few, [&](auto be, auto fw) {
            hipLaunchKernelGGL((k_adj_chunk_phi<be, fw>), g2, dim3(64), 0, st, *d, *io, ca.lgMp, ca.C, ca.phi, ca.per_xcd, few);
        });
        launch_chunk_scan(ca, st);
        store_gate(io, st);      // phi and scan only read; the sweep stores the dynamic gradients
        with_adj(d, is_few, [&](auto be, auto fw) {
            hipLaunchKernelGGL((k_adj_chunk_sweep<be, fw>), g2, dim3(64), 0, st, *d, *io, ca.lgMp, ca.C, ca.abnd, ca.gpart, ca.per_xcd, few);
        });
        launch_chunk_reduce(ca, d->n_param, st);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "hbvx_adj_backward (chunked) launch");
        return HBVX_OK;
    }
    AdjBwdArgs a;
    a.d = *d;
    a.io = *io;
    a.lgMp = lg_members(d->M);
    const int bpw = 64 >> a.lgMp;
    dim3 grid((d->B + bpw - 1) / bpw);
    store_gate(io, st);
    with_adj(d, false, [&](auto be, auto) { hipLaunchKernelGGL(k_adj_bwd<be>, grid, dim3(64), 0, st, a); });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_adj_backward launch");
    return HBVX_OK;
}

// Forward-mode AD of the implicit scheme, several directions per call (include/hbvx.h).  Every refusal happens here,
// before the launch.
extern "C" int hbvx_adj_tangent_batch(const hbvx_desc *d, const hbvx_tan_batch *tb, const float *traj, void *stream)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (d->model != HBVX_MODEL_HBVADJ)
        return fail(HBVX_E_UNSUPPORTED, "hbvx_adj_tangent_batch: the implicit scheme (HBVADJ) only");
    if (!tb) return fail(HBVX_E_NULL, "tan_batch is NULL");
    if (tb->n_dir < 1) return fail(HBVX_E_SHAPE, "hbvx_adj_tangent_batch: n_dir must be >= 1");
    if (tb->n_dir > 65535) return fail(HBVX_E_SHAPE, "hbvx_adj_tangent_batch: too many directions for one launch");
    if (tb->n_flux != 1) return fail(HBVX_E_SHAPE, "hbvx_adj_tangent_batch: n_flux must be 1");
    if (tb->flux_mask >> tb->n_flux) return fail(HBVX_E_SHAPE, "flux_mask selects a series at or above n_flux");
    if (!traj) return fail(HBVX_E_NULL, "hbvx_adj_tangent_batch: traj is NULL (the trajectory of hbvx_adj_forward)");
    if (!tb->tan_state_out) return fail(HBVX_E_NULL, "tan_state_out is NULL");
    if (tb->flux_mask && !tb->tan_flux) return fail(HBVX_E_NULL, "tan_flux is NULL although flux_mask selects series");
    if (tb->muwts) return fail(HBVX_E_UNSUPPORTED, "hbvx_adj_tangent_batch: muwts must be NULL (the implicit scheme has no ensemble weights)");
    if (tb->dyn_t0 < 0 || tb->dyn_t0 > (d->T > 0 ? d->T - 1 : 0)) return fail(HBVX_E_SHAPE, "dyn_t0 outside the call's days");
    rc = check_tan_params(d, tb->p);
    if (rc) return rc;
    AdjTanArgs a;
    a.d = *d;
    a.tb = *tb;
    a.traj = traj;
    a.lgMp = lg_members(d->M);
    zero_stride_tangents(a.tb, d->n_param);
    const int bpw = 64 >> a.lgMp;
    const dim3 grid((d->B + bpw - 1) / bpw, (tb->n_dir + ADJ_TAN_G - 1) / ADJ_TAN_G);
    AdjFew few;
    with_adj(d, adj_few(d, few), [&](auto be, auto fw) {
        hipLaunchKernelGGL((k_adj_tan_batch<be, fw>), grid, dim3(64), 0, (hipStream_t)stream, a, few);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hbvx_adj_tangent_batch launch");
    return HBVX_OK;
}
