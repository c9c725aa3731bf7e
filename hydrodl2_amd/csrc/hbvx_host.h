// hbvx_host.h -- host-side plumbing shared by the translation units of libhbvx.so.
//
// The library is built from several .hip files compiled in parallel (one per kernel family:
// pipelined / streaming / tiled / time-parallel / implicit / tangent recurrence / LSTM) so that touching
// one family rebuilds one file.  The C ABI (include/hbvx.h) lives in hbvx.hip, apart from the entry points
// that are a family's own (launch_tan.hip, launch_adj.hip); its dispatchers call the family launchers declared here.
// A launcher returns true when its family took the call and has then set *rc to the ABI return code.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>

#include "../../include/hbvx.h"
#include "hbv_step.h"

namespace hbvx_host {

int fail(int code, const char *msg);
int hip_fail(hipError_t e, const char *what);
// hbvx_last_dispatch (include/hbvx.h): the kernel family that took the call; dir 0 forward, 1 adjoint
void note_dispatch(int dir, const char *family);
int env_int(const char *name, int dflt);
int device_cu_count();                   // compute units of the current device (cached per device)
// hbvx_fwd_out.zero_ptr: set by the kernel family that carries fill workgroups in its own launch (the pipelined forward);
// the entry points clear it before dispatch (hbvx_zero_in_launch reports it)
bool &zero_taken();
int lg_members(int M);
int count_dyn(const hbvx_desc *d);
bool use_tiled(const hbvx_desc *d);      // false under HBVX_KERNEL=simple
int check_desc(const hbvx_desc *d);

static const int LDS_BUDGET = 160 * 1024 - 512; // gfx950: 160 KiB per CU, one workgroup may take it all

// The template instance of the descriptor's explicit model: f(model, BETAET) with the two as
// std::integral_constant / std::bool_constant, constant expressions inside f (`k<model, betaet>`,
// `if constexpr`); f's result is returned.  BETAET: HBV 1.0 has it with 13 parameters (not with 12), the
// other models always.  The descriptor has passed check_desc; HBVADJ has launchers of its own.
template <typename F>
auto with_model(const hbvx_desc *d, F &&f)
{
    using namespace hbvx;
    switch (d->model) {
    case HBVX_MODEL_HBV10:
        if (d->n_param == 13) return f(std::integral_constant<int, MODEL_HBV10>{}, std::true_type{});
        return f(std::integral_constant<int, MODEL_HBV10>{}, std::false_type{});
    case HBVX_MODEL_HBV11P: return f(std::integral_constant<int, MODEL_HBV11P>{}, std::true_type{});
    case HBVX_MODEL_HOURLY: return f(std::integral_constant<int, MODEL_HOURLY>{}, std::true_type{});
    default: return f(std::integral_constant<int, MODEL_HBV20>{}, std::true_type{});   // HBVX_MODEL_HBV20
    }
}

// The template instance of the implicit scheme (HBVADJ): f(BETAET, FEW) as std::bool_constant.  BETAET as for HBV 1.0;
// few: the slot-list ("few") instance of the kernels that have one (hbv_adj_kernels.h) -- the others ignore it.
template <typename F>
auto with_adj(const hbvx_desc *d, bool few, F &&f)
{
    if (d->n_param == 13) return few ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    return few ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

// What every tangent entry point checks of the parameter tangents (launch_tan.hip, launch_adj.hip)
inline int check_tan_params(const hbvx_desc *d, const hbvx_param_tan *p)
{
    for (int i = d->n_param; i < HBVX_MAX_PARAM; i++)
        if (p[i].dyn || p[i].sta) return fail(HBVX_E_SHAPE, "tangent for a parameter slot the model lacks");
    for (int i = 0; i < d->n_param; i++)
        if (p[i].dyn && !d->p[i].dyn) return fail(HBVX_E_SHAPE, "dynamic tangent for a static parameter");
    return HBVX_OK;
}
// a stride of 0 is a zero tangent, like a NULL pointer (include/hbvx.h): applied to the kernel's copy of the batch
inline void zero_stride_tangents(hbvx_tan_batch &tb, int n_param)
{
    if (!tb.x_d_stride) tb.x = nullptr;
    if (!tb.mu_d_stride) tb.muwts = nullptr;
    if (!tb.state_d_stride) tb.state_in = nullptr;
    for (int i = 0; i < n_param; i++) {
        if (!tb.dyn_d_stride[i]) tb.p[i].dyn = nullptr;
        if (!tb.sta_d_stride[i]) tb.p[i].sta = nullptr;
    }
}

// launch_pipe.hip
bool try_fwd_pipe(const hbvx_desc *d, const hbvx_fwd_out *out, void *stream, int *rc);
// launch_stream.hip
bool try_fwd_stream(const hbvx_desc *d, const hbvx_fwd_out *out, void *stream, int *rc, bool any_size = false);
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) only when a launch needs MORE than the kernel was ever granted on
// this device: the attribute holds one value per kernel (the last one set) and is a ceiling for the launch, so it is
// raised and never lowered -- a template instance whose LDS request varies with the problem (train and validation
// models with different dynamic sets) would otherwise launch "big, small, big" with the attribute left at "small".
// One process-wide table under a mutex (autograd's backward thread and the main thread share it); hbvx.hip defines it.
hipError_t set_dynamic_lds(const void *kern, int lds);
// one launch of a kernel with dynamic LDS (the attribute raised first when it needs to be)
template <typename Args, typename K>
hipError_t launch_tiled_one(K kern, const Args &a, dim3 grid, int threads, size_t lds, hipStream_t st)
{
    hipError_t e = set_dynamic_lds(reinterpret_cast<const void *>(kern), (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, dim3(threads), lds, st, a);
    return hipGetLastError();
}
// hbvx_bwd_io.store_gate: make `st` wait for the caller's event before a kernel that stores gradients is launched
inline void store_gate(const hbvx_bwd_io *io, hipStream_t st)
{
    if (io->store_gate) (void)hipStreamWaitEvent(st, (hipEvent_t)io->store_gate, 0);
}
// n_live: rows of io->grad_flux4 that exist (hbvx_backward_live, include/hbvx_live_rows.h); below 4 the streaming
// adjoint, which reads four, refuses the call it would take (*rc = HBVX_E_UNSUPPORTED, nothing launched)
bool try_bwd_stream(const hbvx_desc *d, const hbvx_bwd_io *io, void *stream, int *rc, int n_live = 4);
// HBVX_TRAJ_CKPT with the segment in LDS (hbv_stream2_ckpt.h): whether it takes this problem (then no scratch is
// wanted: hbvx_ckpt_workspace_bytes returns 0), and the launch
bool stream_ckpt_applicable(const hbvx_desc *d, int K);
bool try_bwd_stream_ckpt(const hbvx_desc *d, const hbvx_bwd_io *io, void *stream, int *rc);
// launch_tiled.hip (try_fwd_tiled also takes the implicit model, for launch_adj.hip)
bool try_fwd_tiled(const hbvx_desc *d, const hbvx_fwd_out *out, void *stream, int *rc);
bool try_bwd_tiled(const hbvx_desc *d, const hbvx_bwd_io *io, void *stream, int *rc);
// launch_chunked.hip
bool chunked_applicable(const hbvx_desc *d);
int chunk_days();
// n_live as for try_bwd_stream: below 4 only the one-pass runoff-only form takes the call, any other is refused
bool try_bwd_chunked(const hbvx_desc *d, const hbvx_bwd_io *io, void *stream, int *rc, int n_live = 4);

// launch_ckpt.hip
bool try_bwd_ckpt(const hbvx_desc *d, const hbvx_bwd_io *io, void *stream, int *rc);

} // namespace hbvx_host
