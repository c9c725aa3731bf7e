/* hbvx_lstm.h -- C ABI of the sequence LSTM that feeds hbvx_forward (the
 * caller side of the hot path -- delta-MG's parameter network; it is not part of the reference
 * repository, the semantics are torch.nn.LSTM's: one layer, gate order i, f, g, o; the initial state
 * (h0, c0) is zero in the first two calls below and given in the *_hx calls).
 * Exported by the same shared library as include/hbvx.h (libhbvx.so on the GPU, the CPU restatement
 * under oracle/ for tests).  Plain pointers and sizes; device pointers for the HIP library.
 *
 * The input projection x W_ih^T + b_ih + b_hh and the weight gradients are library GEMMs on the
 * caller's side (hydrodl2_amd/lstm.py); these entry points are the recurrence, which a GEMM library
 * cannot fuse.  Gate vectors use the (unit, gate) layout: element [t][b][u][g], g = 0..3 = i, f, g, o.
 *
 * Residency: the kernels are persistent -- the workgroups of a 16-basin row tile hand data to each
 * other inside one launch -- and each launch is sized to fit the whole GPU.  Run a call on a GPU that
 * is not executing another large kernel at the same time (other streams, other processes): partners
 * that cannot become resident are detected by bounded spins and reported (hbvx_lstm_check), never
 * waited for indefinitely.
 *
 * Errors: 0 on success, a negative HBVX_E_* (include/hbvx.h) otherwise; hbvx_last_error() has the text. */
#ifndef HBVX_LSTM_H
#define HBVX_LSTM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HBVX_LSTM_ABI_VERSION 1

typedef struct hbvx_lstm_desc {
    int32_t abi_version; /* HBVX_LSTM_ABI_VERSION */
    int32_t T, B, H;     /* steps, basins (batch), hidden units; the HIP library needs H in {64, 128, 256} */
} hbvx_lstm_desc;

/* Scratch for any call below (bytes; caller-owned, contents undefined afterwards): the per-step
 * exchange slabs through which the workgroups of a 16-basin row tile hand h_t (forward), h'_t (tangent) or
 * the gate gradients (backward) to each other, and the arrival counters. */
uint64_t hbvx_lstm_workspace_bytes(const hbvx_lstm_desc *d);

/* w_hh [4H,H] (torch.nn.LSTM.weight_hh_l0), gx [T,B,H,4] = x W_ih^T + b_ih + b_hh in (unit, gate)
 * layout -> gates [T,B,H,4] (activated i, f, g, o; may alias gx), c_all and h_all [T,B,H]. */
int hbvx_lstm_forward(const hbvx_lstm_desc *d, const float *w_hh, const float *gx, float *gates,
                      float *c_all, float *h_all, void *workspace, uint64_t workspace_bytes,
                      void *stream);

/* grad_h [T,B,H] (gradient of the loss w.r.t. every h_t) -> grad_gates [T,B,H,4]: the gradient
 * w.r.t. the gate pre-activations, from which the caller forms grad_x, grad_W_ih, grad_W_hh and
 * the bias gradients with GEMMs.  grad_gates must not alias gates. */
int hbvx_lstm_backward(const hbvx_lstm_desc *d, const float *w_hh, const float *gates,
                       const float *c_all, const float *grad_h, float *grad_gates,
                       void *workspace, uint64_t workspace_bytes, void *stream);

/* The same recurrence from an initial state (h0, c0) [B,H] (torch.nn.LSTM's hx for one layer), and its adjoint.
 * Additive to ABI version 1: HBVX_LSTM_ABI_VERSION and the workspace size are those of the calls above, which
 * are these calls with every state pointer NULL.  A NULL h0, c0 or grad_c_last stands for zeros.
 *
 * Forward: step 0 multiplies h0 by W_hh on the same path as every later step multiplies h_{t-1}, so a run
 * resumed from (h_all[T1-1], c_all[T1-1]) on rows T1.. of the same gx gives the bits of the uninterrupted run.
 * h0 must be 16-byte aligned like gx.
 *
 * Backward: grad_c_last [B,H] is the gradient w.r.t. c_{T-1} from outside the sequence (torch's c_n);
 * grad_c0 [B,H] (NULL = not wanted) receives the gradient w.r.t. c0.  The gradient w.r.t. h0 is
 * grad_gates[0] W_hh (gate rows in the (unit, gate) order of grad_gates), a GEMM on the caller's side like
 * grad_x; so is the step-0 term grad_gates[0]^T h0 of grad_W_hh.  A time-out poisons grad_c0 with NaN as well. */
int hbvx_lstm_forward_hx(const hbvx_lstm_desc *d, const float *w_hh, const float *gx,
                         const float *h0, const float *c0,
                         float *gates, float *c_all, float *h_all,
                         void *workspace, uint64_t workspace_bytes, void *stream);
int hbvx_lstm_backward_hx(const hbvx_lstm_desc *d, const float *w_hh, const float *gates,
                          const float *c0, const float *c_all, const float *grad_h,
                          const float *grad_c_last,
                          float *grad_gates, float *grad_c0,
                          void *workspace, uint64_t workspace_bytes, void *stream);

/* Forward-mode derivative of hbvx_lstm_forward_hx along one direction (tangents written with a prime), on the
 * primal that call produced: gates [T,B,H,4] (activated, (unit, gate) layout) and c_all [T,B,H], from the same w_hh
 * and c0.  Additive to ABI version 1 like the *_hx calls: the same descriptor, validation and workspace size.
 *
 *   z'_t = gx'_t + h'_{t-1} W_hh^T        gx_t [T,B,H,4], (unit, gate) layout: every time-parallel term of the
 *                                         tangent, formed by the caller -- x' W_ih^T + x W_ih'^T + b_ih' + b_hh'
 *                                         + [h0; h_0 .. h_{T-2}] W_hh'^T
 *   di = i(1-i) z'_i, df = f(1-f) z'_f, dg = (1-g^2) z'_g, do = o(1-o) z'_o
 *   c'_t = df c_{t-1} + f c'_{t-1} + di g + i dg;   h'_t = do tanh(c_t) + o (1 - tanh(c_t)^2) c'_t
 *   (h'_{-1}, c'_{-1}) = (h0_t, c0_t); c_{-1} = c0
 *
 * -> h_t [T,B,H] (h'), c_t_last [B,H] (c'_{T-1}; NULL = not wanted).  A NULL c0, h0_t or c0_t stands for zeros.
 * h0_t must be 16-byte aligned like gx_t.  A time-out poisons h_t[T-1] and c_t_last with NaN (hbvx_lstm_check). */
int hbvx_lstm_tangent(const hbvx_lstm_desc *d, const float *w_hh, const float *gates, const float *c0,
                      const float *c_all, const float *gx_t, const float *h0_t, const float *c0_t,
                      float *h_t, float *c_t_last, void *workspace, uint64_t workspace_bytes, void *stream);

/* hbvx_lstm_tangent along n_dir directions in one call, on one primal (w_hh, gates, c0, c_all are shared):
 * gx_t [D,T,B,H,4], h0_t and c0_t [D,B,H] (NULL = zeros for every direction) -> h_t [D,T,B,H], c_t_last [D,B,H]
 * (NULL = not wanted), D = n_dir, each dense.  Slice d of the outputs holds the bits hbvx_lstm_tangent gives for
 * slice d of gx_t, h0_t, c0_t under the same HBVX_LSTM_UNITS: the unit of work is the pair (direction, row tile)
 * instead of the row tile, with the arithmetic of a pair unchanged, so directions fill the SIMDs that one
 * direction's row tiles leave idle.  Pairs are cut into launches by the residency rule above.
 * Additive to ABI version 1.  The exchange slabs grow with n_dir, so the workspace has a size query of its own
 * (0 for a descriptor without a size or n_dir < 1); hbvx_lstm_check reads this workspace like any other.  Refused
 * before any device work: n_dir < 1, n_dir x ceil(B/16) above 2^26 - 1, and everything hbvx_lstm_tangent refuses.
 * A time-out poisons h_t[d][T-1] and c_t_last[d] of the pairs that saw it. */
uint64_t hbvx_lstm_tangent_batch_workspace_bytes(const hbvx_lstm_desc *d, int32_t n_dir);
int hbvx_lstm_tangent_batch(const hbvx_lstm_desc *d, int32_t n_dir, const float *w_hh, const float *gates,
                            const float *c0, const float *c_all, const float *gx_t, const float *h0_t,
                            const float *c0_t, float *h_t, float *c_t_last, void *workspace,
                            uint64_t workspace_bytes, void *stream);

/* Synchronises `stream` and reports whether the last call that used `workspace` completed: the
 * workgroups of a row tile wait for each other with bounded spins; a time-out (the partners were
 * not resident, e.g. the GPU was shared) poisons the outputs with NaN and is reported here. */
int hbvx_lstm_check(const hbvx_lstm_desc *d, const void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif
