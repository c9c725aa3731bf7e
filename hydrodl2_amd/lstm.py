"""Sequence LSTM for the parameter network that feeds the HBV plug-in (the
caller side, delta-MG's CudnnLstmModel -- outside the reference repository).

`SeqLSTM` is a drop-in for `torch.nn.LSTM(input_size, hidden_size, num_layers)` on [T, B, I] input,
with or without an initial state `hx = (h0, c0)`: same parameter names and shapes (`weight_ih_l0`,
`weight_hh_l0`, `bias_ih_l0`, `bias_hh_l0`), same initialisation, same gate order, so state dicts
interchange; gradients reach h0 and c0 and flow from `out`, h_n and c_n.

The recurrence runs through include/hbvx_lstm.h (`hbvx_lstm_forward` / `hbvx_lstm_backward`, one
persistent HIP kernel per direction; `hbvx_lstm_forward_hx` / `hbvx_lstm_backward_hx` when a state is
given or c_n has a gradient); the time-parallel parts -- input projection, weight, input and h0
gradients -- are plain library GEMMs here.  Like the rest of the package there is no CPU path: on a
host tensor, or without the HIP library, the call raises.

Forward mode: under torch.autograd.forward_ad, `LstmSeq.jvp` carries one tangent direction (on x, the weights
and biases, h0 and c0) to h and c_n through `hbvx_lstm_tangent`, a third persistent kernel; a library without
that export raises HbvxError naming it.  torch.func.jvp / jacfwd are not supported.
"""
from __future__ import annotations

import math

import torch
import torch.autograd.forward_ad as _fwAD

from . import _abi
from ._lib import get_library
from . import ops


_PERM = {}


def _gate_perm(H: int, device) -> torch.Tensor:
    """Row index that turns torch's gate-major [4H] (i|f|g|o blocks) into (unit, gate) order (one tensor per hidden
    size and device, built on first use: four small launches less per call)."""
    key = (H, str(device))
    hit = _PERM.get(key)
    if hit is None:
        if torch.cuda.is_available() and torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
            # a tensor created inside a capture belongs to that graph's pool: do not keep it
            return (torch.arange(4, device=device)[None, :] * H + torch.arange(H, device=device)[:, None]).reshape(-1)
        hit = _PERM[key] = (torch.arange(4, device=device)[None, :] * H + torch.arange(H, device=device)[:, None]).reshape(-1)
    return hit


def _wgrad(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a^T b for a [K, G], b [K, I] with K = T*B in the tens of thousands: the weight gradients.  The library's plain
    call covers the [G, I] output with a few dozen tiles and walks all of K in each (55 TFLOP/s at K = 73 000, G = 1024,
    I = 256); cut into S batches along K and summed it runs at 120 (tools/micro/wgrad_gemm.py,
    profiles/r04_lstm_wgrad.txt).  S: a divisor of K near 8, else the plain product."""
    K = a.shape[0]
    if K >= 8192:
        for S in (8, 10, 9, 12, 6, 7, 5, 4, 16, 14, 15, 11, 13):
            if K % S == 0:
                return torch.bmm(a.view(S, K // S, a.shape[1]).transpose(1, 2), b.view(S, K // S, b.shape[1])).sum(0)
    return a.t() @ b


class LstmSeq(torch.autograd.Function):
    """x [T,B,I], W_ih [4H,I], W_hh [4H,H], b_ih, b_hh [4H] -> h [T,B,H], c [T,B,H] (c carries no
    gradient).  `check=True` synchronises and verifies the kernels' hand-off status word.

    h0, c0 [B,H] (None = zeros): the initial state; gradients reach both.  `cn=True` adds a third
    output, c_n [B,H]: a copy of c[T-1] that carries gradient (torch.nn.LSTM's c_n).  Without a state
    and without a gradient on c_n the call runs the zero-state entry points, as it always has."""

    @staticmethod
    @ops._device_guard
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, check: bool = False, h0=None, c0=None, cn: bool = False):
        lib = get_library()
        x_c, w_hh_c = x.contiguous(), w_hh.contiguous()
        for t, name in ((x_c, 'x'), (w_ih, 'weight_ih'), (w_hh_c, 'weight_hh'), (b_ih, 'bias_ih'), (b_hh, 'bias_hh')):
            ops._check_tensor(lib, t, name)
        if x_c.dim() != 3:
            raise ValueError(f"x must be [T, B, input_size], got {tuple(x_c.shape)}")
        T, B, I = x_c.shape
        H = w_hh_c.shape[1]
        if tuple(w_hh_c.shape) != (4 * H, H) or tuple(w_ih.shape) != (4 * H, I) or \
                tuple(b_ih.shape) != (4 * H,) or tuple(b_hh.shape) != (4 * H,):
            raise ValueError("LSTM parameter shapes do not match torch.nn.LSTM(input_size, hidden_size)")
        if lib.is_device and H not in _abi.LSTM_HIDDEN_SIZES:
            raise ValueError(f"hidden_size {H} not built; the HIP library has {_abi.LSTM_HIDDEN_SIZES}")
        state = []
        for t, name in ((h0, 'h0'), (c0, 'c0')):
            if t is not None:
                ops._check_tensor(lib, t, name)
                if tuple(t.shape) != (B, H):
                    raise ValueError(f"{name} must be [B, hidden_size] = {(B, H)}, got {tuple(t.shape)}")
                t = t.contiguous()
            state.append(t)
        h0, c0 = state
        stateful = h0 is not None or c0 is not None
        if stateful:
            lib.require("hbvx_lstm_forward_hx")
        perm = _gate_perm(H, x_c.device)
        w_ih_p = w_ih.index_select(0, perm)
        gx = torch.addmm((b_ih + b_hh).index_select(0, perm), x_c.reshape(T * B, I), w_ih_p.t())   # [T*B, 4H]
        r = _abi.LstmDesc(abi_version=_abi.LSTM_ABI_VERSION, T=T, B=B, H=H)
        ws_bytes = lib.lstm_workspace_bytes(r)
        ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=x_c.device)
        c_all = ops._out((T, B, H), x_c.device)
        h_all = ops._out((T, B, H), x_c.device)
        st = ops._stream_of(lib, x_c)
        if stateful:      # timed under the zero-state call's name: it is the same kernel (bench.py, tools/bench_lstm.py)
            ops._call(lib, 'hbvx_lstm_forward', lib.lstm_forward_hx, r, ops._ptr(w_hh_c), ops._ptr(gx), ops._ptr(h0),
                      ops._ptr(c0), ops._ptr(gx), ops._ptr(c_all), ops._ptr(h_all), ops._ptr(ws), ws_bytes, st)
        else:
            ops._call(lib, 'hbvx_lstm_forward', lib.lstm_forward, r, ops._ptr(w_hh_c), ops._ptr(gx), ops._ptr(gx),
                      ops._ptr(c_all), ops._ptr(h_all), ops._ptr(ws), ws_bytes, st)
        if check:
            lib.lstm_check(r, ops._ptr(ws), st)
        ctx.save_for_backward(x_c, w_ih_p, w_hh_c, gx, c_all, h_all, perm, h0, c0)
        if _fwAD._current_level >= 0:        # forward mode (jvp) reads the same tensors
            ctx.save_for_forward(x_c, w_ih_p, w_hh_c, gx, c_all, h_all, perm, h0, c0)
        ctx.check = check
        ctx.cn = cn
        ctx.mark_non_differentiable(c_all)
        ctx.set_materialize_grads(False)     # an unused output's gradient stays None: no zeros, no c_n term
        if cn:
            return h_all, c_all, c_all[-1].clone()
        return h_all, c_all

    @staticmethod
    @ops._device_guard
    def backward(ctx, gh, _gc, gcn=None):
        lib = get_library()
        x, w_ih_p, w_hh, gates, c_all, h_all, perm, h0, c0 = ctx.saved_tensors
        T, B, I = x.shape
        H = w_hh.shape[1]
        gh = torch.zeros_like(h_all) if gh is None else gh.contiguous()     # a loss on c_n alone
        need = ctx.needs_input_grad
        r = _abi.LstmDesc(abi_version=_abi.LSTM_ABI_VERSION, T=T, B=B, H=H)
        ws_bytes = lib.lstm_workspace_bytes(r)
        ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=x.device)
        dg = ops._out((T * B, 4 * H), x.device)
        st = ops._stream_of(lib, x)
        gc0 = ops._out((B, H), x.device) if c0 is not None and need[7] else None
        if c0 is not None or gcn is not None:
            gcn = gcn.contiguous() if gcn is not None else None
            ops._call(lib, 'hbvx_lstm_backward', lib.lstm_backward_hx, r, ops._ptr(w_hh), ops._ptr(gates), ops._ptr(c0),
                      ops._ptr(c_all), ops._ptr(gh), ops._ptr(gcn), ops._ptr(dg), ops._ptr(gc0), ops._ptr(ws), ws_bytes, st)
        else:
            ops._call(lib, 'hbvx_lstm_backward', lib.lstm_backward, r, ops._ptr(w_hh), ops._ptr(gates), ops._ptr(c_all),
                      ops._ptr(gh), ops._ptr(dg), ops._ptr(ws), ws_bytes, st)
        if ctx.check:
            lib.lstm_check(r, ops._ptr(ws), st)
        gx = dg @ w_ih_p if need[0] else None                                    # [T*B, I]
        gw_ih = gw_hh = gb = None
        if need[1]:
            gw_ih = torch.empty_like(w_ih_p)
            gw_ih[perm] = _wgrad(dg, x.reshape(T * B, I))
        if need[2]:
            gw_hh = torch.zeros_like(w_hh)
            g = _wgrad(dg[B:], h_all[:-1].reshape((T - 1) * B, H)) if T > 1 else None
            if h0 is not None:                                                   # the step-0 term: h_{-1} = h0
                g = dg[:B].t() @ h0 if g is None else g + dg[:B].t() @ h0
            if g is not None:
                gw_hh[perm] = g
        if need[3] or need[4]:
            gb = torch.empty(4 * H, dtype=dg.dtype, device=dg.device)
            gb[perm] = dg.sum(0)
        gh0 = dg[:B] @ w_hh.index_select(0, perm) if h0 is not None and need[6] else None   # dgates_0 W_hh
        return (gx.view(T, B, I) if gx is not None else None), gw_ih, gw_hh, gb, gb, None, gh0, gc0, None

    @staticmethod
    @ops._device_guard
    def jvp(ctx, x_t, w_ih_t, w_hh_t, b_ih_t, b_hh_t, _check_t, h0_t, c0_t, _cn_t):
        """Forward mode (torch.autograd.forward_ad): tangents of h and c_n along the inputs' tangents.  The time-parallel
        terms of the tangent are library GEMMs here, gx' = x' W_ih^T + x W_ih'^T + b_ih' + b_hh' + [h0; h_0..h_{T-2}]
        W_hh'^T (rows in the (unit, gate) order of gx; a term whose tangent is None is left out); the recurrence
        z'_t = gx'_t + h'_{t-1} W_hh^T and the cell's tangent are hbvx_lstm_tangent, on the primal the forward saved."""
        lib = get_library()
        lib.require("hbvx_lstm_tangent")
        x, w_ih_p, w_hh, gates, c_all, h_all, perm, h0, c0 = ctx.saved_tensors
        T, B, I = x.shape
        H = w_hh.shape[1]
        gt = None                                                               # gx' [T*B, 4H]
        if x_t is not None:
            gt = x_t.reshape(T * B, I) @ w_ih_p.t()
        if w_ih_t is not None:
            term = x.reshape(T * B, I) @ w_ih_t.index_select(0, perm).t()
            gt = term if gt is None else gt.add_(term)
        if b_ih_t is not None or b_hh_t is not None:
            bt = b_ih_t if b_hh_t is None else (b_hh_t if b_ih_t is None else b_ih_t + b_hh_t)
            bt = bt.index_select(0, perm)
            gt = bt.expand(T * B, 4 * H).clone() if gt is None else gt.add_(bt)
        if w_hh_t is not None:
            w_hh_tp = w_hh_t.index_select(0, perm).t()
            if gt is None:
                gt = torch.zeros(T * B, 4 * H, dtype=torch.float32, device=x.device)
            if T > 1:                                                           # h_{t-1} W_hh'^T, t >= 1
                gt[B:].addmm_(h_all[:-1].reshape((T - 1) * B, H), w_hh_tp)
            if h0 is not None:                                                  # the step-0 term: h_{-1} = h0
                gt[:B].addmm_(h0, w_hh_tp)
        if gt is None:
            gt = torch.zeros(T * B, 4 * H, dtype=torch.float32, device=x.device)
        gt = gt.contiguous()
        state_t = []
        for t, name in ((h0_t, 'h0'), (c0_t, 'c0')):
            if t is not None:
                ops._check_tensor(lib, t, f"tangent of {name}")
                t = t.contiguous()
                if t.data_ptr() % 16:                                           # h0' is read in 16-byte granules
                    t = t.clone()
            state_t.append(t)
        h0_t, c0_t = state_t
        r = _abi.LstmDesc(abi_version=_abi.LSTM_ABI_VERSION, T=T, B=B, H=H)
        ws_bytes = lib.lstm_workspace_bytes(r)
        ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=x.device)
        h_t = ops._out((T, B, H), x.device)
        cn_t = ops._out((B, H), x.device) if ctx.cn else None
        st = ops._stream_of(lib, x)
        ops._call(lib, 'hbvx_lstm_tangent', lib.lstm_tangent, r, ops._ptr(w_hh), ops._ptr(gates), ops._ptr(c0),
                  ops._ptr(c_all), ops._ptr(gt), ops._ptr(h0_t), ops._ptr(c0_t), ops._ptr(h_t), ops._ptr(cn_t),
                  ops._ptr(ws), ws_bytes, st)
        if ctx.check:
            lib.lstm_check(r, ops._ptr(ws), st)
        if ctx.cn:
            return h_t, None, cn_t
        return h_t, None


def lstm_seq(x, w_ih, w_hh, b_ih, b_hh, check: bool = False):
    """Functional form: returns (h [T,B,H], c [T,B,H]) for torch.nn.LSTM-layout weights."""
    return LstmSeq.apply(x, w_ih, w_hh, b_ih, b_hh, check)


class SeqLSTM(torch.nn.Module):
    """LSTM over [T, B, input_size]; `forward(x, hx=None)` returns (output [T,B,H], (h_n [L,B,H],
    c_n [L,B,H])) like torch.nn.LSTM(input_size, hidden_size, num_layers): hx = (h0, c0), each [L,B,H]
    float32 on x's device, None = zeros; gradients reach x, the parameters, h0 and c0, from output,
    h_n and c_n.  Layers are stacked on the host: layer l's output sequence is layer l+1's input, layer
    l starts from (h0[l], c0[l]), each layer one pair of persistent kernels.  Parameter names follow
    torch (`weight_ih_l{k}` ...), so state dicts interchange."""

    def __init__(self, input_size: int, hidden_size: int, check: bool = False, dr: float = 0.0,
                 num_layers: int = 1):
        super().__init__()
        if num_layers < 1:
            raise ValueError("SeqLSTM: num_layers must be >= 1")
        self.input_size, self.hidden_size, self.check = input_size, hidden_size, check
        self.num_layers = num_layers
        # dr: weight dropout as in hydroDL / delta-MG's CudnnLstm (one Bernoulli mask on W_ih and one on
        # W_hh per forward call, training mode only); 0 = torch.nn.LSTM behaviour
        self.dr = dr
        k = 1.0 / math.sqrt(hidden_size)
        # same creation order and distribution as torch.nn.LSTM.reset_parameters
        for layer in range(num_layers):
            n_in = input_size if layer == 0 else hidden_size
            self.register_parameter(f"weight_ih_l{layer}", torch.nn.Parameter(torch.empty(4 * hidden_size, n_in).uniform_(-k, k)))
            self.register_parameter(f"weight_hh_l{layer}", torch.nn.Parameter(torch.empty(4 * hidden_size, hidden_size).uniform_(-k, k)))
            self.register_parameter(f"bias_ih_l{layer}", torch.nn.Parameter(torch.empty(4 * hidden_size).uniform_(-k, k)))
            self.register_parameter(f"bias_hh_l{layer}", torch.nn.Parameter(torch.empty(4 * hidden_size).uniform_(-k, k)))

    def _state(self, x, hx):
        """hx -> (h0, c0), each [L,B,H]; ValueError on anything torch.nn.LSTM would not take."""
        if not isinstance(hx, (tuple, list)) or len(hx) != 2 or not all(torch.is_tensor(t) for t in hx):
            raise ValueError("SeqLSTM: hx must be a tuple (h0, c0) of two tensors")
        if x.dim() != 3:
            raise ValueError(f"SeqLSTM: x must be [T, B, input_size], got {tuple(x.shape)}")
        want = (self.num_layers, x.shape[1], self.hidden_size)
        for t, name in zip(hx, ("h0", "c0")):
            if tuple(t.shape) != want:
                raise ValueError(f"SeqLSTM: {name} must be [num_layers, B, hidden_size] = {want}, got {tuple(t.shape)}")
            if t.dtype != torch.float32:
                raise ValueError(f"SeqLSTM: {name} must be float32, got {t.dtype}")
            if t.device != x.device:
                raise ValueError(f"SeqLSTM: {name} is on {t.device}, the input on {x.device}")
        return hx

    def forward(self, x, hx=None):
        if x.is_cuda and self.hidden_size not in _abi.LSTM_HIDDEN_SIZES:
            raise ValueError(f"SeqLSTM: hidden_size must be one of {_abi.LSTM_HIDDEN_SIZES} (the sizes the HIP "
                             f"kernels are instantiated for), got {self.hidden_size}")
        h0, c0 = self._state(x, hx) if hx is not None else (None, None)
        hn, cn = [], []
        for layer in range(self.num_layers):
            w_ih, w_hh = getattr(self, f"weight_ih_l{layer}"), getattr(self, f"weight_hh_l{layer}")
            if self.training and self.dr > 0:
                w_ih = torch.nn.functional.dropout(w_ih, self.dr, training=True)
                w_hh = torch.nn.functional.dropout(w_hh, self.dr, training=True)
            x, _, c_n = LstmSeq.apply(x, w_ih, w_hh, getattr(self, f"bias_ih_l{layer}"), getattr(self, f"bias_hh_l{layer}"),
                                      self.check, None if h0 is None else h0[layer], None if c0 is None else c0[layer],
                                      True)
            hn.append(x[-1])
            cn.append(c_n)
        # c_n of a layer is already a tensor of its own: one layer needs no second copy
        return x, (torch.stack(hn), torch.stack(cn) if len(cn) > 1 else cn[0].unsqueeze(0))
