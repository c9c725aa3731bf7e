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
that export raises HbvxError naming it.  Many directions on one primal: `lstm_jvp_batch` / `SeqLSTM.jvp_batch`
take tangents with a leading direction axis and carry all of them through `hbvx_lstm_tangent_batch` -- one primal run,
the time-parallel terms as library GEMMs, the recurrences of all directions in one launch sequence (the
unit of work is a (direction, row tile) pair, so directions fill the SIMDs one direction leaves idle); their output
feeds `hydrodl2_amd.jvp_batch` as a full-form parameter tangent.  torch.func.jvp / jacfwd / vmap are not supported.
"""
from __future__ import annotations

import contextlib
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


def _primal(x, w_ih, w_hh, b_ih, b_hh, check, h0, c0):
    """One layer's forward through the library: the validated inputs and everything the backward and the tangent calls
    read, (x, w_ih_p, w_hh, gates, c_all, h_all, perm, h0, c0) -- w_ih_p and gates in (unit, gate) row order."""
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
    return x_c, w_ih_p, w_hh_c, gx, c_all, h_all, perm, h0, c0


class LstmSeq(torch.autograd.Function):
    """x [T,B,I], W_ih [4H,I], W_hh [4H,H], b_ih, b_hh [4H] -> h [T,B,H], c [T,B,H] (c carries no
    gradient).  `check=True` synchronises and verifies the kernels' hand-off status word.

    h0, c0 [B,H] (None = zeros): the initial state; gradients reach both.  `cn=True` adds a third
    output, c_n [B,H]: a copy of c[T-1] that carries gradient (torch.nn.LSTM's c_n).  Without a state
    and without a gradient on c_n the call runs the zero-state entry points, as it always has."""

    @staticmethod
    @ops._device_guard
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, check: bool = False, h0=None, c0=None, cn: bool = False):
        x_c, w_ih_p, w_hh_c, gx, c_all, h_all, perm, h0, c0 = _primal(x, w_ih, w_hh, b_ih, b_hh, check, h0, c0)
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


def _dropout_masked(w: torch.Tensor, p: float):
    """(F.dropout(w, p, training=True), d F.dropout / d w): one draw; the second tensor is what F.dropout's own
    forward AD multiplies a tangent of w by (0 or 1 / (1 - p) per element)."""
    with _fwAD.dual_level():
        res = _fwAD.unpack_dual(torch.nn.functional.dropout(_fwAD.make_dual(w.detach(), torch.ones_like(w)), p, training=True))
        return res.primal.detach(), res.tangent.detach()


def _check_tangents(mod, x, hx, tangents, max_directions) -> int:
    """Host-side validation of `lstm_jvp_batch`'s request (no library, no device); the number of directions."""
    if not isinstance(tangents, dict) or not tangents:
        raise ValueError("lstm_jvp_batch needs at least one tangent: a dict name -> [D, ...] tensor")
    if int(max_directions) < 1:
        raise ValueError(f"max_directions must be at least 1, got {max_directions}")
    if x.dim() != 3:
        raise ValueError(f"x must be [T, B, input_size], got {tuple(x.shape)}")
    want = {k: tuple(v.shape) for k, v in mod.named_parameters()}
    want["x"] = tuple(x.shape)
    state = (mod.num_layers, x.shape[1], mod.hidden_size)
    want["h0"] = want["c0"] = state
    unknown = sorted(set(tangents) - set(want))
    if unknown:
        raise ValueError(f"unknown tangent names {unknown}; SeqLSTM takes {sorted(want)}")
    if hx is None and ("h0" in tangents or "c0" in tangents):
        raise ValueError("a tangent on h0 / c0 needs the state it belongs to: pass hx = (h0, c0)")
    for k, t in tangents.items():
        if not torch.is_tensor(t) or t.dim() < 1:
            raise ValueError(f"tangent {k!r} must be a tensor with a leading direction axis")
    sizes = {int(t.shape[0]) for t in tangents.values()}
    if len(sizes) != 1:
        raise ValueError(f"tangents must share their leading direction axis, got sizes {sorted(sizes)}")
    D = sizes.pop()
    if D < 1:
        raise ValueError("tangents hold no direction (leading axis of size 0)")
    for k, t in tangents.items():
        if tuple(t.shape[1:]) != want[k]:
            raise ValueError(f"tangent {k!r} must be [D, {', '.join(map(str, want[k]))}], got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"tangent {k!r} must be float32, got {t.dtype}")
        if t.device != x.device:
            raise ValueError(f"tangent {k!r} is on {t.device}, the input on {x.device}")
    return D


def _layer_tangents(lib, rec, x_t, w_ih_t, w_hh_t, b_t, h0_t, c0_t, D, check):
    """One layer, D directions: (h' [D,T,B,H], c'_{T-1} [D,B,H]) on the primal `rec` (_primal's tuple).  x_t
    [D,T,B,I], w_ih_t [D,4H,I], w_hh_t [D,4H,H], b_t [D,4H] (b_ih' + b_hh'), h0_t / c0_t [D,B,H]; None = zero.  The
    time-parallel terms are library GEMMs, rows in the (unit, gate) order of gx (LstmSeq.jvp)."""
    x, w_ih_p, w_hh, gates, c_all, h_all, perm, h0, c0 = rec
    T, B, I = x.shape
    H = w_hh.shape[1]
    # One GEMM per direction and term, of the one-direction call's shape, into the direction's slice of gx': what a
    # direction gets does not depend on how many directions share the call (pieces of a request are the bits of the
    # whole), and at T x B rows each of them fills the chip on its own.
    gt = torch.empty(D, T * B, 4 * H, dtype=torch.float32, device=x.device)   # gx'
    x2 = x.reshape(T * B, I)
    for d in range(D):
        g, filled = gt[d], False
        if x_t is not None:
            torch.mm(x_t[d].reshape(T * B, I), w_ih_p.t(), out=g)
            filled = True
        if w_ih_t is not None:
            w_ih_tp = w_ih_t[d].index_select(0, perm).t()
            g.addmm_(x2, w_ih_tp) if filled else torch.mm(x2, w_ih_tp, out=g)
            filled = True
        if b_t is not None:
            bt = b_t[d].index_select(0, perm)
            g.add_(bt) if filled else g.copy_(bt.expand(T * B, 4 * H))
            filled = True
        if not filled:
            g.zero_()
        if w_hh_t is not None:
            w_hh_tp = w_hh_t[d].index_select(0, perm).t()
            if T > 1:                                                           # h_{t-1} W_hh'^T, t >= 1
                g[B:].addmm_(h_all[:-1].reshape((T - 1) * B, H), w_hh_tp)
            if h0 is not None:                                                  # the step-0 term: h_{-1} = h0
                g[:B].addmm_(h0, w_hh_tp)
    state_t = []
    for t in (h0_t, c0_t):
        if t is not None:
            t = t.contiguous()
            if t.data_ptr() % 16:                                               # h0' is read in 16-byte granules
                t = t.clone()
        state_t.append(t)
    h0_t, c0_t = state_t
    r = _abi.LstmDesc(abi_version=_abi.LSTM_ABI_VERSION, T=T, B=B, H=H)
    ws_bytes = lib.lstm_tangent_batch_workspace_bytes(r, D)
    ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=x.device)
    h_t = ops._out((D, T, B, H), x.device)
    cn_t = ops._out((D, B, H), x.device)
    st = ops._stream_of(lib, x)
    ops._call(lib, 'hbvx_lstm_tangent_batch', lib.lstm_tangent_batch, r, D, ops._ptr(w_hh), ops._ptr(gates),
              ops._ptr(c0), ops._ptr(c_all), ops._ptr(gt), ops._ptr(h0_t), ops._ptr(c0_t), ops._ptr(h_t),
              ops._ptr(cn_t), ops._ptr(ws), ws_bytes, st)
    if check:
        lib.lstm_check(r, ops._ptr(ws), st)
    return h_t, cn_t


def lstm_jvp_batch(mod: "SeqLSTM", x, hx=None, tangents=None, max_directions: int = 16):
    """Forward-mode derivatives of `mod(x, hx)` along D directions on one primal run.

    tangents  name -> tensor with a leading direction axis D: 'x' [D,T,B,I], 'h0' / 'c0' [D,L,B,H] (with `hx`), any
              parameter name of the module [D, *shape].  Missing names are zero.
    max_directions  directions per launch sequence: gx' and the exchange slabs take T B H x (16 + 4) bytes per
              direction and layer; more directions run in pieces on the one primal run.

    Returns ((out, (h_n, c_n)), (out_t [D,T,B,H], (h_n_t [D,L,B,H], c_n_t [D,L,B,H]))): the primal outputs are the
    bits of a plain `mod(x, hx)` call (run once, without an autograd graph), and slice d of the tangents is what one
    torch.autograd.forward_ad call along direction d returns.  In training mode with weight dropout the masks are
    drawn once, as in one plain call, for the primal and all directions, and mask the weight tangents as F.dropout's
    forward AD does.  A library without hbvx_lstm_tangent_batch raises HbvxError naming it."""
    D = _check_tangents(mod, x, hx, tangents, max_directions)
    lib = get_library()
    lib.require("hbvx_lstm_tangent_batch")
    if x.is_cuda and mod.hidden_size not in _abi.LSTM_HIDDEN_SIZES:
        raise ValueError(f"SeqLSTM: hidden_size must be one of {_abi.LSTM_HIDDEN_SIZES} (the sizes the HIP "
                         f"kernels are instantiated for), got {mod.hidden_size}")
    h0, c0 = mod._state(x, hx) if hx is not None else (None, None)
    dev = x.device if x.is_cuda else None
    with torch.no_grad(), (torch.cuda.device(dev) if dev is not None else contextlib.nullcontext()):
        recs, masks, hn, cn = [], [], [], []
        inp = x.detach()
        for layer in range(mod.num_layers):
            w_ih, w_hh = getattr(mod, f"weight_ih_l{layer}").detach(), getattr(mod, f"weight_hh_l{layer}").detach()
            m_ih = m_hh = None
            if mod.training and mod.dr > 0:
                w_ih, m_ih = _dropout_masked(w_ih, mod.dr)
                w_hh, m_hh = _dropout_masked(w_hh, mod.dr)
            rec = _primal(inp, w_ih, w_hh, getattr(mod, f"bias_ih_l{layer}").detach(),
                          getattr(mod, f"bias_hh_l{layer}").detach(), mod.check,
                          None if h0 is None else h0[layer].detach(), None if c0 is None else c0[layer].detach())
            recs.append(rec)
            masks.append((m_ih, m_hh))
            inp = rec[5]                                                        # h_all
            hn.append(inp[-1])
            cn.append(rec[4][-1].clone())
        primal = (inp, (torch.stack(hn), torch.stack(cn) if len(cn) > 1 else cn[0].unsqueeze(0)))
        pieces = []
        for d0 in range(0, D, int(max_directions)):
            cut = {k: v.detach()[d0:d0 + int(max_directions)] for k, v in tangents.items()}
            n = next(iter(cut.values())).shape[0]
            x_t, hn_t, cn_t = cut.get("x"), [], []
            for layer, (rec, (m_ih, m_hh)) in enumerate(zip(recs, masks)):
                w_ih_t, w_hh_t = cut.get(f"weight_ih_l{layer}"), cut.get(f"weight_hh_l{layer}")
                if m_ih is not None:
                    w_ih_t = None if w_ih_t is None else w_ih_t * m_ih
                    w_hh_t = None if w_hh_t is None else w_hh_t * m_hh
                b_ih_t, b_hh_t = cut.get(f"bias_ih_l{layer}"), cut.get(f"bias_hh_l{layer}")
                b_t = b_ih_t if b_hh_t is None else (b_hh_t if b_ih_t is None else b_ih_t + b_hh_t)
                x_t, c_last_t = _layer_tangents(lib, rec, x_t, w_ih_t, w_hh_t, b_t,
                                                cut["h0"][:, layer] if "h0" in cut else None,
                                                cut["c0"][:, layer] if "c0" in cut else None, n, mod.check)
                hn_t.append(x_t[:, -1])
                cn_t.append(c_last_t)
            pieces.append((x_t, torch.stack(hn_t, 1), torch.stack(cn_t, 1)))
        out_t, hn_t, cn_t = pieces[0] if len(pieces) == 1 else (torch.cat(p) for p in zip(*pieces))
    return primal, (out_t, (hn_t, cn_t))


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

    def jvp_batch(self, x, hx=None, tangents=None, max_directions: int = 16):
        """`lstm_jvp_batch(self, x, hx, tangents, max_directions)`: forward-mode derivatives along many directions on
        one primal run; ((out, (h_n, c_n)), (out_t [D,T,B,H], (h_n_t [D,L,B,H], c_n_t [D,L,B,H])))."""
        return lstm_jvp_batch(self, x, hx, tangents, max_directions)
