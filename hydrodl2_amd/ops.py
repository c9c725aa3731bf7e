"""torch.autograd shim over the C ABI (include/hbvx.h).

One autograd.Function covers the whole hot path of one `_PBM` call
(reference: hbv.py:363-553): parameter prep + daily recurrence + ensemble mean
(`hbvx_forward`) followed by unit-hydrograph routing of the four runoff series
(`hbvx_route_forward`).  Keeping both stages in one Function means the
gradient w.r.t. the raw NN output is written into ONE buffer (the routing
columns and the physical columns live in the same `parameters` tensor).

PyTorch is used for device memory, the current stream and autograd plumbing
only; every arithmetic step of the path runs in the HIP library.
"""
from __future__ import annotations

import contextlib
import ctypes as _C
from dataclasses import dataclass, field
import functools
import os
import struct
import threading
from typing import List, NamedTuple, Optional, Sequence

import torch
import torch.autograd.forward_ad as _fwAD

from . import _abi
from ._lib import get_library


@dataclass
class ParamSource:
    """Where physical-parameter slot `slot` lives inside the input tensors.

    Offsets/strides are in float32 elements relative to tensor `tensor_idx`'s
    first element; `dyn_off` addresses (t=0 of this call, b=0, j=0).
    """
    slot: int
    lo: float
    hi: float
    tensor_idx: int
    sta_off: int
    sta_bs: int
    dyn_tensor_idx: int = -1
    dyn_off: int = -1          # -1: static parameter
    dyn_ts: int = 0
    dyn_bs: int = 0
    drop: Optional[torch.Tensor] = None  # uint8 [B] on the compute device


@dataclass
class RouteSource:
    tensor_idx: int
    a_off: int
    b_off: int
    stride: int
    a_bounds: Sequence[float]
    b_bounds: Sequence[float]


@dataclass
class StepConfig:
    model: int
    n_param: int
    n_flux: int
    T: int                     # steps of this call
    t0: int                    # first row of x used by this call
    B: int
    M: int
    raw_sigmoid: bool
    channels: Sequence[int]    # (prcp, tmean, pet) channel indices in x
    nearzero: float
    params: List[ParamSource] = field(default_factory=list)
    route: Optional[RouteSource] = None
    want_flux: bool = True
    want_traj: bool = False    # keep the state trajectory even without autograd
    adj_gtol: float = 1e-3     # implicit scheme only (hbv_adj.py:519)
    adj_max_iter: int = 3      # implicit scheme only (hbv_adj.py:518)
    adj_stop: int = 0          # implicit scheme only: 0 per-lane stopping rule, 1 per wavefront (hbv_adj.py:544)
    mu_t0: Optional[int] = None  # first row of muwts used by this call (None: same as t0)
    want_bfi: bool = False     # also return BFI (hbv.py:562-567) from the same autograd node (no second Function)
    ckpt_days: int = 0         # 4 / 8 / 16: keep K-day checkpoints instead of the trajectory (memory-lean adjoint)
    persistent_grad: bool = False   # module key grad_buffer='persistent': see _overlapped_grad_buffers


def _device_guard(fn):
    """Run an autograd.Function method with the CUDA device of its tensors current.  The library takes
    the stream from the tensors' device, but HIP calls it makes besides the launch (function attributes
    for dynamic LDS, device properties) go to the calling thread's CURRENT device: a model living on
    cuda:k in a process that never called torch.cuda.set_device(k) would otherwise mix devices."""
    @functools.wraps(fn)
    def wrapped(ctx, *args):
        dev = next((a.device for a in args if torch.is_tensor(a) and a.is_cuda), None)
        if dev is None or torch.cuda.current_device() == dev.index:   # the common case: nothing to switch
            return fn(ctx, *args)
        with torch.cuda.device(dev):
            return fn(ctx, *args)
    return wrapped


# bench.py sets this to a list to collect (abi_call, start_event, end_event) per launch,
# recorded on the stream the kernels are enqueued on.
KERNEL_EVENTS = None


def _call(lib, name, fn, *args):
    if KERNEL_EVENTS is None or not lib.is_device:
        return fn(*args)
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(*args)
    e1.record()
    KERNEL_EVENTS.append((name, e0, e1))


_POISON = os.environ.get("HBVX_DEBUG_POISON", "") not in ("", "0")


def _out(shape, device) -> torch.Tensor:
    """Output buffer the library overwrites completely.  HBVX_DEBUG_POISON=1 (set by the GPU
    test tier) fills it with NaN first, so a kernel that skips an element cannot pass on stale
    memory the caching allocator handed back."""
    if _POISON:
        return torch.full(shape, float("nan"), dtype=torch.float32, device=device)
    return torch.empty(shape, dtype=torch.float32, device=device)


def _zeros_like(lib, t: torch.Tensor) -> torch.Tensor:
    """Dense zero gradient shaped like `t`, filled through hbvx_zero (6.6 TB/s on MI355X against 5.3 for
    torch's fill kernel: the [T,B,ny] gradient of config 2 is 3.8 GB per step)."""
    out = torch.empty_like(t)           # dense like t (same strides when t is dense): numel elements of storage
    if out.numel():
        _call(lib, 'hbvx_zero', lib.zero, out.data_ptr(), out.numel() * out.element_size(), _stream_of(lib, out))
    return out


def _dyn_columns(p: torch.Tensor, cfg: "StepConfig", tensor_idx: int):
    """Which elements of the gradient of parameter tensor `p` the adjoint STORES (never accumulates): the nmul
    columns of every dynamic parameter on the days of this call (hbvx_backward writes each of those elements
    exactly once, 0 for a dy_drop-masked basin).  Returns (keep bit mask over column groups of width nmul,
    first day) for hbvx_zero_except, (0, 0) when the tensor holds no dynamic parameter, or None when its layout
    is not the plain [T,B,width] one (then only a dense fill is safe)."""
    dyn = [ps for ps in cfg.params if ps.dyn_off >= 0 and ps.dyn_tensor_idx == tensor_idx]
    if not dyn:
        return 0, 0
    M, B, T = cfg.M, cfg.B, cfg.T
    if p.dim() != 3 or not p.is_contiguous() or p.shape[1] != B:
        return None
    W = p.shape[2]
    keep, t_first = 0, None
    for ps in dyn:
        tf, rem = divmod(ps.dyn_off, B * W)
        k, j0 = divmod(rem, M)
        if (ps.dyn_ts != B * W or ps.dyn_bs != W or rem >= W or j0 != 0 or (k + 1) * M > W or k >= 32
                or (t_first is not None and tf != t_first) or tf + T > p.shape[0]):
            return None
        t_first = tf
        keep |= 1 << k
    return keep, t_first


def _fill_grad(lib, out: torch.Tensor, cfg: "StepConfig", cols) -> None:
    """Zero `out` (a [T,B,W] gradient buffer) except the columns the adjoint stores (`cols` from _dyn_columns)."""
    keep, t_first = cols
    B, W = out.shape[1], out.shape[2]
    _call(lib, 'hbvx_zero', lib.zero_except, out.data_ptr(), out.shape[0] * B, W, t_first * B, (t_first + cfg.T) * B,
          cfg.M, keep, _stream_of(lib, out))


def _grad_like(lib, p: torch.Tensor, cfg: "StepConfig", tensor_idx: int) -> torch.Tensor:
    """Gradient buffer for parameter tensor `p`: zero wherever the adjoint accumulates (static rows,
    routing columns) or never writes, left alone where it STORES (_dyn_columns).  Falls back to the dense fill
    when the layout is not the plain [T,B,width] one.  Under HBVX_DEBUG_POISON the left-alone part is NaN: an
    element a kernel skipped cannot pass."""
    cols = _dyn_columns(p, cfg, tensor_idx)
    if cols is None or cols[0] == 0:
        return _zeros_like(lib, p)
    out = torch.full_like(p, float("nan")) if _POISON else torch.empty_like(p)
    _fill_grad(lib, out, cfg, cols)
    return out


# Part of the dense zero fill of a [T,B,ny] gradient (3.8 GB at config 2) INSIDE THE FORWARD LAUNCH (hbvx_fwd_out.zero_ptr,
# ABI 10): the pipelined forward is a latency chain on 168 of 256 CUs; surplus workgroups of the same launch, on the CUs
# it leaves idle, write zeros into the buffer front to back for as long as the recurrence runs.  The buffer is allocated
# on the caller's stream in forward and handed to backward through the autograd context (first backward only: a second
# one over a retained graph fills its own); backward fills what is missing (hbvx_zero_rest) on the second stream beside
# the adjoint, as it fills the whole buffer without this.  One stream and one launch in forward: no cross-stream
# ownership (round 5's second-stream fill beside the forward cost a hipMalloc every other step: the caching allocator
# cannot recycle a block another stream still owns -- profiles/r05_earlyzero.txt).
# WHERE IT PAYS (profiles/r05_inlaunch_fill.txt): the implicit scheme, whose 4.2 ms forward (575 ns per day) does not
# notice the fill -- config 4: 6.75-6.84 -> 6.32-6.38 ms, the speed of grad_buffer='persistent' with a fresh gradient
# tensor per step.  The explicit models' recurrence (115 ns per day, a tile of ten days in flight) is sensitive to ANY
# concurrent HBM writes: 22 fill waves (1 TB/s) stretch config 2's forward from 0.90 to 1.08 ms, 88 waves to 1.25 --
# what the adjoint gains (1.33 -> 0.92) the forward loses (2.37-2.55 -> 2.22-2.46 ms over three boxes, config 2 with two
# dynamic parameters +-0).  So: "auto" = the implicit scheme only; HBVX_EARLY_ZERO=1 all models, 0 none.
_EARLY_ZERO = os.environ.get("HBVX_EARLY_ZERO", "auto")
_EARLY_ZERO_MIN = 1 << 26     # elements: below 256 MB the fill is not worth a special path
_SIDE_STREAMS: dict = {}


def _row_split(p: torch.Tensor, cfg: "StepConfig", i: int):
    """Whether parameter tensor i takes the big-buffer + separate-last-row form of its gradient: (ok, base, cols).
    It does when it is large, [T,B,W]-shaped, every static / routing source of it lies in its last row, and at most half
    of its columns belong to dynamic parameters of this call."""
    base = (p.shape[0] - 1) * p[0].numel() if p.dim() == 3 else -1
    offs = [ps.sta_off for ps in cfg.params if ps.tensor_idx == i]
    if cfg.route is not None and cfg.route.tensor_idx == i:
        offs += [cfg.route.a_off, cfg.route.b_off]
    cols = _dyn_columns(p, cfg, i)
    few_dyn = cols is not None and bin(cols[0]).count("1") * cfg.M * 2 <= p.shape[-1]
    ok = (p.dim() == 3 and p.is_contiguous() and p.numel() >= _EARLY_ZERO_MIN and p.shape[0] > 1
          and all(o >= base for o in offs) and cols is not None and (cols[0] == 0 or few_dyn))
    return ok, base, cols


def _early_zero_request(lib, cfg: "StepConfig", ptensors, needs, out) -> Optional[tuple]:
    """Forward side: allocate the gradient buffer of the (one) qualifying parameter tensor and offer it to the forward
    launch (out.zero_ptr / zero_bytes / zero_state).  Returns (tensor index, buffer, state words) for the autograd
    context, or None.  A configuration whose forward carries no fill workgroups (another kernel family, no idle CUs)
    stops offering after its first call: holding the buffer from forward to backward would buy nothing."""
    wanted = _EARLY_ZERO == "1" or (_EARLY_ZERO not in ("", "0") and cfg.model == _abi.MODEL_HBVADJ)
    if not (wanted and lib.is_device and not cfg.persistent_grad and _FILL_OVERLAP):
        return None
    if cfg.__dict__.get("_early_zero_useless"):
        return None
    for i, (p, need) in enumerate(zip(ptensors, needs)):
        if need and _row_split(p, cfg, i)[0]:
            big = torch.empty_like(p)
            state = torch.zeros(2, dtype=torch.int32, device=p.device)
            out.zero_ptr, out.zero_bytes, out.zero_state = big.data_ptr(), big.numel() * big.element_size(), state.data_ptr()
            return i, big, state
    return None


def _early_zero_result(lib, cfg: "StepConfig", early) -> None:
    if early is not None and not lib.zero_in_launch():
        cfg.__dict__["_early_zero_useless"] = True


# Default: the fill runs BESIDE the adjoint.  The adjoint kernels are bound by instruction issue, the
# fill by HBM bandwidth, and the only thing that ties them is the static row: static-parameter and routing
# gradients accumulate into the LAST row of the [T,B,ny] gradient.  So those go to a separate [B,ny] row
# (the C ABI takes any pointer + stride for them), the big buffer is filled on a second HIP stream while
# the adjoint runs on the caller's, and one small add joins them at the end.  Dynamic rows are written
# (not accumulated) by the adjoint and skipped by hbvx_zero_except: disjoint bytes, no ordering needed.
# HBVX_FILL_OVERLAP=0 restores the fill in front of the adjoint.
_FILL_OVERLAP = os.environ.get("HBVX_FILL_OVERLAP", "1") not in ("", "0")


def _side_stream(dev) -> "torch.cuda.Stream":
    side = _SIDE_STREAMS.get(dev.index)
    if side is None:
        side = _SIDE_STREAMS[dev.index] = torch.cuda.Stream(dev)
    return side


def _overlapped_grad_buffers(lib, cfg: "StepConfig", ptensors, needs, early=None):
    """(gp, rows, bases, start): gradient buffers, the separate last rows (None where a tensor keeps the
    plain path), their element offsets inside the big tensors, and `start()` -> event: begins the fills
    of the qualifying tensors on the side stream (call it when the caller's stream has nothing
    bandwidth-bound left in front of the adjoint) and returns the event that marks them complete;
    `start.gated`: that event must reach the library as `store_gate`.  Which tensors qualify: _row_split.
    `early`: (index, buffer) from the forward (_early_zero_request): that tensor's buffer is already zero."""
    dev = ptensors[0].device
    gp, rows, bases, todo = [], [], [], []
    gated = False
    for i, (p, need) in enumerate(zip(ptensors, needs)):
        if not need:
            gp.append(None); rows.append(None); bases.append(0)
            continue
        # A tensor with dynamic columns is filled DENSELY (the fastest fill) and the adjoint's stores into those
        # columns must land after it: the fill's event goes to the library as hbvx_bwd_io.store_gate, which holds
        # back the storing kernel only (the transfer-map and scan passes of the time-parallel adjoint run beside
        # the fill).  Without the gate the two race (measured: wrong gradients).  Worth it while few columns are
        # dynamic -- with most of them dynamic (config 3) hbvx_zero_except in front of the adjoint writes a
        # fraction of the bytes and stays.
        ok, base, cols = _row_split(p, cfg, i)
        if early is not None and early[0] == i and ok:
            # its front part was zeroed inside the forward's launch (_early_zero_request); what is missing is filled below,
            # beside the adjoint, like a whole buffer
            gp.append(early[1])
            rows.append(torch.zeros_like(p[0]))
            bases.append(base)
            todo.append((early[1], early[2]))
            gated = gated or cols[0] != 0
            continue
        if not ok:
            gp.append(_grad_like(lib, p, cfg, i)); rows.append(None); bases.append(0)
            continue
        if cfg.persistent_grad:
            # grad_buffer='persistent' (opt-in): the [T,B,W] gradient lives in a buffer this configuration keeps.  All
            # of it but the last row and the dynamic columns is zero and STAYS zero (nothing ever writes there), the
            # dynamic columns are overwritten by every adjoint, the last row is reset below -- so the dense zero fill
            # the autograd contract costs (3.8 GB per step at config 2, and the bandwidth it takes from the adjoint
            # beside it) happens once.  The contract of a captured graph's static outputs: the tensor handed to
            # autograd is valid until this module's next backward with the same shapes (no gradient accumulation across
            # calls on a leaf).  The memo keeps the STORAGE and hands out a fresh tensor each time, so that autograd's
            # AccumulateGrad may adopt it (a tensor someone else references would be cloned: 3.8 GB).
            memo = cfg.__dict__.setdefault("_memo", {})
            key = ("pgrad", i, tuple(p.shape), str(p.device))
            st = memo.get(key)
            if st is None:
                big = _zeros_like(lib, p)
                memo[key] = big.untyped_storage()
            else:
                big = torch.empty(0, dtype=p.dtype, device=p.device).set_(st, 0, p.shape)
                big[-1].zero_()
            gp.append(big)
            rows.append(torch.zeros_like(p[0]))
            bases.append(base)
            continue
        # on the caller's stream and pool: it is also where it dies
        big = torch.empty_like(p)
        gp.append(big)
        rows.append(torch.zeros_like(p[0]))
        bases.append(base)
        todo.append((big, None))
        gated = gated or cols[0] != 0

    def start():
        if not todo:
            return None
        main = torch.cuda.current_stream(dev)
        side = _side_stream(dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            for big, state in todo:
                if state is None:
                    _call(lib, 'hbvx_zero', lib.zero, big.data_ptr(), big.numel() * big.element_size(), _stream_of(lib, big))
                else:
                    _call(lib, 'hbvx_zero', lib.zero_rest, big.data_ptr(), big.numel() * big.element_size(), state.data_ptr(),
                          _stream_of(lib, big))
            done = torch.cuda.Event()
            done.record(side)
        return done
    start.gated = gated      # the fill covers columns the adjoint stores: pass the event as store_gate
    return gp, rows, bases, start


def _ptr(t: Optional[torch.Tensor], off: int = 0) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr() + 4 * off


def _stream_of(lib, t: torch.Tensor) -> int:
    if lib.is_device:
        return torch.cuda.current_stream(t.device).cuda_stream
    return 0


def _check_tensor(lib, t: torch.Tensor, name: str):
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if lib.is_device and not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); "
                           "hydrodl2_amd has no CPU path")
    if not lib.is_device and t.is_cuda:
        raise RuntimeError(f"{name}: test library expects host tensors")


def has_tangent(*ts) -> bool:
    """Whether any of `ts` (tensors, tuples / lists of tensors, or anything else, which is ignored) carries a
    forward-mode tangent at the current torch.autograd.forward_ad level.  False at once when no level is active."""
    if _fwAD._current_level < 0:
        return False
    for t in ts:
        if isinstance(t, (tuple, list)):
            if has_tangent(*t):
                return True
        elif torch.is_tensor(t) and _fwAD.unpack_dual(t).tangent is not None:
            return True
    return False


def _mu_t0(cfg: StepConfig) -> int:
    return cfg.t0 if cfg.mu_t0 is None else cfg.mu_t0


# ---------------------------------------------------------------------------------------------
# Descriptors.  A StepConfig that a module keeps across calls (same shapes, same dynamic set) carries a
# plan: the hbvx_desc bytes with every shape / bound / stride field filled in once, and the byte offsets of
# the pointer fields.  A call copies the template (1.3 KB) and packs the pointers in place -- the step of the
# deltaMG minibatch shape spent more host time marshalling descriptors than the GPU spent on its kernels.
_PTR = struct.Struct("<Q")
_D = _abi.Desc
_PS_SIZE = _C.sizeof(_abi.ParamSrc)
_OFF_P = _D.p.offset
_OFF_DYN, _OFF_STA, _OFF_DROP = _abi.ParamSrc.dyn.offset, _abi.ParamSrc.sta.offset, _abi.ParamSrc.drop.offset


class _DescPlan:
    __slots__ = ("key", "template", "sta", "dyn", "drop")


def _desc_plan(cfg: StepConfig, x, has_mu: bool) -> _DescPlan:
    key = (x.stride(0), x.stride(1), has_mu, len(cfg.params), cfg.T, cfg.t0, cfg.B, cfg.M)
    plan = getattr(cfg, "_plan", None)
    if plan is not None and plan.key == key:
        return plan
    d = _abi.Desc()
    d.abi_version = _abi.ABI_VERSION
    d.model = cfg.model
    d.T, d.B, d.M = cfg.T, cfg.B, cfg.M
    d.n_param = cfg.n_param
    d.raw_sigmoid = 1 if cfg.raw_sigmoid else 0
    d.ch_prcp, d.ch_tmean, d.ch_pet = cfg.channels
    d.nearzero = cfg.nearzero
    d.x_t_stride, d.x_b_stride = x.stride(0), x.stride(1)
    if has_mu:  # full [Tx,B,M] contiguous (the module expands broadcasts)
        d.mu_t_stride, d.mu_b_stride = cfg.B * cfg.M, cfg.M
    plan = _DescPlan()
    plan.key, plan.sta, plan.dyn, plan.drop = key, [], [], []
    for i, ps in enumerate(cfg.params):
        s = d.p[ps.slot]
        base = _OFF_P + ps.slot * _PS_SIZE
        s.sta_b_stride = ps.sta_bs
        plan.sta.append((base + _OFF_STA, ps.tensor_idx, 4 * ps.sta_off))
        if ps.dyn_off >= 0:
            s.dyn_t_stride, s.dyn_b_stride = ps.dyn_ts, ps.dyn_bs
            plan.dyn.append((base + _OFF_DYN, ps.dyn_tensor_idx, 4 * ps.dyn_off))
            plan.drop.append((base + _OFF_DROP, i))
        s.lo, s.hi = ps.lo, ps.hi
    d.adj_gtol, d.adj_max_iter, d.adj_stop = cfg.adj_gtol, cfg.adj_max_iter, cfg.adj_stop
    plan.template = bytes(d)
    cfg._plan = plan
    return plan


def _fill_desc(cfg: StepConfig, x, state_in, muwts, ac, elev, ptensors) -> _abi.Desc:
    plan = _desc_plan(cfg, x, muwts is not None)
    buf = bytearray(plan.template)
    pk = _PTR.pack_into
    pk(buf, _D.x.offset, x.data_ptr() + 4 * cfg.t0 * x.stride(0))
    if ac is not None:
        pk(buf, _D.ac.offset, ac.data_ptr())
    if elev is not None:
        pk(buf, _D.elev.offset, elev.data_ptr())
    if muwts is not None:
        pk(buf, _D.muwts.offset, muwts.data_ptr() + 4 * _mu_t0(cfg) * cfg.B * cfg.M)
    if state_in is not None:
        pk(buf, _D.state_in.offset, state_in.data_ptr())
    bases = [t.data_ptr() for t in ptensors]
    for off, ti, boff in plan.sta:
        pk(buf, off, bases[ti] + boff)
    for off, ti, boff in plan.dyn:
        pk(buf, off, bases[ti] + boff)
    params = cfg.params
    for off, i in plan.drop:
        m = params[i].drop
        if m is not None:
            pk(buf, off, m.data_ptr())
    return _abi.Desc.from_buffer(buf)      # the struct keeps `buf` alive


# The library's layout / workspace answers also depend on its (test and tool) environment knobs; their values are
# part of the memo key, so a knob changed between two calls on the same module is seen (a stale TRAJ_PACKED under
# HBVX_STREAM=0 made hbvx_forward refuse the call; a stale workspace size silently demoted the adjoint).
_MEMO_ENV = ("HBVX_KERNEL", "HBVX_FWD", "HBVX_BWD", "HBVX_STREAM", "HBVX_STREAM_MIN", "HBVX_STREAM_MW_MIN", "HBVX_CHUNK",
             "HBVX_CKPT_BLOCK", "HBVX_CKPT_SCRATCH_MB", "HBVX_CKPT_BLOCKWISE", "HBVX_CKPT_ONCHIP")
# os.environ.get() encodes the key and decodes the value on every call (~1 us; ten knobs x several memo look-ups per
# step is a tenth of the delta-MG minibatch's enqueue time): read the mapping underneath it, plain bytes -> bytes
_ENV_DATA = getattr(os.environ, "_data", None)
_MEMO_ENV_B = tuple(os.fsencode(k) for k in _MEMO_ENV)


def _env_key() -> tuple:
    if isinstance(_ENV_DATA, dict):
        return tuple(map(_ENV_DATA.get, _MEMO_ENV_B))
    return tuple(os.environ.get(k) for k in _MEMO_ENV)


def _cached(cfg: StepConfig, key, fn):
    """Per-config memo for the library's size / layout queries (functions of the shape and the knobs above, not of
    the pointers)."""
    memo = cfg.__dict__.setdefault("_memo", {})
    key = (key, _env_key())
    v = memo.get(key)
    if v is None:
        v = memo[key] = fn()
    return v


def _live_rows(n_live4: int) -> int:
    """Rows of a runoff-gradient buffer handed to hbvx_backward_live: the leading 1 .. 4 of [4,T,B]."""
    if not isinstance(n_live4, int) or not 1 <= n_live4 <= 4:
        raise ValueError(f"n_live4 must be an integer in 1 .. 4, got {n_live4!r}")
    return n_live4


def _route_desc(cfg: StepConfig, ptensors, S: int = 4) -> _abi.RouteDesc:
    r = _abi.RouteDesc()
    rs = cfg.route
    r.abi_version = _abi.ABI_VERSION
    r.T, r.B, r.S = cfg.T, cfg.B, S
    r.L = min(cfg.T, _abi.UH_MAXLEN)
    r.raw_sigmoid = 1 if cfg.raw_sigmoid else 0
    r.ra = _ptr(ptensors[rs.tensor_idx], rs.a_off)
    r.rb = _ptr(ptensors[rs.tensor_idx], rs.b_off)
    r.r_stride = rs.stride
    r.a_lo, r.a_hi = rs.a_bounds
    r.b_lo, r.b_hi = rs.b_bounds
    return r


class _NoCtx:
    """Stands in for the autograd context when a call needs no gradient (warm-up under no_grad, inference):
    the forward then runs as a plain function, without the ~20 us of autograd.Function.apply."""
    needs_input_grad = ()

    def save_for_backward(self, *a):
        pass

    def mark_non_differentiable(self, *a):
        pass

    def set_materialize_grads(self, v):
        pass


class PathRecord(NamedTuple):
    """What one call of the path worked on and produced: the inputs hbv_tangent_batch differentiates along."""
    cfg: StepConfig
    x: torch.Tensor
    state_in: Optional[torch.Tensor]
    muwts: Optional[torch.Tensor]
    ac: Optional[torch.Tensor]
    elev: Optional[torch.Tensor]
    ptensors: tuple
    flux: Optional[torch.Tensor]
    uh: Optional[torch.Tensor]
    routed: Optional[torch.Tensor]
    state_out: torch.Tensor
    traj: Optional[torch.Tensor] = None     # the implicit scheme only: its tangent is taken at the solved states


# sensitivity.jvp_batch runs the primal through the module's own forward (warm-up pass, dy_drop draws, caches and
# all) and then needs what each call of the path worked on: inside `record_paths()` every _hbv_forward of THIS thread
# appends its PathRecord to the list the context manager hands out (other threads' calls are not seen).
_TAP = threading.local()


@contextlib.contextmanager
def record_paths(want_traj: bool = True):
    """with record_paths() as records: ... -- the PathRecords of the path calls this thread makes inside the block.
    want_traj=False: the implicit scheme does not keep its trajectory of solved states for the record (the population
    calls re-solve every day themselves; at 671 x 16 x 7300 the trajectory is 1.5 GB)."""
    outer = getattr(_TAP, "records", None), getattr(_TAP, "want_traj", True)
    _TAP.records = records = []
    _TAP.want_traj = want_traj
    try:
        yield records
    finally:
        _TAP.records, _TAP.want_traj = outer


def _hbv_forward(ctx, cfg: StepConfig, x, state_in, muwts, ac, elev, ptensors):
    lib = get_library()
    _check_tensor(lib, x, "x_phy")
    for i, p in enumerate(ptensors):
        _check_tensor(lib, p, f"parameters[{i}]")
        if not p.is_contiguous():
            raise ValueError("parameter tensors must be contiguous")
    if x.stride(2) != 1:
        raise ValueError("x_phy must have unit stride on the forcing axis")
    if muwts is not None:
        _check_tensor(lib, muwts, "muwts")
        if not muwts.is_contiguous() or tuple(muwts.shape[1:]) != (cfg.B, cfg.M):
            raise ValueError("muwts must be a contiguous [T,B,nmul] tensor")
    dev = x.device
    T, B, M = cfg.T, cfg.B, cfg.M
    needs_grad = any(ctx.needs_input_grad)
    keep = needs_grad or cfg.want_traj
    stream = _stream_of(lib, x)

    desc = _fill_desc(cfg, x, state_in, muwts, ac, elev, ptensors)
    out = _abi.FwdOut()
    flux = _out((cfg.n_flux, T, B), dev) \
        if cfg.want_flux else None
    state_out = _out((5, B, M), dev)
    # same two buffers whatever the layout the library asks for (include/hbvx.h, hbvx_traj_layout)
    ckpt = cfg.ckpt_days if (needs_grad and cfg.want_flux and not cfg.want_traj) else 0
    if ckpt:
        # K-day checkpoints [ceil(T/K), 5, N] instead of the trajectory; the adjoint recomputes
        traj = _out(((T + ckpt - 1) // ckpt * 5, B * M), dev)
        layout = _abi.TRAJ_CKPT | (ckpt << 8)
    else:
        traj = _out((5, T + 1, B * M), dev) if keep else None
        layout = (_cached(cfg, ("layout", x.stride(0), x.stride(1)), lambda: lib.preferred_traj_layout(desc))
                  if (keep and cfg.want_flux) else _abi.TRAJ_ROWS)
    out.flux, out.state_out = _ptr(flux), _ptr(state_out)
    out.traj = _ptr(traj)      # (out.aux stays NULL: the library neither writes nor reads it)
    out.n_flux, out.traj_layout = cfg.n_flux, layout
    ctx.early_gp = None
    if needs_grad and cfg.want_flux and any(ctx.needs_input_grad[6:]):
        ctx.early_gp = _early_zero_request(lib, cfg, ptensors, ctx.needs_input_grad[6:], out)
    _call(lib, 'hbvx_forward', lib.forward, desc, out, stream)
    _early_zero_result(lib, cfg, ctx.early_gp)

    routed = uh = None
    if cfg.route is not None and cfg.want_flux:
        r = _route_desc(cfg, ptensors)
        routed = _out((4, T, B), dev)
        uh = _out((B, r.L), dev)
        _call(lib, 'hbvx_route_forward', lib.route_forward, r, _ptr(flux), _ptr(uh), _ptr(routed), stream)

    # BFI (hbv.py:562-567) of the routed (or, without routing, the raw) streamflow and groundwater series: one
    # more output of this node instead of a second autograd.Function on the caller's side
    bfi = None
    if cfg.want_bfi and cfg.want_flux:
        src = routed if routed is not None else flux
        k2 = 3 if routed is not None else _abi.F_Q2
        bfi = _out((B,), dev)
        _call(lib, 'hbvx_bfi', lib.bfi, T, B, _ptr(src), _ptr(src, k2 * T * B), float(cfg.nearzero), _ptr(bfi), stream)

    ctx.cfg = cfg
    ctx.traj_layout = layout
    ctx.desc = desc if needs_grad else None        # its pointers stay valid: every tensor it names is saved below
    ctx.has_bfi = bfi is not None
    ctx.set_materialize_grads(False)
    if needs_grad:
        ctx.save_for_backward(x, state_in, muwts, ac, elev, traj, flux, uh, routed, *ptensors)
    # Under a forward-AD level the final storages carry a tangent (HbvPath.jvp): a state warm-up hands it to the
    # main call.  Otherwise they are a non-differentiable output, as always.
    fwd_ad = _fwAD._current_level >= 0 and not isinstance(ctx, _NoCtx)
    if fwd_ad:
        ctx.save_for_forward(x, state_in, muwts, ac, elev, flux, uh, routed, *ptensors)
    ctx.state_tangent = fwd_ad
    nondiff = [] if fwd_ad else [state_out]
    if traj is not None:
        nondiff.append(traj)
    if nondiff:
        ctx.mark_non_differentiable(*nondiff)
    # every series leaves as its own [T,B,1] view (the shape the flux dictionary holds): one autograd
    # output each, no select / unsqueeze nodes on the caller's side (16 of them cost the host 0.1 ms
    # per call, a fifth of a deltaMG-sized step)
    rrows = tuple(routed.unsqueeze(-1).unbind(0)) if routed is not None else ()
    rows = tuple(flux.unsqueeze(-1).unbind(0)) if flux is not None else ()
    ctx.n_routed = len(rrows)
    tap = getattr(_TAP, "records", None)
    if tap is not None:
        tap.append(PathRecord(cfg, x, state_in, muwts, ac, elev, tuple(ptensors), flux, uh, routed, state_out))
    return (state_out, traj, layout, bfi) + rrows + rows


class HbvPath(torch.autograd.Function):
    """state_out, traj, *routed_rows, *flux_rows = HbvPath.apply(cfg, x, state_in, muwts, ac, elev, *ptensors)
    (use `hbv_path`, which regroups the outputs).

    flux_rows  n_flux tensors [T, B, 1]: the ensemble-mean series (enum hbvx_flux order), views of one
               [n_flux, T, B] buffer.  Separate autograd outputs, so that the adjoint learns WHICH
               series carry gradient (a loss on streamflow touches 1-4 of 12) instead of receiving a
               dense, mostly zero [n_flux, T, B] gradient.
    routed_rows  four [T, B, 1] views: UH-routed Qsim, Q0, Q1, Q2 (none when cfg.route is None)
    state_out  [5, B, M]
    traj       saved trajectory or None; layout `cfg.traj_layout` (see `state_series`).
    """

    @staticmethod
    @_device_guard
    def forward(ctx, cfg: StepConfig, x, state_in, muwts, ac, elev, *ptensors):
        return _hbv_forward(ctx, cfg, x, state_in, muwts, ac, elev, ptensors)

    @staticmethod
    @_device_guard
    def backward(ctx, _g_state, _g_traj, _g_layout, g_bfi, *g_all):
        g_rr, g_rows = list(g_all[:ctx.n_routed]), list(g_all[ctx.n_routed:])
        if g_bfi is not None:
            # the gradient a streamflow loss never asks for: two broadcasts in torch, added to the series' own
            saved_ = ctx.saved_tensors
            flux_, routed_ = saved_[6], saved_[8]
            src = routed_ if routed_ is not None else flux_
            qs, q2 = src[0], src[3 if routed_ is not None else _abi.F_Q2]
            den = qs.sum(0) + ctx.cfg.nearzero
            g_q2 = (100.0 * g_bfi / den).unsqueeze(0).expand_as(q2).unsqueeze(-1)
            g_qs = (-100.0 * g_bfi * q2.sum(0) / (den * den)).unsqueeze(0).expand_as(qs).unsqueeze(-1)
            tgt = g_rr if routed_ is not None else g_rows
            for k, g in ((0, g_qs), (3 if routed_ is not None else _abi.F_Q2, g_q2)):
                tgt[k] = g if tgt[k] is None else tgt[k] + g
        # routed series with gradient: the routing adjoint runs over the leading n_live of the four (a
        # streamflow loss: one), the rows behind them stay zero
        g_routed, n_live = None, 0
        live = [k for k, g in enumerate(g_rr) if g is not None]
        if live:
            n_live = max(live) + 1
            first = g_rr[live[0]]
            if n_live == 1:
                g_routed = first[..., 0].unsqueeze(0)
            else:
                g_routed = torch.zeros((n_live,) + tuple(first.shape[:2]), dtype=torch.float32, device=first.device)
                for k in live:
                    g_routed[k] = g_rr[k][..., 0]
        g_rows = tuple(None if g is None else g[..., 0] for g in g_rows)
        lib = get_library()
        cfg: StepConfig = ctx.cfg
        saved = ctx.saved_tensors
        x, state_in, muwts, ac, elev, traj, flux, uh = saved[:8]
        ptensors = saved[9:]
        dev = x.device
        T, B, M = cfg.T, cfg.B, cfg.M
        stream = _stream_of(lib, x)

        early, ctx.early_gp = ctx.early_gp, None
        rows = [None] * len(ptensors)
        bases = [0] * len(ptensors)
        fill_done, start_fill = None, None
        if _FILL_OVERLAP and lib.is_device:
            gp, rows, bases, start_fill = _overlapped_grad_buffers(lib, cfg, ptensors, ctx.needs_input_grad[6:], early)
        else:
            gp = [_grad_like(lib, p, cfg, i) if ctx.needs_input_grad[6 + i] else None
                  for i, p in enumerate(ptensors)]

        def sta_ptr(idx, off):
            """static / routing gradient address: in the separate last row when the tensor has one"""
            return _ptr(rows[idx], off - bases[idx]) if rows[idx] is not None else _ptr(gp[idx], off)

        def join():
            nonlocal fill_done
            if start_fill is not None and fill_done is None:
                fill_done = start_fill()       # (nothing ran in between: the fill simply starts now)
            if fill_done is not None:
                torch.cuda.current_stream(dev).wait_event(fill_done)
            for big, row in zip(gp, rows):      # (also without a fill: the persistent buffers have separate rows too)
                if row is not None:
                    big[-1] += row

        gq = None
        have = [k for k, g in enumerate(g_rows) if g is not None]
        # rows of gq the adjoint is told exist (hbvx_backward_live, include/hbvx_live_rows.h): below 4 the rows behind
        # them are neither written nor read.  Asked for only where the one-pass static adjoint can take the call --
        # Hbv with every parameter static, row trajectory, routed gradient alone -- and not again for a configuration
        # the library has refused once (a grid the streaming adjoint takes, a knob that pins another family).
        # gq keeps its four rows either way (an allocation from the cache, not a pass over memory): a refused call
        # falls back to `gq[live4:].zero_()` and the four-row entry on the SAME buffer, so do not shrink it
        live4 = 4
        if g_routed is not None and cfg.route is not None:
            r = _route_desc(cfg, ptensors, S=n_live)
            gq = _out((4, T, B), dev)
            if (n_live < 4 and "hbvx_backward_live" not in lib.missing and not have and muwts is None
                    and cfg.model == _abi.MODEL_HBV10 and ctx.traj_layout == _abi.TRAJ_ROWS
                    and not ctx.needs_input_grad[1] and all(ps.dyn_off < 0 for ps in cfg.params)
                    and not _cached(cfg, "live_rows_refused", list)):
                live4 = n_live
            # the rows without a routed gradient must be zero: the routing adjoint's own launch writes them where the
            # library has hbvx_route_backward_rows, else a fill of its own before the call
            in_launch = live4 == 4 and n_live < 4 and "hbvx_route_backward_rows" not in lib.missing
            if live4 == 4 and n_live < 4 and not in_launch:
                gq[n_live:].zero_()
            rs = cfg.route
            gt = gp[rs.tensor_idx]
            ws_bytes = _cached(cfg, ("route_ws", n_live), lambda: lib.route_workspace_bytes(r))
            ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=dev)
            g_routed = g_routed.contiguous()
            g_ab = (sta_ptr(rs.tensor_idx, rs.a_off) if gt is not None else None,
                    sta_ptr(rs.tensor_idx, rs.b_off) if gt is not None else None)
            if in_launch:
                _call(lib, 'hbvx_route_backward', lib.route_backward_rows, r, _ptr(flux), _ptr(uh),
                      _ptr(g_routed), _ptr(gq), 4, *g_ab, _ptr(ws), ws_bytes, stream)
            else:
                _call(lib, 'hbvx_route_backward', lib.route_backward, r, _ptr(flux), _ptr(uh),
                      _ptr(g_routed), _ptr(gq), *g_ab, _ptr(ws), ws_bytes, stream)
        # Which series carry gradient?  Only the four runoff series (the usual losses: streamflow,
        # with or without routing) -> a [4,T,B] buffer and the adjoint's 4-series kernels; anything
        # else -> the dense [n_flux,T,B] form.
        g_flux = None
        if have and max(have) < 4:
            if gq is None:
                gq = torch.zeros((4, T, B), dtype=torch.float32, device=dev)
            for k in have:
                gq[k] += g_rows[k]
        elif have:
            g_flux = torch.zeros((cfg.n_flux, T, B), dtype=torch.float32, device=dev)
            for k in have:
                g_flux[k] = g_rows[k]

        io = _abi.BwdIO()
        io.traj = _ptr(traj)
        io.grad_flux, io.grad_flux4 = _ptr(g_flux), _ptr(gq)
        io.n_flux, io.traj_layout = cfg.n_flux, ctx.traj_layout
        gx = gmu = None
        if ctx.needs_input_grad[1]:
            gx = _zeros_like(lib, x)
            if gx.stride() != x.stride():
                raise ValueError("x_phy must be dense for a forcing gradient")
            io.grad_x = _ptr(gx, cfg.t0 * x.stride(0))
        if muwts is not None and ctx.needs_input_grad[3]:
            gmu = torch.zeros_like(muwts)
            io.grad_muwts = _ptr(gmu, _mu_t0(cfg) * B * M)
        for ps in cfg.params:
            g = io.g[ps.slot]
            gs = gp[ps.tensor_idx]
            if gs is not None:
                g.sta = sta_ptr(ps.tensor_idx, ps.sta_off)
                g.sta_b_stride = ps.sta_bs
            if ps.dyn_off >= 0 and gp[ps.dyn_tensor_idx] is not None:
                g.dyn = _ptr(gp[ps.dyn_tensor_idx], ps.dyn_off)
                g.dyn_t_stride, g.dyn_b_stride = ps.dyn_ts, ps.dyn_bs
        desc = ctx.desc if ctx.desc is not None else _fill_desc(cfg, x, state_in, muwts, ac, elev, ptensors)
        if g_flux is None and gq is None:
            # nothing flows back through the series (a loss on nothing): gradients are zero
            join()
            for ps in cfg.params:
                if ps.dyn_off >= 0 and gp[ps.dyn_tensor_idx] is not None:
                    gp[ps.dyn_tensor_idx].zero_()
            return (None, gx, None, gmu, None, None, *gp)
        if (ctx.traj_layout & 0xFF) == _abi.TRAJ_CKPT:    # block-wise re-materialisation
            ws_bytes = _cached(cfg, ("ckpt_ws", ctx.traj_layout), lambda: lib.ckpt_workspace_bytes(desc, ctx.traj_layout >> 8))
        elif ctx.traj_layout == _abi.TRAJ_ROWS:
            ws_bytes = _cached(cfg, "bwd_ws", lambda: lib.backward_workspace_bytes(desc))
        else:
            ws_bytes = 0                                     # packed: single pass
        if ws_bytes:
            ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
            io.workspace, io.workspace_bytes = _ptr(ws), ws_bytes
        if start_fill is not None:
            fill_done = start_fill()           # beside the adjoint kernels, behind the routing adjoint
            if fill_done is not None and start_fill.gated:
                io.store_gate = fill_done.cuda_event      # the storing kernel waits for the fill; the others do not
        if live4 < 4:
            took = []
            _call(lib, 'hbvx_backward', lambda *a: took.append(lib.backward_live(*a)),
                  desc, io, _live_rows(live4), stream)
            if not took[0]:
                # refused before any launch: the dead rows as zeros after all, and the four-row call from now on
                _cached(cfg, "live_rows_refused", list).append(True)
                gq[live4:].zero_()
                live4 = 4
        if live4 == 4:
            _call(lib, 'hbvx_backward', lib.backward, desc, io, stream)
        join()

        return (None, gx, None, gmu, None, None, *gp)

    @staticmethod
    @_device_guard
    def jvp(ctx, _cfg_t, x_t, s_t, mu_t, ac_t, elev_t, *p_t):
        """Forward mode (torch.autograd.forward_ad): tangents of every output along the inputs' tangents."""
        return _hbv_tangent(ctx, x_t, s_t, mu_t, ac_t, elev_t, p_t)


def _hbv_tangent(ctx, x_t, s_t, mu_t, ac_t, elev_t, p_t):
    """Forward-mode derivative of _hbv_forward along one direction: hbvx_forward_tangent (the recurrence),
    hbvx_route_tangent (the unit hydrograph) and hbvx_bfi_tangent, on the tensors the forward saved."""
    if ac_t is not None or elev_t is not None:
        raise ValueError("forward-mode AD: tangents of ac_all / elev_all are not supported")
    lib = get_library()
    cfg: StepConfig = ctx.cfg
    x, state_in, muwts, ac, elev, flux, uh, routed, *ptensors = ctx.saved_tensors
    dev = x.device
    T, B, M = cfg.T, cfg.B, cfg.M
    stream = _stream_of(lib, x)
    io = _abi.TanIO()
    keep = []                   # the tangent buffers the launch reads: alive until it is enqueued
    if x_t is not None:
        xt = x_t
        if xt.stride() != x.stride():
            xt = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=dev).copy_(x_t)
        keep.append(xt)
        io.x = _ptr(xt, cfg.t0 * x.stride(0))
    if mu_t is not None and muwts is not None:
        mt = mu_t.contiguous()
        keep.append(mt)
        io.muwts = _ptr(mt, _mu_t0(cfg) * B * M)
    if s_t is not None and state_in is not None:
        stt = s_t.contiguous()
        keep.append(stt)
        io.state_in = _ptr(stt)
    pts = [None if t is None else t.contiguous() for t in p_t]
    for ps in cfg.params:
        g = io.p[ps.slot]
        if pts[ps.tensor_idx] is not None:
            g.sta, g.sta_b_stride = _ptr(pts[ps.tensor_idx], ps.sta_off), ps.sta_bs
        if ps.dyn_off >= 0 and pts[ps.dyn_tensor_idx] is not None:
            g.dyn = _ptr(pts[ps.dyn_tensor_idx], ps.dyn_off)
            g.dyn_t_stride, g.dyn_b_stride = ps.dyn_ts, ps.dyn_bs
    tflux = _out((cfg.n_flux, T, B), dev) if cfg.want_flux else None
    tstate = _out((5, B, M), dev)
    io.tan_flux, io.tan_state_out, io.n_flux = _ptr(tflux), _ptr(tstate), cfg.n_flux
    desc = _fill_desc(cfg, x, state_in, muwts, ac, elev, ptensors)
    _call(lib, 'hbvx_forward_tangent', lib.forward_tangent, desc, io, stream)

    troute = None
    if routed is not None:
        r = _route_desc(cfg, ptensors)
        rs = cfg.route
        rt = pts[rs.tensor_idx]
        troute = _out((4, T, B), dev)
        _call(lib, 'hbvx_route_tangent', lib.route_tangent, r, _ptr(flux), _ptr(uh), _ptr(tflux),
              _ptr(rt, rs.a_off), _ptr(rt, rs.b_off), _ptr(troute), stream)
    tbfi = None
    if ctx.has_bfi:
        src, tsrc = (routed, troute) if routed is not None else (flux, tflux)
        k2 = 3 if routed is not None else _abi.F_Q2
        tbfi = _out((B,), dev)
        _call(lib, 'hbvx_bfi_tangent', lib.bfi_tangent, T, B, _ptr(src), _ptr(src, k2 * T * B), _ptr(tsrc),
              _ptr(tsrc, k2 * T * B), float(cfg.nearzero), _ptr(tbfi), stream)
    rrows = tuple(troute.unsqueeze(-1).unbind(0)) if troute is not None else ()
    rows = tuple(tflux.unsqueeze(-1).unbind(0)) if tflux is not None else ()
    return (tstate if ctx.state_tangent else None, None, None, tbfi) + rrows + rows


class BatchOut(NamedTuple):
    """Tangents of one call of the path along D directions.  `flux` [D,n_sel,T,B]: the series of `flux_mask` in
    ascending order; `routed` [D,S,T,B]; `bfi` [D,B]; `state_out` [D,5,B,M] (None: all zero, nothing was launched)."""
    flux: Optional[torch.Tensor]
    routed: Optional[torch.Tensor]
    bfi: Optional[torch.Tensor]
    state_out: Optional[torch.Tensor]


def _batch_source(p: torch.Tensor, t: torch.Tensor, off: int):
    """Where element `off` of parameter tensor `p` lies in its batched tangent `t`: (element offset, per-direction
    stride) or None when the tangent holds nothing for it.  `t` is full ([D, *p.shape]) or, for a [T,B,W] tensor,
    compact ([D,B,W]: the full tangent that is zero everywhere but in row T-1)."""
    if tuple(t.shape[1:]) == tuple(p.shape):
        return off, p.numel()
    row = p[0].numel()
    r, rem = divmod(off, row)
    return (rem, row) if r == p.shape[0] - 1 else None


def hbv_tangent_batch(rec: PathRecord, D: int, x_t=None, mu_t=None, s_t=None, p_t=(), flux_mask: int = 0,
                      n_routed: int = 0, want_bfi: bool = False) -> BatchOut:
    """Forward-mode derivative of one call of the path along D directions at once: hbvx_forward_tangent_batch
    (the hourly model: hbvx_hourly_tangent_batch), hbvx_route_tangent_batch and hbvx_bfi_tangent_batch on what the
    forward worked on (`rec`).  A record of the implicit scheme (HbvAdjPath) goes to hbvx_adj_tangent_batch with the
    trajectory it kept: one series, so flux_mask is 0 or 1 and n_routed 0 or 1, no muwts, no BFI.

    x_t [D, *x.shape], mu_t [D, *muwts.shape], s_t [D,5,B,M], p_t: one tangent per parameter tensor, full or compact
    (_batch_source); None: zero.  Only the flux series of `flux_mask` (bits: enum hbvx_flux) are computed and stored,
    the leading `n_routed` of the four runoff series are routed (their bits must be set), `want_bfi` needs all four
    routed or, without routing, Qsim and Q2."""
    lib = get_library()
    cfg = rec.cfg
    x, ptensors = rec.x, rec.ptensors
    dev = x.device
    T, B, M = cfg.T, cfg.B, cfg.M
    stream = _stream_of(lib, x)
    tb = _abi.TanBatch()
    tb.n_dir, tb.n_flux, tb.flux_mask = D, cfg.n_flux, flux_mask
    keep = []                   # the tangent buffers the launch reads: alive until it is enqueued
    if x_t is not None:
        xt = x_t
        if tuple(xt.stride()[1:]) != tuple(x.stride()):
            span = sum((n - 1) * st for n, st in zip(x.shape, x.stride())) + 1
            xt = torch.empty(D * span, dtype=x.dtype, device=dev).as_strided((D,) + tuple(x.shape),
                                                                              (span,) + tuple(x.stride()))
            xt.copy_(x_t)
        keep.append(xt)
        tb.x, tb.x_d_stride = _ptr(xt, cfg.t0 * x.stride(0)), xt.stride(0)
    if mu_t is not None and rec.muwts is not None:
        mt = mu_t.contiguous()
        keep.append(mt)
        tb.muwts, tb.mu_d_stride = _ptr(mt, _mu_t0(cfg) * B * M), mt.stride(0)
    if s_t is not None and rec.state_in is not None:
        stt = s_t.contiguous()
        keep.append(stt)
        tb.state_in, tb.state_d_stride = _ptr(stt), 5 * B * M
    pts = [None if t is None else t.contiguous() for t in p_t]
    pts += [None] * (len(ptensors) - len(pts))
    keep += pts
    dyn_t0 = None
    for ps in cfg.params:
        g = tb.p[ps.slot]
        t = pts[ps.tensor_idx]
        src = None if t is None else _batch_source(ptensors[ps.tensor_idx], t, ps.sta_off)
        if src is not None:
            g.sta, g.sta_b_stride, tb.sta_d_stride[ps.slot] = _ptr(t, src[0]), ps.sta_bs, src[1]
        t = pts[ps.dyn_tensor_idx] if ps.dyn_off >= 0 else None
        if t is None:
            continue
        p = ptensors[ps.dyn_tensor_idx]
        if tuple(t.shape[1:]) == tuple(p.shape):
            off, ds, t0 = ps.dyn_off, p.numel(), 0
        else:
            # compact: its one row is the tensor's last, day (T_total - 1 - first row of the call) of this call
            row = p[0].numel()
            first, col = divmod(ps.dyn_off, row)
            t0 = p.shape[0] - 1 - first
            if t0 != T - 1:
                raise ValueError("compact parameter tangents need a call that ends at the tensor's last row")
            off, ds = col, row
        if dyn_t0 is not None and dyn_t0 != t0:
            raise ValueError("full and compact tangents cannot be mixed over dynamic parameter tensors")
        dyn_t0 = t0
        g.dyn, tb.dyn_d_stride[ps.slot] = _ptr(t, off), ds
        g.dyn_t_stride, g.dyn_b_stride = ps.dyn_ts, ps.dyn_bs
    tb.dyn_t0 = dyn_t0 or 0
    have_any = bool(tb.x or tb.muwts or tb.state_in or any(tb.p[ps.slot].sta or tb.p[ps.slot].dyn for ps in cfg.params))
    rs = cfg.route if n_routed else None
    rt = pts[rs.tensor_idx] if rs is not None else None
    if not flux_mask and not have_any:
        return BatchOut(None, None, None, None)     # a warm-up nothing moves: its state tangent is zero
    nsel = bin(flux_mask).count("1")
    tflux = _out((D, nsel, T, B), dev) if flux_mask else None
    tstate = _out((D, 5, B, M), dev)
    tb.tan_flux, tb.tan_state_out = _ptr(tflux), _ptr(tstate)
    desc = _fill_desc(cfg, x, rec.state_in, rec.muwts, rec.ac, rec.elev, ptensors)
    if cfg.model == _abi.MODEL_HOURLY:      # a kernel and an entry point of its own (include/hbvx.h)
        _call(lib, 'hbvx_hourly_tangent_batch', lib.hourly_tangent_batch, desc, tb, stream)
    elif cfg.model == _abi.MODEL_HBVADJ:    # likewise; differentiates at the solved states of the recorded call
        _call(lib, 'hbvx_adj_tangent_batch', lib.adj_tangent_batch, desc, tb, _ptr(rec.traj), stream)
    else:
        _call(lib, 'hbvx_forward_tangent_batch', lib.forward_tangent_batch, desc, tb, stream)

    troute = None
    if rs is not None:
        if flux_mask & ((1 << n_routed) - 1) != (1 << n_routed) - 1:
            raise ValueError("routing needs the leading runoff series in flux_mask")
        r = _route_desc(cfg, ptensors, S=n_routed)
        a = b = None
        if rt is not None:
            a = _batch_source(ptensors[rs.tensor_idx], rt, rs.a_off)
            b = _batch_source(ptensors[rs.tensor_idx], rt, rs.b_off)
        troute = _out((D, n_routed, T, B), dev)
        _call(lib, 'hbvx_route_tangent_batch', lib.route_tangent_batch, r, D, _ptr(rec.flux), _ptr(rec.uh), _ptr(tflux),
              nsel * T * B, _ptr(rt, a[0]) if a else None, _ptr(rt, b[0]) if b else None, a[1] if a else 0,
              _ptr(troute), stream)
    tbfi = None
    if want_bfi:
        if troute is not None:
            src, tsrc, k2, tk2, ds = rec.routed, troute, 3, 3, n_routed * T * B
        else:
            src, tsrc, k2, ds = rec.flux, tflux, _abi.F_Q2, nsel * T * B
            tk2 = bin(flux_mask & ((1 << k2) - 1)).count("1")
        if tsrc is None or (troute is not None and n_routed != 4) or (troute is None and flux_mask & 9 != 9):
            raise ValueError("BFI needs the streamflow and groundwater series")
        tbfi = _out((D, B), dev)
        _call(lib, 'hbvx_bfi_tangent_batch', lib.bfi_tangent_batch, T, B, D, _ptr(src), _ptr(src, k2 * T * B), _ptr(tsrc),
              _ptr(tsrc, tk2 * T * B), ds, float(cfg.nearzero), _ptr(tbfi), stream)
    return BatchOut(tflux, troute, tbfi, tstate)


def gram(series: torch.Tensor, w: Optional[torch.Tensor] = None, r: Optional[torch.Tensor] = None):
    """Per-basin normal equations of C series on a [T,B] grid through hbvx_gram (include/hbvx.h), on the current stream:
        gram[b,c,e] = sum_t w s_c s_e [B,C,C],  rhs[b,c] = sum_t w s_c r [B,C],  cost[b] = sum_t w r^2 [B].
    series [C,T,B] float32 with [T,B] contiguous inside each series (any stride >= T*B between series: the layout the
    tangent kernels write, a slice of it included); w, r [T,B] or None (w: ones; r: rhs and cost come back None).
    The kernel multiplies what it is given: w = 0 does not neutralise a NaN in r or series (masking is the caller's)."""
    lib = get_library()
    lib.require("hbvx_gram")
    _check_tensor(lib, series, "series")
    if series.dim() != 3 or min(series.shape) < 1:
        raise ValueError(f"series must be a non-empty [C,T,B] tensor, got {tuple(series.shape)}")
    Cn, T, B = (int(n) for n in series.shape)
    if series.stride(2) != 1 or series.stride(1) != B or (Cn > 1 and series.stride(0) < T * B):
        series = series.contiguous()
    g = _abi.GramDesc(abi_version=_abi.ABI_VERSION, T=T, B=B, C=Cn, series_stride=series.stride(0) if Cn > 1 else T * B)
    for name, t in (("w", w), ("r", r)):
        if t is None:
            continue
        _check_tensor(lib, t, name)
        if tuple(t.shape) != (T, B):
            raise ValueError(f"{name} must be [{T},{B}] like a series, got {tuple(t.shape)}")
        if t.device != series.device:
            raise ValueError(f"{name} lives on {t.device}, series on {series.device}")
    wc = None if w is None else w.contiguous()
    rc = None if r is None else r.contiguous()
    dev = series.device
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        out = _out((B, Cn, Cn), dev)
        rhs = _out((B, Cn), dev) if rc is not None else None
        cost = _out((B,), dev) if rc is not None else None
        ws_bytes = lib.gram_workspace_bytes(g)
        ws = _out(((max(ws_bytes, 4) + 3) // 4,), dev)      # poisoned with the outputs: the call must not need it cleared
        _call(lib, 'hbvx_gram', lib.gram, g, _ptr(series), _ptr(wc), _ptr(rc), _ptr(out), _ptr(rhs), _ptr(cost), _ptr(ws),
              ws_bytes, _stream_of(lib, series))
    return out, rhs, cost


def quadform(series: torch.Tensor, factor: torch.Tensor) -> torch.Tensor:
    """Per-basin quadratic form of C series on a [T,B] grid through hbvx_quadform (include/hbvx.h), on the current
    stream:  q[t,b] = |factor[b] @ series[:,t,b]|^2 = s^T (factor[b]^T factor[b]) s, [T,B] float32, >= 0.
    series [C,T,B] float32 with [T,B] contiguous inside each series (any stride >= T*B between series: the layout the
    tangent kernels write, a slice of it included); factor [B,C,C] float32, lower-triangular: what lies above the
    diagonal is never read."""
    lib = get_library()
    lib.require("hbvx_quadform")
    _check_tensor(lib, series, "series")
    _check_tensor(lib, factor, "factor")
    if series.dim() != 3 or min(series.shape) < 1:
        raise ValueError(f"series must be a non-empty [C,T,B] tensor, got {tuple(series.shape)}")
    Cn, T, B = (int(n) for n in series.shape)
    if tuple(factor.shape) != (B, Cn, Cn):
        raise ValueError(f"factor must be [{B},{Cn},{Cn}] (one lower-triangular matrix per basin), got {tuple(factor.shape)}")
    if factor.device != series.device:
        raise ValueError(f"factor lives on {factor.device}, series on {series.device}")
    if series.stride(2) != 1 or series.stride(1) != B or (Cn > 1 and series.stride(0) < T * B):
        series = series.contiguous()
    g = _abi.GramDesc(abi_version=_abi.ABI_VERSION, T=T, B=B, C=Cn, series_stride=series.stride(0) if Cn > 1 else T * B)
    fc = factor.contiguous()
    dev = series.device
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        out = _out((T, B), dev)
        ws_bytes = lib.quadform_workspace_bytes(g)
        ws = _out(((max(ws_bytes, 4) + 3) // 4,), dev)      # poisoned with the output: the call must not need it cleared
        _call(lib, 'hbvx_quadform', lib.quadform, g, _ptr(series), _ptr(fc), _ptr(out), _ptr(ws), ws_bytes,
              _stream_of(lib, series))
    return out


POP_MAX_CAND = 65535       # candidates of one launch of a population export (a grid dimension)


class PopTerm(NamedTuple):
    """One scored series of a population call, the flow or the aux term; what a form does not use stays None.
    target, w   [rows,B] float32, rows = T_out, or the periods of `ends`; w may be None (ones).  The target is ALREADY
                transformed, and the kernel multiplies what it is given: the caller masks.
    shift       [B] float32, the point the moments are taken about (the weighted mean of target); not for the cost form.
    eps         [B] float32, read under transform 'log' only.
    transform   'none' | 'sqrt' | 'log', the flow's (the aux series is never transformed); not for the cost form.
    ends        the period form: 1-D int32 tensor on the device of the record, the closing days of the periods, 0-based
                in the scored days, ascending (the caller checks that; the kernel is safe either way).
    series      the aux term: which series, a value of the entry's table in _abi.POPULATION."""
    target: Optional[torch.Tensor]
    w: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    eps: Optional[torch.Tensor] = None
    transform: Optional[str] = None
    ends: Optional[torch.Tensor] = None
    series: Optional[int] = None


def population(rec: PathRecord, entry: str, cand_sources: dict, route_cands, flow: PopTerm,
               aux: Optional[PopTerm] = None, t_first: int = 0, want_sim: bool = False):
    """The scores of P candidate static-parameter sets on one recorded call of the path, through the population export
    `entry` (a key of _abi.POPULATION; include/hbvx.h states each one's arithmetic) on the current stream:
    (flow_out, aux_out), each (sse, s1, s2, s3, sim) -- [P,B] float32 sums and the series [P,rows,B] or None without
    want_sim; rows = T_out = rec.cfg.T - t_first, under the period form the periods of the term's calendar.  The cost
    form (hbvx_[adj_]population_cost) gives its cost as sse and None moments.  aux_out is None without an aux term.

    cand_sources  {parameter slot: (cands, column)}: candidate c's values of that slot for basin b are
                  cands[c, b, column : column + M] of the compact float32 [P,B,C] tensor `cands`; slots not named keep
                  the recorded call's static values.
    route_cands   (a, b), each None or (cands, column): the candidates' routing inputs; None keeps the recorded one.
                  Ignored when the recorded call does not route.
    flow, aux     `PopTerm`s.  The joint form needs `aux`, the period form takes it or not (aux None, or all of its
                  fields None), the others refuse it.  The entries of the implicit scheme take a record of HbvAdjPath
                  only, and their aux series is one of the five solved storages.
    More than POP_MAX_CAND candidates go in several launches; a candidate's bits do not depend on the split."""
    return _population(rec, entry, _abi.POPULATION[entry], cand_sources, route_cands, flow, aux, t_first, want_sim)[:2]


def _out_i32(shape, device) -> torch.Tensor:
    """`_out` for int32 counts: under HBVX_DEBUG_POISON the fill is -1, which no count can be."""
    if _POISON:
        return torch.full(shape, -1, dtype=torch.int32, device=device)
    return torch.empty(shape, dtype=torch.int32, device=device)


def population_fdc(rec: PathRecord, cand_sources: dict, route_cands, flow: PopTerm, thresholds: torch.Tensor,
                   t_first: int = 0, want_sim: bool = False):
    """hbvx_population_fdc (include/hbvx_pop_fdc.h) on one recorded call of the path: `population` on
    hbvx_population_stats -- the same arguments, the same flow_out bit for bit -- and the simulated flow-duration curve at
    `thresholds`, [K,B] float32 on the device of the record, K in 1.._abi.POP_FDC_MAX_THR, in the units of the flow.
    Returns (flow_out, (count [P,K,B] int32, volume [P,K,B] float32)): on how many scored days with a weight > 0 the
    routed flow was above each threshold, and the sum of the flow over those days."""
    return _population(rec, "hbvx_population_fdc", _abi.POP_FDC_ENTRY, cand_sources, route_cands, flow, None, t_first,
                       want_sim, thresholds)[:3:2]


def population_events(rec: PathRecord, cand_sources: dict, route_cands, flow: PopTerm, starts: torch.Tensor,
                      ends: torch.Tensor, t_first: int = 0, want_sim: bool = False):
    """hbvx_population_events (include/hbvx_pop_events.h) on one recorded call of the path: `population` on
    hbvx_population_stats -- the same arguments, the same flow_out bit for bit -- and the peak, the day of the peak and the
    volume of every candidate's routed flow inside E event windows per basin.
    starts, ends  [E,B] int32 contiguous on the device of the record, E in 1..T_out: inclusive SCORED days (day 0 is
                  t_first), walked in row order by the header's cursor rule -- a row that is not ahead of the basin's
                  previous live one, start < 0 or end < start is an absent slot, end is clamped to T_out - 1: any content
                  is safe.
    Returns (flow_out, (peak [P,E,B] float32, peak_day [P,E,B] int32, volume [P,E,B] float32)); an absent slot holds
    -inf, -1, +0."""
    return _population(rec, "hbvx_population_events", _abi.POP_EVENTS_ENTRY, cand_sources, route_cands, flow, None, t_first,
                       want_sim, None, (starts, ends))[::3]


class EnsTerm(NamedTuple):
    """What `population_ensemble` adds to a stats call: the window, the particle count and the per-particle inputs."""
    P: int
    t_begin: int
    t_end: int
    state_in: Optional[torch.Tensor] = None
    hist_in: Optional[torch.Tensor] = None
    ancestor: Optional[torch.Tensor] = None
    p_mul: Optional[torch.Tensor] = None
    t_add: Optional[torch.Tensor] = None


def population_ensemble(rec: PathRecord, cand_sources: dict, route_cands, flow: PopTerm, ens: EnsTerm, t_first: int = 0,
                        want_sim: bool = False):
    """hbvx_population_ensemble (include/hbvx_pop_ens.h) on one recorded call of the path: `population` on
    hbvx_population_stats over the days ens.t_begin .. ens.t_end-1 of the record, every candidate a PARTICLE with
    storages, routing history and forcing noise of its own.  All tensors float32 (ancestor int32), contiguous, on the
    device of the record:
    ens.P         the particles; the candidate columns are optional here (none: every particle has the record's values),
                  and a candidate tensor must hold ens.P sets.
    flow          target / w are WINDOW-RELATIVE, [rows,B] with rows = t_end - max(t_begin, t_first) the scored days of the
                  window; rows == 0 is valid (target may be None) and gives +0 chains.
    state_in      [Ps,5,B,M] or None (the record's start state); hist_in [Ps,14,B] or None (zeros): Ps = P, or with
                  `ancestor` any count >= 1.
    ancestor      [P,B] int32 or None (the identity): the source particle c of basin b starts from.  Values outside
                  0..Ps-1 are clamped by the kernel; validity is the caller's.
    p_mul, t_add  None (no operation), [P,B] (a constant per particle) or [P,t_end-t_begin,B].
    Returns (flow_out, (state_out [P,5,B,M], hist_out [P,14,B] or None when the record does not route)); the series of
    flow_out is [P,rows,B].  More than POP_MAX_CAND particles go in several launches; a particle's bits do not depend on
    the split."""
    return _population(rec, "hbvx_population_ensemble", _abi.POP_ENS_ENTRY, cand_sources, route_cands, flow, None, t_first,
                       want_sim, ens=ens)[::4]


def _check_ens(lib, ens, cfg, t_first, dev):
    """population_ensemble's own checks -> (rows, Ps, W): the scored days and the days of the window, the sources."""
    T, B, M = cfg.T, cfg.B, cfg.M
    if not all(isinstance(v, int) and not isinstance(v, bool) for v in (ens.P, ens.t_begin, ens.t_end)):
        raise TypeError("n_particles, t_begin and t_end must be integers")
    if ens.P < 1:
        raise ValueError(f"population_ensemble needs at least one particle, got {ens.P}")
    if not 0 <= ens.t_begin < ens.t_end <= T:
        raise ValueError(f"the window must satisfy 0 <= t_begin < t_end <= {T}, got {ens.t_begin} .. {ens.t_end}")
    W = ens.t_end - ens.t_begin
    Ps = ens.P
    if ens.ancestor is not None:        # the sources may then be any number: the leading size of what is given
        for t in (ens.hist_in, ens.state_in):
            if t is not None and t.dim() >= 1:
                Ps = int(t.shape[0])
    for name, t, tail in (("state_in", ens.state_in, (5, B, M)), ("hist_in", ens.hist_in, (_abi.POP_ENS_HIST, B))):
        if t is None:
            continue
        _check_tensor(lib, t, name)
        if tuple(t.shape) != (Ps,) + tail or Ps < 1 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous {[Ps] + list(tail)} tensor on {dev}, got {tuple(t.shape)} on "
                             f"{t.device}")
    if ens.ancestor is not None:
        a = ens.ancestor
        if not torch.is_tensor(a) or a.dtype != torch.int32:
            raise TypeError(f"ancestor must be an int32 tensor, got {a.dtype if torch.is_tensor(a) else type(a).__name__}")
        if tuple(a.shape) != (ens.P, B) or not a.is_contiguous() or a.device != dev:
            raise ValueError(f"ancestor must be a contiguous [{ens.P},{B}] tensor on {dev}, got {tuple(a.shape)} on {a.device}")
    for name, t in (("p_mul", ens.p_mul), ("t_add", ens.t_add)):
        if t is None:
            continue
        _check_tensor(lib, t, name)
        if tuple(t.shape) not in ((ens.P, B), (ens.P, W, B)) or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous [{ens.P},{B}] or [{ens.P},{W},{B}] tensor on {dev}, got "
                             f"{tuple(t.shape)} on {t.device}")
    return max(0, ens.t_end - max(ens.t_begin, t_first)), Ps, W


def _population(rec, entry, info, cand_sources, route_cands, flow, aux, t_first, want_sim, thr=None, events=None, ens=None):
    """`population` / `population_fdc` / `population_events` / `population_ensemble`: (flow_out, aux_out, fdc_out,
    events_out, ens_out), fdc_out None without `thr`, events_out None without `events`, ens_out None without `ens`."""
    what = entry[len("hbvx_"):]
    cost_form, period_form = info.struct is _abi.Pop, info.struct is _abi.PopPeriod
    if not cost_form:
        if flow.transform not in _abi.POP_TRANSFORMS:
            raise ValueError(f"transform must be one of {sorted(_abi.POP_TRANSFORMS)}, got {flow.transform!r}")
        if flow.transform == "log" and flow.eps is None:
            raise ValueError(f"{what}: transform 'log' needs eps")
    cfg = rec.cfg
    if info.implicit:
        if cfg.model != _abi.MODEL_HBVADJ:
            raise ValueError(f"{what}: the record is not a call of the implicit scheme (HbvAdjPath)")
        if cfg.adj_stop == 1:
            raise ValueError(f"{what}: the batch-wide Newton stopping rule (newton_stop='global') votes over the 64 lanes "
                             "of a wave; a candidate's cost must not depend on that")
    if info.aux_series is None:
        if aux is not None:
            raise ValueError(f"{what} has no aux term")
    elif period_form and (aux is None or aux.series is None):
        if aux is not None and any(t is not None for t in (aux.target, aux.w, aux.shift, aux.ends)):
            raise ValueError(f"{what}: aux arguments without aux_series")
        aux = None
    else:
        if aux is None or aux.series not in info.aux_series.values():
            raise ValueError(f"{what}: aux_series must be one of {sorted(info.aux_series.values())} "
                             f"({'storage' if info.implicit else 'hbvx_flux'} indices), got "
                             f"{None if aux is None else aux.series!r}")
        if period_form and (aux.target is None or aux.shift is None or aux.ends is None):
            raise ValueError(f"{what} needs aux_target, aux_shift and aux_end with aux_series")
        if aux.target is None or aux.shift is None:
            raise ValueError(f"{what} needs aux_target and aux_shift")
    lib = get_library()
    lib.require(entry)
    call = getattr(lib, what)
    x, ptensors = rec.x, rec.ptensors
    dev = x.device
    T, B, M = cfg.T, cfg.B, cfg.M
    T_out = T - t_first
    if not 0 <= t_first < T:
        raise ValueError(f"t_first must be in 0..{T - 1}, got {t_first}")
    named = list(cand_sources.values()) + [s for s in (route_cands or ()) if s is not None]
    if not named and ens is None:
        raise ValueError(f"{what} needs at least one candidate column")
    if ens is not None:
        rows_e, Ps, W = _check_ens(lib, ens, cfg, t_first, dev)
    if named:
        cands = named[0][0]
        _check_tensor(lib, cands, "candidates")
        if cands.dim() != 3 or int(cands.shape[1]) != B or not cands.is_contiguous() or cands.device != dev:
            raise ValueError(f"candidates must be a contiguous [P,{B},C] tensor on {dev}, got {tuple(cands.shape)} on {cands.device}")
        P, Cn = int(cands.shape[0]), int(cands.shape[2])
        if P < 1:
            raise ValueError(f"{what} needs at least one candidate")
        if ens is not None and P != ens.P:
            raise ValueError(f"{what}: the candidates hold {P} sets for {ens.P} particles")
    else:
        cands, P, Cn = None, ens.P, 0       # (the ensemble form: every particle has the record's static values)
    for t, col in named:
        if t is not cands:
            raise ValueError("all candidate columns must lie in one compact tensor")
    for slot, (_, col) in cand_sources.items():
        if not 0 <= col <= Cn - M:
            raise ValueError(f"candidate column {col} of slot {slot} does not hold {M} members in {Cn} columns")
    for s in (route_cands or ()):
        if s is not None and not 0 <= s[1] < Cn:
            raise ValueError(f"routing candidate column {s[1]} outside the {Cn} columns")
    rows_f = rows_a = T_out         # rows of the flow's and the aux term's targets, weights and series
    if ens is not None:
        rows_f = rows_e             # the scored days of the window
        if rows_f > 0 and flow.target is None:
            raise ValueError(f"{what}: the window has {rows_f} scored days and no target")
    ends = [None, None]
    if period_form:
        for i, (name, e) in enumerate((("flow_end", flow.ends), ("aux_end", None if aux is None else aux.ends))):
            if e is None:
                continue
            if e.dtype != torch.int32 or e.dim() != 1 or e.device != dev or not 1 <= e.numel() <= T_out:
                raise ValueError(f"{name} must be a 1-D int32 tensor of 1..{T_out} closing days on {dev}, got "
                                 f"{e.dtype} {tuple(e.shape)} on {e.device}")
            ends[i] = e.contiguous()
        rows_f = int(ends[0].numel())
        rows_a = int(ends[1].numel()) if ends[1] is not None else 0
    no_aux = PopTerm(None)
    for name, t, rows in (("target", flow.target, rows_f), ("w", flow.w, rows_f),
                          ("aux_target", (aux or no_aux).target, rows_a), ("aux_w", (aux or no_aux).w, rows_a)):
        if t is None:
            continue
        _check_tensor(lib, t, name)
        if tuple(t.shape) != (rows, B) or t.device != dev:
            raise ValueError(f"{name} must be [{rows},{B}] on {dev}, got {tuple(t.shape)} on {t.device}")
    shift, eps = (None, None) if cost_form else (flow.shift, flow.eps if flow.transform == "log" else None)
    for name, t in (("shift", shift), ("eps", eps), ("aux_shift", (aux or no_aux).shift)):
        if t is None:
            continue
        _check_tensor(lib, t, name)
        if tuple(t.shape) != (B,) or t.device != dev:
            raise ValueError(f"{name} must be [{B}] on {dev}, got {tuple(t.shape)} on {t.device}")
    if thr is not None:
        _check_tensor(lib, thr, "thresholds")
        if thr.dim() != 2 or int(thr.shape[1]) != B or not 1 <= int(thr.shape[0]) <= _abi.POP_FDC_MAX_THR or thr.device != dev:
            raise ValueError(f"thresholds must be [K,{B}] on {dev} with K in 1..{_abi.POP_FDC_MAX_THR}, got "
                             f"{tuple(thr.shape)} on {thr.device}")
        thr = thr.contiguous()
    if events is not None:
        for name, t in zip(("starts", "ends"), events):
            if not torch.is_tensor(t) or t.dtype != torch.int32:
                raise TypeError(f"{name} must be an int32 tensor, got {t.dtype if torch.is_tensor(t) else type(t).__name__}")
            if t.dim() != 2 or int(t.shape[1]) != B or not 1 <= int(t.shape[0]) <= T_out or not t.is_contiguous() \
                    or t.device != dev:
                raise ValueError(f"{name} must be a contiguous [E,{B}] tensor of 1..{T_out} events on {dev}, got "
                                 f"{tuple(t.shape)} on {t.device}")
        if tuple(events[0].shape) != tuple(events[1].shape):
            raise ValueError(f"starts is {tuple(events[0].shape)}, ends {tuple(events[1].shape)}")
    tc, wc, shc, epc = (None if t is None else t.contiguous() for t in (flow.target, flow.w, shift, eps))
    atc, awc, ashc = (None if t is None else t.contiguous() for t in (aux or no_aux)[:3])
    stream = _stream_of(lib, x)
    desc = _fill_desc(cfg, x, rec.state_in, rec.muwts, rec.ac, rec.elev, ptensors)
    route = _route_desc(cfg, ptensors, S=1) if cfg.route is not None else None
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        cost = _out((P, B), dev)
        moments = (None, None, None) if cost_form else tuple(_out((P, B), dev) for _ in range(3))
        sim = _out((P, rows_f, B), dev) if want_sim else None
        aux_out = None
        if aux is not None:
            aux_out = tuple(_out((P, B), dev) for _ in range(4)) + ((_out((P, rows_a, B), dev) if want_sim else None),)
        fdc_out = None
        if thr is not None:
            K = int(thr.shape[0])
            fdc_out = (_out_i32((P, K, B), dev), _out((P, K, B), dev))
        ev_out = None
        if events is not None:
            E = int(events[0].shape[0])
            ev_out = (_out((P, E, B), dev), _out_i32((P, E, B), dev), _out((P, E, B), dev))
            if _POISON:
                ev_out[1].fill_(-2 ** 31)       # (-1, _out_i32's fill, is what an absent slot holds)
        ens_out = None
        if ens is not None:
            ens_out = (_out((P, 5, B, M), dev), _out((P, _abi.POP_ENS_HIST, B), dev) if route is not None else None)
        for c0 in range(0, P, POP_MAX_CAND):
            args = info.struct()
            pq, pj, ps, pop = _abi.pop_levels(args)
            pop.n_cand, pop.t_first = min(POP_MAX_CAND, P - c0), t_first
            for slot, (_, col) in cand_sources.items():
                s = pop.p[slot]
                s.sta, s.c_stride, s.b_stride = _ptr(cands, c0 * B * Cn + col), B * Cn, Cn
            if route is not None:
                pop.route = _C.pointer(route)
                ra, rb = route_cands or (None, None)
                if ra is not None:
                    pop.ra = _ptr(cands, c0 * B * Cn + ra[1])
                if rb is not None:
                    pop.rb = _ptr(cands, c0 * B * Cn + rb[1])
                pop.r_c_stride, pop.r_b_stride = B * Cn, Cn
            pop.target, pop.w = _ptr(tc), _ptr(wc)
            pop.cost = _ptr(cost, c0 * B)
            pop.sim = _ptr(sim, c0 * rows_f * B)
            if ps is not None:
                ps.transform, ps.shift, ps.eps = _abi.POP_TRANSFORMS[flow.transform], _ptr(shc), _ptr(epc)
                ps.s1, ps.s2, ps.s3 = (_ptr(m, c0 * B) for m in moments)
            if pj is not None and aux is None:
                pj.aux_series = _abi.POP_NO_AUX
            elif pj is not None:
                pj.aux_series, pj.aux_target, pj.aux_w, pj.aux_shift = aux.series, _ptr(atc), _ptr(awc), _ptr(ashc)
                pj.aux_sse, pj.aux_s1, pj.aux_s2, pj.aux_s3 = (_ptr(m, c0 * B) for m in aux_out[:4])
                pj.aux_sim = _ptr(aux_out[4], c0 * rows_a * B)
            if pq is not None:
                pq.n_flow_periods, pq.flow_end = rows_f, ends[0].data_ptr()
                if ends[1] is not None:
                    pq.n_aux_periods, pq.aux_end = rows_a, ends[1].data_ptr()
            if thr is not None:
                args.abi_version, args.n_thr, args.thr = _abi.POP_FDC_ABI_VERSION, K, _ptr(thr)
                args.count, args.volume = fdc_out[0].data_ptr() + 4 * c0 * K * B, _ptr(fdc_out[1], c0 * K * B)
            if events is not None:
                args.abi_version, args.n_events = _abi.POP_EVENTS_ABI_VERSION, E
                args.start, args.end = events[0].data_ptr(), events[1].data_ptr()
                args.peak, args.volume = _ptr(ev_out[0], c0 * E * B), _ptr(ev_out[2], c0 * E * B)
                args.peak_day = ev_out[1].data_ptr() + 4 * c0 * E * B
            if ens is not None:
                args.t_begin, args.t_end, args.n_src, args.src_first = ens.t_begin, ens.t_end, Ps, c0
                args.state_in, args.hist_in = _ptr(ens.state_in), _ptr(ens.hist_in)
                args.state_out, args.hist_out = _ptr(ens_out[0], c0 * 5 * B * M), _ptr(ens_out[1], c0 * _abi.POP_ENS_HIST * B)
                if ens.ancestor is not None:
                    args.ancestor = ens.ancestor.data_ptr() + 4 * c0 * B
                for t, name in ((ens.p_mul, "pm"), (ens.t_add, "ta")):
                    if t is not None:
                        per_day = t.dim() == 3
                        cs = W * B if per_day else B
                        setattr(args, "p_mul" if name == "pm" else "t_add", _ptr(t, c0 * cs))
                        setattr(args, name + "_c_stride", cs)
                        setattr(args, name + "_t_stride", B if per_day else 0)
            _call(lib, entry, call, desc, args, stream)
    return (cost,) + moments + (sim,), aux_out, fdc_out, ev_out, ens_out


class PathOut(NamedTuple):
    """What one call of the path returns.  `flux`: tuple of the n_flux series [T,B,1] (index it with the hbvx_flux
    enum) or None when cfg.want_flux is False; `routed`: tuple of the four UH-routed runoff series [T,B,1] or
    None; `traj` + `traj_layout`: the saved trajectory (see `state_series`); `bfi` [B] when cfg.want_bfi."""
    flux: Optional[tuple]
    routed: Optional[tuple]
    state_out: torch.Tensor
    traj: Optional[torch.Tensor]
    traj_layout: int
    bfi: Optional[torch.Tensor]


def hbv_path(cfg: StepConfig, x, state_in, muwts, ac, elev, *ptensors) -> PathOut:
    """Run the path.  A call that cannot need a gradient (grad mode off, or no input requires one) runs the
    forward as a plain function; otherwise through the autograd node `HbvPath`."""
    dual = has_tangent(x, state_in, muwts, ac, elev, ptensors)
    if dual and has_tangent(ac, elev):
        raise ValueError("forward-mode AD: tangents of ac_all / elev_all are not supported")
    if dual or (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in ptensors)
                                             or (muwts is not None and muwts.requires_grad)
                                             or (state_in is not None and state_in.requires_grad))):
        outs = HbvPath.apply(cfg, x, state_in, muwts, ac, elev, *ptensors)
    elif x.is_cuda and torch.cuda.current_device() != x.device.index:
        with torch.cuda.device(x.device):
            outs = _hbv_forward(_NoCtx(), cfg, x, state_in, muwts, ac, elev, ptensors)
    else:
        outs = _hbv_forward(_NoCtx(), cfg, x, state_in, muwts, ac, elev, ptensors)
    state_out, traj, layout, bfi = outs[:4]
    nr = 4 if (cfg.route is not None and cfg.want_flux) else 0
    return PathOut((outs[4 + nr:] or None), (outs[4:4 + nr] or None), state_out, traj, layout, bfi)


def state_series(traj: torch.Tensor, layout: int, T: int, B: int, M: int):
    """The five storages entering day t, t = 0..T (t = T: after the last day), as [T+1, B, M] views of
    the saved trajectory, whatever its layout (include/hbvx.h, hbvx_traj_layout).  Zero-copy."""
    flat = traj.reshape(-1)
    N = B * M
    if layout == _abi.TRAJ_PACKED:
        rec = flat[: 4 * (T + 1) * N].view(T + 1, B, M, 4)
        slz = flat[4 * (T + 1) * N: 5 * (T + 1) * N].view(T + 1, B, M)
        return tuple(rec[..., k] for k in range(4)) + (slz,)
    rows = flat.view(5, T + 1, B, M)
    return tuple(rows[k] for k in range(5))


class HbvAdjPath(torch.autograd.Function):
    """flux, routed, state_out = HbvAdjPath.apply(cfg, x, state_in, *ptensors)

    Implicit (backward-Euler) HBV, reference hbv_adj.py:227-330.  flux [1,T,B] = ensemble-mean
    q0+q1+q2 at the solved states; routed [1,T,B] = its UH routing; state_out [5,B,M] is
    differentiable so that a warm-up call can be chained in front of the main call (the reference
    differentiates through its warm-up, hbv_adj.py:257-274)."""

    @staticmethod
    @_device_guard
    def forward(ctx, cfg: StepConfig, x, state_in, *ptensors):
        lib = get_library()
        _check_tensor(lib, x, "x_phy")
        for i, p in enumerate(ptensors):
            _check_tensor(lib, p, f"parameters[{i}]")
            if not p.is_contiguous():
                raise ValueError("parameter tensors must be contiguous")
        dev = x.device
        T, B, M = cfg.T, cfg.B, cfg.M
        needs_grad = any(ctx.needs_input_grad)
        stream = _stream_of(lib, x)
        out = _abi.FwdOut()
        flux = _out((1, T, B), dev) if cfg.want_flux else None
        state_out = _out((5, B, M), dev)
        tap = getattr(_TAP, "records", None)    # inside record_paths(): the tangent needs the solved states too
        traj = _out((5, T + 1, B * M), dev) if (needs_grad or (tap is not None and _TAP.want_traj)) else None
        out.flux, out.state_out, out.traj, out.n_flux = _ptr(flux), _ptr(state_out), _ptr(traj), 1
        if state_in is not None:
            state_in = state_in.contiguous()
        desc = _fill_desc(cfg, x, state_in, None, None, None, ptensors)
        ctx.early_gp = None
        if needs_grad and any(ctx.needs_input_grad[3:]):
            ctx.early_gp = _early_zero_request(lib, cfg, ptensors, ctx.needs_input_grad[3:], out)
        _call(lib, 'hbvx_adj_forward', lib.adj_forward, desc, out, stream)
        _early_zero_result(lib, cfg, ctx.early_gp)
        routed = uh = None
        if cfg.route is not None and cfg.want_flux:
            r = _route_desc(cfg, ptensors, S=1)
            routed = _out((1, T, B), dev)
            uh = _out((B, r.L), dev)
            _call(lib, 'hbvx_route_forward', lib.route_forward, r, _ptr(flux), _ptr(uh),
                  _ptr(routed), stream)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        if needs_grad:
            ctx.save_for_backward(x, state_in, traj, flux, uh, *ptensors)
        if tap is not None:
            tap.append(PathRecord(cfg, x, state_in, None, None, None, tuple(ptensors), flux, uh, routed, state_out, traj))
        return flux, routed, state_out

    @staticmethod
    @_device_guard
    def backward(ctx, g_flux, g_routed, g_state):
        lib = get_library()
        cfg: StepConfig = ctx.cfg
        saved = ctx.saved_tensors
        x, state_in, traj, flux, uh = saved[:5]
        ptensors = saved[5:]
        dev = x.device
        T, B, M = cfg.T, cfg.B, cfg.M
        stream = _stream_of(lib, x)
        # gradient buffers: the [T,B,ny] fill beside the adjoint kernels on a second stream, static rows apart
        # (as HbvPath.backward; _overlapped_grad_buffers)
        rows = [None] * len(ptensors)
        bases = [0] * len(ptensors)
        start_fill = None
        early, ctx.early_gp = ctx.early_gp, None
        if _FILL_OVERLAP and lib.is_device:
            gp, rows, bases, start_fill = _overlapped_grad_buffers(lib, cfg, ptensors, ctx.needs_input_grad[3:], early)
        else:
            gp = [_grad_like(lib, p, cfg, i) if ctx.needs_input_grad[3 + i] else None
                  for i, p in enumerate(ptensors)]

        def sta_ptr(idx, off):
            return _ptr(rows[idx], off - bases[idx]) if rows[idx] is not None else _ptr(gp[idx], off)

        gq = None
        if g_routed is not None and cfg.route is not None:
            r = _route_desc(cfg, ptensors, S=1)
            gq = _out((1, T, B), dev)
            rs = cfg.route
            gt = gp[rs.tensor_idx]
            ws_bytes = lib.route_workspace_bytes(r)
            ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=dev)
            g_routed_c = g_routed.contiguous()     # named: must outlive the launch that reads its pointer
            _call(lib, 'hbvx_route_backward', lib.route_backward, r, _ptr(flux), _ptr(uh),
                  _ptr(g_routed_c), _ptr(gq), sta_ptr(rs.tensor_idx, rs.a_off) if gt is not None else None,
                  sta_ptr(rs.tensor_idx, rs.b_off) if gt is not None else None,
                  _ptr(ws), ws_bytes, stream)
        # contiguous copies of incoming gradients are bound to locals that live until after the launch:
        # a temporary would be freed at once and the caching allocator could hand its block to gs_in / ws
        g_flux_c = g_flux.contiguous() if g_flux is not None else None
        g_state_c = g_state.contiguous() if g_state is not None else None
        io = _abi.BwdIO()
        io.traj = _ptr(traj)
        io.grad_flux = _ptr(g_flux_c)
        io.grad_flux4 = _ptr(gq)
        io.grad_state_out = _ptr(g_state_c)
        io.n_flux = 1
        gs_in = None
        if state_in is not None and ctx.needs_input_grad[2]:
            gs_in = _out((5, B, M), dev)
            io.grad_state_in = _ptr(gs_in)
        for ps in cfg.params:
            g = io.g[ps.slot]
            gs = gp[ps.tensor_idx]
            if gs is not None:
                g.sta = sta_ptr(ps.tensor_idx, ps.sta_off)
                g.sta_b_stride = ps.sta_bs
            if ps.dyn_off >= 0 and gp[ps.dyn_tensor_idx] is not None:
                g.dyn = _ptr(gp[ps.dyn_tensor_idx], ps.dyn_off)
                g.dyn_t_stride, g.dyn_b_stride = ps.dyn_ts, ps.dyn_bs
        desc = _fill_desc(cfg, x, state_in, None, None, None, ptensors)
        ws_bytes = lib.backward_workspace_bytes(desc)
        if ws_bytes:
            ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
            io.workspace, io.workspace_bytes = _ptr(ws), ws_bytes
        fill_done = start_fill() if start_fill is not None else None     # beside the adjoint kernels
        if fill_done is not None and start_fill.gated:
            io.store_gate = fill_done.cuda_event
        _call(lib, 'hbvx_adj_backward', lib.adj_backward, desc, io, stream)
        if fill_done is not None:
            torch.cuda.current_stream(dev).wait_event(fill_done)
        for big, row in zip(gp, rows):
            if row is not None:
                big[-1] += row
        return (None, None, gs_in, *gp)


class Bfi(torch.autograd.Function):
    """BFI = 100 * sum_t q2 / (sum_t qs + nearzero)  (hbv.py:562-567), qs/q2 [T,B] or [T,B,1] views.

    Forward in the library (one deterministic pass); the gradient, which a streamflow loss never
    asks for, is two broadcasts in torch."""

    @staticmethod
    @_device_guard
    def forward(ctx, qs, q2, nearzero: float):
        lib = get_library()
        ctx.cols = qs.dim() == 3
        T, B = qs.shape[:2]
        qs_c, q2_c = qs.contiguous().view(T, B), q2.contiguous().view(T, B)
        out = _out((B,), qs.device)
        _call(lib, 'hbvx_bfi', lib.bfi, T, B, _ptr(qs_c), _ptr(q2_c), float(nearzero), _ptr(out),
              _stream_of(lib, qs_c))
        ctx.save_for_backward(qs_c, q2_c)
        if _fwAD._current_level >= 0:
            ctx.save_for_forward(qs_c, q2_c)
        ctx.nearzero = float(nearzero)
        return out

    @staticmethod
    @_device_guard
    def jvp(ctx, qs_t, q2_t, _nz_t):
        """Forward mode: the quotient rule in the library (hbvx_bfi_tangent)."""
        lib = get_library()
        qs, q2 = ctx.saved_tensors
        T, B = qs.shape
        tqs = qs_t.contiguous().view(T, B) if qs_t is not None else None
        tq2 = q2_t.contiguous().view(T, B) if q2_t is not None else None
        out = _out((B,), qs.device)
        _call(lib, 'hbvx_bfi_tangent', lib.bfi_tangent, T, B, _ptr(qs), _ptr(q2), _ptr(tqs), _ptr(tq2),
              ctx.nearzero, _ptr(out), _stream_of(lib, qs))
        return out

    @staticmethod
    @_device_guard
    def backward(ctx, g):
        qs, q2 = ctx.saved_tensors
        den = qs.sum(0) + ctx.nearzero
        num = q2.sum(0)
        g_q2 = (100.0 * g / den).unsqueeze(0).expand_as(q2)
        g_qs = (-100.0 * g * num / (den * den)).unsqueeze(0).expand_as(qs)
        if ctx.cols:
            g_qs, g_q2 = g_qs.unsqueeze(-1), g_q2.unsqueeze(-1)
        return g_qs, g_q2, None


class GageRecord(NamedTuple):
    """What one call of the gage routing worked on and produced: what gage_route_tangent_batch differentiates along."""
    topo: "GageTopology"
    qs: torch.Tensor
    dp: torch.Tensor
    uh: torch.Tensor
    out: torch.Tensor


@contextlib.contextmanager
def record_gage_routes():
    """with record_gage_routes() as records: ... -- the GageRecords of the GageRoute calls this thread makes inside
    the block, in call order (what record_paths is to the recurrence)."""
    outer = getattr(_TAP, "gage_records", None)
    _TAP.gage_records = records = []
    try:
        yield records
    finally:
        _TAP.gage_records = outer


def gage_route_tangent_batch(rec: GageRecord, D: int, qs_t=None, dp_t=None) -> torch.Tensor:
    """Forward-mode derivative of one GageRoute call along D directions: hbvx_gage_route_tangent_batch on what the
    forward saved.  qs_t [D,T,U], dp_t [D,n_pair,3]; None: zero tangent, its term is skipped.  Returns [D,T,G]."""
    lib = get_library()
    topo = rec.topo
    dev = rec.qs.device
    for name, t, shape in (("qs_t", qs_t, (D, topo.T, topo.U)), ("dp_t", dp_t, (D, topo.n_pair, 3))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {shape}")
    qt = None if qs_t is None else qs_t.to(torch.float32).contiguous()
    dt = None if dp_t is None else dp_t.to(torch.float32).contiguous()
    out = _out((D, topo.T, topo.G), dev)
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        r = topo.desc(rec.dp)
        ws_bytes = lib.gage_route_tangent_workspace_bytes(r, D)
        ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=dev)
        _call(lib, 'hbvx_gage_route_tangent_batch', lib.gage_route_tangent_batch, r, D, _ptr(rec.qs), _ptr(rec.uh),
              _ptr(qt), topo.T * topo.U if qt is not None else 0, _ptr(dt), topo.n_pair * 3 if dt is not None else 0,
              _ptr(out), _ptr(ws), ws_bytes, _stream_of(lib, rec.qs))
    return out


# How often each stage of the hourly model's population evaluation has been launched in this process: a routing-only
# call must leave 'runoff' alone (tests read it; nothing else does).
HOURLY_POP_LAUNCHES = {'runoff': 0, 'gage': 0}


def hourly_population_runoff(rec: PathRecord, cand_sources: dict, P: int) -> torch.Tensor:
    """Stage 1 of the hourly model's population evaluation (include/hbvx_gage_pop.h): the unit runoff [P,T,U] of P
    candidate static-parameter sets on one recorded call of the path, the module's Qs (ensemble mean times 1/24), through
    hbvx_hourly_population_runoff on the current stream.  cand_sources as `population` takes them: {parameter slot:
    (cands, column)} into one compact contiguous float32 [P,U,C] tensor; at least one."""
    lib = get_library()
    lib.require('hbvx_hourly_population_runoff')
    cfg, x = rec.cfg, rec.x
    if cfg.model != _abi.MODEL_HOURLY:
        raise ValueError("hourly_population_runoff: the record is not a call of the hourly model")
    if not cand_sources:
        raise ValueError("hourly_population_runoff needs at least one candidate column")
    dev = x.device
    B, M = cfg.B, cfg.M
    cands = next(iter(cand_sources.values()))[0]
    _check_tensor(lib, cands, "candidates")
    if cands.dim() != 3 or tuple(cands.shape[:2]) != (P, B) or not cands.is_contiguous() or cands.device != dev or P < 1:
        raise ValueError(f"candidates must be a contiguous [{P},{B},C] tensor on {dev}, got {tuple(cands.shape)} on {cands.device}")
    Cn = int(cands.shape[2])
    for slot, (t, col) in cand_sources.items():
        if t is not cands:
            raise ValueError("all candidate columns must lie in one compact tensor")
        if not 0 <= col <= Cn - M:
            raise ValueError(f"candidate column {col} of slot {slot} does not hold {M} members in {Cn} columns")
    desc = _fill_desc(cfg, x, rec.state_in, rec.muwts, rec.ac, rec.elev, rec.ptensors)
    stream = _stream_of(lib, x)
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        runoff = _out((P, cfg.T, B), dev)
        for c0 in range(0, P, POP_MAX_CAND):
            pr = _abi.PopRunoff(abi_version=_abi.GAGE_POP_ABI_VERSION, n_cand=min(POP_MAX_CAND, P - c0))
            for slot, (_, col) in cand_sources.items():
                s = pr.p[slot]
                s.sta, s.c_stride, s.b_stride = _ptr(cands, c0 * B * Cn + col), B * Cn, Cn
            pr.runoff = _ptr(runoff, c0 * cfg.T * B)
            _call(lib, 'hbvx_hourly_population_runoff', lib.hourly_population_runoff, desc, pr, stream)
            HOURLY_POP_LAUNCHES['runoff'] += 1
    return runoff


def gage_population(grec: GageRecord, runoff: torch.Tensor, distr_cands: Optional[torch.Tensor], term: PopTerm,
                    ends: torch.Tensor, return_series: bool = False, want_gage: bool = False):
    """Stage 2 (include/hbvx_gage_pop.h): routes P candidates' unit runoff to the gages of one recorded GageRoute call and
    scores the period means there, through hbvx_gage_population_stats on the current stream.
    runoff       [P,T,U] float32 contiguous, or [T,U]: one runoff for every candidate (P then comes from distr_cands).
    distr_cands  [P,n_pair,3] float32 unit-interval route_a / route_b / route_tau, or None: the record's taps serve all.
    term         PopTerm per GAGE: target / w [K,G], shift / eps [G], transform.
    ends         [K] int32 on the device: the closing hours, ascending.
    Returns (sse, s1, s2, s3, sim, gage): [P,G] float32 chains, sim [P,K,G] the period means with return_series (else
    None), gage [P,T,G] the hourly gage series with want_gage (else None; it then lives in scratch only)."""
    lib = get_library()
    lib.require('hbvx_gage_population_stats')
    topo = grec.topo
    dev = grec.qs.device
    T, U, G = topo.T, topo.U, topo.G
    if term.transform not in _abi.POP_TRANSFORMS:
        raise ValueError(f"transform must be one of {sorted(_abi.POP_TRANSFORMS)}, got {term.transform!r}")
    if term.transform == "log" and term.eps is None:
        raise ValueError("gage_population: transform 'log' needs eps")
    _check_tensor(lib, runoff, "runoff")
    shared = runoff.dim() == 2
    if tuple(runoff.shape[-2:]) != (T, U) or runoff.dim() not in (2, 3) or not runoff.is_contiguous() or runoff.device != dev:
        raise ValueError(f"runoff must be a contiguous [P,{T},{U}] or [{T},{U}] tensor on {dev}, got {tuple(runoff.shape)}")
    if distr_cands is not None:
        _check_tensor(lib, distr_cands, "distr_candidates")
        if distr_cands.dim() != 3 or tuple(distr_cands.shape[1:]) != (topo.n_pair, 3) or not distr_cands.is_contiguous() \
                or distr_cands.device != dev:
            raise ValueError(f"distr_candidates must be a contiguous [P,{topo.n_pair},3] tensor on {dev}, got "
                             f"{tuple(distr_cands.shape)}")
    if shared and distr_cands is None:
        raise ValueError("gage_population: one runoff and no routing candidates leaves nothing to evaluate")
    P = int(distr_cands.shape[0]) if shared else int(runoff.shape[0])
    if P < 1 or (distr_cands is not None and int(distr_cands.shape[0]) != P):
        raise ValueError(f"gage_population: {P} runoff candidates, "
                         f"{None if distr_cands is None else int(distr_cands.shape[0])} routing candidates")
    if ends.dtype != torch.int32 or ends.dim() != 1 or ends.device != dev or not 1 <= ends.numel() <= T:
        raise ValueError(f"ends must be a 1-D int32 tensor of 1..{T} closing hours on {dev}")
    ends = ends.contiguous()
    K = int(ends.numel())
    for name, t, shape in (("target", term.target, (K, G)), ("w", term.w, (K, G)), ("shift", term.shift, (G,)),
                           ("eps", term.eps if term.transform == "log" else None, (G,))):
        if t is None and name in ("w", "eps"):
            continue
        if t is None:
            raise ValueError(f"gage_population needs {name}")
        _check_tensor(lib, t, name)
        if tuple(t.shape) != shape or t.device != dev:
            raise ValueError(f"{name} must be {list(shape)} on {dev}, got {tuple(t.shape)} on {t.device}")
    tc, wc, shc = (None if t is None else t.contiguous() for t in (term.target, term.w, term.shift))
    epc = term.eps.contiguous() if term.transform == "log" else None
    stream = _stream_of(lib, grec.qs)
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        r = topo.desc(grec.dp)
        sums = tuple(_out((P, G), dev) for _ in range(4))
        sim = _out((P, K, G), dev) if return_series else None
        gage = _out((P, T, G), dev) if want_gage else None
        for c0 in range(0, P, POP_MAX_CAND):
            n = min(POP_MAX_CAND, P - c0)
            gp = _abi.GagePop(abi_version=_abi.GAGE_POP_ABI_VERSION, n_cand=n,
                              runoff=_ptr(runoff, 0 if shared else c0 * T * U), runoff_c_stride=0 if shared else T * U,
                              dp=_ptr(distr_cands, c0 * topo.n_pair * 3), uh=_ptr(grec.uh),
                              transform=_abi.POP_TRANSFORMS[term.transform], n_periods=K, period_end=ends.data_ptr(),
                              target=_ptr(tc), w=_ptr(wc), shift=_ptr(shc), eps=_ptr(epc),
                              sim=_ptr(sim, c0 * K * G), series=_ptr(gage, c0 * T * G))
            gp.sse, gp.s1, gp.s2, gp.s3 = (_ptr(m, c0 * G) for m in sums)
            ws_bytes = lib.gage_population_workspace_bytes(r, gp)
            ws = _out(((max(ws_bytes, 4) + 3) // 4,), dev)      # poisoned with the outputs: the call must not need it cleared
            _call(lib, 'hbvx_gage_population_stats', lib.gage_population_stats, r, gp, _ptr(ws), ws_bytes, stream)
            HOURLY_POP_LAUNCHES['gage'] += 1
    return sums + (sim, gage)


def gage_events(series: torch.Tensor, starts: torch.Tensor, ends: torch.Tensor):
    """The peak, the hour of the peak and the volume of every candidate's hourly gage series inside E event windows per
    gage (include/hbvx_gage_events.h), through hbvx_gage_population_events on the current stream.
    series        [P,T,G] float32 contiguous: `gage_population`'s series (want_gage=True).
    starts, ends  [E,G] int32 contiguous on the series' device: inclusive hours, 0-based; start < 0 or end < start is an
                  absent slot, end is clamped to T - 1 -- any content is safe.
    Returns (peak [P,E,G] float32, peak_hour [P,E,G] int32, volume [P,E,G] float32); an absent slot holds -inf, -1, +0."""
    lib = get_library()
    lib.require('hbvx_gage_population_events')
    _check_tensor(lib, series, "series")
    dev = series.device
    if series.dim() != 3 or not series.is_contiguous() or min(series.shape) < 1:
        raise ValueError(f"series must be a contiguous [P,T,G] tensor, got {tuple(series.shape)}")
    P, T, G = (int(n) for n in series.shape)
    for name, t in (("starts", starts), ("ends", ends)):
        if not torch.is_tensor(t) or t.dtype != torch.int32:
            raise TypeError(f"{name} must be an int32 tensor, got {t.dtype if torch.is_tensor(t) else type(t).__name__}")
        if t.dim() != 2 or int(t.shape[1]) != G or not 1 <= int(t.shape[0]) <= T or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous [E,{G}] tensor of 1..{T} events on {dev}, got {tuple(t.shape)} "
                             f"on {t.device}")
    if tuple(starts.shape) != tuple(ends.shape):
        raise ValueError(f"starts is {tuple(starts.shape)}, ends {tuple(ends.shape)}")
    E = int(starts.shape[0])
    stream = _stream_of(lib, series)
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        peak, hour, volume = _out((P, E, G), dev), _out_i32((P, E, G), dev), _out((P, E, G), dev)
        if _POISON:
            hour.fill_(-2 ** 31)        # (-1, _out_i32's fill, is what an absent slot holds)
        for c0 in range(0, P, POP_MAX_CAND):
            ev = _abi.GageEvents(abi_version=_abi.GAGE_EVENTS_ABI_VERSION, n_cand=min(POP_MAX_CAND, P - c0), T=T, G=G,
                                 n_events=E, series=_ptr(series, c0 * T * G), start=starts.data_ptr(), end=ends.data_ptr(),
                                 peak=_ptr(peak, c0 * E * G), peak_hour=_ptr(hour, c0 * E * G),
                                 volume=_ptr(volume, c0 * E * G))
            _call(lib, 'hbvx_gage_population_events', lib.gage_population_events, ev, stream)
    return peak, hour, volume


class EnkfArray(NamedTuple):
    """One array of `enkf_update`: `values` [P,...] float32 contiguous whose trailing sizes are [...,B,M] (M the trailing
    size, 1 for a [P,k,B] array: pass M=1), floored at `lo` (-inf: no floor); `out` None (a new tensor) or a tensor of the
    same shape -- `values` itself is an update in place."""
    values: torch.Tensor
    M: int = 1
    lo: float = float("-inf")
    out: Optional[torch.Tensor] = None


def enkf_update(y: torch.Tensor, obs: torch.Tensor, obs_var: torch.Tensor, arrays: Sequence[EnkfArray], method: int,
                inflation: float = 1.0, eps: Optional[torch.Tensor] = None, active: Optional[torch.Tensor] = None):
    """hbvx_enkf_update (include/hbvx_enkf.h) on the current stream: the ensemble Kalman analysis of 1 .. 4 arrays of
    particle values against one observation per basin.  All float32 on one device:
    y          [P,B] the predicted observation; the basins contiguous, any particle stride >= B (a row of a series).
    obs        [B], NaN where missing; obs_var [B] its error variance (a value <= 0 is status 2, not an error).
    arrays     `EnkfArray`s; an array's elements per particle must be a multiple of B * M.
    method     _abi.ENKF_METHODS: 0 perturbed observations (eps [P,B] contiguous required), 1 square root (eps ignored).
    active     [B] bool / uint8 or None (every basin).
    Returns (outs, status [B] int32, stats [3,B] float64: ybar, the variance of y, the mean innovation)."""
    lib = get_library()
    lib.require('hbvx_enkf_update')
    _check_tensor(lib, y, "y")
    dev = y.device
    if y.dim() != 2 or int(y.shape[0]) < 2 or int(y.shape[1]) < 1 or y.stride(1) != 1 or y.stride(0) < int(y.shape[1]):
        raise ValueError(f"y must be [P,B] with P >= 2, contiguous basins and a particle stride >= B, got {tuple(y.shape)} "
                         f"with strides {tuple(y.stride())}")
    P, B = int(y.shape[0]), int(y.shape[1])
    if method not in _abi.ENKF_METHODS.values():
        raise ValueError(f"method must be one of {_abi.ENKF_METHODS}, got {method!r}")
    if not (float(inflation) > 0.0 and float(inflation) != float("inf")):
        raise ValueError(f"inflation must be finite and > 0, got {inflation!r}")
    for name, t, shape in (("obs", obs, (B,)), ("obs_var", obs_var, (B,)), ("eps", eps, (P, B))):
        if name == "eps" and method != 0:
            continue
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a float32 tensor, got {type(t).__name__}")
        _check_tensor(lib, t, name)
        if tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous {list(shape)} tensor on {dev}, got {tuple(t.shape)} on {t.device}")
    if active is not None:
        if not torch.is_tensor(active) or active.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"active must be a bool or uint8 tensor, got "
                            f"{active.dtype if torch.is_tensor(active) else type(active).__name__}")
        if tuple(active.shape) != (B,) or not active.is_contiguous() or active.device != dev:
            raise ValueError(f"active must be a contiguous [{B}] tensor on {dev}, got {tuple(active.shape)} on {active.device}")
    arrays = list(arrays)
    if not 1 <= len(arrays) <= _abi.ENKF_MAX_ARRAYS:
        raise ValueError(f"enkf_update takes 1 .. {_abi.ENKF_MAX_ARRAYS} arrays, got {len(arrays)}")
    for i, a in enumerate(arrays):
        for name, t in ((f"arrays[{i}].values", a.values), (f"arrays[{i}].out", a.out)):
            if t is None and name.endswith("out"):
                continue
            if not torch.is_tensor(t):
                raise TypeError(f"{name} must be a float32 tensor, got {type(t).__name__}")
            _check_tensor(lib, t, name)
            if t.dim() < 2 or int(t.shape[0]) != P or not t.is_contiguous() or t.device != dev or \
                    tuple(t.shape) != tuple(a.values.shape):
                raise ValueError(f"{name} must be a contiguous [{P},...] tensor on {dev}, got {tuple(t.shape)} on {t.device}")
        n = a.values.numel() // P
        if isinstance(a.M, bool) or not isinstance(a.M, int) or a.M < 1 or n < 1 or n % (B * a.M):
            raise ValueError(f"arrays[{i}]: {n} elements per particle are not a positive multiple of B * M = {B} * {a.M!r}")
        if a.lo != a.lo:
            raise ValueError(f"arrays[{i}].lo is NaN")
    stream = _stream_of(lib, y)
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        outs = [_out(tuple(a.values.shape), dev) if a.out is None else a.out for a in arrays]
        status = _out_i32((B,), dev)
        stats = torch.full((3, B), float("nan"), dtype=torch.float64, device=dev) if _POISON else \
            torch.empty((3, B), dtype=torch.float64, device=dev)
        e = _abi.Enkf(P=P, B=B, method=method, n_arrays=len(arrays), inflation=float(inflation), y=_ptr(y),
                      y_stride=y.stride(0), obs=_ptr(obs), obs_var=_ptr(obs_var),
                      active=None if active is None else active.data_ptr(), eps=None if method != 0 else _ptr(eps),
                      status=status.data_ptr(), stats=stats.data_ptr())
        for i, (a, o) in enumerate(zip(arrays, outs)):
            e.a[i] = _abi.EnkfArray(in_=_ptr(a.values), out=_ptr(o), n=a.values.numel() // P, M=a.M, lo=a.lo)
        _call(lib, 'hbvx_enkf_update', lib.enkf_update, e, stream)
    return outs, status, stats


def _check_gage_levels(series, scored, levels, name, dtype):
    """What `gage_fdc` and `gage_quantiles` check of their arguments -> (P, T, G, K)."""
    dev = series.device
    if series.dim() != 3 or not series.is_contiguous() or min(series.shape) < 1:
        raise ValueError(f"series must be a contiguous [P,T,G] tensor, got {tuple(series.shape)}")
    P, T, G = (int(n) for n in series.shape)
    if not torch.is_tensor(scored) or scored.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"scored must be a bool or uint8 tensor, got {scored.dtype if torch.is_tensor(scored) else type(scored).__name__}")
    if tuple(scored.shape) != (T, G) or not scored.is_contiguous() or scored.device != dev:
        raise ValueError(f"scored must be a contiguous [{T},{G}] tensor on {dev}, got {tuple(scored.shape)} on {scored.device}")
    if not torch.is_tensor(levels) or levels.dtype != dtype:
        raise TypeError(f"{name} must be a {dtype} tensor, got {levels.dtype if torch.is_tensor(levels) else type(levels).__name__}")
    if levels.dim() != 2 or int(levels.shape[1]) != G or not 1 <= int(levels.shape[0]) <= _abi.POP_FDC_MAX_THR \
            or not levels.is_contiguous() or levels.device != dev:
        raise ValueError(f"{name} must be a contiguous [K,{G}] tensor on {dev} with K in 1..{_abi.POP_FDC_MAX_THR}, got "
                         f"{tuple(levels.shape)} on {levels.device}")
    return P, T, G, int(levels.shape[0])


def gage_fdc(series: torch.Tensor, scored: torch.Tensor, thresholds: torch.Tensor):
    """On how many scored hours every candidate's hourly gage series lies above K thresholds per gage, and the volume
    above them (include/hbvx_gage_fdc.h), through hbvx_gage_population_fdc on the current stream.
    series      [P,T,G] float32 contiguous: `gage_population`'s series (want_gage=True).
    scored      [T,G] bool or uint8 contiguous on the series' device: the hours that enter.
    thresholds  [K,G] float32 contiguous, K in 1.._abi.POP_FDC_MAX_THR, any order.
    Returns (count [P,K,G] int32, volume [P,K,G] float32: the float32 sum of those flows in hour order)."""
    lib = get_library()
    lib.require('hbvx_gage_population_fdc')
    _check_tensor(lib, series, "series")
    P, T, G, K = _check_gage_levels(series, scored, thresholds, "thresholds", torch.float32)
    dev = series.device
    stream = _stream_of(lib, series)
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        count, volume = _out_i32((P, K, G), dev), _out((P, K, G), dev)
        for c0 in range(0, P, POP_MAX_CAND):
            gf = _abi.GageFdc(abi_version=_abi.GAGE_FDC_ABI_VERSION, n_cand=min(POP_MAX_CAND, P - c0), T=T, G=G, n_lev=K,
                              series=_ptr(series, c0 * T * G), scored=scored.data_ptr(), thr=_ptr(thresholds),
                              count=count.data_ptr() + 4 * c0 * K * G, volume=_ptr(volume, c0 * K * G))
            _call(lib, 'hbvx_gage_population_fdc', lib.gage_population_fdc, gf, stream)
    return count, volume


def gage_quantiles(series: torch.Tensor, scored: torch.Tensor, rank: torch.Tensor) -> torch.Tensor:
    """Every candidate's own flow-duration curve at K ranks per gage: the scored hours of each (candidate, gage) column
    of the hourly gage series sorted descending on the device, and the flows at the 0-based indices `rank`
    (include/hbvx_gage_fdc.h), through hbvx_gage_population_quantiles on the current stream.
    series  [P,T,G] float32 contiguous, T <= _abi.GAGE_QUANT_MAX_T (the library refuses a longer record).
    scored  [T,G] bool or uint8 contiguous on the series' device.
    rank    [K,G] int32 contiguous, K in 1.._abi.POP_FDC_MAX_THR.
    Returns quantile [P,K,G] float32: a value of the series bit for bit; NaN where the rank is outside 0..n-1 (n the gage's
    scored hours) or a scored hour of the column is NaN.  The workspace, one series' worth, lives for the call."""
    lib = get_library()
    lib.require('hbvx_gage_population_quantiles')
    _check_tensor(lib, series, "series")
    P, T, G, K = _check_gage_levels(series, scored, rank, "rank", torch.int32)
    dev = series.device
    stream = _stream_of(lib, series)
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        quantile = _out((P, K, G), dev)
        for c0 in range(0, P, POP_MAX_CAND):
            n = min(POP_MAX_CAND, P - c0)
            gf = _abi.GageFdc(abi_version=_abi.GAGE_FDC_ABI_VERSION, n_cand=n, T=T, G=G, n_lev=K,
                              series=_ptr(series, c0 * T * G), scored=scored.data_ptr(), rank=rank.data_ptr(),
                              quantile=_ptr(quantile, c0 * K * G))
            ws_bytes = lib.gage_quantiles_workspace_bytes(n, T, G)
            ws = _out(((max(ws_bytes, 4) + 3) // 4,), dev)      # poisoned with the outputs: the call must not need it cleared
            _call(lib, 'hbvx_gage_population_quantiles', lib.gage_population_quantiles, gf, _ptr(ws), ws_bytes, stream)
    return quantile


@dataclass
class GageTopology:
    """Index arrays of the (gage, unit) pairs of `outlet_topo == 1` (hbv_2_hourly.py:813-817), in
    the order `nonzero` yields them (by gage, then unit) plus the unit-side CSR of the backward."""

    T: int = 0
    U: int = 0
    G: int = 0
    n_pair: int = 0
    lag_uh: bool = True
    bounds: tuple = ((0.0, 5.0), (0.0, 12.0), (0.0, 48.0))
    pair_unit: Optional[torch.Tensor] = None
    pair_gage: Optional[torch.Tensor] = None
    gage_ptr: Optional[torch.Tensor] = None
    unit_ptr: Optional[torch.Tensor] = None
    unit_pairs: Optional[torch.Tensor] = None
    areas: Optional[torch.Tensor] = None
    denom: Optional[torch.Tensor] = None

    @staticmethod
    def from_outlet_topo(outlet_topo: torch.Tensor, areas: torch.Tensor, T: int, lag_uh: bool,
                         bounds) -> "GageTopology":
        G, U = int(outlet_topo.shape[0]), int(outlet_topo.shape[1])
        pairs = (outlet_topo == 1).nonzero(as_tuple=False)
        rows, cols = pairs[:, 0], pairs[:, 1]
        dev = outlet_topo.device

        def csr(idx, n):
            ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            ptr[1:] = torch.cumsum(torch.bincount(idx, minlength=n), 0)
            return ptr.to(torch.int32)

        areas32 = areas.to(torch.float32).contiguous()
        denom = (outlet_topo.to(torch.float32) * areas32[None, :]).sum(dim=1).clamp(min=1e-6)
        return GageTopology(
            T=T, U=U, G=G, n_pair=int(rows.numel()), lag_uh=lag_uh, bounds=tuple(map(tuple, bounds)),
            pair_unit=cols.to(torch.int32).contiguous(), pair_gage=rows.to(torch.int32).contiguous(),
            gage_ptr=csr(rows, G), unit_ptr=csr(cols, U),
            unit_pairs=torch.argsort(cols, stable=True).to(torch.int32).contiguous(),
            areas=areas32, denom=denom.contiguous())

    def desc(self, dp: torch.Tensor) -> _abi.GageDesc:
        (alo, ahi), (blo, bhi), (tlo, thi) = self.bounds
        return _abi.GageDesc(
            abi_version=_abi.ABI_VERSION, T=self.T, U=self.U, G=self.G, NPAIR=self.n_pair,
            L=min(self.T, _abi.GAGE_MAXLEN), lag_uh=int(self.lag_uh),
            pair_unit=self.pair_unit.data_ptr(), gage_ptr=self.gage_ptr.data_ptr(),
            pair_gage=self.pair_gage.data_ptr(), unit_ptr=self.unit_ptr.data_ptr(),
            unit_pairs=self.unit_pairs.data_ptr(), areas=self.areas.data_ptr(),
            denom=self.denom.data_ptr(), dp=dp.data_ptr(),
            a_lo=alo, a_hi=ahi, b_lo=blo, b_hi=bhi, tau_lo=tlo, tau_hi=thi)


class GageRoute(torch.autograd.Function):
    """Unit runoff [T,U] -> gage streamflow [T,G] through hbvx_gage_route_forward / _backward
    (hbv_2_hourly.py:800-897)."""

    @staticmethod
    @_device_guard
    def forward(ctx, topo: GageTopology, qs, dp):
        lib = get_library()
        qs_c, dp_c = qs.contiguous(), dp.contiguous()
        _check_tensor(lib, qs_c, 'Qs')
        _check_tensor(lib, dp_c, 'distributed routing parameters')
        if tuple(qs_c.shape) != (topo.T, topo.U):
            raise ValueError(f"Qs has shape {tuple(qs_c.shape)}, topology expects {(topo.T, topo.U)}")
        if tuple(dp_c.shape) != (topo.n_pair, 3):
            raise ValueError(f"distributed routing parameters have shape {tuple(dp_c.shape)}, "
                             f"outlet_topo has {topo.n_pair} (gage, unit) pairs x 3")
        L = min(topo.T, _abi.GAGE_MAXLEN)
        uh = _out((topo.n_pair, L), qs.device)
        out = _out((topo.T, topo.G), qs.device)
        r = topo.desc(dp_c)
        ws_bytes = lib.gage_route_workspace_bytes(r)
        ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=qs.device)
        _call(lib, 'hbvx_gage_route_forward', lib.gage_route_forward, r, _ptr(qs_c), _ptr(uh),
              _ptr(out), _ptr(ws), ws_bytes, _stream_of(lib, qs_c))
        ctx.topo = topo
        ctx.save_for_backward(qs_c, dp_c, uh)
        tap = getattr(_TAP, "gage_records", None)
        if tap is not None:
            tap.append(GageRecord(topo, qs_c.detach(), dp_c.detach(), uh, out))
        return out

    @staticmethod
    @_device_guard
    def backward(ctx, g):
        lib = get_library()
        qs, dp, uh = ctx.saved_tensors
        topo = ctx.topo
        g = g.contiguous()
        gqs = _out(tuple(qs.shape), qs.device)
        gdp = _out(tuple(dp.shape), dp.device)
        r = topo.desc(dp)
        ws_bytes = lib.gage_route_workspace_bytes(r)
        ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=qs.device)
        _call(lib, 'hbvx_gage_route_backward', lib.gage_route_backward, r, _ptr(qs), _ptr(uh),
              _ptr(g), _ptr(gqs), _ptr(gdp), _ptr(ws), ws_bytes, _stream_of(lib, qs))
        return None, gqs, gdp
