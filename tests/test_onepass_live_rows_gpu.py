"""GPU tier: the one-pass static adjoint told how many rows of the runoff-gradient buffer exist (hbvx_backward_live,
include/hbvx_live_rows.h; hbv_chunked.h: k_bwd_chunk_onepass_live) against the four-row call it replaces, bit for bit.

With a loss on routed streamflow alone the routing adjoint fills row 0 of grad_flux4 [4,T,B].  The old entry has it
write zeros to rows 1..3 and the adjoint reads them back; the new one writes and reads row 0 only and takes the
others as +0.0f.  Every sum keeps its terms, so neither the parameter gradient -- the static parameters' and the two
routing parameters' -- nor the state gradient may move by one bit.  The state gradient is hbvx_bwd_io.grad_state_in
[5,B,M], the adjoint of the initial storages, which k_bwd_chunk_scan forms from the Phi / phi rows the one-pass kernel
writes: with one group those rows feed nothing else.  HbvPath.backward does not ask for it, so every run here wraps
the two library calls, hands them a NaN-filled grad_state_in and a fixed non-zero grad_state_out (the seed of the
final storages, so that the maps' Phi rows count and not only their offsets) and reads the buffer back.
The test tier poisons output buffers with NaN (HBVX_DEBUG_POISON), so a read of a row that was not written shows.

Shapes: T = 130 (three 64-day chunks of 64 + 64 + 2 days: one group of three), 200 (four chunks, the last of 8 days:
one full group) and 330 (six chunks, the last of 10 days: a group of four and a group of two, so the scan hops across
two maps of the live-row kernel and the fold sums two groups); B = 5 (the second wave of lanes holds one basin of
four), M = 16, with and without parBETAET.

  old     the library "lacks" the export (lib.missing, as the other optional exports' fallbacks are tested)
  live 1  the export, routed streamflow alone: hbvx_onepass_live_rows() == 1
  live 2  the export, routed streamflow and routed Q0
  live 4  four live routed rows through the export with n_live4 = 4 against hbvx_backward
  refused HBVX_CHUNK_ONEPASS=0 pins the two-pass form: the export refuses before any launch, the caller zeroes the
          dead rows and makes the four-row call -- the two-pass form's own bits -- and does not ask again"""
import ctypes as C

import numpy as np
import pytest
import torch

from hydrodl2_amd import _abi
from hydrodl2_amd.ops import ParamSource, RouteSource, StepConfig, hbv_path

from .abi_util import BOUNDS, MODEL_ID, make_problem
from .test_chunk_onepass_gpu import _form

pytestmark = pytest.mark.gpu

SHAPES = [(130, 5, 16), (200, 5, 16), (330, 5, 16)]
EXPORT = "hbvx_backward_live"


@pytest.fixture
def lib(hip_backend):
    """The handle ops.py uses NOW: other modules' helpers reload it (tests/seam.py), so the session's hip_backend may be
    an older object of the same library -- patching its `missing` would not reach ops.py."""
    from hydrodl2_amd import _lib
    return _lib.get_library()


def _live(lib) -> int:
    f = lib.dll.hbvx_onepass_live_rows
    f.restype = C.c_int
    return f()


def _run(prob, n_routed, lib, steps=1):
    """Forward + backward on cuda:0 with the loss on the first n_routed routed series only, `steps` times on one
    configuration; (parameter gradient, state gradient) of the last step.  lib.backward and lib.backward_live --
    whatever they are at this moment, a test's own wrappers included -- are wrapped for the run: every call gets
    io.grad_state_out = a fixed seed and io.grad_state_in = a NaN-filled [5,B,M] buffer."""
    dev = torch.device("cuda:0")      # (no seam call here: it would reload the handle the test has patched)
    T, B, M, n, ny = prob["T"], prob["B"], prob["M"], prob["n"], prob["ny"]
    seed = torch.from_numpy(np.random.default_rng(7).uniform(-1.0, 1.0, (5, B, M)).astype(np.float32)).to(dev)
    gs_in = torch.full((5, B, M), float("nan"), dtype=torch.float32, device=dev)
    kept = {k: lib.__dict__[k] for k in ("backward", "backward_live") if k in lib.__dict__}
    inner_b, inner_l = lib.backward, lib.backward_live

    def with_state(io):
        io.grad_state_out, io.grad_state_in = seed.data_ptr(), gs_in.data_ptr()

    def backward(desc, io, stream):
        with_state(io)
        return inner_b(desc, io, stream)

    def backward_live(desc, io, n_live4, stream):
        with_state(io)
        return inner_l(desc, io, n_live4, stream)

    lib.backward, lib.backward_live = backward, backward_live
    try:
        return _steps(prob, n_routed, steps, dev, gs_in)
    finally:
        for k in ("backward", "backward_live"):
            if k in kept:
                lib.__dict__[k] = kept[k]
            else:
                del lib.__dict__[k]


def _steps(prob, n_routed, steps, dev, gs_in):
    T, B, M, n, ny = prob["T"], prob["B"], prob["M"], prob["n"], prob["ny"]
    x = torch.from_numpy(prob["x"]).to(dev)
    p = torch.from_numpy(prob["params"]).to(dev).requires_grad_(True)
    srcs = []
    for i, name in enumerate(prob["names"]):
        lo, hi = BOUNDS[name]
        srcs.append(ParamSource(slot=_abi.PARAM_SLOTS.index(name), lo=float(lo), hi=float(hi), tensor_idx=0,
                                sta_off=(T - 1) * B * ny + i * M, sta_bs=ny))
    cfg = StepConfig(model=MODEL_ID[prob["model"]], n_param=n, n_flux=11, T=T, t0=0, B=B, ckpt_days=0, M=M,
                     raw_sigmoid=True, channels=(0, 1, 2), nearzero=1e-5, params=srcs)
    off = (T - 1) * B * ny + n * M
    cfg.route = RouteSource(0, off, off + 1, ny, [0, 2.9], [0, 6.5])
    gr = torch.from_numpy(prob["grouted"]).to(dev)
    for _ in range(steps):
        p.grad = None
        po = hbv_path(cfg, x, None, None, None, None, p)
        loss = sum((po.routed[k][..., 0] * gr[k]).sum() for k in range(n_routed))
        loss.backward()
        torch.cuda.synchronize()
    return p.grad.cpu().numpy(), gs_in.cpu().numpy()


def _same_bits(got, want):
    """(parameter gradient, state gradient) pairs: both finite, the state gradient not all zero, both bit-equal"""
    for name, a, b in zip(("parameter gradient", "state gradient"), got, want):
        assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all(), name
        diff = a.view(np.uint32) != b.view(np.uint32)
        assert not diff.any(), f"{name}: {int(diff.sum())} of {diff.size} elements differ in bits"
    assert np.abs(want[1]).max() > 0.0


def _old(prob, n_routed, lib, monkeypatch):
    monkeypatch.setattr(lib, "missing", list(lib.missing) + [EXPORT])
    g = _run(prob, n_routed, lib)
    assert lib.last_dispatch(1) == "chunked" and _form(lib) == 1 and _live(lib) == 4
    monkeypatch.undo()
    return g


@pytest.mark.parametrize("betaet", [False, True])
@pytest.mark.parametrize("T,B,M", SHAPES)
def test_one_live_row_equals_four_rows_with_zeros(T, B, M, betaet, lib, monkeypatch):
    assert EXPORT not in lib.missing
    prob = make_problem(model="Hbv", T=T, B=B, M=M, betaet=betaet, seed=71)
    old = _old(prob, 1, lib, monkeypatch)
    new = _run(prob, 1, lib)
    assert lib.last_dispatch(1) == "chunked" and _form(lib) == 1 and _live(lib) == 1
    assert np.abs(new[0][-1]).max() > 0.0
    _same_bits(new, old)


@pytest.mark.parametrize("T", [130, 330])
def test_two_live_rows(T, lib, monkeypatch):
    prob = make_problem(model="Hbv", T=T, B=5, M=16, betaet=True, seed=72)
    old = _old(prob, 2, lib, monkeypatch)
    new = _run(prob, 2, lib)
    assert _form(lib) == 1 and _live(lib) == 2
    _same_bits(new, old)


@pytest.mark.parametrize("T,betaet", [(200, False), (200, True), (330, True)])
def test_four_rows_through_the_export_equal_hbvx_backward(T, betaet, lib, monkeypatch):
    prob = make_problem(model="Hbv", T=T, B=5, M=16, betaet=betaet, seed=73)
    plain = _run(prob, 4, lib)
    assert _form(lib) == 1 and _live(lib) == 4
    calls = []

    def through_export(desc, io, stream):
        calls.append(1)
        assert lib.backward_live(desc, io, 4, stream)

    monkeypatch.setattr(lib, "backward", through_export)
    got = _run(prob, 4, lib)
    assert calls and _form(lib) == 1 and _live(lib) == 4
    _same_bits(got, plain)


def test_a_refused_call_clears_the_rows_and_is_not_repeated(lib, monkeypatch):
    prob = make_problem(model="Hbv", T=130, B=5, M=16, seed=74)
    monkeypatch.setenv("HBVX_CHUNK_ONEPASS", "0")
    monkeypatch.setattr(lib, "missing", list(lib.missing) + [EXPORT])
    old = _run(prob, 1, lib)
    assert _form(lib) == 2
    monkeypatch.setattr(lib, "missing", [m for m in lib.missing if m != EXPORT])
    asked = []
    real = lib.backward_live

    def counting(desc, io, n, stream):
        took = real(desc, io, n, stream)
        asked.append((n, took))
        return took

    monkeypatch.setattr(lib, "backward_live", counting)
    got = _run(prob, 1, lib, steps=2)      # the second step of the configuration does not ask again
    assert asked == [(1, False)] and lib.last_dispatch(1) == "chunked" and _form(lib) == 2
    _same_bits(got, old)
