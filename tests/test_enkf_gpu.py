"""GPU tier: hbvx_enkf_update through ops.enkf_update against the float64 restatement at the CPU tier's bound
(tests/enkf_util.py derives it) and, bit for bit, against the host build of the same header on the same inputs.

Shapes: P in {2, 3, 33, 64, 200}, B in {1, 5, 67}, M in {1, 3, 16}; the history at B = 67 is 938 elements per particle --
past a wave, several workgroups, no multiple of either.  The restatement and the host build are computed once per input
set and shared.  Measured on an MI355X: every case agrees with the host build in every bit, so |device - restatement| / bound
is the host build's figure: 0.946 to 0.999 per case, the one float32 rounding (43 cases in 2.8 s)."""
import functools
import os

import numpy as np
import pytest
import torch

from hydrodl2_amd import _abi, ops
from hydrodl2_amd._lib import get_library

from .enkf_util import host_update, inputs, restate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64          # sentinel floats on either side of every output buffer
SENT = -12345.678


@pytest.fixture(autouse=True)
def _product_library(hip_backend):
    """Every test here runs on the HIP library on cuda:0."""


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(P, B, M, seed=0, kind="wet"):
    """An input set with its host-build results and restatements for both methods and both inflations (read-only)."""
    d = inputs(P, B, M, 1000 * P + 10 * B + M + seed, kind)
    ref = {}
    for method in (0, 1):
        for rho in (1.0, 1.05):
            host = host_update(d["y"], d["obs"], d["obs_var"], d["arrays"], method, rho, d["eps"])
            rs = [restate(d["y"], d["obs"], d["obs_var"], x, M_, lo, method, rho, d["eps"]) for x, M_, lo in d["arrays"]]
            ref[method, rho] = (host, rs)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d, ref


def guarded(shape, fill=SENT):
    """A contiguous tensor of `shape` inside a buffer with GUARD sentinels on either side -> (view, whole buffer)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device=DEV)
    return whole[GUARD:GUARD + n].view(shape), whole


def intact(whole):
    w = whole.cpu().numpy()
    return (w[:GUARD] == np.float32(SENT)).all() and (w[-GUARD:] == np.float32(SENT)).all()


def device_update(d, which, method, rho, active=None, inplace=False, y=None, piece=None):
    """ops.enkf_update on the arrays `which` of the input set, outputs in guarded buffers: (outs, status, stats) numpy."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    arrays, wholes = [], []
    for i in which:
        x, M, lo = d["arrays"][i]
        out, whole = guarded(x.shape)
        if inplace:
            out.copy_(t(x))
        arrays.append(ops.EnkfArray(out if inplace else t(x), M, lo, out))
        wholes.append(whole)
    if piece is not None:
        os.environ["HBVX_ENKF_PIECE"] = str(piece)
    try:
        outs, status, stats = ops.enkf_update(t(d["y"]) if y is None else y, t(d["obs"]), t(d["obs_var"]), arrays, method, rho,
                                              t(d["eps"]) if method == 0 else None,
                                              None if active is None else t(np.asarray(active, dtype=bool)))
        torch.cuda.synchronize()
    finally:
        os.environ.pop("HBVX_ENKF_PIECE", None)
    assert all(intact(w) for w in wholes), "a sentinel beside an output buffer was overwritten"
    return [o.cpu().numpy() for o in outs], status.cpu().numpy(), stats.cpu().numpy()


SHAPES = [(2, 1, 1), (3, 5, 3), (33, 67, 16), (64, 67, 3), (200, 5, 1), (64, 1, 16), (200, 67, 1), (2, 67, 16), (33, 5, 3)]


@pytest.mark.parametrize("rho", [1.0, 1.05])
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("P,B,M", SHAPES)
def test_the_device_is_the_host_build_and_the_restatement(P, B, M, method, rho):
    d, ref = case(P, B, M)
    (h_outs, h_status, h_stats), rs = ref[method, rho]
    outs, status, stats = device_update(d, (0, 1, 2), method, rho)
    worst = 0.0
    for out, h, (xa, _, _, bound, _) in zip(outs, h_outs, rs):
        assert np.array_equal(bits(out), bits(h)), "the device's bits are not the host build's"
        err = np.abs(out.astype(np.float64) - xa)
        assert (err <= bound).all()
        worst = max(worst, float((err / bound).max()))
    assert np.array_equal(status, h_status) and not status.any()
    assert np.array_equal(stats.view(np.uint64), h_stats.view(np.uint64))
    print(f"P {P} B {B} M {M} method {method} rho {rho}: max |device - restatement| / bound = {worst:.3f}")
    # two calls, and the arrays one at a time, and in place
    again, _, _ = device_update(d, (0, 1, 2), method, rho)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(outs, again))
    for i in (0, 1, 2):
        alone, st, _ = device_update(d, (i,), method, rho)
        assert np.array_equal(bits(alone[0]), bits(outs[i])) and not st.any()
    inpl, _, _ = device_update(d, (0, 1, 2), method, rho, inplace=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(outs, inpl))


@pytest.mark.parametrize("method", [0, 1])
def test_the_floor_on_the_device(method):
    d, ref = case(33, 5, 3, kind="dry")
    (h_outs, _, _), rs = ref[method, 1.0]
    floored = rs[0][4]
    assert 0.01 < floored.mean() < 0.50
    outs, _, _ = device_update(d, (0, 1, 2), method, 1.0)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(outs, h_outs))
    assert (outs[0] >= np.float32(1e-5)).all() and (np.abs(outs[0].astype(np.float64) - rs[0][0]) <= rs[0][3]).all()


@pytest.mark.parametrize("method", [0, 1])
def test_a_basin_depends_on_its_own_columns_alone(method):
    """Basin 41 of B = 67 has the bits of the same columns as a problem of B = 1; a split launch changes no bit; a strided
    y (a row of a [P,rows,B] series) is read as the contiguous copy is."""
    P, B, M, b = 33, 67, 3, 41
    d, ref = case(P, B, M)
    outs, _, stats = device_update(d, (0, 1, 2), method, 1.05)
    one = {"y": d["y"][:, b:b + 1].copy(), "obs": d["obs"][b:b + 1].copy(), "obs_var": d["obs_var"][b:b + 1].copy(),
           "eps": d["eps"][:, b:b + 1].copy(),
           "arrays": [(np.ascontiguousarray(x.reshape(P, -1, B, M_)[:, :, b:b + 1]), M_, lo) for x, M_, lo in d["arrays"]]}
    outs1, _, stats1 = device_update(one, (0, 1, 2), method, 1.05)
    for o, o1, (x, M_, _) in zip(outs, outs1, d["arrays"]):
        assert np.array_equal(bits(o.reshape(P, -1, B, M_)[:, :, b]), bits(o1.reshape(P, -1, 1, M_)[:, :, 0]))
    assert np.array_equal(stats[:, b].view(np.uint64), stats1[:, 0].view(np.uint64))
    split, _, _ = device_update(d, (0, 1, 2), method, 1.05, piece=256)         # 13 launches for the storages
    assert all(np.array_equal(bits(a), bits(c)) for a, c in zip(outs, split))
    series = torch.full((P, 3, B), 7.0, dtype=torch.float32, device=DEV)
    series[:, 1] = torch.from_numpy(d["y"]).to(DEV)
    strided, _, _ = device_update(d, (0, 1, 2), method, 1.05, y=series[:, 1])
    assert all(np.array_equal(bits(a), bits(c)) for a, c in zip(outs, strided))


@pytest.mark.parametrize("method", [0, 1])
def test_skipped_basins_are_bit_copies_and_their_neighbours_are_untouched(method):
    P, B, M = 33, 67, 3
    d0, _ = case(P, B, M)
    clean, _, _ = device_update(d0, (0, 1, 2), method, 1.0)
    d = {k: (v.copy() if isinstance(v, np.ndarray) else [(x.copy(), M_, lo) for x, M_, lo in v]) for k, v in d0.items()}
    active = np.ones(B, dtype=bool)
    active[7] = False                                   # inactive
    d["obs"][40] = np.nan                               # missing
    d["y"][5, 66] = np.inf                              # a non-finite mean
    d["obs_var"][0] = -1.0                              # R <= 0
    d["arrays"][0][0][2, 3, 20, 1] = np.inf             # one element of basin 20
    skipped = {7: 1, 40: 1, 66: 2, 0: 2}
    outs, status, stats = device_update(d, (0, 1, 2), method, 1.0, active=active)
    h_outs, h_status, h_stats = host_update(d["y"], d["obs"], d["obs_var"], d["arrays"], method, 1.0, d["eps"], active)
    want = np.zeros(B, dtype=np.int32)
    for b, s in skipped.items():
        want[b] = s
    want[20] = 3
    assert np.array_equal(status, want) and np.array_equal(h_status, want)
    assert np.array_equal(np.isnan(stats), np.isnan(h_stats)) and np.array_equal(np.nan_to_num(stats, posinf=1e300),
                                                                                 np.nan_to_num(h_stats, posinf=1e300))
    keep = np.ones(B, dtype=bool)
    keep[list(skipped) + [20]] = False
    for o, h, c, (x, M_, _) in zip(outs, h_outs, clean, d["arrays"]):
        assert np.array_equal(bits(o), bits(h))
        o4, x4, c4 = (bits(a).reshape(P, -1, B, M_) for a in (o, x, c))
        for b in skipped:
            assert np.array_equal(o4[:, :, b], x4[:, :, b])
        assert np.array_equal(o4[:, :, keep], c4[:, :, keep])           # the neighbours are what they were without all this
    assert np.array_equal(bits(outs[0][:, 3, 20, 1]), bits(d["arrays"][0][0][:, 3, 20, 1]))
    assert np.isfinite(outs[0][:, 3, 20, 0]).all()


def test_the_launcher_refuses_with_nothing_written():
    lib = get_library()
    P, B = 4, 3
    y = torch.ones(P, B, device=DEV)
    obs, var = torch.ones(B, device=DEV), torch.ones(B, device=DEV)
    x, whole = guarded((P, 5, B, 2))
    out, whole_out = guarded((P, 5, B, 2))
    status = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    stats = torch.full((3, B), -9.0, dtype=torch.float64, device=DEV)

    def args(**kw):
        e = _abi.Enkf(P=P, B=B, method=1, n_arrays=1, inflation=1.0, y=y.data_ptr(), y_stride=B, obs=obs.data_ptr(),
                      obs_var=var.data_ptr(), status=status.data_ptr(), stats=stats.data_ptr())
        e.a[0] = _abi.EnkfArray(in_=x.data_ptr(), out=out.data_ptr(), n=30, M=2, lo=0.0)
        for k, v in kw.items():
            setattr(e.a[0] if k in ("in_", "out", "n", "M", "lo") else e, k, v)
        return e

    stream = torch.cuda.current_stream().cuda_stream
    for code, kw in ((-2, dict(P=1)), (-2, dict(n_arrays=5)), (-3, dict(method=2)), (-2, dict(inflation=0.0)),
                     (-1, dict(obs=None)), (-1, dict(method=0)), (-2, dict(n=29)), (-2, dict(out=x.data_ptr() + 4)),
                     (-2, dict(out=y.data_ptr())), (-1, dict(out=None))):
        with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*hbvx_enkf_update: "):
            lib.enkf_update(args(**kw), stream)
    torch.cuda.synchronize()
    assert (out == SENT).all() and intact(whole) and intact(whole_out)
    assert (status == -9).all() and (stats == -9.0).all()
    lib.enkf_update(args(), stream)                     # the same arguments, valid: it runs
    torch.cuda.synchronize()
    assert (status == 0).all() and torch.isfinite(out).all() and intact(whole_out)
