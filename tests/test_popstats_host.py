"""CPU tier: the per-basin arithmetic of hbvx_population_stats (hydrodl2_amd/csrc/hbv_pop.h: BasinStats -- Basin's
window and routed value, the transform, the squared-error chain and the three moment chains about the shift), compiled
for the host (tests/hosttest/popstats_host.cpp feeds one BasinStats per basin day by day, as the kernel does) and
checked on random float32 series against float64.

Bounds, with gamma(n) = n u / (1 - n u), u = 2^-24 and T the days of the call, against float64 sums over the float32 y'
the code reports, d = y' - m, e = o' - m, r = y' - o' formed in float64 from the float32 y', o', m:
  |s1  - sum w d|   <= gamma(T + 1) sum w |d|        d rounded, one fused multiply-add per day
  |s2  - sum w d^2| <= gamma(T + 3) sum w d^2        d rounded (it enters twice), w d rounded
  |s3  - sum w d e| <= gamma(T + 3) sum w |d e|      d, e and w d rounded
  |sse - sum w r^2| <= gamma(T + 2) sum w r^2        the bound of tests/test_pop_host.py
A wrong day, basin, shift or operand misses these by orders of magnitude.

The shift at scale: T = 7300 days of a flow with mean about 55 and standard deviation about 0.1.  KGE from the
float32 chains about the shift lies within 1e-5 of float64 (measured here: 2.2e-6 at worst over the nine basins); the same
chains about zero -- raw moments -- leave one basin without a variance at all and miss it by 0.07 in the best of the
others, which is why the shift is part of the design."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from hydrodl2_amd.population import population_score

from .test_pop_host import B, CASES, UH, draw, gamma
from .test_pop_host import run as run_basin

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "hosttest", f) for f in ("popstats_host.cpp", "pop_host.cpp")]
LIB = os.path.join(HERE, "hosttest", "libpopstats_host.so")
HDR = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_pop.h")

TRANSFORMS = {"none": 0, "sqrt": 1, "log": 2}


@pytest.fixture(scope="module")
def statlib():
    newest = max(os.path.getmtime(f) for f in SRCS + [HDR])
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB] + SRCS)
    dll = C.CDLL(LIB)
    dll.popstats_host.argtypes = [C.c_int] * 4 + [C.c_void_p] * 10
    dll.popstats_host.restype = C.c_int
    dll.pop_host.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8
    dll.pop_host.restype = None
    return dll


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def observed(target, w, transform):
    """(o' float32, shift float32 [B], eps float32 [B]) from the raw target as population_stats forms them: the
    transform in float64, the weighted mean of the float32 o' in float64, both rounded to float32."""
    w8 = np.ones(target.shape) if w is None else w.astype(np.float64)
    W = w8.sum(0)
    t8 = target.astype(np.float64)
    eps = np.where(W > 0, 0.01 * (w8 * t8).sum(0) / np.where(W > 0, W, 1.0), 1.0).astype(np.float32)
    if transform == "sqrt":
        t8 = np.sqrt(t8)
    elif transform == "log":
        t8 = np.log(t8 + eps.astype(np.float64))
    ot = np.ascontiguousarray(t8.astype(np.float32))
    shift = np.where(W > 0, (w8 * ot.astype(np.float64)).sum(0) / np.where(W > 0, W, 1.0), 0.0).astype(np.float32)
    return ot, shift, eps


def run(dll, T, t_first, transform, q, ot, w, shift, eps, a, bb, n_basins=B):
    y = np.full((T, n_basins), np.nan, dtype=np.float32)
    yt = np.full((T, n_basins), np.nan, dtype=np.float32)
    out = np.full((4, n_basins), np.nan, dtype=np.float32)
    for arr in (q, ot, w, shift, eps, a, bb):
        assert arr is None or (arr.flags["C_CONTIGUOUS"] and arr.dtype == np.float32)
    ptr = lambda arr: None if arr is None else arr.ctypes.data      # noqa: E731
    rc = dll.popstats_host(T, n_basins, t_first, TRANSFORMS[transform], ptr(a), ptr(bb), ptr(q), ptr(ot), ptr(w), ptr(shift),
                           ptr(eps), y.ctypes.data, yt.ctypes.data, out.ctypes.data)
    assert rc == 0
    return y, yt, out


def check_chains(out, yt, ot, w, shift, T, t_first, what):
    y8, o8, m8 = yt[t_first:].astype(np.float64), ot.astype(np.float64), shift.astype(np.float64)
    w8 = np.ones_like(y8) if w is None else w.astype(np.float64)
    d, e, r = y8 - m8, o8 - m8, y8 - o8
    rows = (("sse", out[0], w8 * r * r, w8 * r * r, T + 2), ("s1", out[1], w8 * d, w8 * np.abs(d), T + 1),
            ("s2", out[2], w8 * d * d, w8 * d * d, T + 3), ("s3", out[3], w8 * d * e, w8 * np.abs(d * e), T + 3))
    assert np.isfinite(out).all(), f"{what}: a chain is not finite"
    for name, got, terms, mags, n in rows:
        err = np.abs(got.astype(np.float64) - terms.sum(0))
        bound = gamma(n) * mags.sum(0)
        need = (err / np.where(bound > 0, bound, 1.0)).max()
        print(f"{what}: {name} worst error / bound {need:.3f}")
        assert (err <= bound).all(), f"{what}: {name} misses its float64 sum by {need:.2f} x the bound"


@pytest.mark.parametrize("routed", [True, False], ids=["routed", "unrouted"])
@pytest.mark.parametrize("transform", list(TRANSFORMS))
@pytest.mark.parametrize("T,t_first", CASES, ids=[f"T{t}-first{f}" for t, f in CASES])
def test_chains_against_float64_and_the_bit_rules(statlib, T, t_first, transform, routed):
    q, target, w, a, bb = draw(T, t_first, seed=100 * T + t_first + (0 if routed else 50))
    if not routed:
        a = bb = None
    ot, shift, eps = observed(target, w, transform)
    y, yt, out = run(statlib, T, t_first, transform, q, ot, w, shift, eps, a, bb)
    assert np.isfinite(y).all() and np.isfinite(yt).all()
    check_chains(out, yt, ot, w, shift, T, t_first, f"{transform}, weighted")

    # the routed value is Basin's in every transform, bit for bit; the transform is the float32 one of the value
    _, y_basin, cost_basin = run_basin(statlib, T, t_first, q, ot, w, a, bb)
    assert np.array_equal(bits(y), bits(y_basin))
    if transform == "none":
        assert np.array_equal(bits(yt), bits(y))
        assert np.array_equal(bits(out[0]), bits(cost_basin)), "sse under 'none' is not Basin's cost"
    elif transform == "sqrt":
        assert np.array_equal(bits(yt), bits(np.sqrt(y)))           # correctly rounded on every platform
    else:
        want = np.log(y.astype(np.float64) + eps.astype(np.float64))
        assert (np.abs(yt - want) <= 4 * 2.0 ** -24 * (1 + np.abs(want))).all()

    # w = NULL is w = 1, bit for bit (the shift is the same number in both calls)
    ones = np.ones_like(w)
    ot1, shift1, eps1 = observed(target, None, transform)
    _, yt1, out1 = run(statlib, T, t_first, transform, q, ot1, None, shift1, eps1, a, bb)
    _, _, out2 = run(statlib, T, t_first, transform, q, ot1, ones, shift1, eps1, a, bb)
    assert np.array_equal(bits(out1), bits(out2))
    check_chains(out1, yt1, ot1, None, shift1, T, t_first, f"{transform}, unweighted")

    if t_first:
        # days before t_first move the window and none of the chains: all days with zero weight in front add exact
        # zeros, so the four numbers are the same bits (and the routed series does not depend on t_first)
        full_t = np.concatenate([np.zeros((t_first, B), np.float32), ot])
        full_w = np.concatenate([np.zeros((t_first, B), np.float32), w])
        y0, _, out0 = run(statlib, T, 0, transform, q, full_t, full_w, shift, eps, a, bb)
        assert np.array_equal(bits(y0), bits(y)) and np.array_equal(bits(out0), bits(out))
        if routed:
            # ... and the history from before t_first is in the counted days' values
            yc, _, _ = run(statlib, T - t_first, 0, transform, np.ascontiguousarray(q[t_first:]), ot, w, shift, eps, a, bb)
            if T - t_first >= 1 and min(T, UH) == min(T - t_first, UH):       # (the taps depend on L = min(T, 15))
                assert np.abs(yc[0] - y[t_first]).max() > 0


def kge_float64(y, o):
    """Gupta 2009 from the series, float64, unit weights: [B]."""
    y8, o8 = y.astype(np.float64), o.astype(np.float64)
    r = ((y8 - y8.mean(0)) * (o8 - o8.mean(0))).mean(0) / (y8.std(0) * o8.std(0))
    return 1 - np.sqrt((r - 1) ** 2 + (y8.std(0) / o8.std(0) - 1) ** 2 + (y8.mean(0) / o8.mean(0) - 1) ** 2)


def kge_from_chains(out, ot, shift, T):
    e = ot.astype(np.float64) - shift.astype(np.float64)
    stats = {"sse": torch.from_numpy(out[0:1].copy()), "s1": torch.from_numpy(out[1:2].copy()),
             "s2": torch.from_numpy(out[2:3].copy()), "s3": torch.from_numpy(out[3:4].copy()),
             "shift": torch.from_numpy(shift.copy()), "n_obs": torch.full((ot.shape[1],), T, dtype=torch.int64),
             "obs": {"W": torch.full((ot.shape[1],), float(T), dtype=torch.float64), "e1": torch.from_numpy(e.sum(0)),
                     "e2": torch.from_numpy((e * e).sum(0))}}
    return population_score(stats, "kge")[0].numpy()


def test_the_shift_at_scale(statlib):
    """Twenty years of a high-baseflow series: mean about 55, standard deviation about 0.1, KGE around 0.9."""
    T = 7300
    rng = np.random.default_rng(7300)
    base = rng.uniform(50.0, 60.0, size=(1, B))
    signal = 0.1 * rng.standard_normal((T, B))
    o = np.ascontiguousarray((base + signal).astype(np.float32))
    q = np.ascontiguousarray((base * (1 + rng.uniform(-2e-4, 2e-4, size=(1, B))) + 1.05 * signal
                              + 0.03 * rng.standard_normal((T, B))).astype(np.float32))
    ot, shift, eps = observed(o, None, "none")
    y, yt, out = run(statlib, T, 0, "none", q, ot, None, shift, eps, None, None)
    want = kge_float64(y, o)
    assert (want > 0.5).all() and (want < 0.99).all(), "the series is not in the range where calibration works"
    miss = np.abs(kge_from_chains(out, ot, shift, T) - want).max()
    # the same chains about zero: the raw moments sum y, sum y^2, sum y o
    zero = np.zeros_like(shift)
    _, _, raw = run(statlib, T, 0, "none", q, ot, None, zero, eps, None, None)
    got_raw = kge_from_chains(raw, ot, zero, T)
    lost = np.isnan(got_raw)                     # a variance that came out as noise: population_score gives no score
    miss_raw = np.abs(got_raw - want)[~lost].min() if not lost.all() else np.inf
    print(f"KGE from float32 chains against float64: worst {miss:.3e} about the shift; about zero {int(lost.sum())} of "
          f"{B} basins have no score and the BEST of the others misses by {miss_raw:.3e}")
    assert miss <= 1e-5
    assert miss_raw > 1e-3, "raw moments were expected to fail here: the case no longer shows what the shift is for"
