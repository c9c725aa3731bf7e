"""CPU tier: the per-basin arithmetic of hbvx_population_cost (hydrodl2_amd/csrc/hbv_pop.h: unit hydrograph, 15-day
window, causal convolution, residual chain), compiled for the host (tests/hosttest/pop_host.cpp feeds one Basin per
basin day by day, as the kernel does) and checked on random float32 series against float64.

Bounds, with gamma(n) = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, ch. 3):
  routed value  y_t = sum_k uh_k q_{t-k} over 15 taps, every product rounded, added in ascending k from 0: a term
                carries its product's rounding and at most 14 additions', so |y - exact| <= gamma(16) sum_k |uh_k q_{t-k}|,
                the exact sum in float64 over the float32 taps the code reports.
  cost          sum_t w r^2 with r = y - target rounded, w r rounded, one fused multiply-add per day: compared with the
                float64 sum over the float32 y the code produced, within gamma(T + 2) sum w r^2 (T the days of the call).
An indexing mistake -- a wrong day, basin or tap, history that is not zero, a day before t_first counted -- misses
these by orders of magnitude."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hosttest", "pop_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libpop_host.so")
HDR = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_pop.h")

U = 2.0 ** -24
UH = 15
B = 9
CASES = [(T, t0) for T in (1, 7, 15, 16, 40) for t0 in (0, 5) if t0 < T]


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


@pytest.fixture(scope="module")
def poplib():
    newest = max(os.path.getmtime(f) for f in (SRC, HDR))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    dll = C.CDLL(LIB)
    dll.pop_host.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8
    dll.pop_host.restype = None
    return dll


def draw(T, t_first, seed):
    """q [T,B] >= 0 with dry spells and basins of different scale, target near it, w >= 0 with exact zeros, physical
    routing parameters over their ranges (route_a 0..2.9, route_b 0..6.5); float32."""
    rng = np.random.default_rng(seed)
    q = (rng.gamma(0.7, 3.0, size=(T, B)) * 10.0 ** rng.uniform(-1, 1, size=(1, B))).astype(np.float32)
    q[rng.random((T, B)) < 0.15] = 0.0
    T_out = T - t_first
    target = (q[t_first:] * rng.uniform(0.5, 1.5, size=(T_out, B)) + rng.uniform(0, 1, size=(T_out, B))).astype(np.float32)
    w = rng.random((T_out, B)).astype(np.float32)
    w[rng.random((T_out, B)) < 0.2] = 0.0
    a = rng.uniform(0.0, 2.9, size=B).astype(np.float32)
    bb = rng.uniform(0.0, 6.5, size=B).astype(np.float32)
    return q, target, w, a, bb


def run(dll, T, t_first, q, target, w, a, bb):
    uh = np.full((B, UH), np.nan, dtype=np.float32)
    y = np.full((T, B), np.nan, dtype=np.float32)
    cost = np.full((B,), np.nan, dtype=np.float32)
    for arr in (q, target, w, a, bb):
        assert arr is None or (arr.flags["C_CONTIGUOUS"] and arr.dtype == np.float32)
    dll.pop_host(T, B, t_first, None if a is None else a.ctypes.data, None if bb is None else bb.ctypes.data, q.ctypes.data,
                 target.ctypes.data, None if w is None else w.ctypes.data, uh.ctypes.data, y.ctypes.data, cost.ctypes.data)
    return uh, y, cost


def check_cost(cost, y, target, w, T, t_first, what):
    r8 = y[t_first:].astype(np.float64) - target.astype(np.float64)
    w8 = np.ones_like(r8) if w is None else w.astype(np.float64)
    want = (w8 * r8 * r8).sum(0)
    err = np.abs(cost.astype(np.float64) - want)
    bound = gamma(T + 2) * want
    need = (err / np.where(bound > 0, bound, 1.0)).max()
    print(f"{what}: cost worst error / bound {need:.3f}")
    assert np.isfinite(cost).all() and (err <= bound).all(), f"{what}: cost error exceeds the bound by {need:.2f}x"


@pytest.mark.parametrize("T,t_first", CASES, ids=[f"T{t}-first{f}" for t, f in CASES])
def test_routed_value_and_cost_against_float64(poplib, T, t_first):
    q, target, w, a, bb = draw(T, t_first, seed=100 * T + t_first)
    uh, y, cost = run(poplib, T, t_first, q, target, w, a, bb)
    L = min(T, UH)
    # the taps: zero from L on, normalised, and the gamma density of uh_routing.py at the mid-points
    assert not uh[:, L:].any() and np.isfinite(uh).all() and (uh[:, :L] > 0).all()
    aa, theta = a.astype(np.float64) + 0.1, bb.astype(np.float64) + 0.5
    t = np.arange(L) + 0.5
    dens = np.array([t ** (aa[b] - 1) * np.exp(-t / theta[b]) / (math.gamma(aa[b]) * theta[b] ** aa[b]) for b in range(B)])
    np.testing.assert_allclose(uh[:, :L], dens / dens.sum(1, keepdims=True), rtol=2e-5, atol=0)
    # the routed value: causal, zero history before day 0, every day of the call (days before t_first included)
    uh8, q8 = uh.astype(np.float64), q.astype(np.float64)
    want, mag = np.zeros((T, B)), np.zeros((T, B))
    for k in range(L):                                           # (the taps from L on are zero: asserted above)
        want[k:] += uh8[:, k] * q8[:T - k]
        mag[k:] += np.abs(uh8[:, k] * q8[:T - k])
    err = np.abs(y.astype(np.float64) - want)
    bound = gamma(16) * mag
    need = (err / np.where(bound > 0, bound, 1.0)).max()
    print(f"routed: worst error / bound {need:.3f}")
    assert np.isfinite(y).all() and (err <= bound).all(), f"routed value exceeds the bound by {need:.2f}x"
    assert np.array_equal(y[0], uh[:, 0] * q[0])                # day 0 sees zero history: one product
    check_cost(cost, y, target, w, T, t_first, "routed, weighted")
    # w = NULL is w = 1, bit for bit
    _, y1, c1 = run(poplib, T, t_first, q, target, None, a, bb)
    _, y2, c2 = run(poplib, T, t_first, q, target, np.ones_like(w), a, bb)
    assert np.array_equal(y1.view(np.uint32), y.view(np.uint32)) and np.array_equal(c1.view(np.uint32), c2.view(np.uint32))
    check_cost(c1, y1, target, None, T, t_first, "routed, unweighted")


@pytest.mark.parametrize("T,t_first", CASES, ids=[f"T{t}-first{f}" for t, f in CASES])
def test_unrouted_cost_and_what_t_first_changes(poplib, T, t_first):
    q, target, w, a, bb = draw(T, t_first, seed=100 * T + t_first + 50)
    uh, y, cost = run(poplib, T, t_first, q, target, w, None, None)
    assert np.array_equal(y.view(np.uint32), q.view(np.uint32)) and not uh.any()    # no routing: the mean itself
    check_cost(cost, y, target, w, T, t_first, "un-routed")
    if t_first:
        # the days before t_first shape the window (the routed series does not depend on t_first) but not the cost
        _, yr, cr = run(poplib, T, t_first, q, target, w, a, bb)
        full_t = np.concatenate([np.zeros((t_first, B), np.float32), target])
        full_w = np.concatenate([np.zeros((t_first, B), np.float32), w])
        _, y0, c0 = run(poplib, T, 0, q, full_t, full_w, a, bb)
        assert np.array_equal(y0.view(np.uint32), yr.view(np.uint32))
        assert yr[t_first:].any() and np.abs(yr[t_first] - y[t_first]).max() > 0     # history from before t_first is in it
        check_cost(cr, yr, target, w, T, t_first, "routed from t_first")
        # zero-weight days in front add exact zeros: the cost over all days with w = 0 there is the same number
        assert np.array_equal(c0.view(np.uint32), cr.view(np.uint32))
