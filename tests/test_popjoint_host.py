"""CPU tier: the per-basin arithmetic of hbvx_population_joint (hydrodl2_amd/csrc/hbv_pop.h: a BasinStats for the flow
term and an AuxStats for the aux term), compiled for the host (tests/hosttest/popjoint_host.cpp feeds one pair per basin
day by day, as k_pop's joint form does) and checked on the random float32 series of tests/test_popstats_host.py.

The aux term: the four chains on a value v that is neither routed nor transformed, against float64 sums over the
float32 v, o, m the code was given, d = v - m, e = o - m, r = v - o formed in float64 -- the bounds of
tests/test_popstats_host.py, gamma(n) = n u / (1 - n u), u = 2^-24, T the days of the call:
  |sse - sum w r^2| <= gamma(T + 2) sum w r^2        |s1 - sum w d|   <= gamma(T + 1) sum w |d|
  |s2  - sum w d^2| <= gamma(T + 3) sum w d^2        |s3 - sum w d e| <= gamma(T + 3) sum w |d e|
The flow term fed beside it keeps BasinStats' bits: the routed value and the four sums of popstats_host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from .test_pop_host import B, CASES, draw, gamma
from .test_popstats_host import TRANSFORMS, bits, observed
from .test_popstats_host import run as run_stats

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "hosttest", f) for f in ("popjoint_host.cpp", "popstats_host.cpp", "pop_host.cpp")]
LIB = os.path.join(HERE, "hosttest", "libpopjoint_host.so")
HDR = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_pop.h")


@pytest.fixture(scope="module")
def jointlib():
    newest = max(os.path.getmtime(f) for f in SRCS + [HDR])
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB] + SRCS)
    dll = C.CDLL(LIB)
    dll.popjoint_host.argtypes = [C.c_int] * 4 + [C.c_void_p] * 14
    dll.popjoint_host.restype = C.c_int
    dll.popstats_host.argtypes = [C.c_int] * 4 + [C.c_void_p] * 10
    dll.popstats_host.restype = C.c_int
    return dll


def run(dll, T, t_first, transform, q, ot, w, shift, eps, a, bb, v, at, aw, ashift):
    y = np.full((T, B), np.nan, dtype=np.float32)
    out = np.full((4, B), np.nan, dtype=np.float32)
    aout = np.full((4, B), np.nan, dtype=np.float32)
    for arr in (q, ot, w, shift, eps, a, bb, v, at, aw, ashift):
        assert arr is None or (arr.flags["C_CONTIGUOUS"] and arr.dtype == np.float32)
    ptr = lambda arr: None if arr is None else arr.ctypes.data      # noqa: E731
    rc = dll.popjoint_host(T, B, t_first, TRANSFORMS[transform], ptr(a), ptr(bb), ptr(q), ptr(ot), ptr(w), ptr(shift),
                           ptr(eps), ptr(v), ptr(at), ptr(aw), ptr(ashift), y.ctypes.data, out.ctypes.data,
                           aout.ctypes.data)
    assert rc == 0
    return y, out, aout


def check_aux(aout, v, at, aw, ashift, T, t_first, what):
    v8, o8, m8 = v[t_first:].astype(np.float64), at.astype(np.float64), ashift.astype(np.float64)
    w8 = np.ones_like(v8) if aw is None else aw.astype(np.float64)
    d, e, r = v8 - m8, o8 - m8, v8 - o8
    rows = (("sse", aout[0], w8 * r * r, w8 * r * r, T + 2), ("s1", aout[1], w8 * d, w8 * np.abs(d), T + 1),
            ("s2", aout[2], w8 * d * d, w8 * d * d, T + 3), ("s3", aout[3], w8 * d * e, w8 * np.abs(d * e), T + 3))
    assert np.isfinite(aout).all(), f"{what}: an aux chain is not finite"
    for name, got, terms, mags, n in rows:
        err = np.abs(got.astype(np.float64) - terms.sum(0))
        bound = gamma(n) * mags.sum(0)
        need = (err / np.where(bound > 0, bound, 1.0)).max()
        print(f"{what}: aux {name} worst error / bound {need:.3f}")
        assert (err <= bound).all(), f"{what}: aux {name} misses its float64 sum by {need:.2f} x the bound"


@pytest.mark.parametrize("routed", [True, False], ids=["routed", "unrouted"])
@pytest.mark.parametrize("transform", list(TRANSFORMS))
@pytest.mark.parametrize("T,t_first", CASES, ids=[f"T{t}-first{f}" for t, f in CASES])
def test_aux_chains_against_float64_and_the_flow_term_keeps_its_bits(jointlib, T, t_first, transform, routed):
    q, target, w, a, bb = draw(T, t_first, seed=100 * T + t_first + (0 if routed else 50))
    if not routed:
        a = bb = None
    ot, shift, eps = observed(target, w, transform)
    # the aux series: that file's random series under another seed -- dry spells, basins of different scale, a target
    # near it, weights with exact zeros; the shift as population_joint_stats forms it
    v, atarget, aw, _, _ = draw(T, t_first, seed=100 * T + t_first + 7000)
    at, ashift, _ = observed(atarget, aw, "none")
    y, out, aout = run(jointlib, T, t_first, transform, q, ot, w, shift, eps, a, bb, v, at, aw, ashift)
    check_aux(aout, v, at, aw, ashift, T, t_first, f"{transform}, weighted")

    # the flow term beside it: BasinStats' bits, routed value and all four sums
    y_stats, _, out_stats = run_stats(jointlib, T, t_first, transform, q, ot, w, shift, eps, a, bb)
    assert np.array_equal(bits(y), bits(y_stats)) and np.array_equal(bits(out), bits(out_stats))

    # the aux term is BasinStats' own lines under 'none' on another value: fed the un-routed flow's numbers, the same bits
    ot0, shift0, eps0 = observed(target, w, "none")
    _, _, flow0 = run_stats(jointlib, T, t_first, "none", q, ot0, w, shift0, eps0, None, None)
    _, _, aux0 = run(jointlib, T, t_first, transform, q, ot, w, shift, eps, a, bb, q, ot0, w, shift0)
    assert np.array_equal(bits(aux0), bits(flow0)), "AuxStats and BasinStats disagree on the same numbers"

    # aux_w = NULL is aux_w = 1, bit for bit, and changes nothing in the flow term
    at1, ashift1, _ = observed(atarget, None, "none")
    _, out1, aout1 = run(jointlib, T, t_first, transform, q, ot, w, shift, eps, a, bb, v, at1, None, ashift1)
    _, _, aout2 = run(jointlib, T, t_first, transform, q, ot, w, shift, eps, a, bb, v, at1, np.ones_like(aw), ashift1)
    assert np.array_equal(bits(aout1), bits(aout2)) and np.array_equal(bits(out1), bits(out))
    check_aux(aout1, v, at1, None, ashift1, T, t_first, f"{transform}, unweighted")

    if t_first:
        # the days before t_first do not reach the aux chains: other values there, the same bits
        v2 = v.copy()
        v2[:t_first] = 1e6
        _, _, aout3 = run(jointlib, T, t_first, transform, q, ot, w, shift, eps, a, bb, v2, at, aw, ashift)
        assert np.array_equal(bits(aout3), bits(aout))


def test_a_sparse_aux_record(jointlib):
    """An 8-day product: weight 1 on every 8th counted day and 0 elsewhere (the target 0 there, as `_observations`
    leaves a NaN).  The zero-weight days add exact zeros: the sums are those of the observed days alone."""
    T, t_first = 40, 5
    q, target, w, a, bb = draw(T, t_first, seed=4005)
    ot, shift, eps = observed(target, w, "none")
    v, atarget, _, _, _ = draw(T, t_first, seed=11005)
    aw = np.zeros_like(atarget)
    aw[::8] = 1.0
    at, ashift, _ = observed(np.where(aw > 0, atarget, 0.0).astype(np.float32), aw, "none")
    _, _, aout = run(jointlib, T, t_first, "none", q, ot, w, shift, eps, a, bb, v, at, aw, ashift)
    check_aux(aout, v, at, aw, ashift, T, t_first, "every 8th day")
    # the same days fed alone, in order, as a record of their own
    days = np.arange(T - t_first)[::8]
    n = len(days)
    vs = np.ascontiguousarray(v[t_first:][days])
    qs = np.ascontiguousarray(q[:n])
    os_, ss, es = observed(np.ascontiguousarray(target[:n]), None, "none")
    _, _, alone = run(jointlib, n, 0, "none", qs, os_, None, ss, es, None, None, vs, np.ascontiguousarray(at[days]), None, ashift)
    assert np.array_equal(bits(alone), bits(aout))
