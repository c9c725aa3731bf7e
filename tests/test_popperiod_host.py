"""CPU tier: the per-basin arithmetic of hbvx_population_period (hydrodl2_amd/csrc/hbv_pop.h: two PeriodMeans feeding a
BasinStats and an AuxStats), compiled for the host (tests/hosttest/popperiod_host.cpp feeds one set per basin day by day
with the cursors of k_pop's period form) and checked on the random float32 series of tests/test_pop_host.py.

With gamma(n) = n u / (1 - n u), u = 2^-24:
  a period value   the mean of n float32 daily values, n - 1 additions in ascending order and one division: against the
                   float64 mean of those float32 values within gamma(n) * mean|y|;
  the eight sums   against float64 sums over the code's own float32 period values (the flow's AFTER its transform): the
                   bounds of tests/test_popstats_host.py and tests/test_popjoint_host.py with the K periods in place of
                   the T days.
Everything else is a statement about bits: daily calendars are popjoint_host; days outside the scored periods reach no
chain; the period values fed as a daily record of K days give the same chains."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hydrodl2_amd.population import _calendar

from .test_pop_host import B, CASES, draw, gamma
from .test_popjoint_host import check_aux
from .test_popjoint_host import run as run_joint
from .test_popstats_host import TRANSFORMS, bits, check_chains, observed

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "hosttest", f)
        for f in ("popperiod_host.cpp", "popjoint_host.cpp", "popstats_host.cpp", "pop_host.cpp")]
LIB = os.path.join(HERE, "hosttest", "libpopperiod_host.so")
HDR = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_pop.h")

MONTHS = [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31, 31]


@pytest.fixture(scope="module")
def periodlib():
    newest = max(os.path.getmtime(f) for f in SRCS + [HDR])
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB] + SRCS)
    dll = C.CDLL(LIB)
    dll.popperiod_host.argtypes = [C.c_int] * 6 + [C.c_void_p] * 19
    dll.popperiod_host.restype = C.c_int
    dll.popjoint_host.argtypes = [C.c_int] * 4 + [C.c_void_p] * 14
    dll.popjoint_host.restype = C.c_int
    return dll


def ends_of(periods, T_out):
    """int32 closing days from what `population_period_stats` takes as a calendar"""
    return np.ascontiguousarray(_calendar(periods, T_out, "periods", "test").numpy().astype(np.int32))


def run(dll, T, t_first, transform, q, ot, w, shift, eps, a, bb, v, at, aw, ashift, fend, aend):
    KF, KA = len(fend), len(aend)
    y = np.full((T, B), np.nan, dtype=np.float32)
    fmean, fmean_t = (np.full((KF, B), np.nan, dtype=np.float32) for _ in range(2))
    amean = np.full((KA, B), np.nan, dtype=np.float32)
    out, aout = (np.full((4, B), np.nan, dtype=np.float32) for _ in range(2))
    for arr in (q, ot, w, shift, eps, a, bb, v, at, aw, ashift):
        assert arr is None or (arr.flags["C_CONTIGUOUS"] and arr.dtype == np.float32)
    assert ot.shape == (KF, B) and at.shape == (KA, B) and fend.dtype == np.int32 and aend.dtype == np.int32
    ptr = lambda arr: None if arr is None else arr.ctypes.data      # noqa: E731
    rc = dll.popperiod_host(T, B, t_first, TRANSFORMS[transform], KF, KA, ptr(a), ptr(bb), ptr(q), ptr(ot), ptr(w),
                            ptr(shift), ptr(eps), ptr(v), ptr(at), ptr(aw), ptr(ashift), ptr(fend), ptr(aend), ptr(y),
                            ptr(fmean), ptr(fmean_t), ptr(amean), ptr(out), ptr(aout))
    assert rc == 0
    return y, fmean, fmean_t, amean, out, aout


def per_period(daily, weights, ends):
    """Period observations from daily ones: the float32 mean of the days of each period, and the weight of its closing
    day (random, with exact zeros)."""
    starts = np.concatenate([[0], ends[:-1] + 1])
    tgt = np.stack([daily[s:e + 1].astype(np.float64).mean(0) for s, e in zip(starts, ends)]).astype(np.float32)
    return np.ascontiguousarray(tgt), np.ascontiguousarray(weights[ends])


def check_means(mean, daily, ends, what):
    """Each period value against the float64 mean of the float32 daily values it was formed from."""
    starts = np.concatenate([[0], ends[:-1] + 1])
    assert np.isfinite(mean).all(), f"{what}: a period was left unclosed"
    for k, (s, e) in enumerate(zip(starts, ends)):
        n = int(e - s + 1)
        d8 = daily[s:e + 1].astype(np.float64)
        err = np.abs(mean[k].astype(np.float64) - d8.mean(0))
        bound = gamma(n) * np.abs(d8).mean(0)
        assert (err <= bound).all(), f"{what}: period {k} of {n} days misses its float64 mean by {(err / bound).max():.2f} x the bound"
        if n == 1:
            assert np.array_equal(bits(mean[k]), bits(daily[s])), f"{what}: a one-day period is not the day's value"


def problem(T, t_first, transform, routed, fcal, acal):
    """The series of tests/test_popjoint_host.py for (T, t_first), with period observations on the two calendars."""
    q, target, w, a, bb = draw(T, t_first, seed=100 * T + t_first + (0 if routed else 50))
    if not routed:
        a = bb = None
    v, atarget, aw, _, _ = draw(T, t_first, seed=100 * T + t_first + 7000)
    fend, aend = ends_of(fcal, T - t_first), ends_of(acal, T - t_first)
    tk, wk = per_period(target, w, fend)
    ak, awk = per_period(atarget, aw, aend)
    ot, shift, eps = observed(tk, wk, transform)
    at, ashift, _ = observed(ak, awk, "none")
    return dict(q=q, ot=ot, w=wk, shift=shift, eps=eps, a=a, bb=bb, v=v, at=at, aw=awk, ashift=ashift, fend=fend, aend=aend)


def calendars(T_out):
    """(flow calendar, aux calendar) pairs for a record of T_out scored days: blocks of 3 and 8 (as far as they fit),
    the two swapped, and a list whose first period is a single day beside blocks of 3."""
    n3, n8 = min(3, T_out), min(8, T_out)
    out = [(n3, n8), (n8, n3)]
    if T_out >= 4:
        out.append(([0] + list(range(3, T_out, 2)), n3))
    return out


@pytest.mark.parametrize("routed", [True, False], ids=["routed", "unrouted"])
@pytest.mark.parametrize("transform", list(TRANSFORMS))
@pytest.mark.parametrize("T,t_first", CASES, ids=[f"T{t}-first{f}" for t, f in CASES])
def test_daily_calendars_are_popjoint_host(periodlib, T, t_first, transform, routed):
    q, target, w, a, bb = draw(T, t_first, seed=100 * T + t_first + (0 if routed else 50))
    if not routed:
        a = bb = None
    ot, shift, eps = observed(target, w, transform)
    v, atarget, aw, _, _ = draw(T, t_first, seed=100 * T + t_first + 7000)
    at, ashift, _ = observed(atarget, aw, "none")
    daily = ends_of(None, T - t_first)
    y, fmean, _, amean, out, aout = run(periodlib, T, t_first, transform, q, ot, w, shift, eps, a, bb, v, at, aw, ashift,
                                        daily, daily)
    y_j, out_j, aout_j = run_joint(periodlib, T, t_first, transform, q, ot, w, shift, eps, a, bb, v, at, aw, ashift)
    assert np.array_equal(bits(y), bits(y_j)), "the routed value"
    assert np.array_equal(bits(out), bits(out_j)) and np.array_equal(bits(aout), bits(aout_j)), "the eight sums"
    assert np.array_equal(bits(fmean), bits(y[t_first:])) and np.array_equal(bits(amean), bits(v[t_first:]))


@pytest.mark.parametrize("routed", [True, False], ids=["routed", "unrouted"])
@pytest.mark.parametrize("transform", list(TRANSFORMS))
@pytest.mark.parametrize("T,t_first", CASES, ids=[f"T{t}-first{f}" for t, f in CASES])
def test_period_means_and_chains_against_float64_and_the_bit_rules(periodlib, T, t_first, transform, routed):
    T_out = T - t_first
    for fcal, acal in calendars(T_out):
        what = f"{transform}, flow {fcal}, aux {acal}"
        p = problem(T, t_first, transform, routed, fcal, acal)
        y, fmean, fmean_t, amean, out, aout = run(periodlib, T, t_first, transform, **p)
        fend, aend = p["fend"], p["aend"]
        KF, KA = len(fend), len(aend)
        check_means(fmean, y[t_first:], fend, what + ": flow")
        check_means(amean, p["v"][t_first:], aend, what + ": aux")
        check_chains(out, fmean_t, p["ot"], p["w"], p["shift"], KF, 0, what)
        check_aux(aout, amean, p["at"], p["aw"], p["ashift"], KA, 0, what)
        got = [bits(x) for x in (fmean, amean, out, aout)]

        # the routed value does not depend on the calendars: BasinStats' own
        daily = ends_of(None, T_out)
        z = np.zeros((T_out, B), np.float32)
        y_j, _, _ = run_joint(periodlib, T, t_first, transform, p["q"], z, None, p["shift"], p["eps"], p["a"], p["bb"],
                              p["v"], z, None, p["ashift"])
        assert np.array_equal(bits(y), bits(y_j)), what

        # an int n and the list of its closing days
        if isinstance(fcal, int):
            lists = dict(p, fend=ends_of(list(range(fcal - 1, T_out, fcal)), T_out),
                         aend=ends_of(list(range(acal - 1, T_out, acal)), T_out))
            again = run(periodlib, T, t_first, transform, **lists)
            assert all(np.array_equal(g, bits(x)) for g, x in zip(got, again[1:2] + again[3:])), what

        # days before t_first and days after a calendar's last closing day reach no chain of that calendar (the flow's
        # days before t_first shape the routing window, so only the aux value moves there)
        other = dict(p, q=p["q"].copy(), v=p["v"].copy())
        other["v"][:t_first] = 1e6
        other["v"][t_first + aend[-1] + 1:] = 1e6
        other["q"][t_first + fend[-1] + 1:] = 1e6
        again = run(periodlib, T, t_first, transform, **other)
        assert all(np.array_equal(g, bits(x)) for g, x in zip(got, again[1:2] + again[3:])), what

        # the K period values as an un-routed daily record of K days: the same chains
        for mean, K, o, wk in ((fmean, KF, p["ot"], p["w"]), (amean, KA, p["at"], p["aw"])):
            rec = dict(p, q=np.ascontiguousarray(fmean if mean is fmean else np.zeros((K, B), np.float32)), a=None, bb=None,
                       v=np.ascontiguousarray(amean if mean is amean else np.zeros((K, B), np.float32)),
                       fend=ends_of(None, K), aend=ends_of(None, K))
            if mean is fmean:
                rec.update(at=np.zeros((K, B), np.float32), aw=None)
                _, _, _, _, out_k, _ = run(periodlib, K, 0, transform, **rec)
                assert np.array_equal(bits(out_k), bits(out)), what
            else:
                rec.update(ot=np.ones((K, B), np.float32), w=None)
                _, _, _, _, _, aout_k = run(periodlib, K, 0, transform, **rec)
                assert np.array_equal(bits(aout_k), bits(aout)), what


@pytest.mark.parametrize("transform", list(TRANSFORMS))
def test_thirteen_months_beside_eight_day_composites(periodlib, transform):
    """A 400-day record after 5 days of warm-up: thirteen months for the flow (four days dropped), 8-day composites for
    the aux series (fifty periods, nothing dropped)."""
    T, t_first = 405, 5
    months = list(np.cumsum(MONTHS) - 1)
    p = problem(T, t_first, transform, True, months, 8)
    y, fmean, fmean_t, amean, out, aout = run(periodlib, T, t_first, transform, **p)
    assert len(p["fend"]) == 13 and p["fend"][-1] == 395 and len(p["aend"]) == 50
    check_means(fmean, y[t_first:], p["fend"], "months")
    check_means(amean, p["v"][t_first:], p["aend"], "8-day")
    check_chains(out, fmean_t, p["ot"], p["w"], p["shift"], 13, 0, f"{transform}, months")
    check_aux(aout, amean, p["at"], p["aw"], p["ashift"], 50, 0, f"{transform}, 8-day")
    # the four dropped days change nothing
    other = dict(p, q=p["q"].copy())
    other["q"][t_first + 396:] = 0.0
    again = run(periodlib, T, t_first, transform, **other)
    assert np.array_equal(bits(again[4]), bits(out)) and np.array_equal(bits(again[1]), bits(fmean))


def test_a_calendar_that_does_not_ascend_leaves_periods_unclosed(periodlib):
    """The cursor rules of the kernel: a closing day that is not ahead is never met; what closed before it stands."""
    T, t_first = 40, 5
    p = problem(T, t_first, "none", True, [2, 5, 8, 11], 3)
    good = run(periodlib, T, t_first, "none", **p)
    bad = dict(p, fend=np.array([2, 5, 4, 11], dtype=np.int32))
    _, fmean, _, amean, out, aout = run(periodlib, T, t_first, "none", **bad)
    assert np.array_equal(bits(fmean[:2]), bits(good[1][:2])) and np.isnan(fmean[2:]).all()
    assert np.array_equal(bits(amean), bits(good[3])) and np.array_equal(bits(aout), bits(good[5]))
    two = dict(p, fend=p["fend"][:2].copy(), ot=p["ot"][:2].copy(), w=p["w"][:2].copy())
    assert np.array_equal(bits(out), bits(run(periodlib, T, t_first, "none", **two)[4]))
