"""GPU tier: `adj_population_period_stats` / `adj_population_search(periods=..., aux_key=...)`
(hydrodl2_amd/adj_population.py) on hbvx_adj_population_period.

The problems are those of tests/test_adj_population_gpu.py (its `Case`, imported, P = 3 and 17 on the bit case); RUNS
gives each one or two calls (flow calendar, aux key, aux calendar): daily (None), blocks of 8, 5, 3 and 2, thirteen
months, an uneven sequence with one-day periods, a period longer than the 15 routing taps and an end before the last
day, and a single period closing on day 0.  Every storage is an aux key somewhere; SM and SNOWPACK on the routed,
masked record, whose period targets carry NaN and whose period weights carry exact zeros.

  bits        on every case, run and transform: with both calendars daily and no aux term the four sums and the series
              are `adj_population_stats`'; an aux term changes no flow bit; two calls agree; a candidate's numbers do not
              depend on the other candidates or on return_series; under the poisoned output buffers every element is
              finite (the Python front end only passes calendars whose periods all close).
  flow means  each [P,K,B] mean against the float64 mean of the kernel's own daily series
              (`adj_population_stats(return_series=True)`) within gamma(n + 1) mean|y|, n the period's days; a one-day
              period is the day's value bit for bit.
  aux series  the yardstick is the module's own route: the candidate written into the static row, the module run under
              ops.record_paths(want_traj=True), the ensemble mean over the members of storage k in row t + 1 of the
              trajectory [5, T + 1, B * M] (hbv_adj_kernels.h: row t is the state ENTERING day t; lane b * M + j), in
              float64.  Daily elements and period means within adj_sets.VALUE_TOL; whether the daily series came out
              bit-equal to the float32 mean of the trajectory is printed, not asserted.
  sums        each of the eight against the float64 sum over the kernel's own period series within gamma(K + 2) of the
              summed magnitudes (test (a) of tests/test_adj_population_gpu.py with K for T_out), plus, under 'sqrt' and
              'log', the spread of the device's transform about the float64 one (K_BOUND of
              tests/test_population_stats_gpu.py, checked against the device here as there).
  scores      `population_score` of either sub-dictionary against float64 textbook scores of the module route's period
              means, |difference| / (1 + |1 - score|); records with fewer than 20 periods take part in the bit rules
              only.  Twin targets: period means of the hidden candidate's series (Case.twin's candidate) times
              exp(0.2 noise).  The tolerance is measured, not derived: worst value over SCORE_RUNS on the MI355X of
              profiles/r20_adj_population_period.md: 8.28e-7 (r of the daily SUZ series of the un-routed 120-day
              record; 5.3e-7 r of its daily flow, 4.0e-7 r of the 8-day flow of the 400-day record under the joint
              solver, 3.5e-7 and below on the others), asserted at four times that, MEASURED_PERIOD_SCORE_DIFF, and held
              below 1e-4."""
import functools

import pytest
import torch

from hydrodl2_amd import _abi, ops
from hydrodl2_amd.adj_population import adj_population_period_stats, adj_population_search
from hydrodl2_amd.population import _calendar, _observations, population_score

from . import adj_sets
from . import synth
from .test_adj_population_gpu import BIT_CASE, SCORED, TRANSFORMS, case, own_problem
from .test_population_gpu import DEV, U, bits, gamma
from .test_population_period_host import period_means64
from .test_population_score_host import textbook
from .test_population_stats_gpu import K_BOUND, device_transform, g64

MEASURED_PERIOD_SCORE_DIFF = 8.28e-7
PERIOD_SCORE_TOL = 4 * MEASURED_PERIOD_SCORE_DIFF
assert PERIOD_SCORE_TOL < 1e-4

STORAGES = tuple(_abi.ADJ_POP_AUX_SERIES)       # SNOWPACK, MELTWATER, SM, SUZ, SLZ: rows 0..4 of the trajectory
SUMS = ("sse", "s1", "s2", "s3")
MONTHS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31, 31)
MONTH_ENDS = tuple(sum(MONTHS[:k + 1]) - 1 for k in range(13))      # ends on day 395 of 400
UNEVEN65 = (0, 3, 4, 24, 31, 40, 50, 60)        # one-day periods (days 0 and 4), 20 days (5..24), ends before day 64
UNEVEN50 = (0, 17, 18, 30, 44)                  # one-day periods (days 0 and 18), 17 days (1..17), ends before day 49
# name -> ((flow calendar, aux key, aux calendar), ...)
RUNS = {
    # T_out 9 < 15 taps, M 3 padded to 4 lanes: one period and one unscored day; a single period closing on day 0
    "wet9": ((8, "MELTWATER", None), ((0,), "SM", (0,))),
    # one full wave plus a partly filled one from the zero start: two periods and four unscored days (eps is the case's)
    "m1-b67-t20-zero": ((8, "SNOWPACK", 5),),
    # the BETAET instance with nd = ADJ_FEW
    "wet65-three": ((UNEVEN65, "SUZ", 3), (3, "SLZ", UNEVEN65)),
    # the generic fetch, per-lane drop masks, NaN period targets and zero period weights; P = 17
    "wet64-list-masked": ((3, "SM", 8), (8, "SNOWPACK", 3)),
    # the start state comes from the warm-up pass (T_out 50)
    "storm90-warmup-wet": ((2, "MELTWATER", None), (UNEVEN50, "SNOWPACK", 8)),
    # un-routed, a column subset
    "wet120-norout-subset": ((None, "SM", 5), (5, "SUZ", None)),
    # the joint solver
    "wet400-joint": ((8, "SM", MONTH_ENDS), (MONTH_ENDS, "SLZ", 8)),
}
ALL_RUNS = [(n, i) for n in RUNS for i in range(len(RUNS[n]))]
MIN_PERIODS = 20


def test_the_tables_cover_what_they_should():
    keys = {r[1] for runs in RUNS.values() for r in runs}
    assert keys == set(STORAGES)
    assert {r[1] for r in RUNS[BIT_CASE]} == {"SM", "SNOWPACK"}
    cals = [c for runs in RUNS.values() for r in runs for c in (r[0], r[2])]
    assert None in cals and 8 in cals and (0,) in cals and UNEVEN65 in cals
    assert any(r[0] != r[2] for runs in RUNS.values() for r in runs)
    for seq, T_out in ((UNEVEN65, 65), (UNEVEN50, 50)):
        days = [e - s for s, e in zip((-1,) + seq[:-1], seq)]
        assert 1 in days and max(days) > 15 and seq[-1] < T_out - 1


def as_arg(cal):
    return list(cal) if isinstance(cal, tuple) else cal


def ends_of(cs, cal):
    return _calendar(as_arg(cal), cs.T_out, "periods", "test").tolist()


def storages_of(rec):
    """[5,T,B] float64: the ensemble mean of each storage at the END of each day of a recorded call, from its trajectory
    [5, T + 1, B * M] (row t: the state entering day t; lane b * M + j)."""
    T, B, M = rec.cfg.T, rec.cfg.B, rec.cfg.M
    traj = rec.traj
    assert traj is not None and tuple(traj.shape) == (5, T + 1, B * M)
    rows = ops.state_series(traj, _abi.TRAJ_ROWS, T, B, M)
    view = traj.view(5, T + 1, B, M)
    for k in range(5):
        assert torch.equal(rows[k], view[k])                            # ops.state_series reads the same layout
        assert torch.equal(view[k, T].reshape(-1), rec.state_out.reshape(5, -1)[k])     # the last row is state_out
    return view[:, 1:].double().mean(-1), view[:, 1:].float().sum(-1) * (1.0 / M)


def run_module(cs, parameters):
    """(flow_sim [T_out,B] float32, storages [5,T_out,B] float64, the same as a float32 sum * (1/M))"""
    cs.prepare()
    with torch.no_grad(), ops.record_paths(want_traj=True) as records:
        out = cs.model(cs.xd, parameters)
    rec = records[-1]
    assert rec.cfg.T == cs.T_out and rec.cfg.B == cs.B and rec.cfg.M == cs.M
    st8, st4 = storages_of(rec)
    return out["flow_sim"][..., 0].clone(), st8, st4


@functools.lru_cache(maxsize=None)
def module_route(name):
    """The yardstick, computed once per case: (flows [P+1,T_out,B] float32, storages [P+1,5,T_out,B] float64, the
    float32 means [P+1,5,T_out,B]) of every candidate and, last, of the hidden candidate of Case.twin."""
    cs = case(name)
    hidden = cs.cand[0] + 0.35 * torch.from_numpy(synth.normalish((cs.B, len(cs.cols)), 192)).to(cs.cand.device)
    got = [run_module(cs, cs.with_row(v)) for v in list(cs.cand) + [hidden]]
    return tuple(torch.stack([g[i] for g in got]) for i in range(3))


@functools.lru_cache(maxsize=None)
def period_twin(name, run):
    """(target [KF,B], weights or None, aux target [KA,B], aux weights or None): period means of the hidden candidate's
    series times exp(0.2 noise).  On the masked case a period is missing where the case's own target is NaN on its
    closing day, and weighs what that day weighs (exact zeros among them)."""
    cs = case(name)
    fcal, key, acal = RUNS[name][run]
    flows, stor, _ = module_route(name)
    out = []
    for series, cal, seed in ((flows[-1], fcal, 300), (stor[-1, STORAGES.index(key)], acal, 301 + STORAGES.index(key))):
        ends = ends_of(cs, cal)
        noise = torch.from_numpy(synth.normalish((len(ends), cs.B), seed)).to(DEV)
        tgt = (period_means64(series, ends) * torch.exp(0.2 * noise.double())).float()
        w = None
        if cs.masked:
            tgt = torch.where(torch.isnan(cs.target[ends]), cs.target[ends], tgt)
            w = cs.weights[ends].contiguous()
        out += [tgt.contiguous(), w]
    return tuple(out)


def period(name, run, transform="none", cand=None, aux=True, cals=None, obs=None, **kw):
    cs = case(name)
    fcal, key, acal = RUNS[name][run]
    if cals is not None:
        fcal, acal = cals
    tgt, w, atgt, aw = obs if obs is not None else period_twin(name, run)
    cs.prepare()
    cand = cs.cand if cand is None else cand
    if not aux:
        return adj_population_period_stats(cs.model, cs.xd, cs.p, cand, tgt, as_arg(fcal), names=cs.names, weights=w,
                                           transform=transform, eps=cs.eps, **kw)
    return adj_population_period_stats(cs.model, cs.xd, cs.p, cand, tgt, as_arg(fcal), atgt, key, as_arg(acal), cs.names, w,
                                       aw, transform, cs.eps, **kw)


@functools.lru_cache(maxsize=None)
def period_with_series(name, run):
    return period(name, run, return_series=True)


@functools.lru_cache(maxsize=None)
def daily_stats(name):
    """The kernel's own daily flow series, through the existing call."""
    return case(name).stats("none", return_series=True)


@functools.lru_cache(maxsize=None)
def daily_aux(name, run):
    """The kernel's own daily aux series of the run's key: the call with a daily aux calendar."""
    cs = case(name)
    fcal, key, _ = RUNS[name][run]
    tgt, w, _, _ = period_twin(name, run)
    atgt = module_route(name)[1][-1, STORAGES.index(key)].float().contiguous()
    return period(name, run, cals=(fcal, None), obs=(tgt, w, atgt, None), return_series=True)["aux"]["series"]


def w8_of(tgt, w):
    w = torch.ones_like(tgt) if w is None else w
    return torch.where(torch.isnan(tgt), torch.zeros_like(w), w).double()


def all_finite(got):
    return all(bool(torch.isfinite(got[t][k]).all()) for t in got if t in ("flow", "aux") for k in SUMS + ("series",)
               if k in got[t])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RUNS))
def test_daily_calendars_without_an_aux_term_are_adj_population_stats(hip_backend, name):
    assert ops._POISON, "the GPU tier runs with NaN-poisoned output buffers"
    cs = case(name)
    tgt = cs.twin
    key = RUNS[name][0][1]
    atgt = module_route(name)[1][-1, STORAGES.index(key)].float().contiguous()
    for transform in TRANSFORMS:
        want = cs.stats(transform, return_series=True)
        cs.prepare()
        got = adj_population_period_stats(cs.model, cs.xd, cs.p, cs.cand, tgt, None, names=cs.names, weights=cs.weights,
                                          transform=transform, eps=cs.eps, return_series=True)
        assert set(got) == {"flow", "columns", "outputs"} and got["columns"] == cs.cols
        flow = got["flow"]
        for k in SUMS + ("series",):
            assert flow[k].dtype == torch.float32
            assert torch.equal(bits(flow[k]), bits(want[k])), f"{transform}: {k} is not adj_population_stats'"
        assert tuple(flow["series"].shape) == (cs.P, cs.T_out, cs.B)
        assert torch.equal(bits(flow["shift"]), bits(want["shift"])) and torch.equal(flow["n_obs"], want["n_obs"])
        assert all(torch.equal(flow["obs"][k], want["obs"][k]) for k in ("W", "e1", "e2"))
        assert flow["period_ends"].tolist() == list(range(cs.T_out)) and flow["period_days"].tolist() == [1] * cs.T_out
        assert flow["transform"] == transform and (flow["eps"] is None) == (transform != "log")
        # a daily aux term beside it: no flow bit moves, and the method is the function
        cs.prepare()
        both = cs.model.population_period_stats(cs.xd, cs.p, cs.cand, tgt, None, atgt, key, None, cs.names, cs.weights, None,
                                                transform, cs.eps, True)
        assert set(both) == {"flow", "aux", "columns", "outputs"} and both["aux"]["key"] == key
        assert both["aux"]["transform"] == "none" and all_finite(both)
        for k in SUMS + ("series",):
            assert torch.equal(bits(both["flow"][k]), bits(want[k])), f"{transform}: flow {k} depends on the aux term"
        assert tuple(both["aux"]["series"].shape) == (cs.P, cs.T_out, cs.B)


@pytest.mark.gpu
@pytest.mark.parametrize("name,run", ALL_RUNS)
def test_bit_rules(hip_backend, name, run):
    assert ops._POISON
    cs = case(name)
    assert cs.P == (17 if name == BIT_CASE else 3)
    fcal, key, acal = RUNS[name][run]
    KF, KA = len(ends_of(cs, fcal)), len(ends_of(cs, acal))
    pick = [0, 3, 8] if cs.P == 17 else [0, 2]

    def same(a, b, ia=slice(None), ib=slice(None), with_series=True, terms=("flow", "aux")):
        return all(torch.equal(bits(a[t][k][ia]), bits(b[t][k][ib]))
                   for t in terms for k in SUMS + (("series",) if with_series else ()))

    for transform in TRANSFORMS:
        a = period(name, run, transform, return_series=True)
        assert all_finite(a), f"{transform}: a poisoned or non-finite element was left"
        assert tuple(a["flow"]["series"].shape) == (cs.P, KF, cs.B) and tuple(a["aux"]["series"].shape) == (cs.P, KA, cs.B)
        assert a["flow"]["period_ends"].tolist() == ends_of(cs, fcal) and a["aux"]["period_ends"].tolist() == ends_of(cs, acal)
        assert a["aux"]["key"] == key and a["columns"] == cs.cols
        b = period(name, run, transform, return_series=True)
        assert same(a, b), f"{transform}: two calls differ"
        plain = period(name, run, transform)
        assert "series" not in plain["flow"] and "series" not in plain["aux"]
        assert same(plain, a, with_series=False), f"{transform}: return_series changes the sums"
        alone = period(name, run, transform, aux=False, return_series=True)
        assert set(alone) == {"flow", "columns", "outputs"}
        assert same(alone, a, terms=("flow",)), f"{transform}: the flow numbers depend on the aux term"
        one = period(name, run, transform, cand=cs.cand[pick[-1]:pick[-1] + 1].contiguous(), return_series=True)
        assert same(one, a, 0, pick[-1]), f"{transform}: candidate {pick[-1]} alone has other bits"
        sub = period(name, run, transform, cand=cs.cand[pick].contiguous(), return_series=True)
        assert same(sub, a, slice(None), pick), f"{transform}: a subset of the candidates has other bits"
    # the candidates differ, and so do their numbers: the candidate index reaches the parameters
    assert not torch.equal(bits(a["flow"]["series"][0]), bits(a["flow"]["series"][-1]))
    assert not torch.equal(bits(a["aux"]["series"][0]), bits(a["aux"]["series"][-1]))


@pytest.mark.gpu
@pytest.mark.parametrize("name,run", ALL_RUNS)
def test_flow_period_means_against_the_kernels_own_daily_series(hip_backend, name, run):
    cs = case(name)
    ends = ends_of(cs, RUNS[name][run][0])
    got = period_with_series(name, run)["flow"]
    days = got["period_days"].tolist()
    assert got["period_ends"].tolist() == ends and sum(days) == ends[-1] + 1
    series, daily = got["series"], daily_stats(name)["series"]
    own, mag = period_means64(daily, ends), period_means64(daily.abs(), ends)
    g = torch.tensor([gamma(n + 1) for n in days], dtype=torch.float64, device=own.device).view(1, -1, 1)
    err = (series.double() - own).abs()
    need = float((err / torch.where(mag > 0, g * mag, torch.ones_like(mag))).max())
    print(f"{name} run {run}: flow period means against the own daily series: worst error / bound {need:.3f}")
    assert bool((err <= g * mag).all()), f"a period mean misses the float64 mean of its days by {need:.2f} x the bound"
    for k, (n, e) in enumerate(zip(days, ends)):
        if n == 1:
            assert torch.equal(bits(series[:, k]), bits(daily[:, e])), f"the one-day period {k} is not day {e}'s value"


@pytest.mark.gpu
@pytest.mark.parametrize("name,run", ALL_RUNS)
def test_aux_series_against_the_trajectory_of_the_module(hip_backend, name, run):
    cs = case(name)
    _, key, acal = RUNS[name][run]
    k = STORAGES.index(key)
    _, stor8, stor4 = module_route(name)
    want = stor8[:cs.P, k]                                              # [P,T_out,B] float64
    rtol, atol_rel = adj_sets.VALUE_TOL
    daily = daily_aux(name, run)
    assert tuple(daily.shape) == (cs.P, cs.T_out, cs.B) and bool(torch.isfinite(daily).all())
    if key in ("SM", "SUZ", "SLZ"):
        assert float(want.abs().max()) > 0.1, "the storage is empty: the comparison would be empty"

    def close(got, ref, what):
        tol = atol_rel * float(ref.abs().max()) + rtol * ref.abs()
        err = (got.double() - ref).abs()
        print(f"{name} {key}: {what} worst error / tolerance {float((err / tol).max()):.4f} (max abs {float(err.max()):.3e})")
        assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} of {err.numel()} elements outside the value tolerance"

    close(daily, want, "daily aux series")
    print(f"{name} {key}: daily aux series bit-equal to the float32 mean of the trajectory: "
          f"{torch.equal(bits(daily), bits(stor4[:cs.P, k]))}")
    ends = ends_of(cs, acal)
    got = period_with_series(name, run)["aux"]
    assert got["period_ends"].tolist() == ends
    close(got["series"], period_means64(want, ends), "aux period means")
    # candidate 0 is the current row: its series is the primal's own trajectory
    primal = run_module(cs, cs.p)[1][k]
    close(daily[0], primal, "candidate 0 against the primal's trajectory")
    # ... and the period means are means of the kernel's own daily aux series
    days = got["period_days"].tolist()
    own, mag = period_means64(daily, ends), period_means64(daily.abs(), ends)
    g = torch.tensor([gamma(n + 1) for n in days], dtype=torch.float64, device=own.device).view(1, -1, 1)
    assert bool(((got["series"].double() - own).abs() <= g * mag).all())
    for i, (n, e) in enumerate(zip(days, ends)):
        if n == 1:
            assert torch.equal(bits(got["series"][:, i]), bits(daily[:, e]))


@pytest.mark.gpu
@pytest.mark.parametrize("name,run", ALL_RUNS)
def test_the_sums_against_float64_over_the_kernels_own_period_series(hip_backend, name, run):
    cs = case(name)
    tgt, w, atgt, aw = period_twin(name, run)
    for transform in TRANSFORMS:
        got = period(name, run, transform, return_series=True)
        for term, o, wts, tr in (("flow", tgt, w, transform), ("aux", atgt, aw, "none")):
            sub = got[term]
            K = int(o.shape[0])
            ob = _observations(cs.req, cs.xd, o, wts, tr, cs.eps if term == "flow" else None, "test", rows=K)
            assert torch.equal(bits(ob["shift"]), bits(sub["shift"]))
            w8 = w8_of(o, wts)
            assert torch.equal(sub["n_obs"], (w8 > 0).sum(0))
            series, eps = sub["series"], sub["eps"]
            y8 = g64(series, tr, eps)
            k = K_BOUND[tr]
            if tr != "none":
                dev = device_transform(hip_backend, series, None if eps is None else eps.expand_as(series), tr)
                assert float(((dev.double() - y8).abs() / (U * (1 + y8.abs()))).max()) <= k
            o8, m8 = ob["target"].double(), ob["shift"].double()
            d, e, r = y8 - m8, o8 - m8, y8 - o8
            delta = k * U * (1 + y8.abs())
            rows = (("sse", w8 * r * r, w8 * r * r, w8 * 2 * r.abs() * delta), ("s1", w8 * d, w8 * d.abs(), w8 * delta),
                    ("s2", w8 * d * d, w8 * d * d, w8 * 2 * d.abs() * delta),
                    ("s3", w8 * d * e, w8 * (d * e).abs(), w8 * e.abs() * delta))
            for key, terms, mags, spread in rows:
                err = (sub[key].double() - terms.sum(1)).abs()
                bound = gamma(K + 2) * mags.sum(1) + spread.sum(1)
                need = float((err / torch.where(bound > 0, bound, torch.ones_like(bound))).max())
                print(f"{name} run {run} {transform}: {term} {key} against its own period series: worst error / bound {need:.3f}")
                assert bool((err <= bound).all()), f"{transform}: {term} {key} misses its float64 sum by {need:.2f} x the bound"


# the runs with a series of at least MIN_PERIODS periods (the short records and the second run of the warm-up record
# have none)
SCORE_RUNS = [("wet65-three", 0), ("wet65-three", 1), ("wet64-list-masked", 0), ("wet64-list-masked", 1),
              ("storm90-warmup-wet", 0), ("wet120-norout-subset", 0), ("wet120-norout-subset", 1), ("wet400-joint", 0),
              ("wet400-joint", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,run", SCORE_RUNS)
def test_scores_against_the_module_route_on_period_means(hip_backend, name, run):
    cs = case(name)
    fcal, key, acal = RUNS[name][run]
    tgt, w, atgt, aw = period_twin(name, run)
    flows, stor8, _ = module_route(name)
    worst, scored = 0.0, 0

    def compare(got, want, metrics, what):
        nonlocal worst
        for metric in metrics:
            assert bool(torch.isfinite(want[metric]).all()), f"{what} {metric}: the yardstick has no score"
            score = population_score(got, metric)
            assert tuple(score.shape) == (cs.P, cs.B) and score.dtype == torch.float64
            assert bool(torch.isfinite(score).all()), f"{what} {metric}: a candidate has no score"
            diff = float(((score - want[metric]).abs() / (1 + (1 - want[metric]).abs())).max())
            worst = max(worst, diff)
            print(f"{what} {metric}: yardstick {float(want[metric].min()):.3f} .. {float(want[metric].max()):.3f}, "
                  f"worst difference {diff:.3e} (asserted {PERIOD_SCORE_TOL:.1e})")

    ends_f, ends_a = ends_of(cs, fcal), ends_of(cs, acal)
    if len(ends_f) >= MIN_PERIODS:
        scored += 1
        means = period_means64(flows[:cs.P], ends_f)
        for transform in TRANSFORMS:
            got = period(name, run, transform)["flow"]
            eps = got["eps"]
            want = textbook(g64(means, transform, eps), g64(tgt, transform, eps), w8_of(tgt, w))
            compare(got, want, SCORED[transform], f"{name} run {run} flow {transform}")
    if len(ends_a) >= MIN_PERIODS:
        scored += 1
        means = period_means64(stor8[:cs.P, STORAGES.index(key)], ends_a)
        got = period(name, run)["aux"]
        compare(got, textbook(means, atgt.double(), w8_of(atgt, aw)), SCORED["none"], f"{name} run {run} {key}")
    assert scored, "a run in SCORE_RUNS has no series with 20 periods"
    print(f"{name} run {run}: worst score difference {worst:.3e}")
    assert worst <= PERIOD_SCORE_TOL


@pytest.mark.gpu
def test_population_search_on_period_means_and_soil_moisture(hip_backend):
    """The 40-day twin of tests/test_adj_population_gpu.py, observed as 8-day means of the truth's flow_sim and SM."""
    T, B, M, P = 40, 5, 2, 32
    prob = own_problem(dict(T=T, B=B, M=M, dyn=()))
    model = adj_sets.model(DEV, prob, "staged", False)
    eager, st = type(model)._forward_eager, torch.from_numpy(synth.wet_states(B, M, 67)).to(DEV)
    model._forward_eager = lambda xd, pp: eager(model, xd, pp, state=st)        # a wet start: the twin has flow
    ny = model.learnable_param_count
    x = {"x_phy": torch.from_numpy(synth.forcing(T, B, seed=61)).to(DEV)}
    truth = torch.from_numpy(synth.raw_parameters(T, B, ny, seed=62)).to(DEV)
    with torch.no_grad(), ops.record_paths(want_traj=True) as records:
        daily = model(x, truth)["flow_sim"][..., 0].clone()
    ends = list(range(7, T, 8))
    obs = period_means64(daily, ends).float().contiguous()
    aobs = period_means64(storages_of(records[-1])[0][STORAGES.index("SM")], ends).float().contiguous()
    assert float(obs.max()) > 0.1 and float(aobs.max()) > 0.1
    start = torch.from_numpy(synth.raw_parameters(T, B, ny, seed=63, scale=1.5)).to(DEV)
    keep = [t.clone() for t in (start, obs, aobs, x["x_phy"])]

    def search(seed, fn=None, **kw):
        g = torch.Generator().manual_seed(seed)
        kw = {"objective": "kge", "aux_target": aobs, "aux_key": "SM", "periods": 8, "aux_periods": 8, **kw}
        fn = fn or (lambda *a, **k: adj_population_search(model, *a, **k))
        return fn(x, start, obs, n_candidates=P, n_rounds=3, generator=g, **kw)

    best, hist = search(5)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((start, obs, aobs, x["x_phy"]), keep)), "an input was modified"
    assert set(hist) == {"cost", "best_index", "columns", "score", "score_aux"}
    cost, score, score_aux = hist["cost"], hist["score"], hist["score_aux"]
    assert tuple(cost.shape) == tuple(score.shape) == tuple(score_aux.shape) == (4, B)
    assert bool(torch.isfinite(cost).all()) and bool((cost[1:] <= cost[:-1]).all()), "a basin's recorded cost rose"
    assert torch.equal(cost, 0.5 * (1.0 - score) + 0.5 * (1.0 - score_aux))
    assert bool((cost[-1] < cost[0]).any()), "32 candidates x 3 rounds improved no basin"
    assert tuple(best.shape) == tuple(start.shape) and torch.equal(best[:-1], start[:-1])
    again, hist2 = search(5)
    assert torch.equal(bits(again), bits(best))
    assert all(torch.equal(hist2[k], hist[k]) for k in ("cost", "score", "score_aux", "best_index"))
    by_method, hist_m = search(5, fn=model.population_search)
    assert torch.equal(bits(by_method), bits(best))
    assert all(torch.equal(hist_m[k], hist[k]) for k in ("cost", "score", "score_aux", "best_index"))
    # without an aux term the periods alone are searched on, and only the flow's score is kept
    _, hist_f = search(5, aux_target=None, aux_key=None, aux_periods=None)
    assert set(hist_f) == {"cost", "best_index", "columns", "score"} and torch.equal(hist_f["cost"], 1.0 - hist_f["score"])
    assert bool((hist_f["cost"][1:] <= hist_f["cost"][:-1]).all())
    # with the new arguments at their defaults -- left out, or given as such -- the search is the one there was
    for kw in (dict(), dict(objective="kge"), dict(objective="nse", transform="sqrt")):
        old = adj_population_search(model, x, start, daily, n_candidates=P, n_rounds=2,
                                    generator=torch.Generator().manual_seed(9), **kw)
        new = adj_population_search(model, x, start, daily, n_candidates=P, n_rounds=2,
                                    generator=torch.Generator().manual_seed(9), periods=None, aux_target=None, aux_key=None,
                                    aux_weights=None, aux_periods=None, aux_objective="nse", aux_share=0.5, **kw)
        assert torch.equal(bits(old[0]), bits(new[0])) and set(old[1]) == set(new[1])
        assert all(torch.equal(old[1][k], new[1][k]) for k in old[1] if k != "columns")
