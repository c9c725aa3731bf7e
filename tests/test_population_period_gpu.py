"""GPU tier: `population_period_stats` / `population_search(periods=...)` (hydrodl2_amd/population.py) on
hbvx_population_period.

The cases are the six of tests/test_population_gpu.py, each with the calendar of CALENDARS: blocks of 3 on the 7-day
record (two periods, one day dropped) and on the 15-day record (five, nothing dropped), blocks of 8 on the three 40-day
records, thirteen months on the wet 400-day record (four days dropped); MIXED is one 40-day record more with the flow in
blocks of 8 and the aux series in blocks of 5 in the same launch.

  daily calendars  for every case and transform, with key AET_hydro, all eight sums and both series equal
                   `population_joint_stats`' bit for bit: the two are forms of one kernel template (k_pop, csrc/
                   hbv_pop.h), and this holds the period form to the joint form.  With the flow daily and the aux series in periods the flow numbers are
                   `population_stats`'; without an aux term they are those of the call with one.
  period series    against float64 period means of the module route's daily series, the project's flux tolerance
                   (tests/abi_util.py) on every element -- a mean of values that are each inside it is inside it, and the
                   rounding of the mean, gamma(31), is far below it; and against float64 means of the kernel's OWN daily
                   series (`population_joint_stats(return_series=True)`) within gamma(n) mean|y|, n the period's days.
  sums             against float64 sums over the kernel's own period series: the bounds of
                   tests/test_population_stats_gpu.py and tests/test_population_joint_gpu.py with K for T_out.
  scores           nse, kge, r, alpha, beta ('log': nse, r, alpha) against float64 scores of the module route on period
                   means, as |score - yardstick| / (1 + |1 - yardstick|).  Twin targets: period means of the hidden
                   row's series times exp(0.2 noise), seed 300 for the flow and 301 + KEYS.index(key) for the aux key,
                   every period observed with weight one.  Two float32 forwards feed a float32 chain: the tolerance is
                   measured, not derived.  Worst value over FLOW_PAIRS and AUX_PAIRS on the MI355X of
                   profiles/r19_population_period.md: 1.07e-6 (the flow of the 15-day record in five periods; 8.7e-7 its
                   AET_hydro, 6.2e-7 srflow_no_rout on the wet 400-day record, 5e-7 and below on the others);
                   asserted: four times that (the margin COST_RTOL, SCORE_TOL and AUX_SCORE_TOL take), and held below
                   1e-4.

FLOW_PAIRS and AUX_PAIRS are literal tables.  Left out, and why: the 7-day record has two periods, so no variance; the
Hbv_2 flow has candidates whose period means barely vary (yardstick alpha down to 0.03 under 'log'); Hbv_2
'gwflow_no_rout' (alpha 0.08) and 'srflow_no_rout' (a candidate without a correlation); the fast and upper-zone runoff on
the three Hbv short records, identically zero in some basin.  The entry conditions are asserted first: the observed
standard deviation above 0.05 of the mean in every basin, every yardstick score finite, yardstick alpha above 0.1."""
import functools

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd.population import (_calendar, _mixed_cost, _objective_cost, _observations, _to_input_space,
                                     population_period_stats, population_score, population_search)
from hydrodl2_amd.sensitivity import jacobian_columns

from . import abi_util as au
from . import synth
from .test_population_gpu import CASES, DEV, U, bits, case, gamma
from .test_population_joint_gpu import KEYS, aux_twin, hidden_outputs, joint, joint_with_series, module_route
from .test_population_period_host import period_means64
from .test_population_score_host import textbook
from .test_population_stats_gpu import K_BOUND, SCORED, TRANSFORMS, device_transform, g64, stats, twin

MONTHS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31, 31)
MONTH_ENDS = tuple(sum(MONTHS[:k + 1]) - 1 for k in range(13))
CALENDARS = {
    "hbv-m1-b67-t7": (3, 3),
    "hbv-m2-b5-t15-drop-masked": (3, 3),
    "hbv-m3-b5-t40-cutoff-subset": (8, 8),
    "hbv11p-m16-b5-t40-muwts": (8, 8),
    "hbv2-m2-b5-t40": (8, 8),
    "hbv-wet400-norout": (MONTH_ENDS, MONTH_ENDS),
}
MIXED = ("hbv11p-m16-b5-t40-muwts", (8, 5))
N_PERIODS = {"hbv-m1-b67-t7": 2, "hbv-m2-b5-t15-drop-masked": 5, "hbv-m3-b5-t40-cutoff-subset": 5,
             "hbv11p-m16-b5-t40-muwts": 5, "hbv2-m2-b5-t40": 5, "hbv-wet400-norout": 13}
FLOW_PAIRS = ("hbv-m2-b5-t15-drop-masked", "hbv-m3-b5-t40-cutoff-subset", "hbv11p-m16-b5-t40-muwts", "hbv-wet400-norout")
AUX_PAIRS = tuple((n, k) for n in FLOW_PAIRS for k in ("AET_hydro", "SWE", "gwflow_no_rout")) \
    + tuple((n, k) for n in FLOW_PAIRS[2:] for k in ("srflow_no_rout", "ssflow_no_rout")) \
    + tuple(("hbv2-m2-b5-t40", k) for k in ("AET_hydro", "SWE", "ssflow_no_rout"))
METRICS = ("nse", "kge", "r", "alpha", "beta")
SUMS = ("sse", "s1", "s2", "s3")
MEASURED_PERIOD_SCORE_DIFF = 1.07e-6
PERIOD_SCORE_TOL = 4 * MEASURED_PERIOD_SCORE_DIFF
assert PERIOD_SCORE_TOL < 1e-4


def test_the_tables_are_what_the_issue_asks_for():
    assert set(CALENDARS) == set(CASES) and MIXED[0] in CASES and len(AUX_PAIRS) == 19 == len(set(AUX_PAIRS))
    assert MONTH_ENDS[-1] == 395 and len(MONTH_ENDS) == 13
    assert all(n in CASES and k in KEYS for n, k in AUX_PAIRS) and all(n in CASES for n in FLOW_PAIRS)


def ends_of(name, which=0, cals=None):
    cs = case(name)
    cal = (cals or CALENDARS[name])[which]
    return _calendar(list(cal) if isinstance(cal, tuple) else cal, cs.T_out, "periods", "test").tolist()


def as_arg(cal):
    return list(cal) if isinstance(cal, tuple) else cal


@functools.lru_cache(maxsize=None)
def hidden_flow(name):
    """The streamflow [T_out,B] of the module at the hidden candidate of `twin(name)` (its lines).  Computed once."""
    cs = case(name)
    n_cols = len(cs.cols)
    row = cs.cand[0]
    if cs.two:
        hidden = 0.5 * (row + torch.from_numpy(synth.unit_parameters((cs.B, n_cols), 191)).to(DEV))
    else:
        hidden = row + 0.35 * torch.from_numpy(synth.normalish((cs.B, n_cols), 192)).to(DEV)
    cs.prepare()
    with torch.no_grad():
        return cs.model(cs.xd, cs.with_row(hidden))["streamflow"][..., 0].clone()


@functools.lru_cache(maxsize=None)
def period_twin(name, key, cals=None, masked=False):
    """(target [KF,B], weights or None, aux target [KA,B], aux weights or None): period means of the hidden row's series
    times exp(0.2 noise).  masked, on the cases that carry a mask: a period is missing where the case's own target is NaN
    on its closing day, and weighs what that day weighs."""
    cs = case(name)
    out = []
    for which, (series, seed) in enumerate(((hidden_flow(name), 300), (hidden_outputs(name)[key], 301 + KEYS.index(key)))):
        ends = ends_of(name, which, cals)
        noise = torch.from_numpy(synth.normalish((len(ends), cs.B), seed)).to(DEV)
        tgt = (period_means64(series, ends) * torch.exp(0.2 * noise.double())).float()
        w = None
        if masked and cs.weights is not None:
            tgt = torch.where(torch.isnan(cs.target[ends]), cs.target[ends], tgt)
            w = cs.weights[ends].contiguous()
        out += [tgt.contiguous(), w]
    return tuple(out)


def period(name, key="AET_hydro", transform="none", cals=None, cand=None, obs=None, masked=True, xd=None, **kw):
    cs = case(name)
    cals = cals or CALENDARS[name]
    tgt, w, atgt, aw = obs if obs is not None else period_twin(name, key or "AET_hydro", cals, masked)
    cs.prepare()
    if key is None:
        return population_period_stats(cs.model, xd or cs.xd, cs.p, cs.cand if cand is None else cand, tgt, as_arg(cals[0]),
                                       names=cs.names, weights=w, transform=transform, **kw)
    return population_period_stats(cs.model, xd or cs.xd, cs.p, cs.cand if cand is None else cand, tgt, as_arg(cals[0]),
                                   atgt, key, as_arg(cals[1]), cs.names, w, aw, transform, **kw)


@functools.lru_cache(maxsize=None)
def period_with_series(name, key, cals=None):
    return period(name, key, cals=cals, return_series=True)


def w8_of(tgt, w):
    w = torch.ones_like(tgt) if w is None else w
    return torch.where(torch.isnan(tgt), torch.zeros_like(w), w).double()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_daily_calendars_are_population_joint_stats(hip_backend, name):
    cs = case(name)
    tgt = twin(name)
    atgt, aw = aux_twin(name, "AET_hydro")
    for transform in TRANSFORMS:
        want = joint(name, "AET_hydro", transform, return_series=True)
        cs.prepare()
        got = population_period_stats(cs.model, cs.xd, cs.p, cs.cand, tgt, None, atgt, "AET_hydro", None, cs.names,
                                      cs.weights, aw, transform, return_series=True)
        assert set(got) == {"flow", "aux", "columns", "outputs"} and got["columns"] == cs.cols
        for term in ("flow", "aux"):
            for k in SUMS + ("series",):
                assert got[term][k].dtype == torch.float32
                assert torch.equal(bits(got[term][k]), bits(want[term][k])), f"{transform}: {term} {k} is not the joint call's"
            assert torch.equal(bits(got[term]["shift"]), bits(want[term]["shift"]))
            assert torch.equal(got[term]["n_obs"], want[term]["n_obs"])
            assert all(torch.equal(got[term]["obs"][k], want[term]["obs"][k]) for k in ("W", "e1", "e2"))
            assert got[term]["period_ends"].tolist() == list(range(cs.T_out))
            assert got[term]["period_days"].tolist() == [1] * cs.T_out and got[term]["period_days"].dtype == torch.int64
        assert got["flow"]["transform"] == transform and got["aux"]["transform"] == "none" and got["aux"]["key"] == "AET_hydro"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_mixed_calendars_keep_the_flow_bits(hip_backend, name):
    cs = case(name)
    tgt = twin(name)
    acal = CALENDARS[name][1]
    _, _, atgt, aw = period_twin(name, "AET_hydro", None, True)
    for transform in TRANSFORMS:
        # flow daily, aux in periods: the flow numbers are population_stats'
        want = stats(name, transform, return_series=True)
        got = period(name, "AET_hydro", transform, cals=(None, acal), obs=(tgt, cs.weights, atgt, aw), return_series=True)
        for k in SUMS + ("series",):
            assert torch.equal(bits(got["flow"][k]), bits(want[k])), f"{transform}: flow {k} is not population_stats'"
        assert tuple(got["aux"]["series"].shape) == (cs.P, N_PERIODS[name], cs.B)
        # both in periods, with and without an aux term: the same flow bits, and nothing aux in the result
        both = period(name, "AET_hydro", transform, return_series=True)
        alone = period(name, None, transform, return_series=True)
        assert set(alone) == {"flow", "columns", "outputs"}
        for k in SUMS + ("series",):
            assert bool(torch.isfinite(both["flow"][k]).all()) and bool(torch.isfinite(both["aux"][k]).all()), \
                f"{transform}: a poisoned or non-finite element in {k}"
            assert torch.equal(bits(alone["flow"][k]), bits(both["flow"][k])), f"{transform}: flow {k} depends on the aux term"
        assert tuple(both["flow"]["series"].shape) == (cs.P, N_PERIODS[name], cs.B)
        assert both["flow"]["period_ends"].tolist() == ends_of(name)


def check_series(name, got, daily_module, daily_own, ends, what):
    days = got["period_days"].tolist()
    assert got["period_ends"].tolist() == ends and len(days) == len(ends) and sum(days) == ends[-1] + 1
    series = got["series"]
    assert tuple(series.shape) == (daily_own.shape[0], len(ends), daily_own.shape[2]) and bool(torch.isfinite(series).all())
    want = period_means64(daily_module, ends)
    err = (series.double() - want).abs()
    tol = au.FLUX_ATOL + au.FLUX_RTOL * want.abs()
    print(f"{name} {what}: period series worst error / tolerance {float((err / tol).max()):.4f}")
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} of {err.numel()} elements outside the flux tolerance"
    own = period_means64(daily_own, ends)
    mag = period_means64(daily_own.abs(), ends)
    g = torch.tensor([gamma(n) for n in days], dtype=torch.float64, device=own.device).view(1, -1, 1)
    err = (series.double() - own).abs()
    need = float((err / torch.where(mag > 0, g * mag, torch.ones_like(mag))).max())
    print(f"{name} {what}: period means against the kernel's own daily series: worst error / bound {need:.3f}")
    assert bool((err <= g * mag).all()), f"{what}: a period mean misses the float64 mean of its days by {need:.2f} x the bound"


SERIES_RUNS = [(n, k, None) for n in CASES for k in ("AET_hydro", "SWE")] + [(MIXED[0], "AET_hydro", MIXED[1]),
                                                                             (MIXED[0], "gwflow_no_rout", MIXED[1])]


@pytest.mark.gpu
@pytest.mark.parametrize("name,key,cals", SERIES_RUNS)
def test_period_series(hip_backend, name, key, cals):
    cs = case(name)
    got = period_with_series(name, key, cals)
    daily = joint_with_series(name, key)
    assert float(cs.yardstick[0].max()) > 0.1
    check_series(name, got["flow"], cs.yardstick[0], daily["flow"]["series"], ends_of(name, 0, cals), "flow")
    check_series(name, got["aux"], module_route(name)[key], daily["aux"]["series"], ends_of(name, 1, cals), key)


@pytest.mark.gpu
@pytest.mark.parametrize("name,cals", [(n, None) for n in CASES] + [MIXED])
def test_the_sums_against_float64_over_the_kernels_own_period_series(hip_backend, name, cals):
    cs = case(name)
    tgt, w, atgt, aw = period_twin(name, "AET_hydro", cals, True)
    for transform in TRANSFORMS:
        got = period(name, "AET_hydro", transform, cals=cals, return_series=True)
        for term, o, wts, tr in (("flow", tgt, w, transform), ("aux", atgt, aw, "none")):
            sub = got[term]
            K = int(o.shape[0])
            ob = _observations(cs.req, cs.xd, o, wts, tr, None, "test", rows=K)
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
            rows = (("sse", w8 * r * r, w8 * r * r, w8 * 2 * r.abs() * delta, K + 2), ("s1", w8 * d, w8 * d.abs(), w8 * delta, K + 1),
                    ("s2", w8 * d * d, w8 * d * d, w8 * 2 * d.abs() * delta, K + 3),
                    ("s3", w8 * d * e, w8 * (d * e).abs(), w8 * e.abs() * delta, K + 3))
            for key, terms, mags, spread, n in rows:
                err = (sub[key].double() - terms.sum(1)).abs()
                bound = gamma(n) * mags.sum(1) + spread.sum(1)
                need = float((err / torch.where(bound > 0, bound, torch.ones_like(bound))).max())
                print(f"{name} {transform}: {term} {key} against its own period series: worst error / bound {need:.3f}")
                assert bool((err <= bound).all()), f"{transform}: {term} {key} misses its float64 sum by {need:.2f} x the bound"


def entry_conditions(o, what):
    mean_o, sd_o = o.mean(0), o.std(0, unbiased=False)
    assert bool((mean_o > 0).all()) and bool((sd_o > 0.05 * mean_o).all()), \
        f"{what}: a basin's period observations have no variance to speak of: the comparison would be empty"


def compare_scores(got, want, metrics, what):
    assert bool((want["alpha"] > 0.1).all()), f"{what}: a candidate's period means barely vary (yardstick alpha " \
        f"{float(want['alpha'].min()):.3f}): its correlation is not a score to hold"
    worst = 0.0
    for metric in metrics:
        assert bool(torch.isfinite(want[metric]).all()), f"{what} {metric}: the yardstick has no score"
        score = population_score(got, metric)
        assert score.dtype == torch.float64 and bool(torch.isfinite(score).all()), f"{what} {metric}: a candidate has no score"
        diff = float(((score - want[metric]).abs() / (1 + (1 - want[metric]).abs())).max())
        worst = max(worst, diff)
        print(f"{what} {metric}: yardstick {float(want[metric].min()):.3f} .. {float(want[metric].max()):.3f}, "
              f"worst difference {diff:.3e} (asserted {PERIOD_SCORE_TOL:.1e})")
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", FLOW_PAIRS)
def test_flow_scores_against_the_module_route_on_period_means(hip_backend, name):
    cs = case(name)
    tgt, w, _, _ = period_twin(name, "AET_hydro", None, False)
    assert w is None and not bool(torch.isnan(tgt).any())
    ends = ends_of(name)
    entry_conditions(tgt.double(), name)
    means = period_means64(cs.yardstick[0], ends)
    ones = torch.ones_like(tgt).double()
    worst = 0.0
    for transform in TRANSFORMS:
        got = period(name, "AET_hydro", transform, masked=False)["flow"]
        assert got["n_obs"].tolist() == [len(ends)] * cs.B
        eps = got["eps"]
        want = textbook(g64(means, transform, eps), g64(tgt, transform, eps), ones)
        worst = max(worst, compare_scores(got, want, SCORED[transform], f"{name} {transform}"))
    print(f"{name}: worst flow score difference {worst:.3e}")
    assert worst <= PERIOD_SCORE_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name,key", AUX_PAIRS)
def test_aux_scores_against_the_module_route_on_period_means(hip_backend, name, key):
    _, _, atgt, aw = period_twin(name, key, None, False)
    assert aw is None and not bool(torch.isnan(atgt).any())
    entry_conditions(atgt.double(), f"{name} {key}")
    want = textbook(period_means64(module_route(name)[key], ends_of(name, 1)), atgt.double(), torch.ones_like(atgt).double())
    got = period(name, key, masked=False)["aux"]
    worst = compare_scores(got, want, METRICS, f"{name} {key}")
    print(f"{name} {key}: worst aux score difference {worst:.3e}")
    assert worst <= PERIOD_SCORE_TOL


@pytest.mark.gpu
def test_bit_rules(hip_backend):
    name = "hbv-m2-b5-t15-drop-masked"
    cs = case(name)
    pick = [0, 3, 8]

    def same(a, b, ia=slice(None), ib=slice(None), with_series=True):
        return all(torch.equal(bits(a[t][k][ia]), bits(b[t][k][ib]))
                   for t in ("flow", "aux") for k in SUMS + (("series",) if with_series else ()))

    for key, transform in (("AET_hydro", "none"), ("ssflow_no_rout", "log")):
        a = period(name, key, transform, return_series=True)
        b = period(name, key, transform, return_series=True)
        assert same(a, b), f"{key} {transform}: two calls differ"
        plain = period(name, key, transform)
        assert "series" not in plain["flow"] and "series" not in plain["aux"]
        assert same(plain, a, with_series=False), f"{key} {transform}: return_series changes the sums"
        for c in pick:
            alone = period(name, key, transform, cand=cs.cand[c:c + 1].contiguous(), return_series=True)
            assert same(alone, a, 0, c), f"{key} {transform}: candidate {c} alone has other bits"
        sub = period(name, key, transform, cand=cs.cand[pick].contiguous(), return_series=True)
        assert same(sub, a, slice(None), pick)

        # a basin whose aux period targets are all NaN: NaN aux scores and n_obs 0 there, every flow number keeps its bits,
        # and so do the other basins' aux numbers
        tgt, w, atgt, aw = period_twin(name, key, None, True)
        blind_t = atgt.clone()
        blind_t[:, 2] = float("nan")
        blind = period(name, key, transform, obs=(tgt, w, blind_t, aw), return_series=True)
        assert all(torch.equal(bits(blind["flow"][k]), bits(a["flow"][k])) for k in SUMS + ("series",))
        others = [i for i in range(cs.B) if i != 2]
        assert all(torch.equal(bits(blind["aux"][k][:, others]), bits(a["aux"][k][:, others])) for k in SUMS)
        assert torch.equal(bits(blind["aux"]["series"]), bits(a["aux"]["series"]))
        assert int(blind["aux"]["n_obs"][2]) == 0
        for metric in METRICS + ("mse", "kge12", "pbias"):
            assert bool(torch.isnan(population_score(blind["aux"], metric)[:, 2]).all()), \
                f"{metric} of a basin without aux observations is not NaN"
        assert bool((population_score(blind["aux"], "sse")[:, 2] == 0).all())


@pytest.mark.gpu
def test_days_after_the_last_closing_day_change_nothing(hip_backend):
    """The 7-day record in blocks of 3: the last day is simulated and scored nowhere."""
    name = "hbv-m1-b67-t7"
    cs = case(name)
    a = period(name, "SWE", "sqrt", return_series=True)
    x2 = cs.xd["x_phy"].clone()
    x2[-1, :, 0] += 25.0                            # a wet, warm last day
    x2[-1, :, 1] += 5.0
    b = period(name, "SWE", "sqrt", xd=dict(cs.xd, x_phy=x2), return_series=True)
    assert all(torch.equal(bits(a[t][k]), bits(b[t][k])) for t in ("flow", "aux") for k in SUMS + ("series",))
    x3 = cs.xd["x_phy"].clone()
    x3[-2, :, 0] += 25.0                            # ... and the day before it is the last one scored
    c = period(name, "SWE", "sqrt", xd=dict(cs.xd, x_phy=x3), return_series=True)
    assert not torch.equal(bits(a["flow"]["series"]), bits(c["flow"]["series"]))


@pytest.mark.gpu
def test_population_search_with_calendars(hip_backend):
    """The 40-day twin problem of tests/test_population_joint_gpu.py, observed as 8-day means of the hidden row's
    streamflow and evapotranspiration."""
    T, B, M, P = 40, 5, 2, 32
    model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "dynamic_params": {"Hbv": []}}, DEV)
    x = {"x_phy": torch.from_numpy(synth.forcing(T, B, seed=61)).to(DEV)}
    truth = torch.from_numpy(synth.raw_parameters(T, B, model.learnable_param_count, seed=62)).to(DEV)
    with torch.no_grad():
        out = model(x, truth)
    ends = list(range(7, T, 8))
    obs = period_means64(out["streamflow"][..., 0], ends).float().contiguous()
    aobs = period_means64(out["AET_hydro"][..., 0], ends).float().contiguous()
    start = torch.from_numpy(synth.raw_parameters(T, B, model.learnable_param_count, seed=63, scale=1.5)).to(DEV)
    keep = [t.clone() for t in (start, obs, aobs, x["x_phy"])]

    def search(seed, n_rounds=3, **kw):
        g = torch.Generator().manual_seed(seed)
        kw = {"objective": "kge", "aux_target": aobs, "aux_key": "AET_hydro", "periods": 8, "aux_periods": 8, **kw}
        return population_search(model, x, start, obs, n_candidates=P, n_rounds=n_rounds, generator=g, **kw)

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

    # round 0's winner is the argmin of the mixed cost recomputed from one population_period_stats call
    _, cols = jacobian_columns(model, None)
    for kw in (dict(), dict(aux_target=None, aux_key=None, aux_periods=None)):
        one, h1 = search(7, n_rounds=1, **kw)
        draws = torch.rand((P - 1, B, len(cols)), generator=torch.Generator().manual_seed(7)).to(DEV)
        cands = torch.cat([start[-1][:, cols].unsqueeze(0), _to_input_space(draws, True)]).contiguous()
        if kw:
            st = population_period_stats(model, x, start, cands, obs, 8)
            mixed = _objective_cost(population_score(st["flow"], "kge"), "kge")
        else:
            st = population_period_stats(model, x, start, cands, obs, 8, aobs, "AET_hydro", ends)
            mixed = _mixed_cost(_objective_cost(population_score(st["flow"], "kge"), "kge"),
                                _objective_cost(population_score(st["aux"], "nse"), "nse"), 0.5)
        low, idx = mixed.min(0)
        idx = torch.where(mixed[0] <= low, torch.zeros_like(idx), idx)
        assert torch.equal(h1["best_index"][0], idx.cpu()) and torch.equal(h1["cost"][1], low.cpu())
        assert torch.equal(h1["cost"][0], mixed[0].cpu())
        assert torch.equal(bits(one[-1][:, cols]), bits(cands.gather(0, idx.view(1, B, 1).expand(1, B, len(cols)))[0]))

    # without the two arguments the search is the one there was: daily observations, the same history and result whether
    # the arguments are left out or given as None
    daily, adaily = out["streamflow"][..., 0].clone(), out["AET_hydro"][..., 0].clone()
    old = dict(periods=None, aux_periods=None)
    r1, h1 = population_search(model, x, start, daily, n_candidates=P, n_rounds=2, generator=torch.Generator().manual_seed(9),
                               objective="kge", aux_target=adaily, aux_key="AET_hydro")
    r2, h2 = population_search(model, x, start, daily, n_candidates=P, n_rounds=2, generator=torch.Generator().manual_seed(9),
                               objective="kge", aux_target=adaily, aux_key="AET_hydro", **old)
    assert torch.equal(bits(r1), bits(r2)) and all(torch.equal(h1[k], h2[k]) for k in ("cost", "score", "score_aux", "best_index"))
    # ... and daily calendars given as such pick the same winners from the same bits
    r3, h3 = population_search(model, x, start, daily, n_candidates=P, n_rounds=2, generator=torch.Generator().manual_seed(9),
                               objective="kge", aux_target=adaily, aux_key="AET_hydro", periods=1, aux_periods=1)
    assert torch.equal(bits(r1), bits(r3)) and all(torch.equal(h1[k], h3[k]) for k in ("cost", "score", "score_aux", "best_index"))
