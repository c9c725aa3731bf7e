"""GPU tier: `population_joint_stats` / `population_search(aux_target=...)` (hydrodl2_amd/population.py) on
hbvx_population_joint.

The cases are the six of tests/test_population_gpu.py; the flow targets are the twin targets of
tests/test_population_stats_gpu.py (`twin`).  The aux twin is the module's outputs[aux_key] at the same hidden
candidate times exp(0.2 noise): on the cases in SPARSE it is NaN except every 8th day (an 8-day product), elsewhere it
carries the case's own NaN mask and weights.

  flow term   for every case and transform, sse, s1, s2, s3 and the series equal `population_stats`' bit for bit:
              the two are forms of one kernel template (k_pop, csrc/hbv_pop.h), and this holds the joint form to the
              stats form.
  aux series  aux.series[c] against outputs[aux_key] of a module call at candidate c, the project's flux tolerance
              (tests/abi_util.py: rtol 1e-4, atol 1e-5), every element, no outlier allowance.
  aux sums    each of sse, s1, s2, s3 against the float64 sum over the kernel's OWN float32 aux series, the bounds of
              tests/test_popjoint_host.py: gamma(T+2), gamma(T+1), gamma(T+3), gamma(T+3).
  aux scores  nse, kge, r, alpha, beta against float64 scores of the module route by their definitions, as
              |score - yardstick| / (1 + |1 - yardstick|).  Two float32 forwards feed a float32 chain: the tolerance is
              measured, not derived.  Worst value over PAIRS on the MI355X of profiles/r18_population_joint.md:
              2.52e-6 (srflow_no_rout on the wet 400-day record; 1.9e-6 and 1.5e-6 next, 1e-6 and below on the
              others); asserted: four times that (the margin COST_RTOL and SCORE_TOL take), and held below 1e-4 as
              SCORE_TOL is.

PAIRS is a literal table, not computed at run time, so that a regression cannot empty it silently: 'AET_hydro' on all
six cases, every other key on at least three, the wet 400-day record among them -- but for 'srflow_no_rout', which has
two.  A pair is in it only if the twin aux target has a variance in every basin and the yardstick has a score for
every candidate there, none of which barely varies -- asserted first.  The candidate pairs were run on the CPU path (the oracle library) before the
table was fixed; what is left out and why:
  'SWE'             the 7-day record: the pack is zero in some of its 67 basins.
  'gwflow_no_rout'  the 7-day record: the outflow of the slow reservoir does not move in a week -- the yardstick's alpha
                    (simulated over observed standard deviation; the observed one is the twin's 20 % noise) goes down
                    to 0.014 there.  The variance of such a series is what is left of s2 / W - (s1 / W)^2 after the
                    two terms cancel, and the loss grows with ((mean_s - shift) / sd_s)^2: float64 chains rounded to
                    float32 ONCE already miss its correlation by 3e-4, so no float32 scheme about the observed mean
                    holds 1e-4 there, and the score is not one to rank by.  The entry condition below says so for
                    every pair: alpha of the yardstick above 0.1 for every candidate and basin (the README's "when not
                    to use it" carries the same limit).
  'ssflow_no_rout'  the 7-, 15- and 40-day Hbv records: the upper zone stays below its threshold in some basin, so the
                    observed series is identically zero there.
  'srflow_no_rout'  one threshold higher, the same on more records: the fast runoff is zero throughout in some basin of
                    the 7- and 15-day Hbv records, in every basin of the 40-day one, and for some candidate of the
                    Hbv_2 record (its yardstick then has no correlation).  That leaves the 40-day Hbv_1_1p record and
                    the wet 400-day record: two cases, not three.  SERIES_ONLY adds the 15-day and the Hbv_2 record
                    for this key to the comparisons that need no score -- the series and the sums -- so that the fast
                    runoff is taken from three models' day steps."""
import functools

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd.sensitivity import jacobian_columns
from hydrodl2_amd.population import (_mixed_cost, _objective_cost, _to_input_space, population_joint_stats,
                                     population_score, population_search)

from . import abi_util as au
from . import synth
from .test_population_gpu import CASES, DEV, bits, case, gamma
from .test_population_score_host import textbook
from .test_population_stats_gpu import TRANSFORMS, stats, twin

KEYS = ("AET_hydro", "SWE", "srflow_no_rout", "ssflow_no_rout", "gwflow_no_rout")
SPARSE = ("hbv-m3-b5-t40-cutoff-subset", "hbv11p-m16-b5-t40-muwts", "hbv-wet400-norout")
PAIRS = (
    ("hbv-m1-b67-t7", "AET_hydro"),
    ("hbv-m2-b5-t15-drop-masked", "AET_hydro"),
    ("hbv-m3-b5-t40-cutoff-subset", "AET_hydro"),
    ("hbv11p-m16-b5-t40-muwts", "AET_hydro"),
    ("hbv2-m2-b5-t40", "AET_hydro"),
    ("hbv-wet400-norout", "AET_hydro"),
    ("hbv-m2-b5-t15-drop-masked", "SWE"),
    ("hbv-m3-b5-t40-cutoff-subset", "SWE"),
    ("hbv11p-m16-b5-t40-muwts", "SWE"),
    ("hbv2-m2-b5-t40", "SWE"),
    ("hbv-wet400-norout", "SWE"),
    ("hbv11p-m16-b5-t40-muwts", "srflow_no_rout"),
    ("hbv-wet400-norout", "srflow_no_rout"),
    ("hbv11p-m16-b5-t40-muwts", "ssflow_no_rout"),
    ("hbv2-m2-b5-t40", "ssflow_no_rout"),
    ("hbv-wet400-norout", "ssflow_no_rout"),
    ("hbv-m2-b5-t15-drop-masked", "gwflow_no_rout"),
    ("hbv-m3-b5-t40-cutoff-subset", "gwflow_no_rout"),
    ("hbv11p-m16-b5-t40-muwts", "gwflow_no_rout"),
    ("hbv2-m2-b5-t40", "gwflow_no_rout"),
    ("hbv-wet400-norout", "gwflow_no_rout"),
)
SERIES_ONLY = (
    ("hbv-m2-b5-t15-drop-masked", "srflow_no_rout"),
    ("hbv2-m2-b5-t40", "srflow_no_rout"),
)
METRICS = ("nse", "kge", "r", "alpha", "beta")
MEASURED_AUX_SCORE_DIFF = 2.52e-6
AUX_SCORE_TOL = 4 * MEASURED_AUX_SCORE_DIFF
assert AUX_SCORE_TOL < 1e-4


def test_the_table_of_pairs_is_what_the_issue_asks_for():
    assert all(n in CASES and k in KEYS for n, k in PAIRS) and len(set(PAIRS)) == len(PAIRS)
    assert {n for n, k in PAIRS if k == "AET_hydro"} == set(CASES)
    for key in KEYS[1:]:
        on = {n for n, k in PAIRS if k == key}
        assert "hbv-wet400-norout" in on, f"{key} is compared on {sorted(on)}"
        assert len(on) >= (2 if key == "srflow_no_rout" else 3), f"{key} is compared on {sorted(on)}"    # (the docstring)
    assert len({n for n, k in PAIRS + SERIES_ONLY if k == "srflow_no_rout"}) >= 3
    assert not set(SERIES_ONLY) & set(PAIRS) and all(n in CASES and k in KEYS for n, k in SERIES_ONLY)
    assert len([n for n in SPARSE if n in CASES]) >= 2


@functools.lru_cache(maxsize=None)
def hidden_outputs(name):
    """The five aux series [T_out,B] of the module at the hidden candidate of `twin(name)` (its lines).  Computed once."""
    cs = case(name)
    n_cols = len(cs.cols)
    row = cs.cand[0]
    if cs.two:
        hidden = 0.5 * (row + torch.from_numpy(synth.unit_parameters((cs.B, n_cols), 191)).to(DEV))
    else:
        hidden = row + 0.35 * torch.from_numpy(synth.normalish((cs.B, n_cols), 192)).to(DEV)
    cs.prepare()
    with torch.no_grad():
        out = cs.model(cs.xd, cs.with_row(hidden))
    return {k: out[k][..., 0].clone() for k in KEYS}


@functools.lru_cache(maxsize=None)
def aux_twin(name, key):
    """(aux target [T_out,B] with NaN where nothing is observed, aux weights or None)."""
    cs = case(name)
    noise = torch.from_numpy(synth.normalish((cs.T_out, cs.B), 194 + KEYS.index(key))).to(DEV)
    target = hidden_outputs(name)[key] * torch.exp(0.2 * noise)
    if name in SPARSE:
        seen = (torch.arange(cs.T_out, device=target.device) % 8 == 0).unsqueeze(1).expand_as(target)
        return torch.where(seen, target, torch.full_like(target, float("nan"))).contiguous(), None
    return torch.where(torch.isnan(cs.target), cs.target, target).contiguous(), cs.weights


def aux_weights_of(name, key):
    tgt, w = aux_twin(name, key)
    w = torch.ones_like(tgt) if w is None else w
    return torch.where(torch.isnan(tgt), torch.zeros_like(w), w).double()


@functools.lru_cache(maxsize=None)
def module_route(name):
    """{key: [P,T_out,B] float32} of every candidate by the module's own route, one module call each; computed once."""
    cs = case(name)
    series = {k: [] for k in KEYS}
    for c in range(cs.P):
        cs.prepare()
        with torch.no_grad():
            out = cs.model(cs.xd, cs.with_row(cs.cand[c]))
        for k in KEYS:
            series[k].append(out[k][..., 0].clone())
    return {k: torch.stack(v) for k, v in series.items()}


def joint(name, key, transform="none", cand=None, aux=None, **kw):
    cs = case(name)
    tgt = twin(name)            # (these run the module when first asked for: before prepare(), not after)
    atgt, aw = aux_twin(name, key) if aux is None else aux
    cs.prepare()
    return population_joint_stats(cs.model, cs.xd, cs.p, cs.cand if cand is None else cand, tgt, atgt, key, cs.names,
                                  cs.weights, aw, transform=transform, **kw)


@functools.lru_cache(maxsize=None)
def joint_with_series(name, key):
    return joint(name, key, return_series=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_the_flow_term_is_population_stats(hip_backend, name):
    cs = case(name)
    for transform in TRANSFORMS:
        want = stats(name, transform, return_series=True)
        got = joint(name, "AET_hydro", transform, return_series=True)
        assert set(got) == {"flow", "aux", "columns", "outputs"} and got["columns"] == cs.cols
        flow, aux = got["flow"], got["aux"]
        for key in ("sse", "s1", "s2", "s3"):
            assert tuple(flow[key].shape) == (cs.P, cs.B) and flow[key].dtype == torch.float32
            assert torch.equal(bits(flow[key]), bits(want[key])), f"{transform}: flow {key} is not population_stats'"
            assert tuple(aux[key].shape) == (cs.P, cs.B) and aux[key].dtype == torch.float32
            assert bool(torch.isfinite(aux[key]).all()), f"{transform}: a poisoned or non-finite element in aux {key}"
        assert torch.equal(bits(flow["series"]), bits(want["series"])), f"{transform}: the flow series differs"
        assert torch.equal(bits(flow["shift"]), bits(want["shift"])) and torch.equal(flow["n_obs"], want["n_obs"])
        assert flow["transform"] == transform and aux["transform"] == "none" and aux["eps"] is None
        assert aux["key"] == "AET_hydro" and (flow["eps"] is None) == (transform != "log")
        assert all(torch.equal(flow["obs"][k], want["obs"][k]) for k in ("W", "e1", "e2"))
        assert tuple(aux["series"].shape) == (cs.P, cs.T_out, cs.B) and bool(torch.isfinite(aux["series"]).all())
        # the aux term does not see the flow's transform
        if transform != "none":
            first = joint_with_series(name, "AET_hydro")["aux"]
            assert all(torch.equal(bits(aux[k]), bits(first[k])) for k in ("sse", "s1", "s2", "s3", "series"))


@pytest.mark.gpu
@pytest.mark.parametrize("name,key", PAIRS + SERIES_ONLY)
def test_aux_series_against_the_module(hip_backend, name, key):
    cs = case(name)
    got = joint_with_series(name, key)
    series, want = got["aux"]["series"], module_route(name)[key]
    assert tuple(series.shape) == (cs.P, cs.T_out, cs.B) and bool(torch.isfinite(series).all())
    assert float(want.max()) > 0.1, "the record produces nothing of this series: the comparison would be empty"
    err = (series.double() - want.double()).abs()
    tol = au.FLUX_ATOL + au.FLUX_RTOL * want.double().abs()
    print(f"{name} {key}: aux series worst error / tolerance {float((err / tol).max()):.4f} (max abs {float(err.max()):.3e})")
    assert bool((err <= tol).all()), f"{int((err > tol).sum())} of {err.numel()} elements outside the flux tolerance"
    # candidate 0 is the current row: its series is the primal's own output
    own = got["outputs"][key][..., 0].double()
    assert bool(((series[0].double() - own).abs() <= au.FLUX_ATOL + au.FLUX_RTOL * own.abs()).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name,key", PAIRS + SERIES_ONLY)
def test_aux_sums_against_float64_over_the_kernels_own_series(hip_backend, name, key):
    cs = case(name)
    got = joint_with_series(name, key)["aux"]
    atgt, _ = aux_twin(name, key)
    w8 = aux_weights_of(name, key)
    assert torch.equal(got["n_obs"], (w8 > 0).sum(0))
    o8 = torch.where(torch.isnan(atgt), torch.zeros_like(atgt), atgt).double()
    m8 = got["shift"].double()
    v8 = got["series"].double()
    d, e, r = v8 - m8, o8 - m8, v8 - o8
    T = cs.T_out
    rows = (("sse", w8 * r * r, w8 * r * r, T + 2), ("s1", w8 * d, w8 * d.abs(), T + 1),
            ("s2", w8 * d * d, w8 * d * d, T + 3), ("s3", w8 * d * e, w8 * (d * e).abs(), T + 3))
    for k, terms, mags, n in rows:
        err = (got[k].double() - terms.sum(1)).abs()
        bound = gamma(n) * mags.sum(1)
        need = float((err / torch.where(bound > 0, bound, torch.ones_like(bound))).max())
        print(f"{name} {key}: aux {k} against its own series: worst error / bound {need:.3f}")
        assert bool((err <= bound).all()), f"aux {k} misses the float64 sum of its own series by {need:.2f} x the bound"


@pytest.mark.gpu
@pytest.mark.parametrize("name,key", PAIRS)
def test_aux_scores_against_the_module_route(hip_backend, name, key):
    cs = case(name)
    atgt, _ = aux_twin(name, key)
    w8 = aux_weights_of(name, key)
    # first: the aux observations carry a variance in every basin, and the yardstick has every score
    W = w8.sum(0)
    o = torch.where(torch.isnan(atgt), torch.zeros_like(atgt), atgt).double()
    mean_o = (w8 * o).sum(0) / W
    sd_o = ((w8 * (o - mean_o) ** 2).sum(0) / W).sqrt()
    assert bool((W > 0).all()) and bool((mean_o > 0).all()) and bool((sd_o > 0.05 * mean_o).all()), \
        "a basin's aux observations have no variance to speak of: the comparison would be empty"
    want = textbook(module_route(name)[key].double(), atgt.double(), w8)
    assert bool((want["alpha"] > 0.1).all()), "a candidate's series barely varies: its correlation is not a score to hold"
    got = joint(name, key)["aux"]
    worst = 0.0
    for metric in METRICS:
        assert bool(torch.isfinite(want[metric]).all()), f"{metric}: the yardstick has no score"
        score = population_score(got, metric)
        assert tuple(score.shape) == (cs.P, cs.B) and score.dtype == torch.float64
        assert bool(torch.isfinite(score).all()), f"{metric}: a candidate has no score"
        diff = float(((score - want[metric]).abs() / (1 + (1 - want[metric]).abs())).max())
        worst = max(worst, diff)
        print(f"{name} {key} {metric}: yardstick {float(want[metric].min()):.3f} .. {float(want[metric].max()):.3f}, "
              f"worst difference {diff:.3e} (asserted {AUX_SCORE_TOL:.1e})")
    print(f"{name} {key}: worst aux score difference {worst:.3e}")
    assert worst <= AUX_SCORE_TOL


@pytest.mark.gpu
def test_bit_rules(hip_backend):
    name = "hbv-m2-b5-t15-drop-masked"
    cs = case(name)
    keys = ("sse", "s1", "s2", "s3")
    pick = [0, 3, 8]

    def same(a, b, ia=slice(None), ib=slice(None), with_series=True):
        return all(torch.equal(bits(a[t][k][ia]), bits(b[t][k][ib]))
                   for t in ("flow", "aux") for k in keys + (("series",) if with_series else ()))

    for key, transform in (("AET_hydro", "none"), ("ssflow_no_rout", "log")):
        a = joint(name, key, transform, return_series=True)
        b = joint(name, key, transform, return_series=True)
        assert same(a, b), f"{key} {transform}: two calls differ"
        plain = joint(name, key, transform)
        assert "series" not in plain["flow"] and "series" not in plain["aux"]
        assert same(plain, a, with_series=False), f"{key} {transform}: return_series changes the sums"
        for c in pick:
            alone = joint(name, key, transform, cs.cand[c:c + 1].contiguous(), return_series=True)
            assert same(alone, a, 0, c), f"{key} {transform}: candidate {c} alone has other bits"
        sub = joint(name, key, transform, cs.cand[pick].contiguous(), return_series=True)
        assert same(sub, a, slice(None), pick)
        for k in keys:      # (whole rows: in a single basin two candidates can share an aux series, evaporation at its limit)
            assert len({tuple(row.tolist()) for row in a["aux"][k]}) == cs.P, f"{key}: aux {k} repeats between candidates"

        # a basin whose aux weights are all zero: NaN aux scores there, every flow number keeps its bits, and so do the
        # other basins' aux numbers
        atgt, aw = aux_twin(name, key)
        aw0 = (torch.ones_like(atgt) if aw is None else aw).clone()
        aw0[:, 2] = 0.0
        blind = joint(name, key, transform, aux=(atgt, aw0), return_series=True)
        assert all(torch.equal(bits(blind["flow"][k]), bits(a["flow"][k])) for k in keys + ("series",))
        others = [i for i in range(cs.B) if i != 2]
        assert all(torch.equal(bits(blind["aux"][k][:, others]), bits(a["aux"][k][:, others])) for k in keys)
        assert torch.equal(bits(blind["aux"]["series"]), bits(a["aux"]["series"]))
        assert int(blind["aux"]["n_obs"][2]) == 0
        for metric in METRICS + ("mse", "kge12", "pbias"):
            score = population_score(blind["aux"], metric)
            assert bool(torch.isnan(score[:, 2]).all()), f"{metric} of a basin without aux observations is not NaN"
            assert bool(torch.isfinite(population_score(blind["flow"], "nse")).all())
        assert bool((population_score(blind["aux"], "sse")[:, 2] == 0).all())


@pytest.mark.gpu
def test_population_search_with_the_aux_term(hip_backend):
    """The twin problem of tests/test_population_gpu.py::test_population_search, which also observes the hidden row's
    evapotranspiration every 8th day."""
    T, B, M, P = 40, 5, 2, 32
    model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "dynamic_params": {"Hbv": []}}, DEV)
    x = {"x_phy": torch.from_numpy(synth.forcing(T, B, seed=61)).to(DEV)}
    truth = torch.from_numpy(synth.raw_parameters(T, B, model.learnable_param_count, seed=62)).to(DEV)
    with torch.no_grad():
        out = model(x, truth)
    obs, aet = out["streamflow"][..., 0].clone(), out["AET_hydro"][..., 0].clone()
    aobs = torch.full_like(aet, float("nan"))
    aobs[::8] = aet[::8]
    start = torch.from_numpy(synth.raw_parameters(T, B, model.learnable_param_count, seed=63, scale=1.5)).to(DEV)
    keep = [t.clone() for t in (start, obs, aobs, x["x_phy"])]

    def search(seed, n_rounds=3, **kw):
        g = torch.Generator().manual_seed(seed)
        kw = {"objective": "kge", "aux_target": aobs, "aux_key": "AET_hydro", **kw}
        return population_search(model, x, start, obs, n_candidates=P, n_rounds=n_rounds, generator=g, **kw)

    best, hist = search(5)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((start, obs, aobs, x["x_phy"]), keep)), "an input was modified"
    assert set(hist) == {"cost", "best_index", "columns", "score", "score_aux"}
    cost, score, score_aux = hist["cost"], hist["score"], hist["score_aux"]
    assert tuple(cost.shape) == tuple(score.shape) == tuple(score_aux.shape) == (4, B)
    assert tuple(hist["best_index"].shape) == (3, B) and cost.dtype == torch.float64
    assert bool(torch.isfinite(cost).all()) and bool((cost[1:] <= cost[:-1]).all()), "a basin's recorded cost rose"
    assert torch.equal(cost, 0.5 * (1.0 - score) + 0.5 * (1.0 - score_aux))          # kge and the default nse, equal shares
    assert bool((cost[-1] < cost[0]).any()), "32 candidates x 3 rounds improved no basin"
    assert torch.equal(hist["best_index"] != 0, cost[1:] < cost[:-1])
    assert tuple(best.shape) == tuple(start.shape) and torch.equal(best[:-1], start[:-1])
    again, hist2 = search(5)
    assert torch.equal(bits(again), bits(best)) and all(torch.equal(hist2[k], hist[k]) for k in ("cost", "score", "score_aux", "best_index"))

    # the winner of a round is the argmin of the mixed cost recomputed from a population_joint_stats call on the same
    # candidates: round 0's are the start row and the generator's first draws
    for share, aux_objective in ((0.5, "nse"), (0.3, "kge")):
        one, h1 = search(7, n_rounds=1, aux_share=share, aux_objective=aux_objective)
        _, cols = jacobian_columns(model, None)
        draws = torch.rand((P - 1, B, len(cols)), generator=torch.Generator().manual_seed(7)).to(DEV)
        cands = torch.cat([start[-1][:, cols].unsqueeze(0), _to_input_space(draws, True)]).contiguous()
        st = population_joint_stats(model, x, start, cands, obs, aobs, "AET_hydro")
        mixed = _mixed_cost(_objective_cost(population_score(st["flow"], "kge"), "kge"),
                            _objective_cost(population_score(st["aux"], aux_objective), aux_objective), share)
        low, idx = mixed.min(0)
        idx = torch.where(mixed[0] <= low, torch.zeros_like(idx), idx)
        assert torch.equal(h1["best_index"][0], idx.cpu()) and torch.equal(h1["cost"][1], low.cpu())
        assert torch.equal(h1["cost"][0], mixed[0].cpu())
        assert torch.equal(bits(one[-1][:, cols]), bits(cands.gather(0, idx.view(1, B, 1).expand(1, B, len(cols)))[0]))

    # aux_share = 0 picks the flow-only search's winners
    flow_only, hf = search(5, aux_target=None, aux_key=None)
    zero, hz = search(5, aux_share=0.0)
    assert set(hf) == {"cost", "best_index", "columns", "score"}
    assert torch.equal(hz["best_index"], hf["best_index"]) and torch.equal(bits(zero), bits(flow_only))
    assert torch.equal(hz["cost"], hf["cost"]) and torch.equal(hz["score"], hf["score"])
    assert not torch.equal(hist["best_index"], hf["best_index"])                     # the aux term moves the search

    # a basin without aux observations admits no mixed score: +inf throughout, and its row stays
    blind = aobs.clone()
    blind[:, 2] = float("nan")
    kept, hb = search(5, aux_target=blind)
    assert bool(torch.isinf(hb["cost"][:, 2]).all()) and bool(torch.isnan(hb["score_aux"][:, 2]).all())
    assert bool(torch.isfinite(hb["score"][:, 2]).all()) and bool((hb["best_index"][:, 2] == 0).all())
    assert torch.equal(bits(kept[-1, 2]), bits(start[-1, 2]))
