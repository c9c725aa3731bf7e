"""GPU tier: `adj_population_cost` / `adj_population_stats` / `adj_population_search` (hydrodl2_amd/adj_population.py) on
hbvx_adj_population_cost / hbvx_adj_population_stats.

The yardstick is the module itself, which tests/test_adj_f64_gpu.py holds to float64: for each candidate the candidate
is written into the static row, the module is called under no_grad and outputs['flow_sim'] is taken -- the forward
kernels of the implicit scheme (the staged pipeline, the tiled stepper), hbvx_route_forward and the float64
`calibrate._series_cost`.  Problems are those of tests/adj_sets.py; a problem's wet start reaches both routes the
same way (`Case.__init__` binds it to the module's eager forward).

  series   every element within adj_sets.VALUE_TOL of the module's flow_sim (rtol 2e-4, atol 2e-5 of the largest
           value), no outlier allowance.  The kernel calls the day functions the module's forward calls, on the same
           parameter bits, so bit equality is likely: whether it held is printed, not asserted.
  cost     (a) against the float64 sum over the kernel's OWN float32 series: within gamma(T_out + 2) sum w r^2, the
           bound of tests/test_pop_host.py.
           (b) against the module-route float64 cost of the same candidate: the tolerance is measured, not derived.
           (The series came out equal bit for bit in every case, so what was measured is the float32 chain against
           the float64 sum.)  Worst relative difference over the cases below on the MI355X of
           profiles/r17_adj_population.md: 8.21e-7 (the 400-day record under the joint iteration; 1.2e-7 .. 6.3e-7 on
           the others); asserted: four times that, COST_RTOL, and held below 1e-3, the level at which ranking
           candidates a percent apart is safe.
  scores   `population_score` of `adj_population_stats` against float64 scores of the module-route series, in the
           measure |difference| / (1 + |1 - score|); the limit is measured the same way: worst 1.08e-6 (r on the raw
           flow of the 400-day record; 3.0e-7 .. 6.0e-7 on the others), asserted at four times that, SCORE_TOL.  Under
           'log' beta and kge are left out, as in
           tests/test_population_stats_gpu.py (the mean of log(Q + eps) has no scale); records shorter than 20 days
           have no variance to score and take part in the bit rules only."""
import functools

import numpy as np
import pytest
import torch

from hydrodl2_amd import ops
from hydrodl2_amd.adj_population import adj_population_cost, adj_population_search, adj_population_stats
from hydrodl2_amd.calibrate import _check_request, _series_cost
from hydrodl2_amd.population import population_score
from hydrodl2_amd.sensitivity import jacobian_columns

from . import adj_sets
from . import synth
from .test_population_gpu import DEV, bits, gamma
from .test_population_score_host import textbook

MEASURED_COST_RDIFF = 8.21e-7
COST_RTOL = 4 * MEASURED_COST_RDIFF
assert COST_RTOL < 1e-3
MEASURED_SCORE_DIFF = 1.08e-6
SCORE_TOL = 4 * MEASURED_SCORE_DIFF
assert SCORE_TOL < 1e-4
TRANSFORMS = ("none", "sqrt", "log")
SCORED = {"none": ("nse", "kge", "kge12", "r", "alpha", "beta"), "sqrt": ("nse", "kge", "kge12", "r", "alpha", "beta"),
          "log": ("nse", "r", "alpha")}

# name -> the problem of tests/adj_sets.py (or `own`: one built here the same way) and what the case is there for
CASES = {
    # L = T < 15, padded members (M 3), the few fetch with no dynamic parameter
    "wet1": dict(prob="wet1"),
    "wet9": dict(prob="wet9"),
    # one full wave plus a partly filled one, routing on, the reference's zero start
    # (from empty storages some basins have no flow at all in 20 days: no observed mean to score against, and the
    # default eps -- a hundredth of it -- is refused, so eps is given)
    "m1-b67-t20-zero": dict(own=dict(T=20, B=67, M=1, dyn=(), pscale=4.0), scored=False, eps=0.1),
    # nd = ADJ_FEW, the BETAET instance, four basins per wave; staged under the reference and the tight policy
    "wet65-three": dict(prob="wet65-three"),
    "wet65-three-tight": dict(prob="wet65-three", tight=True),
    # the generic fetch, per-lane drop masks, NaN targets and weights with exact zeros; the bit rules run here
    "wet64-list-masked": dict(prob="wet64-list", P=17, masked=True),
    # the start state comes out of the warm-up pass; storm branches
    "storm90-warmup-wet": dict(prob="storm90-warmup-wet"),
    # the un-routed path and a column subset
    "wet120-norout-subset": dict(prob="wet120", routing=False, names=["parFC", "parK1"]),
    "wet120-norout-subset-tight": dict(prob="wet120", routing=False, names=["parFC", "parK1"], tight=True),
    # the joint iteration (adj_newton) over a 400-day chain
    "wet400-joint": dict(prob="wet400", solver="joint"),
}
BIT_CASE = "wet64-list-masked"


def own_problem(k):
    """A problem built as adj_sets.inputs builds its own (zero start: the module's)."""
    T, B, M = k["T"], k["B"], k["M"]
    x = synth.forcing(T, B, adj_sets.SEED, day0=60.0)
    x[..., 0] *= np.float32(k.get("pscale", 1.0))
    p = synth.raw_parameters(T, B, 12 * M + 2, adj_sets.SEED, 2.0)
    cfg = dict(nmul=M, warm_up=0, dy_drop=0.0, dynamic_params={"HbvAdj": list(k["dyn"])})
    return dict(T=T, B=B, M=M, x=torch.from_numpy(x), p=torch.from_numpy(p), state=None, cfg=cfg)


class Case:
    """One problem: the model, its inputs, the candidates (candidate 0 is the current row), target and weights."""

    def __init__(self, name, device=DEV):
        c = CASES[name]
        self.name, self.names, self.P = name, c.get("names"), c.get("P", 3)
        prob = adj_sets.inputs(c["prob"]) if "prob" in c else own_problem(c["own"])
        extra = {"routing": False} if c.get("routing") is False else {}
        self.model = adj_sets.model(device, prob, c.get("solver", "staged"), c.get("tight", False), **extra)
        self.B, self.M = prob["B"], prob["M"]
        self.T_out = prob["T"] - prob["cfg"]["warm_up"]
        self.scored, self.eps = c.get("scored", self.T_out >= 20), c.get("eps")
        if prob["state"] is not None:
            # the wet start, for every run of the module: the population call's one run and the yardstick's
            eager, st = type(self.model)._forward_eager, prob["state"].to(device)
            self.model._forward_eager = lambda xd, pp: eager(self.model, xd, pp, state=st)
        self.xd = {"x_phy": prob["x"].to(device)}
        self.p = prob["p"].to(device)
        _, self.cols = jacobian_columns(self.model, self.names)
        n_cols = len(self.cols)
        row = self.p[-1][:, self.cols]
        draws = row.unsqueeze(0) + 0.7 * torch.from_numpy(synth.normalish((self.P, self.B, n_cols), 92)).to(device)
        draws[0] = row
        self.cand = draws.contiguous()
        self.target = torch.from_numpy(synth.uniform((self.T_out, self.B), 93) * 6.0).to(device)
        self.weights = None
        self.masked = bool(c.get("masked"))
        if self.masked:
            self.miss = torch.from_numpy(synth.uniform((self.T_out, self.B), 94) < 0.2).to(device)
            self.target = torch.where(self.miss, torch.full_like(self.target, float("nan")), self.target)
            wts = torch.from_numpy(synth.uniform((self.T_out, self.B), 95) + 0.25).to(device)
            self.weights = torch.where(torch.from_numpy(synth.uniform((self.T_out, self.B), 96) < 0.2).to(device),
                                       torch.zeros_like(wts), wts)
        self.req = _check_request(self.model, self.xd, self.p, self.target, self.names, None, self.weights, 1)

    def prepare(self):
        """What every run of the module starts from: the same dy_drop draws."""
        torch.manual_seed(4321)

    def with_row(self, values):
        t = self.p.clone()
        t[-1][:, self.cols] = values
        return t

    def cost(self, cand=None, **kw):
        self.prepare()
        return adj_population_cost(self.model, self.xd, self.p, self.cand if cand is None else cand, self.target,
                                   self.names, self.weights, **kw)

    def stats(self, transform, cand=None, **kw):
        tgt = self.twin             # (runs the module when it is first asked for: before prepare(), not after)
        self.prepare()
        return adj_population_stats(self.model, self.xd, self.p, self.cand if cand is None else cand, tgt, self.names,
                                    self.weights, transform=transform, eps=self.eps, **kw)

    def flow(self, values):
        self.prepare()
        with torch.no_grad():
            return self.model(self.xd, self.with_row(values))

    @functools.cached_property
    def yardstick(self):
        """(series [P,T_out,B] float32, cost [P,B] float64) of every candidate by the module's own route; computed once."""
        series, cost = [], []
        for c in range(self.P):
            out = self.flow(self.cand[c])
            series.append(out["flow_sim"][..., 0].clone())
            cost.append(_series_cost(self.req, out, self.target, self.weights))
        return torch.stack(series), torch.stack(cost)

    @functools.cached_property
    def twin(self):
        """A twin target [T_out,B]: flow_sim at a hidden candidate (half a draw away from the row) times exp(0.2 noise),
        NaN where the case's own target is NaN."""
        hidden = self.cand[0] + 0.35 * torch.from_numpy(synth.normalish((self.B, len(self.cols)), 192)).to(self.cand.device)
        flow = self.flow(hidden)["flow_sim"][..., 0].clone()
        noise = torch.from_numpy(synth.normalish((self.T_out, self.B), 193)).to(flow.device)
        target = flow * torch.exp(0.2 * noise)
        return torch.where(torch.isnan(self.target), self.target, target).contiguous()

    @property
    def twin_weights(self):
        tgt = self.twin
        w = torch.ones_like(tgt) if self.weights is None else self.weights
        return torch.where(torch.isnan(tgt), torch.zeros_like(w), w).double()


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_series_and_cost_against_the_module(hip_backend, name):
    assert ops._POISON, "the GPU tier runs with NaN-poisoned output buffers"
    cs = case(name)
    got = cs.cost(return_series=True)
    series, cost = got["series"], got["cost"]
    want_series, want_cost = cs.yardstick
    assert tuple(series.shape) == (cs.P, cs.T_out, cs.B) and tuple(cost.shape) == (cs.P, cs.B)
    assert got["columns"] == cs.cols and cost.dtype == torch.float32 and series.dtype == torch.float32
    assert bool(torch.isfinite(series).all()) and bool(torch.isfinite(cost).all()), "a poisoned element was left"
    assert float(want_series.max()) > 0.1, "the record produces no flow: the comparison would be empty"

    # the series: adj_sets.VALUE_TOL, every element
    rtol, atol_rel = adj_sets.VALUE_TOL
    w8 = want_series.double()
    tol = atol_rel * float(w8.abs().max()) + rtol * w8.abs()
    err = (series.double() - w8).abs()
    same = torch.equal(bits(series), bits(want_series))
    print(f"{name}: series worst error / tolerance {float((err / tol).max()):.4f} (max abs {float(err.max()):.3e}); "
          f"bit-equal to the module's: {same}")
    assert bool((err <= tol).all()), f"{int((err > tol).sum())} of {err.numel()} elements outside the value tolerance"
    # candidate 0 is the current row: its series is the primal's own flow_sim
    own = got["outputs"]["flow_sim"][..., 0].double()
    assert tuple(own.shape) == (cs.T_out, cs.B)
    assert bool(((series[0].double() - own).abs() <= atol_rel * float(own.abs().max()) + rtol * own.abs()).all())

    # n_obs: the days with a positive weight once NaN targets are masked
    tgt = cs.target
    wts = torch.ones_like(tgt) if cs.weights is None else cs.weights
    seen = (~torch.isnan(tgt)) & (wts > 0)
    assert torch.equal(got["n_obs"], seen.sum(0)) and got["n_obs"].dtype == torch.int64

    # (a) the summation alone: float64 over the kernel's own float32 series
    w8 = torch.where(torch.isnan(tgt), torch.zeros_like(wts), wts).double()
    r8 = series.double() - torch.where(torch.isnan(tgt), torch.zeros_like(tgt), tgt).double()
    sum8 = (w8 * r8 * r8).sum(1)
    err = (cost.double() - sum8).abs()
    bound = gamma(cs.T_out + 2) * sum8
    need = float((err / torch.where(bound > 0, bound, torch.ones_like(bound))).max())
    print(f"{name}: cost against its own series: worst error / bound {need:.3f}")
    assert bool((err <= bound).all()), f"the cost misses the float64 sum of its own series by {need:.2f} x the bound"

    # (b) the module-route float64 cost of the same candidates
    assert bool((want_cost > 0).all()) and bool(torch.isfinite(want_cost).all())
    rdiff = float(((cost.double() - want_cost).abs() / want_cost).max())
    print(f"{name}: cost against the module route: worst relative difference {rdiff:.3e} (asserted {COST_RTOL:.1e})")
    assert rdiff <= COST_RTOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_stats_are_the_same_model_and_score_as_the_module_route(hip_backend, name):
    cs = case(name)
    tgt, w8 = cs.twin, cs.twin_weights
    cs.prepare()
    cost = adj_population_cost(cs.model, cs.xd, cs.p, cs.cand, tgt, cs.names, cs.weights, return_series=True)
    want_series = cs.yardstick[0]
    scored = cs.scored
    worst = 0.0
    for transform in TRANSFORMS:
        got = cs.stats(transform, return_series=True)
        for key in ("sse", "s1", "s2", "s3"):
            assert tuple(got[key].shape) == (cs.P, cs.B) and got[key].dtype == torch.float32
            assert bool(torch.isfinite(got[key]).all()), f"{transform}: a poisoned or non-finite element in {key}"
        assert torch.equal(bits(got["series"]), bits(cost["series"])), f"{transform}: the series is not the cost call's"
        assert got["columns"] == cs.cols and got["transform"] == transform and torch.equal(got["n_obs"], cost["n_obs"])
        assert (got["eps"] is None) == (transform != "log")
        if transform == "none":
            assert torch.equal(bits(got["sse"]), bits(cost["cost"])), "sse under 'none' is not adj_population_cost's cost"
        if not scored:
            continue
        eps = got["eps"]

        def g64(y):
            y = y.double()
            return y if transform == "none" else y.sqrt() if transform == "sqrt" else torch.log(y + eps.double())

        want = textbook(g64(want_series), g64(tgt), w8)
        for metric in SCORED[transform]:
            assert bool(torch.isfinite(want[metric]).all()), f"{transform} {metric}: the yardstick has no score"
            score = population_score(got, metric)
            assert tuple(score.shape) == (cs.P, cs.B) and score.dtype == torch.float64
            assert bool(torch.isfinite(score).all()), f"{transform} {metric}: a candidate has no score"
            diff = float(((score - want[metric]).abs() / (1 + (1 - want[metric]).abs())).max())
            worst = max(worst, diff)
            print(f"{name} {transform} {metric}: yardstick {float(want[metric].min()):.3f} .. {float(want[metric].max()):.3f}, "
                  f"worst difference {diff:.3e} (asserted {SCORE_TOL:.1e})")
    print(f"{name}: worst score difference {worst:.3e}")
    assert worst <= SCORE_TOL


@pytest.mark.gpu
def test_bit_rules(hip_backend):
    cs = case(BIT_CASE)
    assert cs.P == 17 and cs.masked
    a = cs.cost(return_series=True)
    b = cs.cost(return_series=True)
    assert torch.equal(bits(a["cost"]), bits(b["cost"])) and torch.equal(bits(a["series"]), bits(b["series"])), "two calls differ"
    plain = cs.cost()
    assert "series" not in plain and torch.equal(bits(plain["cost"]), bits(a["cost"])), "return_series changes the cost"
    pick = [0, 3, 8]
    for c in pick:
        alone = cs.cost(cs.cand[c:c + 1].contiguous(), return_series=True)
        assert torch.equal(bits(alone["cost"][0]), bits(a["cost"][c])), f"candidate {c} alone has other cost bits"
        assert torch.equal(bits(alone["series"][0]), bits(a["series"][c])), f"candidate {c} alone has other series bits"
    sub = cs.cost(cs.cand[pick].contiguous(), return_series=True)
    assert torch.equal(bits(sub["cost"]), bits(a["cost"][pick])) and torch.equal(bits(sub["series"]), bits(a["series"][pick]))
    # the candidates differ, and so do their costs: the candidate index reaches the parameters
    assert len({float(v) for v in a["cost"][:, 0]}) == cs.P
    # the same rules for the four sums of the stats entry
    keys = ("sse", "s1", "s2", "s3")
    for transform in TRANSFORMS:
        s = cs.stats(transform, return_series=True)
        s2 = cs.stats(transform)
        assert "series" not in s2 and all(torch.equal(bits(s[k]), bits(s2[k])) for k in keys), f"{transform}: the sums move"
        part = cs.stats(transform, cs.cand[pick].contiguous(), return_series=True)
        assert all(torch.equal(bits(part[k]), bits(s[k][pick])) for k in keys + ("series",)), f"{transform}: a subset differs"


@pytest.mark.gpu
def test_population_search(hip_backend):
    """A twin problem: observations from hidden parameters, the start far from them.  The search keeps the best of every
    round as candidate 0 of the next, so a basin's recorded cost cannot rise."""
    T, B, M = 40, 5, 2
    prob = own_problem(dict(T=T, B=B, M=M, dyn=()))
    model = adj_sets.model(DEV, prob, "staged", False)
    eager, st = type(model)._forward_eager, torch.from_numpy(synth.wet_states(B, M, 67)).to(DEV)
    model._forward_eager = lambda xd, pp: eager(model, xd, pp, state=st)        # a wet start: the twin has flow
    ny = model.learnable_param_count
    x = {"x_phy": torch.from_numpy(synth.forcing(T, B, seed=61)).to(DEV)}
    truth = torch.from_numpy(synth.raw_parameters(T, B, ny, seed=62)).to(DEV)
    with torch.no_grad():
        obs = model(x, truth)["flow_sim"][..., 0].clone()
    assert float(obs.max()) > 0.1
    start = torch.from_numpy(synth.raw_parameters(T, B, ny, seed=63, scale=1.5)).to(DEV)
    keep = [t.clone() for t in (start, obs, x["x_phy"])]

    def search(seed, **kw):
        g = torch.Generator().manual_seed(seed)
        return adj_population_search(model, x, start, obs, n_candidates=32, n_rounds=3, generator=g, **kw)

    best, hist = search(5)
    assert all(torch.equal(a, b) for a, b in zip((start, obs, x["x_phy"]), keep)), "an input was modified"
    _, cols = jacobian_columns(model, None)
    cost = hist["cost"]
    assert tuple(cost.shape) == (4, B) and tuple(hist["best_index"].shape) == (3, B) and hist["columns"] == cols
    assert set(hist) == {"cost", "best_index", "columns"}
    assert bool(torch.isfinite(cost).all()) and bool((cost[1:] <= cost[:-1]).all()), "a basin's recorded cost rose"
    assert bool((cost[-1] < cost[0]).any()), "32 candidates x 3 rounds improved no basin"
    assert torch.equal(hist["best_index"] != 0, cost[1:] < cost[:-1])
    # the returned row by the module's own route: the cost the history ends with, and not above the start's
    req = _check_request(model, x, start, obs, None, None, None, 1)
    with torch.no_grad():
        final = _series_cost(req, model(x, best), obs, None).cpu()
        first = _series_cost(req, model(x, start), obs, None).cpu()
    rdiff = float(((final - cost[-1]).abs() / final).max())
    print(f"adj_population_search: summed cost {float(first.sum()):.6g} -> {float(final.sum()):.6g}; history against the "
          f"module route: worst relative difference {rdiff:.3e}")
    assert rdiff <= COST_RTOL and bool((final <= first).all())
    # only the static row moved, and the same seed reproduces everything
    assert tuple(best.shape) == tuple(start.shape) and torch.equal(best[:-1], start[:-1])
    again, hist2 = search(5)
    assert torch.equal(bits(again), bits(best)) and torch.equal(hist2["cost"], cost)
    assert torch.equal(hist2["best_index"], hist["best_index"])
    other, _ = search(6)
    assert not torch.equal(other, best)
    # the method forwards, and another objective returns its score
    by_method, hist_m = model.population_search(x, start, obs, n_candidates=32, n_rounds=3,
                                                generator=torch.Generator().manual_seed(5))
    assert torch.equal(bits(by_method), bits(best)) and torch.equal(hist_m["cost"], cost)
    _, hist_k = search(5, objective="kge")
    assert tuple(hist_k["score"].shape) == (4, B) and torch.equal(hist_k["cost"], 1.0 - hist_k["score"])
    assert bool((hist_k["cost"][1:] <= hist_k["cost"][:-1]).all())
