"""GPU tier: `population_cost` / `population_search` (hydrodl2_amd/population.py) on hbvx_population_cost.

The yardstick is the module itself: for each candidate the candidate is written into the static row, the module is
called under no_grad and outputs['streamflow'] is taken -- the forward kernels, hbvx_route_forward and the float64
`calibrate._series_cost` that the parent commit has.

  series   within the project's stated flux tolerance (tests/abi_util.py: rtol 1e-4, atol 1e-5), every element, no
           outlier allowance: the records are at most 400 days.
  cost     (a) against the float64 sum over the kernel's OWN float32 series: the summation alone.  r = y - target is
           rounded, w r is rounded, one fused multiply-add per day: within gamma(T_out + 2) sum w r^2, gamma(n) =
           n u / (1 - n u), u = 2^-24 (the bound of tests/test_pop_host.py).
           (b) against the module-route float64 cost of the same candidate: two float32 forwards whose series differ
           in the last bits, so the tolerance is measured, not derived.  (At the shapes below the forward takes its
           one-wave kernel, whose day step and routing arithmetic k_pop restates: the series came out equal bit for
           bit, and what was measured is the float32 chain against the float64 sum.)  Worst relative difference over the cases
           below on the MI355X of profiles/r15_population.md: 8.91e-7 (the wet 400-day record;
           the short records 1.2e-7 .. 2.2e-7); asserted: four times that, COST_RTOL, for another
           summation order on another card -- and held below 1e-3, the level at which the ranking of candidates whose
           costs differ by a percent is safe."""
import functools

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import ops
from hydrodl2_amd.calibrate import _check_request, _series_cost
from hydrodl2_amd.population import population_cost, population_search
from hydrodl2_amd.sensitivity import jacobian_columns

from . import abi_util as au
from . import daily_sets as ds
from . import synth

DEV = "cuda:0"
U = 2.0 ** -24
MEASURED_COST_RDIFF = 8.91e-7
COST_RTOL = 4 * MEASURED_COST_RDIFF
assert COST_RTOL < 1e-3


def gamma(n):
    return n * U / (1.0 - n * U)


def bits(t):
    return t.contiguous().view(torch.int32)


# name -> what the case is.  Lane mapping: (M, B) = (1, 67) one wave of 64 basins and a partly filled second one,
# (2, 5) and (3, 5) padded members / a partly filled wave, (16, 5) four basins per wave in two waves; (4, 17) beside them.
# Time: T_out 7 and 15 (L = T), 40 and 400 (L = 15); warm_up 10 with warm_up_states True (a warm-up pass) and False
# (t_first = 10).
CASES = {
    "hbv-m1-b67-t7": dict(cls=("hbv", "Hbv"), M=1, B=67, T=17, warm_up=10, P=3),
    "hbv-m2-b5-t15-drop-masked": dict(cls=("hbv", "Hbv"), M=2, B=5, T=25, warm_up=10, P=17, dyn=["parBETA", "parBETAET"],
                                      dy_drop=0.5, masked=True),
    "hbv-m3-b5-t40-cutoff-subset": dict(cls=("hbv", "Hbv"), M=3, B=5, T=50, warm_up=10, warm_up_states=False, P=3,
                                        names=["parFC", "parK1", "route_a"]),
    "hbv11p-m16-b5-t40-muwts": dict(cls=("hbv_1_1p", "Hbv_1_1p"), M=16, B=5, T=50, warm_up=10, P=1, muwts=True),
    "hbv2-m2-b5-t40": dict(cls=("hbv_2", "Hbv_2"), M=2, B=5, T=40, P=3, dyn=["parBETA", "parK0"], masked=True),
    "hbv-wet400-norout": dict(cls=("hbv", "Hbv"), P=3, wet="wet400"),
}


class Case:
    """One problem: the model, its inputs, the candidates (candidate 0 is the current row), target and weights."""

    def __init__(self, name):
        c = CASES[name]
        self.name, self.names, self.P = name, c.get("names"), c["P"]
        fam, cls = c["cls"]
        self.states = None
        if "wet" in c:
            # the wet 400-day record of tests/daily_sets.py: carried-in wet storages, parameters spread over their
            # ranges, so that soil excess, fast runoff and PERC = parPERC are taken; routing off
            kw = ds.ABI_PROBLEMS[cls][c["wet"]]
            prob = ds.make(cls, kw)
            self.M, self.B, self.T, self.T_out = prob["M"], prob["B"], prob["T"], prob["T"]
            cfg = {"nmul": self.M, "routing": prob["routing"], "cache_states": True, "dynamic_params": {cls: list(prob["dyn"])}}
            self.model = hydrodl2_amd.load_model(fam, cls)(cfg, DEV)
            assert self.model.learnable_param_count == prob["ny"] - (0 if prob["routing"] else 2)
            self.xd = {"x_phy": torch.from_numpy(prob["x"]).to(DEV)}
            self.p = torch.from_numpy(prob["params"]).to(DEV)
            self.states = tuple(torch.from_numpy(prob["state_in"]).to(DEV).unbind(0))
        else:
            self.M, self.B, self.T = c["M"], c["B"], c["T"]
            two = cls == "Hbv_2"
            warm = 0 if two else c.get("warm_up", 0)
            self.T_out = self.T - warm
            cfg = {"nmul": self.M, "routing": c.get("routing", True), "dynamic_params": {cls: c.get("dyn", [])},
                   "dy_drop": c.get("dy_drop", 0.0), "cache_states": True}
            if not two:
                cfg.update(warm_up=warm, warm_up_states=c.get("warm_up_states", True))
            self.model = hydrodl2_amd.load_model(fam, cls)(cfg, DEV)
            seed = 7 * self.T + self.B + self.M
            # carried-in wet storages (synth.wet_states): a record of a few weeks from the default start (0.001 mm
            # everywhere) has flows below the tolerance's absolute part
            self.states = tuple(torch.from_numpy(synth.wet_states(self.B, self.M, seed + 6)).to(DEV).unbind(0))
            self.xd = {"x_phy": torch.from_numpy(synth.forcing(self.T, self.B, seed=seed)).to(DEV)}
            if two:
                self.p = (torch.from_numpy(synth.unit_parameters((self.T, self.B, self.model.learnable_param_count1), seed + 1)).to(DEV),
                          torch.from_numpy(synth.unit_parameters((self.B, self.model.learnable_param_count2), seed + 2)).to(DEV))
                self.xd["ac_all"] = torch.from_numpy(synth.uniform((self.B,), seed + 3) * 2000 + 10).to(DEV)
                self.xd["elev_all"] = torch.from_numpy(synth.uniform((self.B,), seed + 4) * 3000).to(DEV)
            else:
                self.p = torch.from_numpy(synth.raw_parameters(self.T, self.B, self.model.learnable_param_count, seed + 1)).to(DEV)
            if c.get("muwts"):
                u = torch.from_numpy(synth.uniform((self.T_out, self.B, self.M), seed + 5)).double() + 0.25
                self.xd["muwts"] = (u / u.sum(-1, keepdim=True)).float().to(DEV)
        self.two = isinstance(self.p, tuple)
        _, self.cols = jacobian_columns(self.model, self.names)
        C = len(self.cols)
        row = (self.p[1] if self.two else self.p[-1])[:, self.cols]
        if self.two:
            draws = torch.from_numpy(synth.unit_parameters((self.P, self.B, C), 91)).to(DEV)
        else:
            draws = row.unsqueeze(0) + 0.7 * torch.from_numpy(synth.normalish((self.P, self.B, C), 92)).to(DEV)
        draws[0] = row
        self.cand = draws.contiguous()
        self.target = torch.from_numpy(synth.uniform((self.T_out, self.B), 93) * 6.0).to(DEV)
        self.weights = None
        if c.get("masked"):
            # NaN targets (missing observations) and weights with exact zeros
            miss = torch.from_numpy(synth.uniform((self.T_out, self.B), 94) < 0.2).to(DEV)
            self.target = torch.where(miss, torch.full_like(self.target, float("nan")), self.target)
            wts = torch.from_numpy(synth.uniform((self.T_out, self.B), 95) + 0.25).to(DEV)
            self.weights = torch.where(torch.from_numpy(synth.uniform((self.T_out, self.B), 96) < 0.2).to(DEV),
                                       torch.zeros_like(wts), wts)
        self.req = _check_request(self.model, self.xd, self.p, self.target, self.names, None, self.weights, 1)

    def prepare(self):
        """What every run of the module starts from: the same dy_drop draws, the same carried-in storages."""
        torch.manual_seed(4321)
        if self.states is not None:
            self.model.load_states(self.states)

    def with_row(self, values):
        """`parameters` with [B,C] `values` written into the columns of the static row (a new tensor)."""
        t = (self.p[1] if self.two else self.p).clone()
        (t if self.two else t[-1])[:, self.cols] = values
        return (self.p[0], t) if self.two else t

    def population(self, cand=None, **kw):
        self.prepare()
        return population_cost(self.model, self.xd, self.p, self.cand if cand is None else cand, self.target, self.names,
                               self.weights, **kw)

    @functools.cached_property
    def yardstick(self):
        """(series [P,T_out,B] float32, cost [P,B] float64) of every candidate by the module's own route; computed once."""
        series, cost = [], []
        for c in range(self.P):
            self.prepare()
            with torch.no_grad():
                out = self.model(self.xd, self.with_row(self.cand[c]))
            series.append(out["streamflow"][..., 0].clone())
            cost.append(_series_cost(self.req, out, self.target, self.weights))
        return torch.stack(series), torch.stack(cost)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_series_and_cost_against_the_module(hip_backend, name):
    assert ops._POISON, "the GPU tier runs with NaN-poisoned output buffers"
    cs = case(name)
    got = cs.population(return_series=True)
    series, cost = got["series"], got["cost"]
    want_series, want_cost = cs.yardstick
    assert tuple(series.shape) == (cs.P, cs.T_out, cs.B) and tuple(cost.shape) == (cs.P, cs.B)
    assert got["columns"] == cs.cols and cost.dtype == torch.float32
    assert bool(torch.isfinite(series).all()) and bool(torch.isfinite(cost).all()), "a poisoned element was left"
    assert float(want_series.max()) > 0.1, "the record produces no flow: the comparison would be empty"

    # the series: the stated flux tolerance, every element
    err = (series.double() - want_series.double()).abs()
    tol = au.FLUX_ATOL + au.FLUX_RTOL * want_series.double().abs()
    print(f"{name}: series worst error / tolerance {float((err / tol).max()):.4f} (max abs {float(err.max()):.3e})")
    assert bool((err <= tol).all()), f"{int((err > tol).sum())} of {err.numel()} elements outside the flux tolerance"
    # candidate 0 is the current row: its series is the primal's own streamflow
    own = got["outputs"]["streamflow"][..., 0].double()
    assert bool(((series[0].double() - own).abs() <= au.FLUX_ATOL + au.FLUX_RTOL * own.abs()).all())

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
def test_bit_rules(hip_backend):
    cs = case("hbv-m2-b5-t15-drop-masked")
    a = cs.population(return_series=True)
    b = cs.population(return_series=True)
    assert torch.equal(bits(a["cost"]), bits(b["cost"])) and torch.equal(bits(a["series"]), bits(b["series"])), "two calls differ"
    plain = cs.population()
    assert "series" not in plain and torch.equal(bits(plain["cost"]), bits(a["cost"])), "return_series changes the cost"
    pick = [0, 3, 8]
    for c in pick:
        alone = cs.population(cs.cand[c:c + 1].contiguous(), return_series=True)
        assert torch.equal(bits(alone["cost"][0]), bits(a["cost"][c])), f"candidate {c} alone has other cost bits"
        assert torch.equal(bits(alone["series"][0]), bits(a["series"][c])), f"candidate {c} alone has other series bits"
    sub = cs.population(cs.cand[pick].contiguous(), return_series=True)
    assert torch.equal(bits(sub["cost"]), bits(a["cost"][pick])) and torch.equal(bits(sub["series"]), bits(a["series"][pick]))
    # the candidates differ, and so do their costs: the candidate index reaches the parameters
    assert len({float(v) for v in a["cost"][:, 0]}) == cs.P


@pytest.mark.gpu
def test_population_search(hip_backend):
    """A twin problem: observations from hidden parameters, the start far from them.  The search keeps the best of every
    round as candidate 0 of the next, so a basin's recorded cost cannot rise."""
    T, B, M = 40, 5, 2
    model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "dynamic_params": {"Hbv": []}}, DEV)
    x = {"x_phy": torch.from_numpy(synth.forcing(T, B, seed=61)).to(DEV)}
    truth = torch.from_numpy(synth.raw_parameters(T, B, model.learnable_param_count, seed=62)).to(DEV)
    with torch.no_grad():
        obs = model(x, truth)["streamflow"][..., 0].clone()
    start = torch.from_numpy(synth.raw_parameters(T, B, model.learnable_param_count, seed=63, scale=1.5)).to(DEV)
    keep = [t.clone() for t in (start, obs, x["x_phy"])]

    def search(seed):
        g = torch.Generator().manual_seed(seed)
        return population_search(model, x, start, obs, n_candidates=32, n_rounds=3, generator=g)

    best, hist = search(5)
    assert all(torch.equal(a, b) for a, b in zip((start, obs, x["x_phy"]), keep)), "an input was modified"
    _, cols = jacobian_columns(model, None)
    cost = hist["cost"]
    assert tuple(cost.shape) == (4, B) and tuple(hist["best_index"].shape) == (3, B) and hist["columns"] == cols
    assert bool(torch.isfinite(cost).all()) and bool((cost[1:] <= cost[:-1]).all()), "a basin's recorded cost rose"
    assert bool((cost[-1] < cost[0]).any()), "32 candidates x 3 rounds improved no basin"
    assert torch.equal(hist["best_index"] != 0, cost[1:] < cost[:-1])
    # the returned row by the module's own route: the cost the history ends with, and not above the start's
    req = _check_request(model, x, start, obs, None, None, None, 1)
    with torch.no_grad():
        final = _series_cost(req, model(x, best), obs, None).cpu()
        first = _series_cost(req, model(x, start), obs, None).cpu()
    rdiff = float(((final - cost[-1]).abs() / final).max())
    print(f"population_search: summed cost {float(first.sum()):.6g} -> {float(final.sum()):.6g}; history against the "
          f"module route: worst relative difference {rdiff:.3e}")
    assert rdiff <= COST_RTOL and bool((final <= first).all())
    # only the static row moved, and the same seed reproduces everything
    assert tuple(best.shape) == tuple(start.shape) and torch.equal(best[:-1], start[:-1])
    again, hist2 = search(5)
    assert torch.equal(bits(again), bits(best)) and torch.equal(hist2["cost"], cost)
    assert torch.equal(hist2["best_index"], hist["best_index"])
    other, _ = search(6)
    assert not torch.equal(other, best)
