"""GPU tier: `hourly_population_stats` (Hbv_2_hourly.population_stats; include/hbvx_gage_pop.h) on three golden hourly
module cases and three synthetic records, P = 5 candidates of both kinds each.

Per record, from ONE evaluation that every test shares (the front end's own sequence through the ops layer, so that the
call's own runoff and hourly gage series can be looked at; the front end itself is held to its bits):
  runoff   each candidate's unit runoff against the module's Qs from a module forward with that candidate substituted:
           every element within abi_util.FLUX_ATOL + FLUX_RTOL |Qs|;
  series   each candidate's hourly gage series bit for bit GageRoute's (hbvx_gage_route_forward) on the call's own
           runoff and that candidate's routing parameters;
  sums     under 'none' bit for bit tests/hosttest/gagepop_host.cpp fed the call's own series; under 'sqrt' and 'log'
           within tests/test_popstats_host.py's bounds of float64 sums over the device's own transform of the call's own
           period means;
  scores   nse, kge, r, alpha, beta against float64 scores of the module route (P module forwards, period means and
           scores in float64), every record x transform x {hourly, 24-hour} calendar, in the neighbouring tests' measure
           |difference| / (1 + |1 - score|) over the gages that have observations.  Largest value measured on these
           records on an MI355X: 1.45e-4 (MEASURED_SCORE_DIFF: r on the 50-hour record's two 24-hour periods, a
           degenerate score); asserted: four times that, 5.8e-4, below the sanity cap 1e-3 of
           tests/test_population_gpu.py.  The records of 120 hours and more measure 2.27e-6 and are held to 9.1e-6;
  bits     two calls agree; return_series changes nothing; a candidate alone, in another order or under another
           max_candidates (2 of 5: uneven chunks, and 1) has the same bits -- with both families on three records, and
           routing-only and units-only on 'tiles'; distr_candidates equal to parameters[2] repeated gives the bits of
           distr_candidates=None, and candidates equal to the p_sta row repeated the bits of candidates=None (the four
           sums and the period means: stage 1 then restates the primal run's runoff to the bit); the primal row as a
           candidate reproduces the primal streamflow within the flux tolerance;
  routing-only   candidates=None: the same checks, and the front end launches no stage 1 (ops.HOURLY_POP_LAUNCHES
           around the call itself, on every record);
  the inputs are unmodified and the module is left as one plain forward leaves it.
The synthetic record 'tiles' has T = 1100 (two 1024-hour tiles, the 72-tap halo crossing the edge), 37 units (no full
wave), a gage with one pair, a gage draining most units, two nested gages, a gage with no pair (its series is 0) and
route_tau values whose floor pushes taps past tap 71; 'short' has L = T = 50 < 72; 'm16_muwts' 16 members with weights."""
import functools

import numpy as np
import pytest
import torch

from hydrodl2_amd import _abi, ops
from hydrodl2_amd.hourly_population import hourly_population_columns, hourly_population_stats
from hydrodl2_amd.population import _calendar, _observations, population_score

from . import abi_util as au
from . import golden_cases as gc
from . import synth
from .test_hourly_population_host import gagelib  # noqa: F401  (fixture)
from .test_population_period_host import period_means64
from .test_population_score_host import textbook
from .test_population_stats_gpu import device_transform, g64
from .test_popstats_host import check_chains

pytestmark = pytest.mark.gpu

DEV = "cuda"
P = 5
TRANSFORMS = ("none", "sqrt", "log")
METRICS = ("nse", "kge", "r", "alpha", "beta")
CALENDARS = (None, 24)
KEYS = ("sse", "s1", "s2", "s3")
MEASURED_SCORE_DIFF = 1.45e-4     # the largest |difference| / (1 + |1 - score|) on these records (MI355X)
SCORE_TOL = 4 * MEASURED_SCORE_DIFF
assert SCORE_TOL < 1e-3
# Where that value comes from: 'short' under the 24-hour calendar has TWO periods, and r of two points is +-1 whatever
# the candidate: var_s var_o = cov^2 exactly, and the float32 chains leave 1.4e-4 of that cancellation (3.3e-5 with its
# 50 hourly values).  Every other record (120 hours and more) agrees to 2.27e-6, and is held to four times THAT:
MEASURED_LONG_DIFF = 2.27e-6
LONG_TOL = 4 * MEASURED_LONG_DIFF


def bits(t):
    return t.contiguous().view(torch.int32)


def _golden(name, **over):
    cfg = dict(gc.CASES[name]["config"])
    cfg.update(over)
    inp = gc.build_inputs(name)
    return dict(config=cfg, inp=inp, seed=gc.CASES[name].get("torch_seed", 0), names=None)


def _synthetic(T, U, M, G, seed, dyn=(), topo=None, muwts=False, names=None, tau_high=(), **cfg):
    config = {"nmul": M, "dynamic_params": {"Hbv_2_hourly": list(dyn)}, **cfg}
    n_st = 19 - len(dyn)
    if topo is None:
        topo = (synth.uniform((G, U), seed, 13) < np.float32(0.45)).astype(np.float32)
        topo[np.arange(U) % G, np.arange(U)] = 1.0
    inp = {"x_phy": synth.forcing_hourly(T, U, seed, storm=5.0, day0=100.25),
           "p_dyn": synth.unit_parameters((T, U, len(dyn) * M), seed, 4),
           "p_sta": synth.unit_parameters((U, n_st * M), seed, 6),
           "ac_all": (synth.uniform((U,), seed, 7) * np.float32(5000.0)).astype(np.float32),
           "elev_all": (synth.uniform((U,), seed, 8) * np.float32(3000.0)).astype(np.float32),
           "outlet_topo": topo,
           "areas": (synth.uniform((U,), seed, 14) * np.float32(90.0) + np.float32(5.0)).astype(np.float32),
           "p_distr": synth.unit_parameters((int(topo.sum()), 3), seed, 15)}
    for pair in tau_high:
        inp["p_distr"][pair, 2] = np.float32(0.97)      # route_tau = 46.56 hours: the taps from 26 on leave the window
    if muwts:
        u = synth.uniform((T, U, M), seed, 9).astype(np.float64) + 0.25
        inp["muwts"] = (u / u.sum(-1, keepdims=True)).astype(np.float32)
    return dict(config=config, inp=inp, seed=seed, names=names)


def _tiles_topology(U=37, G=5):
    topo = np.zeros((G, U), np.float32)
    topo[0, 3] = 1.0                        # a gage with one pair
    topo[1, :33] = 1.0                      # a gage draining most units
    topo[2, 10:25] = 1.0                    # two nested gages sharing units
    topo[3, 14:20] = 1.0
    return topo                             # gage 4 has no pair


RECORDS = {
    "hourly_long_dyn3": lambda: _golden("hourly_long_dyn3"),
    "hourly_long_drop_m16": lambda: _golden("hourly_long_routing", routing=False),        # dynamic parameters, dy_drop
    "hourly_wet_muwts": lambda: _golden("hourly_wet_muwts", cache_states=False),
    "tiles": lambda: _synthetic(1100, 37, 4, 5, 701, topo=_tiles_topology(), tau_high=(0, 5, 40),
                                names=["parFC", "parK1", "parF0", "parALPHA", "parBETA"]),
    # (seed 705: rain above freezing on every unit within the 50 hours, so both gages see water that varies)
    "short": lambda: _synthetic(50, 5, 2, 2, 705, dyn=("parBETA",),
                                topo=np.array([[1, 1, 1, 1, 0], [0, 0, 1, 1, 1]], np.float32)),
    "m16_muwts": lambda: _synthetic(120, 6, 16, 3, 703, dyn=("parK0", "parF0"), muwts=True, dy_drop=0.3),
}


class Case:
    def __init__(self, name):
        import hydrodl2_amd
        rec = RECORDS[name]()
        self.name, self.seed, self.names = name, rec["seed"], rec["names"]
        self.model = hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")(rec["config"], torch.device(DEV))
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in rec["inp"].items()}
        self.xd = {k: t[k] for k in ("x_phy", "ac_all", "elev_all", "outlet_topo", "areas", "muwts") if k in t}
        self.p = (t["p_dyn"], t["p_sta"], t["p_distr"])
        self.T, self.U = (int(s) for s in t["x_phy"].shape[:2])
        self.G, self.n_pair = int(t["outlet_topo"].shape[0]), int(t["p_distr"].shape[0])
        self.cols = hourly_population_columns(self.model, self.names)
        col = torch.as_tensor(self.cols, device=DEV)
        row = t["p_sta"][:, col]
        draws = torch.from_numpy(synth.unit_parameters((P - 1, self.U, len(self.cols)), self.seed, 191)).to(DEV)
        self.cand = torch.cat([row.unsqueeze(0), 0.5 * (row.unsqueeze(0) + draws)]).contiguous()
        ddraws = torch.from_numpy(synth.unit_parameters((P - 1, self.n_pair, 3), self.seed, 192)).to(DEV)
        self.dcand = torch.cat([t["p_distr"].unsqueeze(0), 0.5 * (t["p_distr"].unsqueeze(0) + ddraws)]).contiguous()
        self._col = col

    def prepare(self):
        torch.manual_seed(self.seed)        # the dy_drop draws: the same masks in every run of the module

    def with_candidate(self, cand_row=None, dcand_row=None):
        p_sta = self.p[1]
        if cand_row is not None:
            p_sta = p_sta.clone()
            p_sta[:, self._col] = cand_row
        return (self.p[0], p_sta, self.p[2] if dcand_row is None else dcand_row)

    def forward(self, params):
        self.prepare()
        with torch.no_grad():
            out = self.model(self.xd, params)
        return out["Qs"][..., 0].clone(), out["streamflow"][..., 0].clone()

    def observed_gages(self):
        return self.xd["outlet_topo"].sum(1) > 0


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def module_route(name, mode):
    """(Qs [P,Tq,U], streamflow [P,T,G]) of P module forwards with each candidate substituted.  Computed once per mode."""
    cs = case(name)
    runs = [cs.forward(cs.with_candidate(cs.cand[c] if mode != "routing" else None, cs.dcand[c] if mode != "units" else None))
            for c in range(P)]
    return torch.stack([r[0] for r in runs]), torch.stack([r[1] for r in runs])


@functools.lru_cache(maxsize=None)
def hourly_target(name):
    """The hourly twin target [T,G]: streamflow at a hidden candidate times exp(0.2 noise); NaN in a tenth of the hours
    and at gages without a pair."""
    cs = case(name)
    hidden = 0.5 * (cs.cand[0] + torch.from_numpy(synth.unit_parameters(tuple(cs.cand[0].shape), cs.seed, 193)).to(DEV))
    hd = 0.5 * (cs.dcand[0] + torch.from_numpy(synth.unit_parameters(tuple(cs.dcand[0].shape), cs.seed, 194)).to(DEV))
    _, flow = cs.forward(cs.with_candidate(hidden, hd))
    noise = torch.from_numpy(synth.normalish((cs.T, cs.G), cs.seed, 195)).to(DEV)
    # (a twentieth of the record's mean flow is added: a gage that sees no water in a short record still has a positive
    # mean, which the default eps under 'log' needs)
    tgt = (flow * torch.exp(0.2 * noise) + 0.05 * flow.mean()).double()
    return torch.where(cs.observed_gages().unsqueeze(0), tgt, torch.full_like(tgt, float("nan")))


def observations(name, cal):
    """(target [K,G] float64 with NaNs, weights [K,G] float32) on the calendar."""
    cs = case(name)
    ends = _calendar(cal, cs.T, "periods", "test")
    K = int(ends.numel())
    tgt = period_means64(hourly_target(name), ends.tolist())
    gone = torch.from_numpy(synth.uniform((K, cs.G), cs.seed, 196)).to(DEV) < 0.1
    if K > 4:
        tgt = torch.where(gone, torch.full_like(tgt, float("nan")), tgt)
    w = (torch.from_numpy(synth.uniform((K, cs.G), cs.seed, 197)).to(DEV) + 0.5).contiguous()
    return tgt.contiguous(), w, ends


def kwargs_of(cs, mode):
    return dict(candidates=None if mode == "routing" else cs.cand, distr_candidates=None if mode == "units" else cs.dcand,
                names=None if mode == "routing" else cs.names)


def call(name, mode, cal, transform, **kw):
    cs = case(name)
    tgt, w, _ = observations(name, cal)
    cs.prepare()
    args = kwargs_of(cs, mode)
    args.update(kw)
    return hourly_population_stats(cs.model, cs.xd, cs.p, tgt, weights=w, periods=cal, transform=transform, **args)


@functools.lru_cache(maxsize=None)
def staged(name, mode, cal, transform):
    """The front end's own sequence through the ops layer, keeping what the front end drops: (runoff [P,T,U] or the
    primal's [T,U], sums, period means [P,K,G], hourly gage series [P,T,G], the gage record, the observation side)."""
    cs = case(name)
    tgt, w, ends = observations(name, cal)
    ob = _observations(type("G", (), {"T_out": cs.T, "B": cs.G}), cs.xd, tgt, w, transform, None, "test", rows=int(ends.numel()))
    cs.prepare()
    with torch.no_grad(), ops.record_paths() as records, ops.record_gage_routes() as routes:
        cs.model(cs.xd, cs.p)
    main, grec = records[-1], routes[-1]
    if mode == "routing":
        runoff = grec.qs
    else:
        slots = {_abi.PARAM_SLOTS.index(n): (cs.cand, i * cs.model.nmul)
                 for i, n in enumerate(cs.names or [n for n in cs.model.parameter_bounds if n not in cs.model.dynamic_params])}
        runoff = ops.hourly_population_runoff(main, slots, P)
    term = ops.PopTerm(ob["target"], ob["w"], ob["shift"], ob["eps"], transform)
    got = ops.gage_population(grec, runoff, None if mode == "units" else cs.dcand, term,
                              ends.to(device=DEV, dtype=torch.int32), True, want_gage=True)
    torch.cuda.synchronize()
    return runoff, got[:4], got[4], got[5], grec, ob


MODES = ("both", "routing")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(RECORDS))
def test_runoff_series_and_sums(hip_backend, gagelib, name, mode):  # noqa: F811
    assert ops._POISON, "the GPU tier runs with NaN-poisoned output buffers"
    cs = case(name)
    runoff, sums, means, gage, grec, ob = staged(name, mode, 24, "none")
    qs_want, flow_want = module_route(name, mode)
    # (0) the front end itself: the bits of its own sequence through the ops layer, and which stages it launches
    before = dict(ops.HOURLY_POP_LAUNCHES)
    front = call(name, mode, 24, "none", return_series=True)
    launched = {k: ops.HOURLY_POP_LAUNCHES[k] - before[k] for k in before}
    assert launched == {"runoff": 0 if mode == "routing" else 1, "gage": 1}, launched
    for k, s in zip(KEYS, sums):
        assert torch.equal(bits(front[k]), bits(s)), f"{k}: the front end is not its own sequence through the ops layer"
    assert torch.equal(bits(front["series"]), bits(means))
    # (1) the unit runoff against the module's Qs
    if mode != "routing":
        assert tuple(runoff.shape) == (P, cs.T, cs.U) and bool(torch.isfinite(runoff).all())
        Tq = int(qs_want.shape[1])
        err = (runoff[:, cs.T - Tq:].double() - qs_want.double()).abs()
        tol = au.FLUX_ATOL + au.FLUX_RTOL * qs_want.double().abs()
        print(f"{name}: runoff against the module's Qs, worst error / tolerance {float((err / tol).max()):.3g}")
        assert bool((err <= tol).all())
        assert float(qs_want.max()) > 0.01, "the record moves no water"
        assert not torch.equal(runoff[0], runoff[1])
    # (2) the hourly gage series: GageRoute's bits on the call's own runoff and the candidate's routing parameters
    assert tuple(gage.shape) == (P, cs.T, cs.G) and bool(torch.isfinite(gage).all())
    for c in range(P):
        q = runoff if runoff.dim() == 2 else runoff[c]
        want = ops.GageRoute.apply(grec.topo, q, cs.p[2] if mode == "units" else cs.dcand[c])
        assert torch.equal(bits(gage[c]), bits(want)), f"candidate {c}: the gage series is not hbvx_gage_route_forward's"
    none = ~cs.observed_gages()
    assert bool((gage[:, :, none] == 0).all())
    # ... and against the module route within the flux tolerance; the primal row reproduces the primal run's streamflow
    err = (gage.double() - flow_want.double()).abs()
    tol = au.FLUX_ATOL + au.FLUX_RTOL * flow_want.double().abs()
    print(f"{name}: gage series against the module route, worst error / tolerance {float((err / tol).max()):.3g}")
    assert bool((err <= tol).all())
    _, primal = cs.forward(cs.p)
    assert bool(((gage[0].double() - primal.double()).abs() <= au.FLUX_ATOL + au.FLUX_RTOL * primal.double().abs()).all())
    # (3) the sums
    _, _, ends = observations(name, 24)
    K = int(ends.numel())
    e32 = np.ascontiguousarray(ends.numpy().astype(np.int32))
    for transform in TRANSFORMS:
        _, sums, means, gage_t, _, ob = staged(name, mode, 24, transform)
        assert torch.equal(bits(gage_t), bits(gage)), "the gage series depends on the transform"
        assert tuple(means.shape) == (P, K, cs.G) and bool(torch.isfinite(means).all())
        ot, w, shift = (ob[k].cpu().numpy() for k in ("target", "w", "shift"))
        eps = None if ob["eps"] is None else ob["eps"].cpu().numpy()
        for c in range(P):
            out = np.stack([s[c].cpu().numpy() for s in sums])
            if transform == "none":
                series = np.ascontiguousarray(gage[c].cpu().numpy())
                mean_h = np.full((K, cs.G), np.nan, np.float32)
                out_h = np.full((4, cs.G), np.nan, np.float32)
                ptr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
                assert gagelib.gagepop_host(cs.T, cs.G, K, 0, ptr(e32), ptr(series), ptr(ot), ptr(w), ptr(shift), None,
                                            ptr(mean_h), None, ptr(out_h)) == 0
                assert np.array_equal(mean_h.view(np.uint32), means[c].cpu().numpy().view(np.uint32)), "the period means"
                assert np.array_equal(out_h.view(np.uint32), out.view(np.uint32)), "the four sums are not the host restatement's"
            else:
                yt = device_transform(hip_backend, means[c], None if eps is None else ob["eps"].expand_as(means[c]), transform)
                assert bool(torch.isfinite(yt).all())
                check_chains(out, yt.cpu().numpy(), ot, w, shift, K, 0, f"{name} {mode} {transform} candidate {c}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(RECORDS))
def test_scores_against_the_module_route(hip_backend, name, mode):
    cs = case(name)
    _, flow_want = module_route(name, mode)
    seen = cs.observed_gages()
    worst = 0.0
    for cal in CALENDARS:
        tgt, w, ends = observations(name, cal)
        miss = torch.isnan(tgt)
        w8 = torch.where(miss, torch.zeros_like(tgt), w.double())
        sim8 = period_means64(flow_want, ends.tolist())                 # [P,K,G] float64
        for transform in TRANSFORMS:
            got = call(name, mode, cal, transform)
            assert got["columns"] == ([] if mode == "routing" else cs.cols) and got["transform"] == transform
            assert ("period_ends" in got) == (cal is not None)
            eps = got["eps"]
            want = textbook(g64(sim8, transform, eps), g64(tgt, transform, eps), w8)
            for metric in METRICS:
                score = population_score(got, metric)
                assert tuple(score.shape) == (P, cs.G) and score.dtype == torch.float64
                assert bool(torch.isfinite(want[metric][:, seen]).all()), f"{transform} {metric}: the yardstick has no score"
                assert bool(torch.isfinite(score[:, seen]).all()), f"{transform} {metric}: a candidate has no score"
                assert bool(torch.isnan(score[:, ~seen]).all())
                diff = float(((score - want[metric]).abs() / (1 + (1 - want[metric]).abs()))[:, seen].max())
                worst = max(worst, diff)
                print(f"{name} {mode} {cal} {transform} {metric}: yardstick {float(want[metric][:, seen].min()):.3f} .. "
                      f"{float(want[metric][:, seen].max()):.3f}, worst difference {diff:.3e}")
    tol = SCORE_TOL if name == "short" else LONG_TOL
    print(f"{name} {mode}: worst score difference {worst:.3e} (asserted {tol:.1e})")
    assert worst <= tol


def _module_state(model):
    st = model.get_states()
    return dict(series=None if st is None else [s.cpu() for s in st], states=None if not model.states else [s.cpu() for s in model.states],
                buffer=[q.cpu() for q in model._qs_buffer], rng=torch.get_rng_state())


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return torch.equal(a, b)


@pytest.mark.parametrize("name,mode", [("tiles", "both"), ("tiles", "routing"), ("tiles", "units"),
                                       ("hourly_long_drop_m16", "both"), ("short", "both")])
def test_the_bit_rules(hip_backend, name, mode):
    cs = case(name)
    kept = [t.clone() for t in (cs.cand, cs.dcand, *cs.p, *cs.xd.values())]
    base = call(name, mode, 24, "sqrt", return_series=True)
    after = _module_state(cs.model)
    staged_sums, staged_means = staged(name, mode, 24, "sqrt")[1:3]
    for k, s in zip(KEYS, staged_sums):
        assert tuple(base[k].shape) == (P, cs.G) and base[k].dtype == torch.float32
        assert torch.equal(bits(base[k]), bits(s)), f"{k}: the front end is not its own sequence through the ops layer"
    assert torch.equal(bits(base["series"]), bits(staged_means))
    again = call(name, mode, 24, "sqrt")
    split = call(name, mode, 24, "sqrt", max_candidates=2, return_series=True)
    one = call(name, mode, 24, "sqrt", max_candidates=1)
    assert "series" not in again and torch.equal(bits(split["series"]), bits(base["series"]))
    order = [3, 0, 4, 2, 1]

    def subset(idx):
        """The families of the mode, candidates `idx` of each."""
        kw = {}
        if mode != "routing":
            kw["candidates"] = cs.cand[idx].contiguous()
        if mode != "units":
            kw["distr_candidates"] = cs.dcand[idx].contiguous()
        return kw

    shuffled = call(name, mode, 24, "sqrt", **subset(order))
    alone = call(name, mode, 24, "sqrt", **subset([2]))
    for k in KEYS:
        for other, what in ((again, "a second call"), (split, "max_candidates=2"), (one, "max_candidates=1")):
            assert torch.equal(bits(other[k]), bits(base[k])), f"{k}: {what}"
        assert torch.equal(bits(shuffled[k]), bits(base[k][order])), f"{k}: another order"
        assert torch.equal(bits(alone[k]), bits(base[k][2:3])), f"{k}: a candidate alone"
    for o in (again, split):
        for k in base["outputs"]:
            assert torch.equal(o["outputs"][k], base["outputs"][k])
    if mode == "both":
        # a family held at the primal's values is the call without that family, bit for bit, either way round
        units = call(name, "units", 24, "sqrt", return_series=True)
        held = call(name, "both", 24, "sqrt", distr_candidates=cs.p[2].unsqueeze(0).repeat(P, 1, 1), return_series=True)
        routing = call(name, "routing", 24, "sqrt", return_series=True)
        col = torch.as_tensor(cs.cols, device=DEV)
        row = cs.p[1][:, col].unsqueeze(0).repeat(P, 1, 1).contiguous()
        pinned = call(name, "both", 24, "sqrt", candidates=row, names=cs.names, return_series=True)
        for k in KEYS + ("series",):
            assert torch.equal(bits(held[k]), bits(units[k])), f"{k}: distr_candidates = parameters[2] is not distr_candidates=None"
            assert torch.equal(bits(pinned[k]), bits(routing[k])), f"{k}: candidates = the p_sta row is not candidates=None"
    # inputs unmodified; the module is left as one plain forward leaves it
    for t, k in zip((cs.cand, cs.dcand, *cs.p, *cs.xd.values()), kept):
        assert torch.equal(t, k)
    import hydrodl2_amd
    plain = hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")(RECORDS[name]()["config"], torch.device(DEV))
    cs.prepare()
    with torch.no_grad():
        ref = plain(cs.xd, cs.p)
    for k in ref:
        assert torch.equal(base["outputs"][k], ref[k]), k
    want_state = _module_state(plain)
    for k in want_state:
        assert _same(after[k], want_state[k]), k


def test_routing_only_launches_no_stage_one_and_the_method_is_the_function(hip_backend):
    cs = case("short")
    tgt, w, _ = observations("short", None)
    before = dict(ops.HOURLY_POP_LAUNCHES)
    cs.prepare()
    got = cs.model.population_stats(cs.xd, cs.p, tgt, distr_candidates=cs.dcand, weights=w, max_candidates=2)
    assert ops.HOURLY_POP_LAUNCHES["runoff"] == before["runoff"], "stage 1 ran in a routing-only call"
    assert ops.HOURLY_POP_LAUNCHES["gage"] == before["gage"] + 3
    want = call("short", "routing", None, "none")
    for k in KEYS:
        assert torch.equal(bits(got[k]), bits(want[k]))
    assert "period_ends" not in got and got["columns"] == []
    cs.prepare()
    both = cs.model.population_stats(cs.xd, cs.p, tgt, cs.cand, cs.dcand, weights=w)
    assert ops.HOURLY_POP_LAUNCHES["runoff"] == before["runoff"] + 1
    # the hourly calendar given as a one-hour calendar: the same bits
    cs.prepare()
    hourly = cs.model.population_stats(cs.xd, cs.p, tgt, cs.cand, cs.dcand, weights=w, periods=1)
    for k in KEYS:
        assert torch.equal(bits(both[k]), bits(hourly[k]))
