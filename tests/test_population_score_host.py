"""CPU tier: `population_score` (pure float64 algebra on what `population_stats` returns), every new refusal of
`population_stats` / `population_search` that happens before a library call (hydrodl2_amd/population.py), the exports,
and -- on the cross-compiled library, without a launch -- the argument checks of hbvx_population_stats with their
messages and the layout of hbvx_pop_stats.

The score test builds the sums in float64 from random weighted series with NaN gaps and zero weights and holds every
metric to its textbook definition evaluated on the series directly, to 1e-10: what differs is the algebra alone -- moments
about the shift m against moments about the means."""
import ctypes as C

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi
from hydrodl2_amd.population import (METRICS, _objective_cost, population_score, population_search, population_stats)

from .test_hbv_adj import host_math_backend  # noqa: F401  (fixture)
from .test_population_host import _desc, _model, _pop, _route
from .test_step_math_host import steptest_lib  # noqa: F401  (fixture)

NAN = float("nan")


def stats_of(sim, obs, w):
    """`population_stats`' dictionary in exact float64 from sim [P,T,B], obs [T,B] (NaN: missing), w [T,B] >= 0: the
    shift is the float32 weighted mean of the observations, as the call forms it."""
    miss = torch.isnan(obs)
    w = torch.where(miss, torch.zeros_like(w), w)
    o = torch.where(miss, torch.zeros_like(obs), obs)
    W = w.sum(0)
    m = torch.where(W > 0, (w * o).sum(0) / W.clamp_min(1e-300), torch.zeros_like(W)).float()
    d, e = sim - m.double(), o - m.double()
    return {"sse": (w * (sim - o) ** 2).sum(1), "s1": (w * d).sum(1), "s2": (w * d * d).sum(1), "s3": (w * d * e).sum(1),
            "shift": m, "obs": {"W": W, "e1": (w * e).sum(0), "e2": (w * e * e).sum(0)},
            "n_obs": (w > 0).sum(0, dtype=torch.int64), "transform": "none", "eps": None}


def textbook(sim, obs, w):
    """Every metric from the series by its definition: weighted population moments about the means, float64."""
    miss = torch.isnan(obs)
    w = torch.where(miss, torch.zeros_like(w), w)
    o = torch.where(miss, torch.zeros_like(obs), obs)
    W = w.sum(0)
    mo, ms = (w * o).sum(0) / W, (w * sim).sum(1) / W
    vo, vs = (w * (o - mo) ** 2).sum(0) / W, (w * (sim - ms.unsqueeze(1)) ** 2).sum(1) / W
    cov = (w * (sim - ms.unsqueeze(1)) * (o - mo)).sum(1) / W
    sse = (w * (sim - o) ** 2).sum(1)
    r, alpha, beta = cov / (vs.sqrt() * vo.sqrt()), (vs / vo).sqrt(), ms / mo
    cvr = (vs.sqrt() / ms) / (vo.sqrt() / mo)
    return {"sse": sse, "mse": sse / W, "nse": 1 - sse / (W * vo), "r": r, "alpha": alpha, "beta": beta,
            "pbias": 100 * (ms - mo) / mo,
            "kge": 1 - ((r - 1) ** 2 + (alpha - 1) ** 2 + (beta - 1) ** 2).sqrt(),
            "kge12": 1 - ((r - 1) ** 2 + (cvr - 1) ** 2 + (beta - 1) ** 2).sqrt()}


def test_every_metric_is_its_textbook_definition():
    P, T, B = 5, 200, 7
    g = torch.Generator().manual_seed(11)
    obs = torch.rand(T, B, generator=g, dtype=torch.float64) * 5 + 10 ** torch.linspace(-1, 2, B, dtype=torch.float64)
    sim = obs.unsqueeze(0) * (0.6 + 0.8 * torch.rand(P, T, B, generator=g, dtype=torch.float64)) \
        + torch.rand(P, 1, B, generator=g, dtype=torch.float64)
    w = torch.rand(T, B, generator=g, dtype=torch.float64) + 0.1
    w[torch.rand(T, B, generator=g) < 0.2] = 0.0
    obs[torch.rand(T, B, generator=g) < 0.15] = NAN
    st = stats_of(sim, obs, w)
    want = textbook(sim, obs, w)
    assert set(want) == set(METRICS)
    for metric in METRICS:
        got = population_score(st, metric)
        assert got.dtype == torch.float64 and tuple(got.shape) == (P, B)
        err = float(((got - want[metric]).abs() / (1 + want[metric].abs())).max())
        print(f"{metric}: worst difference from the definition {err:.2e}")
        assert bool(torch.isfinite(got).all()) and err <= 1e-10, metric
    with pytest.raises(ValueError, match="metric must be one of"):
        population_score(st, "rmse")


def _case(sim, obs):
    sim, obs = torch.tensor(sim, dtype=torch.float64), torch.tensor(obs, dtype=torch.float64)
    return stats_of(sim.reshape(1, -1, 1), obs.reshape(-1, 1), torch.ones(obs.numel(), 1, dtype=torch.float64))


def test_every_undefined_case_is_nan_and_costs_infinity():
    needs_two = ("nse", "r", "alpha", "kge", "kge12")
    needs_mean = ("beta", "pbias", "kge", "kge12")
    cases = {
        # name: (stats, the metrics that are NaN there; every other one is finite)
        "a single observation": (_case([1.5, 2.0, 4.0], [1.0, NAN, NAN]), needs_two),
        "no observation": (_case([1.5, 2.0], [NAN, NAN]), tuple(m for m in METRICS if m != "sse")),
        "constant observations": (_case([1.0, 2.0, 4.0, 3.0], [2.5, 2.5, 2.5, 2.5]), needs_two),
        "zero observed mean": (_case([1.0, -0.5, 2.5, -2.0], [1.0, -1.0, 2.0, -2.0]), needs_mean),
        "constant simulation": (_case([3.1, 3.1, 3.1, 3.1], [1.0, 2.0, 4.0, 3.0]), ("r", "kge", "kge12")),
        "zero simulated mean": (_case([1.0, -1.0, 2.0, -2.0], [1.0, 2.0, 4.0, 3.0]), ("kge12",)),
    }
    for name, (st, nan_metrics) in cases.items():
        for metric in METRICS:
            got = population_score(st, metric)
            if metric in nan_metrics:
                assert bool(torch.isnan(got).all()), f"{name}: {metric} = {got.tolist()}, expected NaN"
            else:
                assert bool(torch.isfinite(got).all()), f"{name}: {metric} = {got.tolist()}, expected a number"
    # a non-finite chain (a flow without a transform): every metric
    st = _case([1.0, 2.0, 4.0, 3.0], [1.5, 2.5, 3.0, 3.5])
    for key in ("sse", "s1", "s2", "s3"):
        bad = dict(st)
        bad[key] = torch.full_like(st[key], NAN if key != "s2" else float("inf"))
        for metric in METRICS:
            assert bool(torch.isnan(population_score(bad, metric)).all()), f"{key} non-finite: {metric}"
    # what the search minimises: 1 - score, +inf where there is no score; the squared error itself for 'sse'
    score = torch.tensor([[0.75, NAN], [NAN, -3.0]], dtype=torch.float64)
    for objective in ("nse", "kge", "kge12"):
        assert torch.equal(_objective_cost(score, objective),
                           torch.tensor([[0.25, float("inf")], [float("inf"), 4.0]], dtype=torch.float64))
    assert torch.equal(_objective_cost(score, "sse"),
                       torch.tensor([[0.75, float("inf")], [float("inf"), -3.0]], dtype=torch.float64))


def test_the_calls_are_exported():
    assert hydrodl2_amd.population_stats is population_stats and hydrodl2_amd.population_score is population_score
    assert {"population_stats", "population_score"} <= set(hydrodl2_amd.__all__)
    assert "hbvx_population_stats" in _abi.OPTIONAL_EXPORTS and "hbvx_population_stats" not in _abi.EXPORTS
    assert _abi.POP_TRANSFORMS == {"none": 0, "sqrt": 1, "log": 2}


def test_the_new_refusals_happen_before_anything_runs():
    """No library call is reached and the tensors are host tensors: a call that got as far as the module's forward
    would fail with the package's own 'no CPU path' error instead of the refusal under test."""
    T, B, P = 8, 3, 4
    x = {"x_phy": torch.zeros(T, B, 3)}
    state = torch.get_rng_state()
    hbv = _model(dyn=["parBETA"])
    ny = hbv.learnable_param_count
    p, cand = torch.zeros(T, B, ny), torch.zeros(P, B, ny - 2)
    tgt = torch.rand(T, B, generator=torch.Generator().manual_seed(3)) + 0.5
    neg = tgt.clone()
    neg[2, 1] = -0.25

    def stats(target, **kw):
        return population_stats(hbv, x, p, cand, target, **kw)

    def search(target, **kw):
        return population_search(hbv, x, p, target, objective=kw.pop("objective", "kge"), **kw)

    for fn in (stats, search):
        with pytest.raises(ValueError, match="transform must be one of"):
            fn(tgt, transform="cbrt")
        for bad in (0.0, -1e-3, NAN, float("inf"), torch.tensor([0.1, 0.0, 0.1])):
            with pytest.raises(ValueError, match="eps must be finite and > 0"):
                fn(tgt, transform="log", eps=bad)
        with pytest.raises(ValueError, match="eps must be finite and > 0"):      # checked even where it is not read
            fn(tgt, transform="sqrt", eps=-1.0)
        with pytest.raises(ValueError, match="eps must be a scalar or"):
            fn(tgt, transform="log", eps=torch.ones(B + 1))
        with pytest.raises(ValueError, match="negative target has no square root"):
            fn(neg, transform="sqrt")
        with pytest.raises(ValueError, match="target <= -eps has no logarithm"):
            fn(neg, transform="log", eps=0.25)
        with pytest.raises(ValueError, match="eps must be finite and > 0"):       # the default eps of an all-zero record
            fn(torch.zeros(T, B), transform="log")
        # what population_cost refuses is refused here too, under the caller's name
        with pytest.raises(ValueError, match="target must be"):
            fn(torch.zeros(T - 1, B))
        with pytest.raises(ValueError, match="infinities"):
            fn(torch.full((T, B), float("inf")))
    with pytest.raises(ValueError, match="candidates must be"):
        population_stats(hbv, x, p, torch.zeros(P, B, ny), tgt)
    with pytest.raises(ValueError, match="float32"):
        population_stats(hbv, x, p, cand.double(), tgt)
    with pytest.raises(NotImplementedError, match="HbvAdj.*Newton"):
        population_stats(_model(("hbv_adj", "HbvAdj")), x, torch.zeros(T, B, 12 * 2 + 2), cand, tgt)
    with pytest.raises(ValueError, match="objective must be one of"):
        population_search(hbv, x, p, tgt, objective="r")
    with pytest.raises(ValueError, match="objective must be one of"):
        population_search(hbv, x, p, tgt, objective="mse", transform="log")
    assert torch.equal(torch.get_rng_state(), state)            # nothing ran: no draw was made


def test_a_library_without_the_export_is_named_before_the_primal(host_math_backend):  # noqa: F811
    """The host build of the math header lacks hbvx_population_stats: `population_stats` and a `population_search` that
    goes through it raise the error naming the export before the module ran (no dy_drop draw, no candidate draw)."""
    model = _model(dyn=["parBETA"], dy_drop=0.5)
    T, B = 6, 3
    ny = model.learnable_param_count
    xs, p = {"x_phy": torch.rand(T, B, 3)}, torch.randn(T, B, ny)
    tgt = torch.rand(T, B) + 0.5
    state = torch.get_rng_state()
    for transform in ("none", "log"):
        with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_stats"):
            population_stats(model, xs, p, torch.zeros(2, B, ny - 2), tgt, transform=transform)
    still = _model(dyn=["parBETA"])
    for kw in (dict(objective="kge"), dict(transform="sqrt")):
        with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_stats"):
            population_search(still, xs, p, tgt, **kw)
    assert torch.equal(torch.get_rng_state(), state)


def _stats_args(**kw):
    ps = _abi.PopStats()
    ps.pop = _pop(**{k: kw.pop(k) for k in list(kw) if k in ("n_cand", "t_first", "target", "cost", "route")})
    ps.transform, ps.shift, ps.eps, ps.s1, ps.s2, ps.s3 = _abi.POP_T_NONE, 64, None, 64, 64, 64
    for k, v in kw.items():
        setattr(ps, k, v)
    return ps


def test_the_abi_refuses_bad_arguments_before_any_launch_and_the_layout_matches():
    """Host-side checks (no launch): runs without a GPU on the cross-compiled library."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    assert "hbvx_population_stats" not in lib.missing and hasattr(lib.dll, "hbvx_population_stats")
    assert lib.dll.hbvx_sizeof(11) == C.sizeof(_abi.PopStats) and lib.dll.hbvx_version() == 10
    assert lib.dll.hbvx_sizeof(10) == C.sizeof(_abi.Pop)                        # hbvx_pop keeps its layout
    assert C.sizeof(_abi.PopStats) == C.sizeof(_abi.Pop) + 8 + 5 * 8

    def refused(code, msg, d, ps):
        with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*{msg}"):
            lib.population_stats(d, ps, 0)

    who = "hbvx_population_stats: "
    refused(-1, "desc is NULL", None, _stats_args())
    refused(-4, "abi_version", _desc(abi_version=9), _stats_args())
    refused(-1, who + "ps is NULL", _desc(), None)
    # hbvx_population_cost's checks, under this entry point's name
    refused(-1, who + "target is NULL", _desc(), _stats_args(target=None))
    refused(-1, who + "cost is NULL", _desc(), _stats_args(cost=None))
    for n in (0, -1, 65536):
        refused(-2, who + "n_cand must be in 1..65535", _desc(), _stats_args(n_cand=n))
    for t in (-1, 20, 21):
        refused(-2, who + "t_first outside", _desc(), _stats_args(t_first=t))
    for model, n_param in ((_abi.MODEL_HBVADJ, 12), (_abi.MODEL_HOURLY, 19)):
        d = _desc(model=model, n_param=n_param, ac=64, elev=64)
        for i in range(12, n_param):
            d.p[i].sta, d.p[i].lo, d.p[i].hi = 64, 0.3, 5.0
        refused(-3, who + "HBV 1.0 / 1.1p / 2.0 only", d, _stats_args())
    extra = _stats_args()
    extra.pop.p[12].sta = 64
    refused(-2, who + "candidate values for a parameter slot the model lacks", _desc(), extra)
    r = _route(L=14)
    refused(-2, who + "route L must be min", _desc(), _stats_args(route=C.pointer(r)))
    r = _route(B=4)
    refused(-2, who + "route T / B", _desc(), _stats_args(route=C.pointer(r)))
    r = _route(abi_version=9)
    refused(-4, who + "route abi_version", _desc(), _stats_args(route=C.pointer(r)))
    r = _route(ra=None)
    refused(-1, who + "a routing input", _desc(), _stats_args(route=C.pointer(r)))
    # its own
    for bad in (-1, 3, 17):
        refused(-3, who + "transform must be", _desc(), _stats_args(transform=bad))
    refused(-1, who + "shift is NULL", _desc(), _stats_args(shift=None))
    refused(-1, who + "eps is NULL under HBVX_POP_T_LOG", _desc(), _stats_args(transform=_abi.POP_T_LOG))
    for name in ("s1", "s2", "s3"):
        refused(-1, who + "s1 / s2 / s3 is NULL", _desc(), _stats_args(**{name: None}))
    lib.missing.append("hbvx_population_stats")      # a library built before the export existed
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_stats"):
        lib.population_stats(_desc(), _stats_args(), 0)
