"""CPU tier: every refusal of `population_cost` / `population_search` that happens before a library call
(hydrodl2_amd/population.py), the exports, and -- on the cross-compiled library, without a launch -- the argument
checks of hbvx_population_cost with their messages and the layout of hbvx_pop."""
import ctypes as C

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi
from hydrodl2_amd.population import population_cost, population_search

from .test_hbv_adj import host_math_backend  # noqa: F401  (fixture)
from .test_step_math_host import steptest_lib  # noqa: F401  (fixture)


def _model(name=("hbv", "Hbv"), **cfg):
    cls = name[1]
    cfg = {"nmul": 2, "dynamic_params": {cls: cfg.pop("dyn", [])}, **cfg}
    return hydrodl2_amd.load_model(*name)(cfg, torch.device("cpu"))


def test_the_calls_are_exported():
    assert hydrodl2_amd.population_cost is population_cost and hydrodl2_amd.population_search is population_search
    assert {"population_cost", "population_search"} <= set(hydrodl2_amd.__all__)
    assert "hbvx_population_cost" in _abi.OPTIONAL_EXPORTS


def test_refusals_happen_before_anything_runs():
    """No library is selected here and the tensors are host tensors: a call that got as far as the module's forward
    would fail with the package's own 'no CPU path' error instead of the refusal under test."""
    T, B, P = 8, 3, 4
    x = {"x_phy": torch.zeros(T, B, 3)}
    state = torch.get_rng_state()
    hbv = _model(dyn=["parBETA"])
    ny = hbv.learnable_param_count
    C_all = ny - 2                                   # every column but the dynamic parameter's two
    p, tgt, cand = torch.zeros(T, B, ny), torch.zeros(T, B), torch.zeros(P, B, C_all)

    def cost(model, xd, pp, target, **kw):
        return population_cost(model, xd, pp, kw.pop("candidates", cand), target, **kw)

    def search(model, xd, pp, target, **kw):
        kw.pop("candidates", None)
        return population_search(model, xd, pp, target, **kw)

    for fn in (cost, search):
        hourly = hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")({"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}},
                                                                        torch.device("cpu"))
        with pytest.raises(NotImplementedError, match="Hbv_2_hourly"):
            fn(hourly, x, p, tgt)
        hf = {"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}, "train_spatial_chunk_size": 4,
              "simulate_spatial_chunk_size": 4, "simulate_temporal_chunk_size": 4, "train_warmup": 1}
        mts = hydrodl2_amd.load_model("hbv_2_mts", "Hbv_2_mts")({"nmul": 2, "dynamic_params": {"Hbv_2": []}}, hf,
                                                                torch.device("cpu"))
        with pytest.raises(NotImplementedError, match="Hbv_2_mts"):
            fn(mts, x, p, tgt)
        with pytest.raises(NotImplementedError, match="HbvAdj.*Newton"):
            fn(_model(("hbv_adj", "HbvAdj")), x, torch.zeros(T, B, 12 * 2 + 2), tgt)
        with pytest.raises(ValueError, match="graph=True"):
            fn(_model(graph=True), x, p, tgt)
        init = _model()
        init.initialize = True
        with pytest.raises(ValueError, match="initialize"):
            fn(init, x, p, tgt)
        with pytest.raises(ValueError, match="comprout"):
            fn(_model(nmul=1, comprout=True), x, torch.zeros(T, B, 14), tgt, candidates=torch.zeros(P, B, 14))
        with pytest.raises(ValueError, match="no static parameter"):
            fn(hbv, x, p, tgt, names=["parNOPE"])
        with pytest.raises(ValueError, match="dynamic parameter"):
            fn(hbv, x, p, tgt, names=["parBETA"])
        with pytest.raises(ValueError, match="routing is off"):
            fn(_model(routing=False), x, p, tgt, names=["route_a"])
        for bad in (torch.zeros(T - 1, B), torch.zeros(T, B + 1), torch.zeros(T, B, 2), torch.zeros(B, T)):
            with pytest.raises(ValueError, match="target must be"):
                fn(hbv, x, p, bad)
        with pytest.raises(ValueError, match="target must be"):        # the days after the warm-up
            fn(_model(warm_up=3), x, p, tgt)
        with pytest.raises(ValueError, match="infinities"):
            fn(hbv, x, p, torch.full((T, B), float("inf")))
        w = torch.ones(T, B)
        w[2, 1] = -1e-3
        with pytest.raises(ValueError, match="must not be negative"):
            fn(hbv, x, p, tgt, weights=w)
        w[2, 1] = float("nan")
        with pytest.raises(ValueError, match="weights must be finite"):
            fn(hbv, x, p, tgt, weights=w)
        with pytest.raises(ValueError, match="weights must be"):
            fn(hbv, x, p, tgt, weights=torch.ones(T, B, 1))
    # the candidates: shape (P, basins, the columns of `names`), dtype, device
    for bad in (torch.zeros(B, C_all), torch.zeros(P, B + 1, C_all), torch.zeros(P, B, C_all + 1), torch.zeros(0, B, C_all),
                [[0.0]]):
        with pytest.raises(ValueError, match="candidates must be"):
            population_cost(hbv, x, p, bad, tgt)
    with pytest.raises(ValueError, match="candidates must be"):        # three columns for names of 2 + 2 + 1
        population_cost(hbv, x, p, torch.zeros(P, B, 3), tgt, names=["parFC", "parK1", "route_a"])
    with pytest.raises(ValueError, match="float32"):
        population_cost(hbv, x, p, cand.double(), tgt)
    with pytest.raises(ValueError, match="live on"):
        population_cost(hbv, x, p, cand.to("meta"), tgt)
    # the search's own arguments
    with pytest.raises(ValueError, match="dy_drop"):
        population_search(_model(dyn=["parBETA"], dy_drop=0.3), x, p, tgt)
    with pytest.raises(ValueError, match="n_candidates"):
        population_search(hbv, x, p, tgt, n_candidates=1)
    with pytest.raises(ValueError, match="n_rounds"):
        population_search(hbv, x, p, tgt, n_rounds=0)
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError, match="shrink"):
            population_search(hbv, x, p, tgt, shrink=bad)
    assert torch.equal(torch.get_rng_state(), state)            # nothing ran: no draw was made


def test_a_library_without_the_export_is_named_before_the_primal(host_math_backend):  # noqa: F811
    """The host build of the math header lacks hbvx_population_cost: the operator and `population_cost` raise the error
    naming the export, the latter before the module ran (no dy_drop draw is consumed)."""
    model = _model(dyn=["parBETA"], dy_drop=0.5)
    T, B = 6, 3
    ny = model.learnable_param_count
    xs, p = {"x_phy": torch.rand(T, B, 3)}, torch.randn(T, B, ny)
    state = torch.get_rng_state()
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_cost"):
        population_cost(model, xs, p, torch.zeros(2, B, ny - 2), torch.zeros(T, B))
    assert torch.equal(torch.get_rng_state(), state)


def _desc(**kw):
    """A descriptor that passes check_desc for HBV 1.0 with 12 parameters (pointers are never followed: no launch)."""
    d = _abi.Desc()
    d.abi_version, d.model, d.T, d.B, d.M, d.n_param = _abi.ABI_VERSION, _abi.MODEL_HBV10, 20, 3, 2, 12
    d.ch_prcp, d.ch_tmean, d.ch_pet, d.nearzero, d.x = 0, 1, 2, 1e-5, 64
    bounds = [(1, 6), (50, 1000), (.05, .9), (.01, .5), (.001, .2), (.2, 1), (0, 10), (0, 100), (-2.5, 2.5), (.5, 10),
              (0, .1), (0, .2)]
    for i, (lo, hi) in enumerate(bounds):
        d.p[i].sta, d.p[i].sta_b_stride, d.p[i].lo, d.p[i].hi = 64, 24, lo, hi
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _pop(**kw):
    pop = _abi.Pop()
    pop.n_cand, pop.t_first, pop.target, pop.cost = 4, 0, 64, 64
    for k, v in kw.items():
        setattr(pop, k, v)
    return pop


def _route(**kw):
    r = _abi.RouteDesc(abi_version=_abi.ABI_VERSION, T=20, B=3, S=1, L=15, raw_sigmoid=1, ra=64, rb=64, r_stride=26,
                       a_lo=0, a_hi=2.9, b_lo=0, b_hi=6.5)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_the_abi_refuses_bad_arguments_before_any_launch_and_the_layout_matches():
    """Host-side checks (no launch): runs without a GPU on the cross-compiled library."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    assert "hbvx_population_cost" not in lib.missing and hasattr(lib.dll, "hbvx_population_cost")
    assert lib.dll.hbvx_sizeof(10) == C.sizeof(_abi.Pop) and lib.dll.hbvx_version() == 10

    def refused(code, msg, d, pop):
        with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*{msg}"):
            lib.population_cost(d, pop, 0)

    refused(-1, "desc is NULL", None, _pop())
    refused(-4, "abi_version", _desc(abi_version=9), _pop())
    refused(-1, "pop is NULL", _desc(), None)
    refused(-1, "target is NULL", _desc(), _pop(target=None))
    refused(-1, "cost is NULL", _desc(), _pop(cost=None))
    for n in (0, -1, 65536):
        refused(-2, "n_cand must be in 1..65535", _desc(), _pop(n_cand=n))
    for t in (-1, 20, 21):
        refused(-2, "t_first outside", _desc(), _pop(t_first=t))
    refused(-2, "t_first outside", _desc(T=0), _pop())
    for model, n_param in ((_abi.MODEL_HBVADJ, 12), (_abi.MODEL_HOURLY, 19)):
        d = _desc(model=model, n_param=n_param, ac=64, elev=64)
        for i in range(12, n_param):
            d.p[i].sta, d.p[i].lo, d.p[i].hi = 64, 0.3, 5.0
        refused(-3, "HBV 1.0 / 1.1p / 2.0 only", d, _pop())
    extra = _pop()
    extra.p[12].sta = 64
    refused(-2, "slot the model lacks", _desc(), extra)
    for L in (14, 16, 20):
        r = _route(L=L)
        refused(-2, "route L must be min", _desc(), _pop(route=C.pointer(r)))
    r = _route(L=7)
    refused(-2, "route L must be min", _desc(), _pop(route=C.pointer(r)))      # min(T, 15) = 15 at T = 20 ...
    r7 = _route(L=15, T=7)
    refused(-2, "route L must be min", _desc(T=7), _pop(route=C.pointer(r7)))  # ... and 7 at T = 7
    r = _route(B=4)
    refused(-2, "route T / B", _desc(), _pop(route=C.pointer(r)))
    r = _route(abi_version=9)
    refused(-4, "route abi_version", _desc(), _pop(route=C.pointer(r)))
    r = _route(ra=None)
    refused(-1, "routing input", _desc(), _pop(route=C.pointer(r)))
    lib.missing.append("hbvx_population_cost")      # a library built before the export existed
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_cost"):
        lib.population_cost(_desc(), _pop(), 0)
