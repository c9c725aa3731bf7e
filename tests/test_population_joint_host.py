"""CPU tier: what `population_joint_stats` and `population_search(aux_target=...)` (hydrodl2_amd/population.py) refuse
before anything runs, how the search mixes the two costs, and what hbvx_population_joint (include/hbvx.h) refuses before
any launch -- on host tensors and on the cross-compiled library, no GPU."""
import ctypes as C

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi
from hydrodl2_amd.population import (AUX_KEYS, _mixed_cost, _objective_cost, population_joint_stats, population_score,
                                     population_search)

from .test_hbv_adj import host_math_backend  # noqa: F401  (fixture)
from .test_population_host import _desc, _model, _route
from .test_population_score_host import _stats_args, stats_of
from .test_step_math_host import steptest_lib  # noqa: F401  (fixture)

NAN, INF = float("nan"), float("inf")


def test_the_calls_are_exported():
    assert hydrodl2_amd.population_joint_stats is population_joint_stats
    assert "population_joint_stats" in hydrodl2_amd.__all__
    assert "hbvx_population_joint" in _abi.OPTIONAL_EXPORTS and "hbvx_population_joint" not in _abi.EXPORTS
    # the five series and their hbvx_flux indices (include/hbvx.h: QSIM = 0, Q0, Q1, Q2, AET, SWE)
    assert _abi.POP_AUX_SERIES == {"srflow_no_rout": 1, "ssflow_no_rout": 2, "gwflow_no_rout": 3, "AET_hydro": 4, "SWE": 5}
    assert set(AUX_KEYS) == set(_abi.POP_AUX_SERIES)


def test_the_refusals_happen_before_anything_runs():
    """No library call is reached and the tensors are host tensors: a call that got as far as the module's forward
    would fail with the package's own 'no CPU path' error instead of the refusal under test."""
    T, B, P = 8, 3, 4
    x = {"x_phy": torch.zeros(T, B, 3)}
    state = torch.get_rng_state()
    hbv = _model(dyn=["parBETA"])
    ny = hbv.learnable_param_count
    p, cand = torch.zeros(T, B, ny), torch.zeros(P, B, ny - 2)
    tgt = torch.rand(T, B, generator=torch.Generator().manual_seed(3)) + 0.5
    aux = torch.rand(T, B, generator=torch.Generator().manual_seed(4))
    aux[1::2] = NAN                                                 # a sparse record is the normal case: no refusal for it

    def joint(target=tgt, aux_target=aux, aux_key="AET_hydro", **kw):
        return population_joint_stats(hbv, x, p, cand, target, aux_target, aux_key, **kw)

    def search(target=tgt, aux_target=aux, aux_key="AET_hydro", **kw):
        return population_search(hbv, x, p, target, objective=kw.pop("objective", "kge"), aux_target=aux_target,
                                 aux_key=aux_key, **kw)

    for fn in (joint, search):
        # the aux term's own
        for bad in ("streamflow", "recharge", "capillary", "BFI", "swe", 4):
            with pytest.raises(ValueError, match="aux_key must be one of"):
                fn(aux_key=bad)
        with pytest.raises(ValueError, match="aux_target and aux_key go together"):
            fn(aux_key=None)
        with pytest.raises(ValueError, match="aux_target and aux_key go together"):
            fn(aux_target=None)
        for bad in (torch.zeros(T - 1, B), torch.zeros(T, B + 1), torch.zeros(T, B, 2), torch.zeros(T * B), [[0.0] * B] * T):
            with pytest.raises(ValueError, match="aux_target must be"):
                fn(aux_target=bad)
        fn_ok_shape = torch.zeros(T, B, 1)                          # [T_out,B,1] is a legal shape: the next refusal is the dtype's
        with pytest.raises(ValueError, match="aux_target must be float32 or float64"):
            fn(aux_target=fn_ok_shape.to(torch.int32))
        with pytest.raises(ValueError, match="aux_target must be float32 or float64"):
            fn(aux_target=aux.half())
        with pytest.raises(ValueError, match="aux_target lives on meta"):
            fn(aux_target=torch.zeros(T, B, device="meta"))
        with pytest.raises(ValueError, match="aux_target holds infinities"):
            fn(aux_target=torch.full((T, B), INF))
        for bad in (torch.ones(T - 1, B), torch.ones(T, B, 1)):
            with pytest.raises(ValueError, match="aux_weights must be"):
                fn(aux_weights=bad)
        with pytest.raises(ValueError, match="aux_weights must be float32 or float64"):
            fn(aux_weights=torch.ones(T, B, dtype=torch.int64))
        with pytest.raises(ValueError, match="aux_weights lives on meta"):
            fn(aux_weights=torch.ones(T, B, device="meta"))
        with pytest.raises(ValueError, match="aux_weights must be finite"):
            fn(aux_weights=torch.full((T, B), NAN))
        with pytest.raises(ValueError, match="aux_weights must not be negative"):
            fn(aux_weights=-torch.ones(T, B))
        # what population_stats refuses is refused here too, under the caller's name
        with pytest.raises(ValueError, match="transform must be one of"):
            fn(transform="cbrt")
        with pytest.raises(ValueError, match="eps must be finite and > 0"):
            fn(transform="log", eps=0.0)
        neg = tgt.clone()
        neg[2, 1] = -0.25
        with pytest.raises(ValueError, match="negative target has no square root"):
            fn(target=neg, transform="sqrt")
        with pytest.raises(ValueError, match="target must be"):
            fn(target=torch.zeros(T - 1, B))
        with pytest.raises(ValueError, match="infinities"):
            fn(target=torch.full((T, B), INF))
    with pytest.raises(ValueError, match="candidates must be"):
        population_joint_stats(hbv, x, p, torch.zeros(P, B, ny), tgt, aux, "SWE")
    with pytest.raises(ValueError, match="float32"):
        population_joint_stats(hbv, x, p, cand.double(), tgt, aux, "SWE")
    with pytest.raises(NotImplementedError, match="HbvAdj.*Newton"):
        population_joint_stats(_model(("hbv_adj", "HbvAdj")), x, torch.zeros(T, B, 12 * 2 + 2), cand, tgt, aux, "SWE")
    # the search's own
    for bad in (-0.01, 1.01, NAN, INF):
        with pytest.raises(ValueError, match=r"aux_share must lie in \[0, 1\]"):
            search(aux_share=bad)
    with pytest.raises(ValueError, match="aux_objective must be one of"):
        search(aux_objective="r")
    for objective in ("nse", "kge", "kge12"):
        with pytest.raises(ValueError, match="two scales in one sum"):
            search(objective=objective, aux_objective="sse")
    with pytest.raises(ValueError, match="objective must be one of"):
        search(objective="mse")
    # aux_weights alone is a call without the aux term's two required arguments
    with pytest.raises(ValueError, match="aux_target and aux_key go together"):
        population_search(hbv, x, p, tgt, aux_key="SWE", aux_weights=torch.ones(T, B))
    assert torch.equal(torch.get_rng_state(), state)            # nothing ran: no draw was made


def test_a_library_without_the_export_is_named_before_the_primal(host_math_backend):  # noqa: F811
    """The host build of the math header lacks hbvx_population_joint: both calls raise the error naming the export
    before the module ran (no dy_drop draw, no candidate draw)."""
    model = _model(dyn=["parBETA"], dy_drop=0.5)
    T, B = 6, 3
    ny = model.learnable_param_count
    xs, p = {"x_phy": torch.rand(T, B, 3)}, torch.randn(T, B, ny)
    tgt, aux = torch.rand(T, B) + 0.5, torch.rand(T, B)
    state = torch.get_rng_state()
    for key in AUX_KEYS:
        with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_joint"):
            population_joint_stats(model, xs, p, torch.zeros(2, B, ny - 2), tgt, aux, key)
    still = _model(dyn=["parBETA"])
    for kw in (dict(), dict(objective="kge"), dict(objective="sse", aux_objective="sse"), dict(aux_share=0.0)):
        with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_joint"):
            population_search(still, xs, p, tgt, aux_target=aux, aux_key="SWE", **kw)
    assert torch.equal(torch.get_rng_state(), state)


def test_the_mixed_cost_on_hand_made_stats():
    """`_objective_cost` on each term's own score, then (1 - share) flow + share aux: +inf where either is +inf."""
    g = torch.Generator().manual_seed(11)
    T, B, P = 30, 4, 3
    obs = torch.rand(T, B, generator=g).double() + 0.5
    aobs = 3.0 * torch.rand(T, B, generator=g).double()
    w = torch.ones(T, B).double()
    sim = obs.unsqueeze(0) * (0.8 + 0.4 * torch.rand(P, T, B, generator=g).double())
    asim = aobs.unsqueeze(0) + 0.3 * torch.rand(P, T, B, generator=g).double()
    asim[1, :, 2] = asim[1, 0, 2]                                   # a constant aux series: no correlation, no KGE
    flow, aux = stats_of(sim, obs, w), stats_of(asim, aobs, w)
    nse_f, kge_a = population_score(flow, "nse"), population_score(aux, "kge")
    assert bool(torch.isnan(kge_a[1, 2])) and int(torch.isnan(kge_a).sum()) == 1 and bool(torch.isfinite(nse_f).all())
    cf, ca = _objective_cost(nse_f, "nse"), _objective_cost(kge_a, "kge")
    assert torch.equal(cf, 1.0 - nse_f) and bool(torch.isinf(ca[1, 2]))
    for share in (0.0, 0.25, 0.5, 1.0):
        mixed = _mixed_cost(cf, ca, share)
        want = (1.0 - share) * cf + share * torch.where(torch.isinf(ca), torch.zeros_like(ca), ca)
        want[1, 2] = INF                                            # at every share, 0 and 1 included
        assert torch.equal(mixed, want) and not bool(torch.isnan(mixed).any())
    assert torch.equal(_mixed_cost(cf, ca, 0.0)[0], cf[0]) and torch.equal(_mixed_cost(cf, ca, 1.0)[0], ca[0])
    # 'sse' with 'sse': the squared errors themselves, one scale
    sf, sa = population_score(flow, "sse"), population_score(aux, "sse")
    assert torch.equal(_mixed_cost(_objective_cost(sf, "sse"), _objective_cost(sa, "sse"), 0.5), 0.5 * sf + 0.5 * sa)
    # a flow term without a score costs +inf too
    cf2 = cf.clone()
    cf2[0, 0] = INF
    assert bool(torch.isinf(_mixed_cost(cf2, ca, 1.0)[0, 0])) and bool(torch.isinf(_mixed_cost(cf2, ca, 0.3)[0, 0]))


def _joint_args(**kw):
    pj = _abi.PopJoint()
    flow_keys = ("n_cand", "t_first", "target", "cost", "route", "transform", "shift", "eps", "s1", "s2", "s3")
    pj.flow = _stats_args(**{k: kw.pop(k) for k in list(kw) if k in flow_keys})
    pj.aux_series, pj.aux_target, pj.aux_w, pj.aux_shift = 4, 64, None, 64
    pj.aux_sse, pj.aux_s1, pj.aux_s2, pj.aux_s3, pj.aux_sim = 64, 64, 64, 64, None
    for k, v in kw.items():
        setattr(pj, k, v)
    return pj


def test_the_abi_refuses_bad_arguments_before_any_launch_and_the_layout_matches():
    """Host-side checks (no launch): runs without a GPU on the cross-compiled library."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    assert "hbvx_population_joint" not in lib.missing and hasattr(lib.dll, "hbvx_population_joint")
    assert lib.dll.hbvx_sizeof(12) == C.sizeof(_abi.PopJoint) and lib.dll.hbvx_version() == 10
    assert lib.dll.hbvx_sizeof(11) == C.sizeof(_abi.PopStats)                   # hbvx_pop_stats keeps its layout
    assert lib.dll.hbvx_sizeof(10) == C.sizeof(_abi.Pop)
    assert C.sizeof(_abi.PopJoint) == C.sizeof(_abi.PopStats) + 8 + 8 * 8

    def refused(code, msg, d, pj):
        with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*{msg}"):
            lib.population_joint(d, pj, 0)

    who = "hbvx_population_joint: "
    refused(-1, "desc is NULL", None, _joint_args())
    refused(-4, "abi_version", _desc(abi_version=9), _joint_args())
    refused(-1, who + "pj is NULL", _desc(), None)
    # hbvx_population_cost's and hbvx_population_stats' checks, under this entry point's name
    refused(-1, who + "target is NULL", _desc(), _joint_args(target=None))
    refused(-1, who + "cost is NULL", _desc(), _joint_args(cost=None))
    for n in (0, -1, 65536):
        refused(-2, who + "n_cand must be in 1..65535", _desc(), _joint_args(n_cand=n))
    for t in (-1, 20, 21):
        refused(-2, who + "t_first outside", _desc(), _joint_args(t_first=t))
    for model, n_param in ((_abi.MODEL_HBVADJ, 12), (_abi.MODEL_HOURLY, 19)):
        d = _desc(model=model, n_param=n_param, ac=64, elev=64)
        for i in range(12, n_param):
            d.p[i].sta, d.p[i].lo, d.p[i].hi = 64, 0.3, 5.0
        refused(-3, who + "HBV 1.0 / 1.1p / 2.0 only", d, _joint_args())
    extra = _joint_args()
    extra.flow.pop.p[12].sta = 64
    refused(-2, who + "candidate values for a parameter slot the model lacks", _desc(), extra)
    r = _route(L=14)
    refused(-2, who + "route L must be min", _desc(), _joint_args(route=C.pointer(r)))
    r = _route(ra=None)
    refused(-1, who + "a routing input", _desc(), _joint_args(route=C.pointer(r)))
    for bad in (-1, 3, 17):
        refused(-3, who + "transform must be", _desc(), _joint_args(transform=bad))
    refused(-1, who + "shift is NULL", _desc(), _joint_args(shift=None))
    refused(-1, who + "eps is NULL under HBVX_POP_T_LOG", _desc(), _joint_args(transform=_abi.POP_T_LOG))
    for name in ("s1", "s2", "s3"):
        refused(-1, who + "s1 / s2 / s3 is NULL", _desc(), _joint_args(**{name: None}))
    # its own: the five series and nothing else (0 is the flow term; 6 .. 11 are RECHARGE .. CAPILLARY)
    for bad in (0, 6, 7, 8, 9, 10, 11, 12, -1, 1 << 20):
        refused(-3, who + "aux_series must be", _desc(), _joint_args(aux_series=bad))
    refused(-1, who + "aux_target is NULL", _desc(), _joint_args(aux_target=None))
    refused(-1, who + "aux_shift is NULL", _desc(), _joint_args(aux_shift=None))
    for name in ("aux_sse", "aux_s1", "aux_s2", "aux_s3"):
        refused(-1, who + "aux_sse / aux_s1 / aux_s2 / aux_s3 is NULL", _desc(), _joint_args(**{name: None}))
    lib.missing.append("hbvx_population_joint")      # a library built before the export existed
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_joint"):
        lib.population_joint(_desc(), _joint_args(), 0)
