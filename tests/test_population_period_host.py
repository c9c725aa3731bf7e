"""CPU tier: what `population_period_stats` and `population_search(periods=...)` (hydrodl2_amd/population.py) refuse
before anything runs, the calendar helper, the float64 restatement of the period means that the GPU tier compares
against, and what hbvx_population_period (include/hbvx.h) refuses before any launch -- on host tensors and on the
cross-compiled library, no GPU."""
import ctypes as C

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi
from hydrodl2_amd.population import _calendar, _period_days, population_period_stats, population_search

from .test_hbv_adj import host_math_backend  # noqa: F401  (fixture)
from .test_population_host import _desc, _model
from .test_population_joint_host import _joint_args
from .test_step_math_host import steptest_lib  # noqa: F401  (fixture)

NAN, INF = float("nan"), float("inf")


def period_means64(series: torch.Tensor, ends) -> torch.Tensor:
    """float64 period means of a daily series [..., T_out, B] on the calendar `ends` (closing days, 0-based in the scored
    days): [..., K, B].  Period k covers the days after ends[k-1] up to and including ends[k]."""
    ends = [int(e) for e in ends]
    starts = [0] + [e + 1 for e in ends[:-1]]
    s8 = series.double()
    return torch.stack([s8[..., s:e + 1, :].mean(-2) for s, e in zip(starts, ends)], dim=-2)


def test_the_call_is_exported():
    assert hydrodl2_amd.population_period_stats is population_period_stats
    assert "population_period_stats" in hydrodl2_amd.__all__
    assert "hbvx_population_period" in _abi.OPTIONAL_EXPORTS and "hbvx_population_period" not in _abi.EXPORTS
    assert _abi.POP_NO_AUX == -1 and _abi.POP_NO_AUX not in _abi.POP_AUX_SERIES.values()


def test_the_calendar_helper():
    cal = lambda p, T: _calendar(p, T, "periods", "test").tolist()      # noqa: E731
    assert cal(None, 5) == [0, 1, 2, 3, 4]
    assert cal(1, 5) == [0, 1, 2, 3, 4]
    assert cal(3, 7) == [2, 5]                      # the trailing block of one day is dropped
    assert cal(3, 15) == [2, 5, 8, 11, 14]          # nothing dropped
    assert cal(8, 40) == [7, 15, 23, 31, 39]
    assert cal(7, 7) == [6]
    assert cal([0, 3, 6], 7) == [0, 3, 6] and cal((1,), 7) == [1]
    assert cal(torch.tensor([2, 5], dtype=torch.int32), 7) == [2, 5]
    assert cal(range(1, 7, 2), 7) == [1, 3, 5]
    got = _calendar([30, 58, 89], 90, "periods", "test")
    assert got.dtype == torch.int64 and got.device.type == "cpu"
    assert _period_days(got).tolist() == [31, 28, 31] and _period_days(_calendar(3, 7, "p", "t")).tolist() == [3, 3]
    assert _period_days(_calendar([0, 5, 6], 7, "p", "t")).tolist() == [1, 5, 1]
    for bad in (0, -1, 8):
        with pytest.raises(ValueError, match="days per period"):
            cal(bad, 7)
    for bad in ([], torch.zeros(0, dtype=torch.int64), [[1, 2]], torch.tensor(3)):
        with pytest.raises(ValueError, match="at least one closing day in one dimension"):
            cal(bad, 7)
    for bad in ([1.0, 2.0], torch.tensor([1.0]), [True, False]):
        with pytest.raises(ValueError, match="must hold integers"):
            cal(bad, 7)
    for bad in ([2, 2], [3, 2], [-1, 2], [2, 7], [0, 1, 2, 9]):
        with pytest.raises(ValueError, match="strictly ascending closing days in 0..6"):
            cal(bad, 7)
    for bad in (True, 2.0, "monthly", 3j):
        with pytest.raises(ValueError, match="None, an int or a 1-D sequence"):
            cal(bad, 7)


def test_the_float64_restatement_of_the_period_means():
    g = torch.Generator().manual_seed(5)
    s = torch.rand(2, 11, 3, generator=g)
    ends = [0, 4, 9]                                                  # a one-day period, four days, five days; day 10 dropped
    got = period_means64(s, ends)
    assert got.shape == (2, 3, 3) and got.dtype == torch.float64
    for c in range(2):
        for b in range(3):
            col = [float(x) for x in s[c, :, b]]
            want = [col[0], sum(col[1:5]) / 4, sum(col[5:10]) / 5]
            assert torch.allclose(got[c, :, b], torch.tensor(want, dtype=torch.float64), rtol=1e-15, atol=0)
    assert torch.equal(period_means64(s, range(11)), s.double())          # daily: the series itself
    assert torch.equal(period_means64(s[0], ends), got[0])                # a [T_out,B] series as well


def test_the_refusals_happen_before_anything_runs():
    """No library call is reached and the tensors are host tensors: a call that got as far as the module's forward
    would fail with the package's own 'no CPU path' error instead of the refusal under test."""
    T, B, P = 8, 3, 4
    x = {"x_phy": torch.zeros(T, B, 3)}
    state = torch.get_rng_state()
    hbv = _model(dyn=["parBETA"])
    ny = hbv.learnable_param_count
    p, cand = torch.zeros(T, B, ny), torch.zeros(P, B, ny - 2)
    K, KA = 2, 4                                                    # blocks of 3 (two days dropped), blocks of 2
    tgt = torch.rand(K, B, generator=torch.Generator().manual_seed(3)) + 0.5
    aux = torch.rand(KA, B, generator=torch.Generator().manual_seed(4))
    aux[1::2] = NAN                                                 # missing periods are no refusal

    def stats(target=tgt, periods=3, aux_target=aux, aux_key="AET_hydro", aux_periods=2, **kw):
        return population_period_stats(hbv, x, p, cand, target, periods, aux_target, aux_key, aux_periods, **kw)

    def search(target=tgt, periods=3, aux_target=aux, aux_key="AET_hydro", aux_periods=2, **kw):
        return population_search(hbv, x, p, target, objective=kw.pop("objective", "kge"), aux_target=aux_target,
                                 aux_key=aux_key, periods=periods, aux_periods=aux_periods, **kw)

    for fn in (stats, search):
        # the calendars
        for name in ("periods", "aux_periods"):
            for bad in ([], [[1, 2]]):
                with pytest.raises(ValueError, match=f"{name} must hold at least one closing day"):
                    fn(**{name: bad})
            for bad in ([1.0, 2.0], torch.tensor([2.0, 5.0])):
                with pytest.raises(ValueError, match=f"{name} must hold integers"):
                    fn(**{name: bad})
            for bad in ([2, 2], [5, 2], [-1, 2], [2, T], [2, T + 3]):
                with pytest.raises(ValueError, match=f"{name} must be strictly ascending closing days in 0..{T - 1}"):
                    fn(**{name: bad})
            for bad in (0, -3, T + 1):
                with pytest.raises(ValueError, match=f"{name} = {bad} days per period"):
                    fn(**{name: bad})
            for bad in (True, 2.5, "8D"):
                with pytest.raises(ValueError, match=f"{name} must be None, an int or a 1-D sequence"):
                    fn(**{name: bad})
        # a leading size that is not the calendar's K -- the daily shape included
        for bad in (torch.ones(K + 1, B), torch.ones(T, B), torch.ones(K, B + 1), torch.ones(K, B, 2), [[1.0] * B] * K):
            with pytest.raises(ValueError, match=rf"target must be \[{K}, {B}\] or \[{K}, {B}, 1\]"):
                fn(target=bad)
        with pytest.raises(ValueError, match=rf"target must be \[{T}, {B}\]"):
            fn(periods=None)                                        # daily flow: K = T_out
        for bad in (torch.ones(KA + 1, B), torch.ones(T, B), torch.ones(KA, B, 2)):
            with pytest.raises(ValueError, match=rf"aux_target must be \[{KA}, {B}\] or \[{KA}, {B}, 1\]"):
                fn(aux_target=bad)
        for bad in (torch.ones(K + 1, B), torch.ones(T, B), torch.ones(K, B, 1)):
            with pytest.raises(ValueError, match=rf"weights must be \[{K}, {B}\]"):
                fn(weights=bad)
        for bad in (torch.ones(KA - 1, B), torch.ones(T, B)):
            with pytest.raises(ValueError, match=rf"aux_weights must be \[{KA}, {B}\]"):
                fn(aux_weights=bad)
        # an aux calendar or aux weights without an aux term
        with pytest.raises(ValueError, match="aux_periods without aux_key"):
            fn(aux_target=None, aux_key=None)
        with pytest.raises(ValueError, match="aux_weights without aux_key"):
            fn(aux_target=None, aux_key=None, aux_periods=None, aux_weights=torch.ones(KA, B))
        # population_joint_stats' refusals, under the caller's name
        for bad in ("streamflow", "recharge", "BFI", 4):
            with pytest.raises(ValueError, match="aux_key must be one of"):
                fn(aux_key=bad)
        with pytest.raises(ValueError, match="aux_target and aux_key go together"):
            fn(aux_key=None)
        with pytest.raises(ValueError, match="aux_target and aux_key go together"):
            fn(aux_target=None)
        with pytest.raises(ValueError, match="aux_target must be float32 or float64"):
            fn(aux_target=aux.half())
        with pytest.raises(ValueError, match="aux_target lives on meta"):
            fn(aux_target=torch.zeros(KA, B, device="meta"))
        with pytest.raises(ValueError, match="aux_target holds infinities"):
            fn(aux_target=torch.full((KA, B), INF))
        with pytest.raises(ValueError, match="aux_weights must be finite"):
            fn(aux_weights=torch.full((KA, B), NAN))
        with pytest.raises(ValueError, match="aux_weights must not be negative"):
            fn(aux_weights=-torch.ones(KA, B))
        with pytest.raises(ValueError, match="target must be float32 or float64"):
            fn(target=tgt.half())
        with pytest.raises(ValueError, match="target lives on meta"):
            fn(target=torch.zeros(K, B, device="meta"))
        with pytest.raises(ValueError, match="target holds infinities"):
            fn(target=torch.full((K, B), INF))
        with pytest.raises(ValueError, match="weights must be finite"):
            fn(weights=torch.full((K, B), INF))
        with pytest.raises(ValueError, match="weights must not be negative"):
            fn(weights=-torch.ones(K, B))
        with pytest.raises(ValueError, match="transform must be one of"):
            fn(transform="cbrt")
        with pytest.raises(ValueError, match="eps must be finite and > 0"):
            fn(transform="log", eps=0.0)
        neg = tgt.clone()
        neg[1, 1] = -0.25
        with pytest.raises(ValueError, match="negative target has no square root"):
            fn(target=neg, transform="sqrt")
        with pytest.raises(ValueError, match="has no logarithm"):
            fn(target=neg, transform="log", eps=0.1)
    with pytest.raises(ValueError, match="candidates must be"):
        population_period_stats(hbv, x, p, torch.zeros(P, B, ny), tgt, 3)
    with pytest.raises(ValueError, match="float32"):
        population_period_stats(hbv, x, p, cand.double(), tgt, 3)
    with pytest.raises(ValueError, match="graph=True"):
        population_period_stats(_model(dyn=["parBETA"], graph=True), x, p, cand, tgt, 3)
    with pytest.raises(NotImplementedError, match="HbvAdj.*Newton"):
        population_period_stats(_model(("hbv_adj", "HbvAdj")), x, torch.zeros(T, B, 12 * 2 + 2), cand, tgt, 3)
    hourly = hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")({"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}},
                                                                    torch.device("cpu"))
    hf = {"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}, "train_spatial_chunk_size": 4,
          "simulate_spatial_chunk_size": 4, "simulate_temporal_chunk_size": 4, "train_warmup": 1}
    mts = hydrodl2_amd.load_model("hbv_2_mts", "Hbv_2_mts")({"nmul": 2, "dynamic_params": {"Hbv_2": []}}, hf,
                                                            torch.device("cpu"))
    for other, name in ((hourly, "Hbv_2_hourly"), (mts, "Hbv_2_mts")):
        with pytest.raises(NotImplementedError, match=name):
            population_period_stats(other, x, p, cand, tgt, 3)
        with pytest.raises(NotImplementedError, match=name):
            population_search(other, x, p, tgt, periods=3)
    # the search's own, in period mode
    for bad in (-0.01, 1.01, NAN):
        with pytest.raises(ValueError, match=r"aux_share must lie in \[0, 1\]"):
            search(aux_share=bad)
    with pytest.raises(ValueError, match="aux_objective must be one of"):
        search(aux_objective="r")
    with pytest.raises(ValueError, match="two scales in one sum"):
        search(objective="nse", aux_objective="sse")
    with pytest.raises(ValueError, match="objective must be one of"):
        search(objective="mse")
    assert torch.equal(torch.get_rng_state(), state)            # nothing ran: no draw was made


def test_a_library_without_the_export_is_named_before_the_primal(host_math_backend):  # noqa: F811
    """The host build of the math header lacks hbvx_population_period: both calls raise the error naming the export
    before the module ran (no dy_drop draw, no candidate draw)."""
    model = _model(dyn=["parBETA"], dy_drop=0.5)
    T, B = 6, 3
    ny = model.learnable_param_count
    xs, p = {"x_phy": torch.rand(T, B, 3)}, torch.randn(T, B, ny)
    tgt, aux, aux_daily = torch.rand(2, B) + 0.5, torch.rand(3, B), torch.rand(T, B)
    state = torch.get_rng_state()
    for kw in (dict(), dict(aux_target=aux, aux_key="SWE", aux_periods=2), dict(aux_target=aux_daily, aux_key="SWE")):
        with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_period"):
            population_period_stats(model, xs, p, torch.zeros(2, B, ny - 2), tgt, 3, **kw)
    still = _model(dyn=["parBETA"])
    for kw in (dict(), dict(objective="kge"), dict(aux_target=aux, aux_key="SWE", aux_periods=2)):
        with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_period"):
            population_search(still, xs, p, tgt, periods=3, **kw)
    assert torch.equal(torch.get_rng_state(), state)


def _period_args(**kw):
    pq = _abi.PopPeriod()
    own = {k: kw.pop(k) for k in list(kw) if k in ("n_flow_periods", "flow_end", "n_aux_periods", "aux_end")}
    pq.joint = _joint_args(**kw)
    pq.n_flow_periods, pq.flow_end, pq.n_aux_periods, pq.aux_end = 2, 64, 3, 64
    for k, v in own.items():
        setattr(pq, k, v)
    return pq


def test_the_abi_refuses_bad_arguments_before_any_launch_and_the_layout_matches():
    """Host-side checks (no launch): runs without a GPU on the cross-compiled library."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    assert "hbvx_population_period" not in lib.missing and hasattr(lib.dll, "hbvx_population_period")
    assert lib.dll.hbvx_sizeof(13) == C.sizeof(_abi.PopPeriod) and lib.dll.hbvx_version() == 10
    assert lib.dll.hbvx_sizeof(12) == C.sizeof(_abi.PopJoint)                   # hbvx_pop_joint keeps its layout
    assert C.sizeof(_abi.PopPeriod) == C.sizeof(_abi.PopJoint) + 4 * 8

    def refused(code, msg, d, pq):
        with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*{msg}"):
            lib.population_period(d, pq, 0)

    who = "hbvx_population_period: "
    refused(-1, "desc is NULL", None, _period_args())
    refused(-4, "abi_version", _desc(abi_version=9), _period_args())
    refused(-1, who + "pq is NULL", _desc(), None)
    # everything hbvx_population_joint refuses, under this entry point's name
    refused(-1, who + "target is NULL", _desc(), _period_args(target=None))
    refused(-1, who + "cost is NULL", _desc(), _period_args(cost=None))
    for n in (0, 65536):
        refused(-2, who + "n_cand must be in 1..65535", _desc(), _period_args(n_cand=n))
    for t in (-1, 20):
        refused(-2, who + "t_first outside", _desc(), _period_args(t_first=t))
    for model, n_param in ((_abi.MODEL_HBVADJ, 12), (_abi.MODEL_HOURLY, 19)):
        d = _desc(model=model, n_param=n_param, ac=64, elev=64)
        for i in range(12, n_param):
            d.p[i].sta, d.p[i].lo, d.p[i].hi = 64, 0.3, 5.0
        refused(-3, who + "HBV 1.0 / 1.1p / 2.0 only", d, _period_args())
    for bad in (-1, 3):
        refused(-3, who + "transform must be", _desc(), _period_args(transform=bad))
    refused(-1, who + "shift is NULL", _desc(), _period_args(shift=None))
    refused(-1, who + "eps is NULL under HBVX_POP_T_LOG", _desc(), _period_args(transform=_abi.POP_T_LOG))
    refused(-1, who + "s1 / s2 / s3 is NULL", _desc(), _period_args(s2=None))
    for bad in (0, 6, 11, -2, 1 << 20):                             # (-1 is HBVX_POP_NO_AUX)
        refused(-3, who + "aux_series must be", _desc(), _period_args(aux_series=bad))
    refused(-1, who + "aux_target is NULL", _desc(), _period_args(aux_target=None))
    refused(-1, who + "aux_shift is NULL", _desc(), _period_args(aux_shift=None))
    for name in ("aux_sse", "aux_s1", "aux_s2", "aux_s3"):
        refused(-1, who + "aux_sse / aux_s1 / aux_s2 / aux_s3 is NULL", _desc(), _period_args(**{name: None}))
    # its own: the calendars (T = 20: with t_first = 5 fifteen days are scored)
    refused(-1, who + "flow_end is NULL", _desc(), _period_args(flow_end=None))
    refused(-1, who + "aux_end is NULL", _desc(), _period_args(aux_end=None))
    for n in (0, -1, 21):
        refused(-2, who + "n_flow_periods must be in 1..T - t_first", _desc(), _period_args(n_flow_periods=n))
        refused(-2, who + "n_aux_periods must be in 1..T - t_first", _desc(), _period_args(n_aux_periods=n))
    refused(-2, who + "n_flow_periods must be in", _desc(), _period_args(t_first=5, n_flow_periods=16))
    refused(-2, who + "n_aux_periods must be in", _desc(), _period_args(t_first=5, n_aux_periods=16))
    # without an aux term the flow's rules stay and the aux term's are not applied: the first refusal is the flow's
    none = dict(aux_series=_abi.POP_NO_AUX, aux_target=None, aux_shift=None, aux_sse=None, aux_s1=None, aux_s2=None,
                aux_s3=None, aux_end=None, n_aux_periods=0)
    refused(-1, who + "flow_end is NULL", _desc(), _period_args(flow_end=None, **none))
    refused(-2, who + "n_flow_periods must be in", _desc(), _period_args(n_flow_periods=0, **none))
    lib.missing.append("hbvx_population_period")      # a library built before the export existed
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_period"):
        lib.population_period(_desc(), _period_args(), 0)
