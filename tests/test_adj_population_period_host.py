"""CPU tier: what `adj_population_period_stats` and the period / aux arguments of `adj_population_search`
(hydrodl2_amd/adj_population.py) refuse before the model runs, the calendar forms, the exports, and -- on the
cross-compiled library, without a launch -- the argument checks of hbvx_adj_population_period (include/hbvx.h).  The
model under test raises if its forward is reached: every refusal here happens before that."""
import ctypes as C
import os

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi
from hydrodl2_amd import adj_population as ap
from hydrodl2_amd import population as pop
from hydrodl2_amd.adj_population import adj_population_period_stats, adj_population_search
from hydrodl2_amd.population import (_calendar, _period_days, population_joint_stats, population_period_stats,
                                     population_search)

from .test_adj_population_host import _desc, _other
from .test_hbv_adj import host_math_backend  # noqa: F401  (fixture)
from .test_population_period_host import _period_args
from .test_step_math_host import steptest_lib  # noqa: F401  (fixture)

NAN, INF = float("nan"), float("inf")
EXPORT = "hbvx_adj_population_period"
STORAGES = ("SNOWPACK", "MELTWATER", "SM", "SUZ", "SLZ")


class Ran(Exception):
    """The model's forward was reached."""


def _adj(**cfg):
    cfg = {"nmul": 2, "dynamic_params": {"HbvAdj": cfg.pop("dyn", [])}, **cfg}
    model = hydrodl2_amd.load_model("hbv_adj", "HbvAdj")(cfg, torch.device("cpu"))

    def forward(*a, **k):
        raise Ran("the model ran")

    model.forward = forward
    model._forward_eager = forward
    return model


def test_the_call_is_exported():
    assert hydrodl2_amd.adj_population_period_stats is adj_population_period_stats
    assert "adj_population_period_stats" in hydrodl2_amd.__all__
    assert EXPORT in _abi.OPTIONAL_EXPORTS and EXPORT not in _abi.EXPORTS
    assert tuple(_abi.ADJ_POP_AUX_SERIES) == STORAGES == ap.AUX_KEYS
    assert list(_abi.ADJ_POP_AUX_SERIES.values()) == [0, 1, 2, 3, 4]        # HBVX_ADJ_AUX_*: the index of the solved state
    assert _abi.POP_NO_AUX not in _abi.ADJ_POP_AUX_SERIES.values()
    cls = hydrodl2_amd.load_model("hbv_adj", "HbvAdj")
    assert callable(cls.population_period_stats) and hasattr(_abi.Library, "adj_population_period")
    root = os.path.dirname(os.path.dirname(os.path.abspath(hydrodl2_amd.__file__)))
    with open(os.path.join(root, "include", "hbvx.h")) as f:
        header = f.read()
    for k, name in enumerate(STORAGES):
        assert f"#define HBVX_ADJ_AUX_{name} {k}\n" in header
    assert "int hbvx_adj_population_period(const hbvx_desc *d, const hbvx_pop_period *pq, void *stream);" in header


def test_the_method_forwards(monkeypatch):
    model, seen = _adj(), []
    monkeypatch.setattr(ap, "adj_population_period_stats", lambda *a: seen.append(a) or "result")
    args = ({"x_phy": 1}, "p", "cands", "tgt", 8, "aux", "SM", 4, ["parFC"], "w", "aw", "sqrt", 0.1, True)
    assert model.population_period_stats(*args) == "result" and seen == [(model,) + args]


def test_the_refusals_happen_before_the_model_runs():
    T, B, P = 8, 3, 4
    x = {"x_phy": torch.zeros(T, B, 3)}
    state = torch.get_rng_state()
    adj = _adj(dyn=["parBETA"])
    ny = adj.learnable_param_count
    p, cand = torch.zeros(T, B, ny), torch.zeros(P, B, ny - 2)
    with pytest.raises(Ran):                                        # the guard works: a forward that is reached raises
        adj({"x_phy": x["x_phy"]}, p)
    K, KA = 2, 4                                                    # blocks of 3 (two days dropped), blocks of 2
    tgt = torch.rand(K, B, generator=torch.Generator().manual_seed(3)) + 0.5
    aux = torch.rand(KA, B, generator=torch.Generator().manual_seed(4))
    aux[1::2] = NAN                                                 # missing periods are no refusal

    def stats(model=adj, target=tgt, periods=3, aux_target=aux, aux_key="SM", aux_periods=2, **kw):
        return adj_population_period_stats(model, x, kw.pop("p", p), kw.pop("candidates", cand), target, periods,
                                           aux_target, aux_key, aux_periods, **kw)

    def method(model=adj, target=tgt, periods=3, aux_target=aux, aux_key="SM", aux_periods=2, **kw):
        return model.population_period_stats(x, kw.pop("p", p), kw.pop("candidates", cand), target, periods, aux_target,
                                             aux_key, aux_periods, **kw)

    def search(model=adj, target=tgt, periods=3, aux_target=aux, aux_key="SM", aux_periods=2, **kw):
        kw.pop("candidates", None)
        return adj_population_search(model, x, kw.pop("p", p), target, objective=kw.pop("objective", "kge"),
                                     aux_target=aux_target, aux_key=aux_key, periods=periods, aux_periods=aux_periods, **kw)

    hbv = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": 2, "dynamic_params": {"Hbv": []}}, torch.device("cpu"))
    for fn in (stats, search):
        # everything adj_population_stats refuses
        with pytest.raises(NotImplementedError, match="is for HbvAdj, not Hbv"):
            fn(model=hbv, p=torch.zeros(T, B, hbv.learnable_param_count))
        with pytest.raises(ValueError, match="graph=True"):
            fn(model=_adj(graph=True))
        with pytest.raises(ValueError, match="newton_stop='global'"):
            fn(model=_adj(newton_stop="global"), candidates=torch.zeros(P, B, ny))
        with pytest.raises(ValueError, match="comprout"):
            fn(model=_adj(comprout=True), candidates=torch.zeros(P, B, ny))
        with pytest.raises(ValueError, match="no static parameter"):
            fn(names=["parNOPE"])
        with pytest.raises(ValueError, match="dynamic parameter"):
            fn(names=["parBETA"])
        with pytest.raises(ValueError, match="routing is off"):
            fn(model=_adj(routing=False), names=["rout_a"])
    for fn in (stats, method, search):
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
        with pytest.raises(ValueError, match=rf"target must be \[1, {B}\]"):
            fn(model=_adj(dyn=["parBETA"], warm_up=3), periods=3)   # T_out = 5: one block of 3
        for bad in (torch.ones(KA + 1, B), torch.ones(T, B), torch.ones(KA, B, 2)):
            with pytest.raises(ValueError, match=rf"aux_target must be \[{KA}, {B}\] or \[{KA}, {B}, 1\]"):
                fn(aux_target=bad)
        for bad in (torch.ones(K + 1, B), torch.ones(T, B), torch.ones(K, B, 1)):
            with pytest.raises(ValueError, match=rf"weights must be \[{K}, {B}\]"):
                fn(weights=bad)
        for bad in (torch.ones(KA - 1, B), torch.ones(T, B)):
            with pytest.raises(ValueError, match=rf"aux_weights must be \[{KA}, {B}\]"):
                fn(aux_weights=bad)
        with pytest.raises(ValueError, match="aux_periods without aux_key"):
            fn(aux_target=None, aux_key=None)
        with pytest.raises(ValueError, match="aux_weights without aux_key"):
            fn(aux_target=None, aux_key=None, aux_periods=None, aux_weights=torch.ones(KA, B))
        # the aux key: the five storages and nothing else -- the explicit models' fluxes are not this kernel's
        for bad in ("AET_hydro", "SWE", "srflow_no_rout", "flow_sim", "sm", 2):
            with pytest.raises(ValueError, match="aux_key must be one of .*SNOWPACK.*MELTWATER.*SM.*SUZ.*SLZ"):
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
    for bad in (torch.zeros(B, ny - 2), torch.zeros(P, B + 1, ny - 2), torch.zeros(P, B, ny), torch.zeros(0, B, ny - 2)):
        with pytest.raises(ValueError, match="candidates must be"):
            stats(candidates=bad)
    with pytest.raises(ValueError, match="float32"):
        stats(candidates=cand.double())
    with pytest.raises(ValueError, match="live on"):
        stats(candidates=cand.to("meta"))
    # the search's own, with the new arguments
    for bad in (-0.01, 1.01, NAN):
        with pytest.raises(ValueError, match=r"aux_share must lie in \[0, 1\]"):
            search(aux_share=bad)
    with pytest.raises(ValueError, match="aux_objective must be one of"):
        search(aux_objective="r")
    with pytest.raises(ValueError, match="two scales in one sum"):
        search(objective="nse", aux_objective="sse")
    with pytest.raises(ValueError, match="objective must be one of"):
        search(objective="mse")
    with pytest.raises(ValueError, match="dy_drop"):
        search(model=_adj(dyn=["parBETA"], dy_drop=0.3))
    # the generic calls keep refusing the model exactly as before
    daily, aux_daily = torch.ones(T, B), torch.ones(T, B)
    for fn in (lambda: population_period_stats(adj, x, p, cand, tgt, 3),
               lambda: population_joint_stats(adj, x, p, cand, daily, aux_daily, "SWE"),
               lambda: population_search(adj, x, p, tgt, periods=3)):
        with pytest.raises(NotImplementedError, match="HbvAdj.*Newton.*adj_population_cost"):
            fn()
    assert torch.equal(torch.get_rng_state(), state)            # nothing ran: no draw was made


def _hbv():
    return hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": 2, "dynamic_params": {"Hbv": []}}, torch.device("cpu"))


# (the model, the period call, the search, an aux key, the family's export prefix)
FAMILIES = {"implicit": (_adj, adj_population_period_stats, adj_population_search, "SLZ", "hbvx_adj_population_"),
            "explicit": (_hbv, population_period_stats, population_search, "SWE", "hbvx_population_")}


@pytest.mark.parametrize("family", FAMILIES)
def test_the_calendar_forms_resolve_as_the_explicit_call_s(monkeypatch, family):
    """None, an int and a sequence of closing days reach the kernel call as the closing days `_calendar` gives, and come
    back as 'period_ends' / 'period_days': the library is stubbed at `_run`, the one route from every front end to the
    kernels, so nothing runs."""
    T, B, P = 20, 3, 2
    make, period_stats, _, aux_key, prefix = FAMILIES[family]
    model = make()
    ny = model.learnable_param_count
    x, p, cand = {"x_phy": torch.zeros(T, B, 3)}, torch.zeros(T, B, ny), torch.zeros(P, B, ny)
    seen = []

    class Lib:
        def require(self, name):
            seen.append(name)

    def run(fam, form, rq):
        assert (fam.prefix, form) == (prefix, "period") and rq.candidates is cand
        return rq.ob, rq.aux_ob, rq.ends

    monkeypatch.setattr(pop, "get_library", lambda: Lib())
    monkeypatch.setattr(pop, "_run", run)
    for periods, aux_periods in ((None, None), (8, None), (None, 8), (8, 5), ([0, 3, 17], [1, 2, 3, 4]),
                                 (torch.tensor([4, 9], dtype=torch.int32), range(0, 20, 7)), ([0], 20)):
        want_f, want_a = _calendar(periods, T, "periods", "t"), _calendar(aux_periods, T, "aux_periods", "t")
        KF, KA = int(want_f.numel()), int(want_a.numel())
        ob, aux_ob, ends = period_stats(model, x, p, cand, torch.ones(KF, B), periods, torch.ones(KA, B, 1), aux_key,
                                        aux_periods)
        assert torch.equal(ends[0], want_f) and torch.equal(ends[1], want_a) and ends[0].dtype == torch.int64
        assert tuple(ob["target"].shape) == (KF, B) and tuple(aux_ob["target"].shape) == (KA, B)
        assert int(_period_days(ends[0]).sum()) == int(want_f[-1]) + 1
        ob, aux_ob, ends = period_stats(model, x, p, cand, torch.ones(KF, B), periods)
        assert torch.equal(ends[0], want_f) and ends[1] is None and aux_ob is None
    assert set(seen) == {prefix + "period"}


def test_a_library_without_the_export_is_named_before_any_draw_or_run(host_math_backend):  # noqa: F811
    """The host build of the math header lacks hbvx_adj_population_period: the calls raise the error naming the export
    before the module ran and before the search drew a candidate."""
    model = _adj(dyn=["parBETA"], dy_drop=0.5)
    T, B = 6, 3
    ny = model.learnable_param_count
    xs, p = {"x_phy": torch.rand(T, B, 3)}, torch.randn(T, B, ny)
    tgt, aux, aux_daily, daily = torch.rand(2, B) + 0.5, torch.rand(3, B), torch.rand(T, B), torch.rand(T, B)
    state = torch.get_rng_state()
    for kw in (dict(), dict(aux_target=aux, aux_key="SM", aux_periods=2), dict(aux_target=aux_daily, aux_key="SNOWPACK")):
        with pytest.raises(_abi.HbvxError, match=f"missing export {EXPORT}"):
            adj_population_period_stats(model, xs, p, torch.zeros(2, B, ny - 2), tgt, 3, **kw)
    still = _adj(dyn=["parBETA"])
    for kw in (dict(periods=3), dict(periods=3, objective="kge"), dict(periods=3, aux_target=aux, aux_key="SM", aux_periods=2),
               dict(target=daily, aux_target=aux_daily, aux_key="SUZ")):
        with pytest.raises(_abi.HbvxError, match=f"missing export {EXPORT}"):
            adj_population_search(still, xs, p, kw.pop("target", tgt), **kw)
    assert torch.equal(torch.get_rng_state(), state)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_search_with_default_arguments_never_reaches_the_new_entry(monkeypatch, family):
    """periods, aux_periods, aux_target, aux_key and aux_weights left at None: every round is one launch of the cost
    export (objective 'sse', transform 'none') or of the stats export (anything else), as before; neither the period nor
    the joint export is reached.  The library is stubbed at `_run`."""
    T, B = 6, 3
    make, _, search, _, prefix = FAMILIES[family]
    model = make()
    ny = model.learnable_param_count
    x, p, tgt = {"x_phy": torch.rand(T, B, 3)}, torch.randn(T, B, ny), torch.rand(T, B) + 0.5
    calls = []

    class Lib:
        def require(self, name):
            calls.append(name)

    def run(fam, form, rq):
        assert fam.prefix == prefix and form in ("cost", "stats"), "the period or the joint entry was reached"
        assert rq.aux_ob is None and rq.ends == (None, None) and not rq.return_series
        calls.append(form)
        n, ob = rq.candidates.shape[0], rq.ob
        if form == "cost":
            return {"cost": torch.arange(n * B, dtype=torch.float32).view(-1, B)}
        z = torch.ones(n, B)
        return {"sse": z * torch.arange(1, n + 1).view(-1, 1), "s1": z * 0, "s2": z, "s3": z, "shift": ob["shift"],
                "obs": ob["obs"], "n_obs": ob["n_obs"]}

    monkeypatch.setattr(pop, "get_library", lambda: Lib())
    monkeypatch.setattr(pop, "_run", run)
    g = torch.Generator().manual_seed(1)
    _, hist = search(model, x, p, tgt, n_candidates=4, n_rounds=2, generator=g)
    assert calls == [prefix + "cost", "cost", "cost"] and set(hist) == {"cost", "best_index", "columns"}
    calls.clear()
    _, hist = search(model, x, p, tgt, n_candidates=4, n_rounds=2, generator=g, objective="nse")
    assert calls == [prefix + "stats", "stats", "stats"] and "score_aux" not in hist


def test_the_abi_refuses_bad_arguments_before_any_launch():
    """Host-side checks (no launch): runs without a GPU on the cross-compiled library.  What hbvx_population_period and
    hbvx_adj_population_stats refuse between them, under this entry point's name."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    assert EXPORT not in lib.missing and hasattr(lib.dll, EXPORT)
    assert lib.dll.hbvx_version() == 10 == _abi.ABI_VERSION                     # an optional export under ABI 10
    assert lib.dll.hbvx_sizeof(13) == C.sizeof(_abi.PopPeriod)                  # the struct is hbvx_population_period's

    def refused(code, msg, d, pq):
        with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*{msg}"):
            lib.adj_population_period(d, pq, 0)

    def args(**kw):
        kw.setdefault("aux_series", 2)
        return _period_args(**kw)

    who = EXPORT + ": "
    refused(-1, "desc is NULL", None, args())
    refused(-4, "abi_version", _desc(abi_version=9), args())
    refused(-1, who + "pq is NULL", _desc(), None)
    # a model that is not HbvAdj, and the Newton policy
    for model, n_param in ((_abi.MODEL_HBV10, 12), (_abi.MODEL_HBV20, 16), (_abi.MODEL_HOURLY, 19)):
        refused(-3, who + "the implicit scheme \\(HBVADJ\\) only", _other(model, n_param), args())
    refused(-3, who + "adj_stop = 1", _desc(adj_stop=1), args())
    for bad in (-1, 3):
        refused(-2, who + "adj_stop must be 0, 1 or 2", _desc(adj_stop=bad), args())
    refused(-3, who + "muwts must be NULL", _desc(muwts=64), args())
    refused(-2, who + "bad Newton policy", _desc(adj_max_iter=65), args())
    refused(-2, who + "bad Newton policy", _desc(adj_gtol=float("nan")), args())
    # the flow term
    refused(-1, who + "target is NULL", _desc(), args(target=None))
    refused(-1, who + "cost is NULL", _desc(), args(cost=None))
    for n in (0, 65536):
        refused(-2, who + "n_cand must be in 1..65535", _desc(), args(n_cand=n))
    for t in (-1, 20):
        refused(-2, who + "t_first outside", _desc(), args(t_first=t))
    for bad in (-1, 3):
        refused(-3, who + "transform must be", _desc(), args(transform=bad))
    refused(-1, who + "shift is NULL", _desc(), args(shift=None))
    refused(-1, who + "eps is NULL under HBVX_POP_T_LOG", _desc(), args(transform=_abi.POP_T_LOG))
    refused(-1, who + "s1 / s2 / s3 is NULL", _desc(), args(s2=None))
    # the aux term: a storage index 0..4 or HBVX_POP_NO_AUX (-1)
    for bad in (5, 6, 11, -2, 1 << 20):
        refused(-3, who + "aux_series must be HBVX_POP_NO_AUX or HBVX_ADJ_AUX_SNOWPACK", _desc(), args(aux_series=bad))
    for ok in range(5):                                             # every storage passes on to the next check
        refused(-1, who + "aux_target is NULL", _desc(), args(aux_series=ok, aux_target=None))
    refused(-1, who + "aux_shift is NULL", _desc(), args(aux_shift=None))
    for name in ("aux_sse", "aux_s1", "aux_s2", "aux_s3"):
        refused(-1, who + "aux_sse / aux_s1 / aux_s2 / aux_s3 is NULL", _desc(), args(**{name: None}))
    # the calendars (T = 20: with t_first = 5 fifteen days are scored)
    refused(-1, who + "flow_end is NULL", _desc(), args(flow_end=None))
    refused(-1, who + "aux_end is NULL", _desc(), args(aux_end=None))
    for n in (0, -1, 21):
        refused(-2, who + "n_flow_periods must be in 1..T - t_first", _desc(), args(n_flow_periods=n))
        refused(-2, who + "n_aux_periods must be in 1..T - t_first", _desc(), args(n_aux_periods=n))
    refused(-2, who + "n_flow_periods must be in", _desc(), args(t_first=5, n_flow_periods=16))
    refused(-2, who + "n_aux_periods must be in", _desc(), args(t_first=5, n_aux_periods=16))
    # without an aux term the aux rules are not applied: the first refusal is the flow's
    none = dict(aux_series=_abi.POP_NO_AUX, aux_target=None, aux_shift=None, aux_sse=None, aux_s1=None, aux_s2=None,
                aux_s3=None, aux_end=None, n_aux_periods=0)
    refused(-1, who + "flow_end is NULL", _desc(), args(flow_end=None, **none))
    refused(-2, who + "n_flow_periods must be in", _desc(), args(n_flow_periods=0, **none))
    # the explicit entry keeps refusing the implicit scheme
    with pytest.raises(_abi.HbvxError, match=r"\(-3\).*hbvx_population_period: HBV 1.0 / 1.1p / 2.0 only"):
        lib.population_period(_desc(), _period_args(), 0)
    lib.missing.append(EXPORT)          # a library built before the export existed
    with pytest.raises(_abi.HbvxError, match=f"missing export {EXPORT}"):
        lib.adj_population_period(_desc(), args(), 0)
