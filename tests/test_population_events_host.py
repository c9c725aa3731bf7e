"""CPU tier: `population_event_stats` / `population_event_score` (hydrodl2_amd/population_events.py), the `event_share`
term of `population_search` and the exports of include/hbvx_pop_events.h without a GPU -- what the front end refuses
before the model runs (host tensors), the score against its definitions and NaN rules on hand-made dictionaries, the new
header's prototypes against `_abi.POP_EVENTS_SIGNATURES`, and the entry point's argument checks on the cross-compiled
library (no launch)."""
import ctypes as C
import os
import re

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi, hourly_events, population, population_events
from hydrodl2_amd.hourly_events import flood_events, hourly_event_score
from hydrodl2_amd.population import population_search
from hydrodl2_amd.population_events import population_event_score, population_event_stats

from .test_hbv_adj import host_math_backend  # noqa: F401  (fixture)
from .test_population_host import _desc, _model
from .test_step_math_host import steptest_lib  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_the_calls_are_exported():
    assert hydrodl2_amd.population_event_stats is population_event_stats
    assert hydrodl2_amd.population_event_score is population_event_score
    assert {"population_event_stats", "population_event_score"} <= set(hydrodl2_amd.__all__)
    names = [row[0] for row in _abi.POP_EVENTS_SIGNATURES]
    assert names == ["hbvx_pop_events_sizeof", "hbvx_population_events"]
    assert not set(names) & set(_abi.EXPORTS + _abi.OPTIONAL_EXPORTS) and not set(names) & set(_abi.POPULATION)
    assert all(not row[1] for row in _abi.POP_EVENTS_SIGNATURES)
    assert _abi.ABI_VERSION == 10 and _abi.POP_EVENTS_ABI_VERSION == 1
    # one set of metrics and one set of window rules for the hourly and the daily calls
    assert population_events.EVENT_METRICS is hourly_events.EVENT_METRICS
    assert population_events._check_events is hourly_events._check_events
    assert population_events._observed_events is hourly_events._observed_events
    assert population.METRICS == ("sse", "mse", "nse", "kge", "kge12", "r", "alpha", "beta", "pbias")


def _problem(T=8, B=3, P=4):
    hbv = _model(dyn=["parBETA"])
    ny = hbv.learnable_param_count
    g = torch.Generator().manual_seed(3)
    return (hbv, {"x_phy": torch.zeros(T, B, 3)}, torch.zeros(T, B, ny), torch.zeros(P, B, ny - 2),
            torch.rand(T, B, generator=g) + 0.5)


def test_refusals_happen_before_anything_runs():
    """Host tensors: a call that got as far as the module's forward would fail with the package's own 'no CPU path'
    error instead of the refusal under test."""
    T, B, P = 8, 3, 4
    hbv, x, p, cand, tgt = _problem(T, B, P)
    good = flood_events(tgt, 2, 1, 1)
    state = torch.get_rng_state()

    def stats(model=hbv, pp=p, target=tgt, candidates=cand, events=good, **kw):
        return population_event_stats(model, x, pp, candidates, target, events, **kw)

    # what population_stats refuses
    hourly = hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")({"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}},
                                                                    torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="Hbv_2_hourly"):
        stats(model=hourly)
    hf = {"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}, "train_spatial_chunk_size": 4,
          "simulate_spatial_chunk_size": 4, "simulate_temporal_chunk_size": 4, "train_warmup": 1}
    mts = hydrodl2_amd.load_model("hbv_2_mts", "Hbv_2_mts")({"nmul": 2, "dynamic_params": {"Hbv_2": []}}, hf,
                                                            torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="Hbv_2_mts"):
        stats(model=mts)
    with pytest.raises(NotImplementedError, match="HbvAdj.*Newton"):
        stats(model=_model(("hbv_adj", "HbvAdj")), pp=torch.zeros(T, B, 12 * 2 + 2))
    with pytest.raises(ValueError, match="graph=True"):
        stats(model=_model(graph=True))
    with pytest.raises(ValueError, match="comprout"):
        stats(model=_model(nmul=1, comprout=True), pp=torch.zeros(T, B, 14), candidates=torch.zeros(P, B, 14))
    with pytest.raises(ValueError, match="dynamic parameter"):
        stats(names=["parBETA"])
    with pytest.raises(ValueError, match="target must be"):
        stats(target=tgt[:-1])
    with pytest.raises(ValueError, match="infinities"):
        stats(target=torch.full((T, B), INF))
    w = torch.ones(T, B)
    w[2, 1] = -1e-3
    with pytest.raises(ValueError, match="must not be negative"):
        stats(weights=w)
    with pytest.raises(ValueError, match="candidates must be"):
        stats(candidates=cand[:, :2])
    with pytest.raises(ValueError, match="float32"):
        stats(candidates=cand.double())
    with pytest.raises(ValueError, match="transform must be one of"):
        stats(transform="cube")
    with pytest.raises(ValueError, match="eps must be finite and > 0"):
        stats(transform="log", eps=0.0)
    with pytest.raises(ValueError, match="negative target has no square root"):
        stats(target=-tgt, transform="sqrt")
    # what _check_events refuses, under this call's name
    who = "population_event_stats: "
    s, f = good
    with pytest.raises(ValueError, match=who + r"events must be the pair"):
        stats(events=s)
    with pytest.raises(ValueError, match=who + r"events must be the pair"):
        stats(events=None)
    with pytest.raises(ValueError, match=who + "starts must be an int32 or int64"):
        stats(events=(s.float(), f))
    with pytest.raises(ValueError, match=who + "ends must be an int32 or int64"):
        stats(events=(s, f[0]))
    with pytest.raises(ValueError, match=who + "starts is torch.int32.*ends torch.int64"):
        stats(events=(s, f.long()))
    with pytest.raises(ValueError, match=who + "starts lives on meta"):
        stats(events=(s.to("meta"), f))
    with pytest.raises(ValueError, match=who + rf"starts and ends must be \[E,{B}\]"):
        stats(events=(s[:, :2].contiguous(), f[:, :2].contiguous()))
    with pytest.raises(ValueError, match=who + "no event rows"):
        stats(events=(s[:0], f[:0]))
    with pytest.raises(ValueError, match=who + rf"{T + 1} event rows on a record of {T}"):
        stats(events=(torch.full((T + 1, B), -1, dtype=torch.int32), torch.full((T + 1, B), -1, dtype=torch.int32)))

    def windows(rows):
        return tuple(torch.tensor([[r[i]] * B for r in rows], dtype=torch.int32) for i in (0, 1))

    for rows in ([(2, 1)], [(0, T)], [(T, T)]):
        with pytest.raises(ValueError, match=who + rf"a present window must have 0 <= start <= end < {T}"):
            stats(events=windows(rows))
    with pytest.raises(ValueError, match=who + "a present row after an absent one"):
        stats(events=windows([(-1, -1), (2, 3)]))
    for rows in ([(0, 3), (3, 4)], [(4, 5), (0, 1)]):
        with pytest.raises(ValueError, match=who + ".*strictly ascending and disjoint"):
            stats(events=windows(rows))

    # the search's term
    def search(**kw):
        return population_search(hbv, x, p, tgt, **kw)

    for bad in (-0.1, 1.5, NAN):
        with pytest.raises(ValueError, match=r"event_share must lie in \[0, 1\]"):
            search(objective="kge", events=good, event_share=bad)
    with pytest.raises(ValueError, match="objective 'sse'.*no scale to mix with"):
        search(events=good, event_share=0.3)
    with pytest.raises(ValueError, match="daily streamflow alone"):
        search(objective="kge", events=good, event_share=0.3, aux_target=tgt, aux_key="SWE")
    with pytest.raises(ValueError, match="daily streamflow alone"):
        search(objective="kge", events=good, event_share=0.3, periods=4)
    with pytest.raises(ValueError, match="daily streamflow alone"):
        search(objective="kge", events=good, event_share=0.3, aux_periods=4)
    with pytest.raises(ValueError, match="daily streamflow alone"):
        search(objective="kge", events=good, event_share=0.3, fdc_share=0.2)
    with pytest.raises(ValueError, match="event_metric must be one of"):
        search(objective="kge", events=good, event_share=0.3, event_metric="peak_height")
    with pytest.raises(ValueError, match="event_share > 0 needs events"):
        search(objective="kge", event_share=0.3)
    with pytest.raises(ValueError, match="population_search: a present row after an absent one"):
        search(objective="kge", event_share=0.3, events=windows([(-1, -1), (2, 3)]))
    with pytest.raises(ValueError, match="dy_drop"):
        population_search(_model(dyn=["parBETA"], dy_drop=0.3), x, p, tgt, objective="kge", events=good, event_share=0.3)
    assert torch.equal(torch.get_rng_state(), state)            # nothing ran: no draw was made


def test_a_library_without_the_export_is_named_before_the_primal(host_math_backend, monkeypatch):  # noqa: F811
    """The host build of the math header has none of the population exports: the call names the first one it needs, before
    the module ran.  A library that has hbvx_population_stats and lacks the new one names the new one."""
    model = _model(dyn=["parBETA"], dy_drop=0.5)
    T, B = 6, 3
    ny = model.learnable_param_count
    xs, p, tgt = {"x_phy": torch.rand(T, B, 3)}, torch.randn(T, B, ny), torch.rand(T, B)
    ev = flood_events(tgt, 1, 1, 1)
    plain = model.__class__({"nmul": 2, "dynamic_params": {"Hbv": []}}, torch.device("cpu"))
    state = torch.get_rng_state()
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_stats"):
        population_event_stats(model, xs, p, torch.zeros(2, B, ny - 2), tgt, ev)
    lib = population.get_library()
    monkeypatch.setattr(lib, "missing", [n for n in lib.missing if n != "hbvx_population_stats"])
    assert "hbvx_population_events" in lib.missing
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_events"):
        population_event_stats(model, xs, p, torch.zeros(2, B, ny - 2), tgt, ev)
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_events"):
        population_search(plain, xs, p, tgt, objective="kge", events=ev, event_share=0.5)
    assert torch.equal(torch.get_rng_state(), state)


def test_the_default_search_touches_nothing_new(monkeypatch):
    """With event_share == 0 the search does not reach population_events.py or ops.population_events, whatever `events`
    holds: it goes on to run the module (which host tensors stop), as the search without the arguments does."""
    hbv, x, p, _, tgt = _problem()
    hbv = _model()
    p = torch.zeros(8, 3, hbv.learnable_param_count)

    def never(*a, **kw):
        raise AssertionError("the event path was entered")

    monkeypatch.setattr(population_events, "_event_request", never)
    monkeypatch.setattr(population_events, "_event_run", never)
    monkeypatch.setattr(hydrodl2_amd.ops, "population_events", never)
    for kw in ({}, {"objective": "kge"}, {"objective": "kge", "event_share": 0.0, "events": "not even a pair",
                                          "event_metric": "peak_timing", "timing_scale": 3.0}):
        with pytest.raises(Exception) as e:
            population_search(hbv, x, p, tgt, n_candidates=4, **kw)
        assert not isinstance(e.value, AssertionError), kw
    with pytest.raises(AssertionError, match="the event path was entered"):
        population_search(hbv, x, p, tgt, n_candidates=4, objective="kge", events=flood_events(tgt, 1, 1, 1),
                          event_share=0.5)


# ---- the score -------------------------------------------------------------------------------------------------------

def _stats(when="peak_day"):
    """P = 2 candidates, E = 3 rows, B = 4 basins.  Basin 0: two valid events and an absent row; basin 1: one valid event
    and one that is present but not fully observed; basin 2: none valid; basin 3: a valid event with obs_volume == 0."""
    valid = torch.tensor([[True, True, False, True], [True, False, False, False], [False, False, False, False]])
    obs_peak = torch.tensor([[4.0, 2.0, 1.0, 5.0], [8.0, 3.0, -INF, -INF], [-INF, -INF, -INF, -INF]])
    obs_day = torch.tensor([[3, 5, 2, 7], [10, 9, -1, -1], [-1, -1, -1, -1]], dtype=torch.int32)
    obs_vol = torch.tensor([[10.0, 6.0, 2.0, 0.0], [20.0, 9.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    peak = torch.tensor([[[5.0, 1.0, 1.0, 5.0], [6.0, 9.0, -INF, -INF], [-INF] * 4],
                         [[4.0, 2.0, 1.0, 6.0], [8.0, 3.0, -INF, -INF], [-INF] * 4]])
    day = torch.tensor([[[4, 5, 2, 7], [8, 1, -1, -1], [-1] * 4],
                        [[3, -1, 2, 9], [10, 9, -1, -1], [-1] * 4]], dtype=torch.int32)
    vol = torch.tensor([[[12.0, 3.0, 2.0, 1.0], [15.0, 1.0, 0.0, 0.0], [0.0] * 4],
                        [[10.0, NAN, 2.0, 0.0], [20.0, 9.0, 0.0, 0.0], [0.0] * 4]])
    ev = {"valid": valid, "obs_peak": obs_peak, "obs_" + when: obs_day, "obs_volume": obs_vol, "peak": peak, when: day,
          "volume": vol}
    return {"events": ev}


def test_the_scores_are_their_definitions():
    st = _stats()
    pe = population_event_score(st, "peak_error")
    assert pe.dtype == torch.float64 and tuple(pe.shape) == (2, 4)
    #   basin 0: mean(|5-4|/4, |6-8|/8) = 0.25; basin 1: |1-2|/2 (its second event is not valid); basin 2: no valid event
    assert pe[0].tolist()[:2] == [0.25, 0.5] and torch.isnan(pe[0, 2]) and pe[0, 3] == 0.0
    #   candidate 1 hits every peak; in basin 1 its valid event has peak_day == -1: undefined
    assert pe[1, 0] == 0.0 and torch.isnan(pe[1, 1]) and pe[1, 3] == 0.2
    pb = population_event_score(st, "peak_bias")
    assert pb[0].tolist()[:2] == [0.0, -0.5] and pb[1, 3] == 0.2
    pt = population_event_score(st, "peak_timing")                     # in days by default
    assert pt[0].tolist()[:2] == [1.5, 0.0] and pt[0, 3] == 0.0 and pt[1, 3] == 2.0 and torch.isnan(pt[1, 1])
    assert population_event_score(st, "peak_timing", timing_scale=2.0)[0, 0] == 0.75
    assert torch.isnan(population_event_score(st, "peak_timing", timing_scale=0.0)[:, [0, 1, 3]]).all()
    ve = population_event_score(st, "volume_error")
    assert ve[0, 0] == (0.2 + 0.25) / 2 and ve[0, 1] == 0.5 and torch.isnan(ve[:, 2]).all()
    assert torch.isnan(ve[:, 3]).all()                                  # a valid event with obs_volume == 0: no denominator
    assert ve[1, 0] == 0.0 and torch.isnan(ve[1, 1])
    with pytest.raises(ValueError, match="metric must be one of"):
        population_event_score(st, "kge")
    with pytest.raises(ValueError, match="metric must be one of"):
        population.population_score(st, "peak_error")                  # the moment scores do not learn the new names


def test_the_hourly_score_keeps_its_name_default_and_bits():
    hourly, daily = _stats("peak_hour"), _stats()
    for metric in hourly_events.EVENT_METRICS:
        a = hourly_event_score(hourly, metric, timing_scale=1.0)
        b = population_event_score(daily, metric)
        assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num()), metric
    # the hourly default is a day of hours, the daily one a day
    assert hourly_event_score(hourly, "peak_timing")[0, 0] == 1.5 / 24.0
    assert population_event_score(daily, "peak_timing")[0, 0] == 1.5
    with pytest.raises(KeyError):
        hourly_event_score(daily, "peak_timing")                        # each reads its own keys


# ---- the ABI ---------------------------------------------------------------------------------------------------------

def _prototypes():
    with open(os.path.join(ROOT, "include", "hbvx_pop_events.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    found = {}
    for ret, name, args in re.findall(r"^(int|uint64_t|const char \*)\s*(hbvx_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        assert name not in found, name
        args = " ".join(args.split())
        found[name] = (ret, [] if args == "void" else [a.strip() for a in args.split(",")])
    return found, text


def test_every_row_of_the_new_table_is_a_prototype_of_the_new_header():
    protos, text = _prototypes()
    returns = {"int": C.c_int, "uint64_t": C.c_uint64}
    structs = {"hbvx_pop_events": _abi.PopEvents, "hbvx_desc": _abi.Desc}
    assert sorted(protos) == sorted(row[0] for row in _abi.POP_EVENTS_SIGNATURES) and len(protos) == 2
    for name, required, restype, argtypes, layout in _abi.POP_EVENTS_SIGNATURES:
        ret, params = protos[name]
        assert len(params) == len(argtypes), (name, params)
        assert returns[ret] is restype, name
        assert required is False
        for ptext, ct in zip(params, argtypes):
            named = re.fullmatch(r"const (hbvx_\w+) \*\w+", ptext)
            if named:
                assert ct == C.POINTER(structs[named.group(1)]), (name, ptext)
        if layout is not None:
            assert C.POINTER(layout[1]) in argtypes, name
    assert re.search(r"#define HBVX_POP_EVENTS_ABI_VERSION\s+1\b", text)
    # the struct's fields, in order, are the binding's
    body = re.search(r"typedef struct hbvx_pop_events \{(.*?)\} hbvx_pop_events;", text, flags=re.S).group(1)
    fields = [re.sub(r"^\**", "", part.strip().split()[-1]) for part in body.split(";") if part.strip()]
    assert fields == [f[0] for f in _abi.PopEvents._fields_] == ["abi_version", "n_events", "flow", "start", "end", "peak",
                                                                 "peak_day", "volume"]
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    for name in protos:
        assert name not in lib.missing and hasattr(lib.dll, name), name
    assert lib.dll.hbvx_pop_events_sizeof(0) == C.sizeof(_abi.PopEvents) == 8 + C.sizeof(_abi.PopStats) + 40
    assert lib.dll.hbvx_pop_events_sizeof(1) == 0 and lib.dll.hbvx_pop_events_sizeof(-1) == 0
    assert lib.dll.hbvx_version() == 10
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        assert "hbvx_pop_events.h" in f.read()                   # a change to the header rebuilds the library


def _event_args(**kw):
    pe = _abi.PopEvents(abi_version=_abi.POP_EVENTS_ABI_VERSION, n_events=5, start=64, end=64, peak=64, peak_day=64,
                        volume=64)
    pe.flow.pop.n_cand, pe.flow.pop.t_first, pe.flow.pop.target, pe.flow.pop.cost = 4, 0, 64, 64
    pe.flow.transform, pe.flow.shift, pe.flow.s1, pe.flow.s2, pe.flow.s3 = 0, 64, 64, 64, 64
    for k, v in kw.items():
        obj, names = pe, k.split("__")
        for name in names[:-1]:
            obj = getattr(obj, name)
        setattr(obj, names[-1], v)
    return pe


def test_the_abi_refuses_bad_arguments_before_any_launch():
    """Host-side checks (no launch): runs without a GPU on the cross-compiled library."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    who = "hbvx_population_events: "

    def refused(code, msg, d, pe):
        with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*{msg}"):
            lib.population_events(d, pe, 0)

    refused(-1, "desc is NULL", None, _event_args())
    refused(-4, "abi_version", _desc(abi_version=9), _event_args())
    refused(-1, who + "pe is NULL", _desc(), None)
    for v in (0, 2):
        refused(-4, who + "pe abi_version mismatch", _desc(), _event_args(abi_version=v))
    for n in (0, -1, 21, 2 ** 31 - 1):                          # _desc(): T = 20
        refused(-2, who + r"n_events must be in 1\.\.T - t_first", _desc(), _event_args(n_events=n))
    refused(-2, who + r"n_events must be in 1\.\.T - t_first", _desc(), _event_args(n_events=16, flow__pop__t_first=5))
    refused(-2, who + r"n_events \* B must not exceed 2\^30", _desc(T=2 ** 20, B=2 ** 11), _event_args(n_events=2 ** 20))
    for name in ("start", "end"):
        refused(-1, who + "start / end is NULL", _desc(), _event_args(**{name: None}))
    for name in ("peak", "peak_day", "volume"):
        refused(-1, who + "peak / peak_day / volume is NULL", _desc(), _event_args(**{name: None}))
    for model, n_param in ((_abi.MODEL_HBVADJ, 12), (_abi.MODEL_HOURLY, 19)):
        d = _desc(model=model, n_param=n_param, ac=64, elev=64)
        for i in range(12, n_param):
            d.p[i].sta, d.p[i].lo, d.p[i].hi = 64, 0.3, 5.0
        refused(-3, who + "HBV 1.0 / 1.1p / 2.0 only", d, _event_args())
    # hbvx_population_stats' own, under the new name
    refused(-1, who + "target is NULL", _desc(), _event_args(flow__pop__target=None))
    refused(-1, who + "cost is NULL", _desc(), _event_args(flow__pop__cost=None))
    for n in (0, 65536):
        refused(-2, who + "n_cand must be in 1..65535", _desc(), _event_args(flow__pop__n_cand=n))
    refused(-2, who + "t_first outside", _desc(), _event_args(flow__pop__t_first=20))
    for bad in (-1, 3):
        refused(-3, who + "transform must be", _desc(), _event_args(flow__transform=bad))
    refused(-1, who + "shift is NULL", _desc(), _event_args(flow__shift=None))
    refused(-1, who + "eps is NULL under HBVX_POP_T_LOG", _desc(), _event_args(flow__transform=_abi.POP_T_LOG))
    for name in ("s1", "s2", "s3"):
        refused(-1, who + "s1 / s2 / s3 is NULL", _desc(), _event_args(**{"flow__" + name: None}))
    lib.missing.append("hbvx_population_events")        # a library built before the export existed
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_events"):
        lib.population_events(_desc(), _event_args(), 0)
