"""GPU tier: `population_event_stats` / `population_event_score` / `population_search(event_share=...)`
(hydrodl2_amd/population_events.py) on hbvx_population_events, the event form of k_pop.

The cases are those of tests/test_population_gpu.py (its `Case` / `case`, with the reasons for every shape) under the twin
targets of tests/test_population_stats_gpu.py.  Their lane mappings are the ones that can go wrong here: M = 1, B = 67
(64 basins with 64 different cursors in one wave, and a partly filled second wave), M = 2 and M = 3 (padded member lanes
carry a cursor too), M = 16, B = 5 (lanes of basins beyond B read the last basin's windows and store nothing),
warm_up_states=False (t_first > 0: days are relative), T_out = 7 (L = T) and Hbv_2.

Windows: `flood_events` on the twin target, and hand-made ones (`hand_made`): a window starting on scored day 0, one ending
on T_out - 1, a one-day window, basins of one wave with different numbers of events, a basin with none.

  stats bits    the four chains, n_obs and the series are `population_stats`' bit for bit, under every transform.
  own series    peak, peak_day and volume equal, exactly, `ops.gage_events` on the call's own return_series series with
                the same windows (that kernel's lanes are just columns), and the numpy rule `_observed_events` applied to
                that series per candidate.
  module route  first the per-day equality of `population_cost(return_series=True)` and one module forward per candidate
                (`Case.yardstick`), which tests/test_population_fdc_gpu.py records as zero (MEASURED_SERIES_RDIFF); then
                exact equality of the events with the numpy rule on the module's series.  A card on which the two series
                differ fails the first assertion and names the cause.
  written       through the ops layer: no poison is left in the poison-prefilled outputs at E = 1, at the `flood_events`
                count and with absent rows.
  independence  a slot's bits do not change with E, with rows appended after it, with the other candidates, with
                return_series or with a second call.
  ABI rule      malformed windows (overlap, descending, start < 0 mid-list, end < start, not ahead) through the ops layer,
                indices inside the record only: the result is the host restatement's (tests/hosttest/popevents_host.cpp).
  search        event_share = 0 is the search without the arguments bit for bit; at 0.5 no basin's mixed cost rises and
                history['score_event'] is finite where defined."""
import functools

import numpy as np
import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import ops
from hydrodl2_amd import population_events as pev
from hydrodl2_amd.hourly_events import _observed_events, flood_events
from hydrodl2_amd.population import (EXPLICIT, _candidate_sources, _primal, population_cost, population_score,
                                     population_search, population_stats)
from hydrodl2_amd.population_events import population_event_score, population_event_stats

from . import synth
from .test_popevents_host import load_eventlib
from .test_popevents_host import run as run_host
from .test_population_fdc_gpu import MEASURED_SERIES_RDIFF
from .test_population_gpu import CASES, DEV, bits, case
from .test_population_stats_gpu import TRANSFORMS, twin

KEYS = ("sse", "s1", "s2", "s3")
EV_KEYS = ("peak", "peak_day", "volume")


@functools.lru_cache(maxsize=None)
def flood(name):
    """`flood_events` on the twin target: up to 2 windows of 3 days on the 7-day record, up to 5 of 6 days elsewhere."""
    cs = case(name)
    return flood_events(twin(name), 2, 1, 1) if cs.T_out < 15 else flood_events(twin(name), 5, 2, 3)


@functools.lru_cache(maxsize=None)
def hand_made(name):
    """(starts, ends) [3,B] int32: basin 0 has no event; basin b >= 1 has 1 + (b - 1) % 3 of the windows [0, 1] (starts on
    scored day 0), [3, 3] (one day) and [T_out - 2, T_out - 1] (ends on the last day) -- its first ones when b is odd, its
    last ones when b is even, so that neighbours in a wave differ in count and in days."""
    cs = case(name)
    T = cs.T_out
    rows = [(0, 1), (3, 3), (T - 2, T - 1)]
    starts = torch.full((3, cs.B), -1, dtype=torch.int32)
    ends = torch.full((3, cs.B), -1, dtype=torch.int32)
    for b in range(1, cs.B):
        n = 1 + (b - 1) % 3
        for e, (s, f) in enumerate(rows[:n] if b % 2 else rows[3 - n:]):
            starts[e, b], ends[e, b] = s, f
    return starts, ends


WINDOWS = {"flood": flood, "hand": hand_made}


def ev(name, events, transform="none", cand=None, **kw):
    cs = case(name)
    tgt = twin(name)            # (runs the module when it is first asked for: before prepare(), not after)
    cs.prepare()
    return population_event_stats(cs.model, cs.xd, cs.p, cs.cand if cand is None else cand, tgt, events, cs.names,
                                  cs.weights, transform=transform, **kw)


def through_ops(name, starts, ends, want_sim=True):
    """ops.population_events on the case with ANY [E,B] int32 windows (the Python layer admits well-formed ones only):
    (series [P,T_out,B] or None, peak, peak_day, volume)."""
    cs = case(name)
    tgt = twin(name)
    cs.prepare()
    rq, _ = pev._event_request("through_ops", cs.model, cs.xd, cs.p, cs.cand, tgt, flood(name), cs.names, cs.weights,
                               "none", None)
    _, main, t_first = _primal(EXPLICIT, rq.model, rq.req, rq.x_dict, rq.parameters)
    sources, route = _candidate_sources(rq.model, rq.names, rq.candidates)
    ob = rq.ob
    flow = ops.PopTerm(ob["target"], ob["w"], ob["shift"], ob["eps"], "none")
    flow_out, got = ops.population_events(main, sources, route, flow, starts.to(DEV).contiguous(),
                                          ends.to(DEV).contiguous(), t_first, want_sim)
    return (flow_out[4],) + tuple(got)


def numpy_rule(series, starts, ends):
    """`_observed_events` per candidate on series [P,T_out,B]: (peak, day, volume) [P,E,B] numpy."""
    s, f = starts.cpu().numpy(), ends.cpu().numpy()
    per = [_observed_events(np.ascontiguousarray(y), s, f)[:3] for y in series.cpu().numpy()]
    return tuple(np.stack([p[i] for p in per]) for i in range(3))


def same_as_numpy(e, want, what):
    for key, w in zip(EV_KEYS, want):
        g = e[key].cpu().numpy()
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"{what}: {key}"


@pytest.fixture(scope="module")
def eventlib():
    return load_eventlib()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_the_stats_are_population_stats_bit_for_bit(hip_backend, name):
    assert ops._POISON, "the GPU tier runs with poisoned output buffers"
    cs = case(name)
    tgt = twin(name)
    events = flood(name)
    E = int(events[0].shape[0])
    assert int((events[0] >= 0).sum()) > 0, "flood_events found no window: the case would be empty"
    for transform in TRANSFORMS:
        cs.prepare()
        want = population_stats(cs.model, cs.xd, cs.p, cs.cand, tgt, cs.names, cs.weights, transform=transform,
                                return_series=True)
        got = ev(name, events, transform, return_series=True)
        assert set(got) == set(want) | {"events"}
        for key in KEYS + ("series", "shift"):
            assert got[key].dtype == torch.float32 and torch.equal(bits(got[key]), bits(want[key])), (transform, key)
        assert torch.equal(got["n_obs"], want["n_obs"]) and got["columns"] == want["columns"]
        assert got["transform"] == transform and (got["eps"] is None) == (transform != "log")
        if got["eps"] is not None:
            assert torch.equal(bits(got["eps"]), bits(want["eps"]))
        for k in ("W", "e1", "e2"):
            assert torch.equal(got["obs"][k], want["obs"][k])
        for metric in ("nse", "kge"):
            assert torch.equal(population_score(got, metric), population_score(want, metric))
        plain = ev(name, events, transform)
        assert "series" not in plain and all(torch.equal(bits(plain[k]), bits(want[k])) for k in KEYS)
        e = got["events"]
        assert set(e) == {"start", "end", "peak", "peak_day", "volume", "obs_peak", "obs_peak_day", "obs_volume", "valid"}
        assert tuple(e["peak"].shape) == tuple(e["peak_day"].shape) == tuple(e["volume"].shape) == (cs.P, E, cs.B)
        assert e["peak"].dtype == e["volume"].dtype == torch.float32 and e["peak_day"].dtype == torch.int32
        assert e["start"].dtype == torch.int32 and torch.equal(e["start"].cpu(), events[0])
        assert torch.equal(e["end"].cpu(), events[1])
        for k in ("obs_peak", "obs_peak_day", "obs_volume", "valid"):
            assert tuple(e[k].shape) == (E, cs.B)
        # flood_events takes fully observed windows only: every present event is valid
        assert e["valid"].dtype == torch.bool and torch.equal(e["valid"].cpu(), events[0] >= 0)
        # the events do not move with the transform: they are taken on the flow itself
        if transform == "none":
            first = e
        assert all(torch.equal(bits(e[k]), bits(first[k])) for k in EV_KEYS)
        # the observed half is the numpy rule on the target
        op, od, ov, valid = _observed_events(tgt.cpu().numpy(), events[0].numpy(), events[1].numpy())
        same_as_numpy({"peak": e["obs_peak"], "peak_day": e["obs_peak_day"], "volume": e["obs_volume"]}, (op, od, ov), "obs")
        for metric in pev.EVENT_METRICS:
            sc = population_event_score(got, metric)
            assert tuple(sc.shape) == (cs.P, cs.B) and sc.dtype == torch.float64
            # defined exactly where the docstring says: a valid event, positive denominators, a peak day in each
            valid = e["valid"]
            den = {"peak_timing": torch.ones_like(e["obs_peak"]), "volume_error": e["obs_volume"]}.get(metric, e["obs_peak"])
            defined = valid.any(0) & ~(valid & ~(den > 0)).any(0)
            defined = defined.unsqueeze(0) & ~(valid.unsqueeze(0) & (e["peak_day"] == -1)).any(1)
            assert torch.equal(torch.isfinite(sc), defined) and torch.equal(torch.isnan(sc), ~defined), metric
            assert bool(defined.any()), metric


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(WINDOWS))
@pytest.mark.parametrize("name", list(CASES))
def test_events_against_the_calls_own_series(hip_backend, name, which):
    cs = case(name)
    events = WINDOWS[which](name)
    got = ev(name, events, "sqrt", return_series=True)
    e, series = got["events"], got["series"]
    present = events[0] >= 0
    if which == "hand":
        counts = present.sum(0)
        assert int(counts[0]) == 0 and set(counts[1:].tolist()) <= {1, 2, 3}
        assert len(set(counts[1:min(cs.B, 8)].tolist())) > 1           # neighbours in a wave differ
        assert int(events[0][present].min()) == 0 and int(events[1][present].max()) == cs.T_out - 1
        assert bool((events[0] == events[1])[present].any())            # a one-day window
    # ops.gage_events on the call's own series: lanes are columns there
    pk, dy, vol = ops.gage_events(series.contiguous(), e["start"], e["end"])
    assert torch.equal(bits(e["peak"]), bits(pk)), "peak is not gage_events' on the call's own series"
    assert torch.equal(e["peak_day"], dy), "peak_day is not gage_events' on the call's own series"
    assert torch.equal(bits(e["volume"]), bits(vol)), "volume is not gage_events' on the call's own series"
    # the numpy rule on that series, per candidate
    same_as_numpy(e, numpy_rule(series, *events), "the numpy rule on the call's own series")
    # absent slots: -inf, -1, +0; present ones: a day inside the window, the series' own value on that day
    absent = (~present).unsqueeze(0).expand(cs.P, -1, -1).to(DEV)
    assert bool(torch.isneginf(e["peak"][absent]).all()) and bool((e["peak_day"][absent] == -1).all())
    assert bool((bits(e["volume"][absent]) == 0).all())
    inside = ~absent
    day = e["peak_day"].long()
    assert bool((day[inside] >= e["start"].long().unsqueeze(0).expand_as(day)[inside]).all())
    assert bool((day[inside] <= e["end"].long().unsqueeze(0).expand_as(day)[inside]).all())
    at_day = series.gather(1, day.clamp_min(0))
    assert torch.equal(bits(at_day[inside]), bits(e["peak"][inside]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_events_against_the_module_route(hip_backend, name):
    cs = case(name)
    tgt = twin(name)
    want_series = cs.yardstick[0]                                               # [P,T_out,B], one module forward per candidate
    cs.prepare()
    cost_series = population_cost(cs.model, cs.xd, cs.p, cs.cand, tgt, cs.names, cs.weights, return_series=True)["series"]
    a, b = cost_series.double(), want_series.double()
    assert bool(((a == b) | (b != 0)).all())
    rdiff = float(torch.where(b != 0, (a - b).abs() / b.abs().clamp_min(1e-300), torch.zeros_like(b)).max())
    print(f"{name}: population_cost's series against the module route: worst per-day relative difference {rdiff:.3e} "
          f"(recorded {MEASURED_SERIES_RDIFF:.3e})")
    assert rdiff <= MEASURED_SERIES_RDIFF, "population_cost's series and the module's differ: the events cannot be equal"
    for which, make in WINDOWS.items():
        events = make(name)
        e = ev(name, events)["events"]
        same_as_numpy(e, numpy_rule(want_series, *events), f"{which}: the numpy rule on the module's series")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_every_element_is_written(hip_backend, name):
    assert ops._POISON, "the GPU tier runs with poisoned output buffers"
    cs = case(name)
    fs, ff = flood(name)
    hs, hf = hand_made(name)                # (absent rows: basin 0 has nothing but)
    for label, (s, f) in (("E = 1", (fs[:1], ff[:1])), ("flood_events", (fs, ff)), ("absent rows", (hs, hf)),
                          ("all absent", (torch.full_like(hs, -1), torch.full_like(hf, -1)))):
        _, peak, day, vol = through_ops(name, s, f, want_sim=False)
        E = int(s.shape[0])
        assert tuple(peak.shape) == tuple(day.shape) == tuple(vol.shape) == (cs.P, E, cs.B)
        assert not bool(torch.isnan(peak).any()), f"{label}: a poisoned peak was left"
        assert not bool(torch.isnan(vol).any()), f"{label}: a poisoned volume was left"
        assert bool((day >= -1).all()), f"{label}: a poisoned peak_day was left"
        present = (s >= 0).unsqueeze(0).expand(cs.P, -1, -1).to(DEV)
        assert bool((day[present] >= 0).all()) and bool(torch.isfinite(peak[present]).all())
        assert bool((day[~present] == -1).all()) and bool(torch.isneginf(peak[~present]).all())
        assert bool((bits(vol[~present]) == 0).all())
        assert bool((day[:, :, cs.B - 1] >= -1).all())      # the last basin: in a partly filled wave where B % (64 / Mp) != 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_a_slot_depends_on_its_candidate_and_its_rows_alone(hip_backend, name):
    cs = case(name)
    for which, make in WINDOWS.items():
        s, f = make(name)
        E = int(s.shape[0])
        base = ev(name, (s, f), return_series=True)["events"]

        def same(e, rows, what, cands=slice(None)):
            for key in EV_KEYS:
                assert torch.equal(bits(e[key]), bits(base[key][cands][:, rows])), f"{which}, {what}: other {key} bits"

        same(ev(name, (s, f), return_series=True)["events"], slice(None), "a second call")
        same(ev(name, (s, f))["events"], slice(None), "without return_series")
        same(ev(name, (s.long(), f.long()))["events"], slice(None), "int64 windows")
        same(ev(name, (s.to(DEV), f.to(DEV)))["events"], slice(None), "windows on the device")
        for n in (1, 2):
            if n < E:
                same(ev(name, (s[:n], f[:n]))["events"], slice(0, n), f"the first {n} rows alone (E = {n})")
        if E + 2 <= cs.T_out:
            pad = torch.full((2, cs.B), -1, dtype=torch.int32)
            more = ev(name, (torch.cat([s, pad]), torch.cat([f, pad])))["events"]
            same({k: more[k][:, :E] for k in EV_KEYS}, slice(None), "two rows appended")
        if cs.P > 1:
            perm = list(range(cs.P - 1, -1, -1))
            same(ev(name, (s, f), cand=cs.cand[perm].contiguous())["events"], slice(None), "the candidates permuted", perm)
            c = cs.P - 1
            same(ev(name, (s, f), cand=cs.cand[c:c + 1].contiguous())["events"], slice(None), f"candidate {c} alone", [c])
            # the candidates differ, and so do their events: the candidate index reaches the parameters
            assert not torch.equal(bits(base["volume"][0]), bits(base["volume"][1]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_malformed_windows_follow_the_abi_rule(hip_backend, eventlib, name):
    """Through ops (the Python layer refuses these).  Every index is inside -1 .. T_out - 1: nothing is meant to fault."""
    cs = case(name)
    T = cs.T_out
    assert T >= 7
    patterns = [
        [(1, 3), (2, 4), (4, 4), (6, 6)],           # overlap: row 1 starts inside row 0 -> absent; rows 2, 3 live
        [(4, 5), (2, 3), (0, 1), (6, 6)],           # descending: only rows ahead of the last live one
        [(0, 1), (-1, -1), (-1, 3), (4, 4)],        # start < 0 mid-list, a live row behind it
        [(5, 4), (6, 2), (1, 3), (3, 5)],           # end < start twice; then a row that starts ON the last live day
        [(-1, -1), (-1, 5), (6, 2), (-1, -1)],      # no live row
        [(0, 0), (1, 1), (2, 4), (5, T - 1)],       # adjacent windows are live, the last one ends on the last day
        [(T - 1, T - 1), (0, 0), (T - 1, T - 1), (3, 3)],   # the first row takes the last day: nothing can follow
    ]
    starts = torch.tensor([[patterns[b % len(patterns)][e][0] for b in range(cs.B)] for e in range(4)], dtype=torch.int32)
    ends = torch.tensor([[patterns[b % len(patterns)][e][1] for b in range(cs.B)] for e in range(4)], dtype=torch.int32)
    assert int(starts.min()) >= -1 and int(ends.min()) >= -1 and int(starts.max()) < T and int(ends.max()) < T
    series, peak, day, vol = through_ops(name, starts, ends)
    live = 0
    for p in range(cs.P):
        hp, hd, hv, steps = run_host(eventlib, series[p].cpu().numpy(), starts.numpy(), ends.numpy())
        assert np.array_equal(peak[p].cpu().numpy().view(np.uint32), hp.view(np.uint32)), p
        assert np.array_equal(day[p].cpu().numpy(), hd), p
        assert np.array_equal(vol[p].cpu().numpy().view(np.uint32), hv.view(np.uint32)), p
        assert (steps == 4).all()
        live += int((hd >= 0).sum())
    assert live >= cs.P * min(cs.B, 4)                      # the rule left live rows to compare
    # and the series beside it is population_stats' own
    cs.prepare()
    want = population_stats(cs.model, cs.xd, cs.p, cs.cand, twin(name), cs.names, cs.weights, return_series=True)["series"]
    assert torch.equal(bits(series), bits(want))


@pytest.mark.gpu
def test_population_search_with_an_event_term(hip_backend):
    """The twin problem of tests/test_population_stats_gpu.py::test_population_search_on_kge with a flood-event term."""
    T, B, M = 40, 5, 2
    model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "dynamic_params": {"Hbv": []}}, DEV)
    x = {"x_phy": torch.from_numpy(synth.forcing(T, B, seed=61)).to(DEV)}
    truth = torch.from_numpy(synth.raw_parameters(T, B, model.learnable_param_count, seed=62)).to(DEV)
    with torch.no_grad():
        obs = model(x, truth)["streamflow"][..., 0].clone()
    start = torch.from_numpy(synth.raw_parameters(T, B, model.learnable_param_count, seed=63, scale=1.5)).to(DEV)
    events = flood_events(obs, 3, 2, 3)
    assert bool((events[0] >= 0).any(0).all()), "a basin without an event: its mixed cost would be +inf"
    keep = [t.clone() for t in (start, obs, x["x_phy"], events[0], events[1])]

    def search(seed, **kw):
        g = torch.Generator().manual_seed(seed)
        return population_search(model, x, start, obs, n_candidates=32, n_rounds=3, generator=g, **kw)

    # event_share = 0 is the search without the arguments: bits and history keys
    for kw in ({}, {"objective": "kge"}):
        old, hist_old = search(5, **kw)
        new, hist_new = search(5, events=events, event_share=0.0, event_metric="peak_timing", timing_scale=2.0, **kw)
        assert torch.equal(bits(old), bits(new)) and set(hist_old) == set(hist_new) and "score_event" not in hist_new
        for key in set(hist_old) - {"columns"}:
            assert torch.equal(hist_old[key], hist_new[key]), key

    for metric in ("peak_error", "volume_error", "peak_timing"):
        best, hist = search(5, objective="kge", events=events, event_share=0.5, event_metric=metric)
        assert all(torch.equal(a, b) for a, b in zip((start, obs, x["x_phy"]) + tuple(events), keep)), "an input was modified"
        cost, score, score_event = hist["cost"], hist["score"], hist["score_event"]
        assert tuple(cost.shape) == tuple(score.shape) == tuple(score_event.shape) == (4, B)
        assert cost.dtype == score_event.dtype == torch.float64
        assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(score_event[torch.isfinite(score)]).all())
        assert bool((score_event >= 0).all())
        assert bool(torch.isfinite(cost).all()) and bool((cost[1:] <= cost[:-1]).all()), "a basin's mixed cost rose"
        assert torch.allclose(cost, 0.5 * (1.0 - score) + 0.5 * score_event, rtol=1e-14, atol=0)
        assert bool((cost[-1] < cost[0]).any()), "32 candidates x 3 rounds improved no basin"
        assert torch.equal(hist["best_index"] != 0, cost[1:] < cost[:-1])
        assert tuple(best.shape) == tuple(start.shape) and torch.equal(best[:-1], start[:-1])
        print(f"population_search(kge, event_share 0.5, {metric}): mean KGE {float(score[0].mean()):.4f} -> "
              f"{float(score[-1].mean()):.4f}, mean {metric} {float(score_event[0].mean()):.4f} -> "
              f"{float(score_event[-1].mean()):.4f}")
        # the returned row through the call itself: the history's last scores
        cols = hist["columns"]
        st = population_event_stats(model, x, best, best[-1][:, cols].unsqueeze(0).contiguous(), obs, events)
        assert torch.equal(population_score(st, "kge")[0].cpu(), score[-1])
        assert torch.equal(population_event_score(st, metric)[0].cpu(), score_event[-1])
        again, hist2 = search(5, objective="kge", events=events, event_share=0.5, event_metric=metric)
        assert torch.equal(bits(again), bits(best)) and torch.equal(hist2["cost"], cost)
        assert torch.equal(hist2["score_event"], score_event)
