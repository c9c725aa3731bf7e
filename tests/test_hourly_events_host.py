"""CPU tier: the flood-event front end (hydrodl2_amd/hourly_events.py) and the export of include/hbvx_gage_events.h
without a GPU -- `flood_events` on hand-made series, `hourly_event_score` against textbook float64 with its NaN rules,
what `hourly_population_event_stats` and `hourly_routing_search` refuse before the model runs (host tensors), the
observed side of the events, the search loop on a synthetic `evaluate` over a nested-gage topology, the new header's
prototypes against `_abi.GAGE_EVENTS_SIGNATURES` and the entry point's argument checks on the cross-compiled library (no
launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi, hourly_events as he
from hydrodl2_amd.hourly_events import (flood_events, hourly_event_score, hourly_population_event_stats,
                                        hourly_routing_search)

from .test_hourly_population_host import _model, _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_the_calls_are_exported():
    for name in ("flood_events", "hourly_population_event_stats", "hourly_event_score", "hourly_routing_search"):
        assert getattr(hydrodl2_amd, name) is getattr(he, name) and name in hydrodl2_amd.__all__
    names = [row[0] for row in _abi.GAGE_EVENTS_SIGNATURES]
    assert names == ["hbvx_gage_events_sizeof", "hbvx_gage_population_events"]
    assert not set(names) & set(_abi.EXPORTS + _abi.OPTIONAL_EXPORTS)       # a table of its own
    assert not set(names) & {row[0] for row in _abi.GAGE_POP_SIGNATURES}
    assert all(not row[1] for row in _abi.GAGE_EVENTS_SIGNATURES)
    assert _abi.ABI_VERSION == 10 and _abi.GAGE_POP_ABI_VERSION == 1 and _abi.GAGE_EVENTS_ABI_VERSION == 1
    assert callable(_model().population_event_stats)


# ---------------------------------------------------------------------------------------------------------------------
# flood_events
def _events(series, *args, **kw):
    s, f = flood_events(torch.tensor(series, dtype=torch.float32).reshape(len(series), -1), *args, **kw)
    assert s.dtype == torch.int32 and f.dtype == torch.int32 and s.device.type == "cpu" and s.shape == f.shape
    return s.tolist(), f.tolist()


def test_flood_events_on_hand_made_series():
    #         0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15
    y = [1, 2, 9, 2, 1, 1, 7, 1, 1, 9, 1, 1, 1, 8, 1, 1]
    # ties go to the earliest hour: hour 2 before hour 9; windows ascending whatever the order of acceptance
    assert _events(y, 1, 1, 1) == ([[1]], [[3]])
    assert _events(y, 2, 1, 1) == ([[1], [8]], [[3], [10]])
    assert _events(y, 3, 1, 1) == ([[1], [8], [12]], [[3], [10], [14]])
    assert _events(y, 4, 1, 1) == ([[1], [5], [8], [12]], [[3], [7], [10], [14]])
    # overlap rejection: with two hours either side, hour 13's window [11, 15] touches [7, 11] at hour 11 and hour 6's
    # [4, 8] meets both accepted windows.  The hours after them are looked at in the same order, highest first and
    # earliest first: hour 14 is the first whose window, [12, 15] after clipping, is free
    assert _events(y, 4, 2, 2) == ([[0], [7], [12], [-1]], [[4], [11], [15], [-1]])
    s, f = _events(y, 3, 2, 1)
    assert s == [[0], [7], [11]] and f == [[3], [10], [14]]
    # windows are clipped to the record; before and after may differ and may be 0
    assert _events([5, 1, 1, 6], 2, 2, 3) == ([[1], [-1]], [[3], [-1]])
    assert _events([5, 1, 1, 6], 2, 0, 0) == ([[0], [3]], [[0], [3]])
    # fewer events than asked: the padding is trailing
    assert _events([1, 2, 3], 4, 5, 5) == ([[0], [-1], [-1], [-1]], [[2], [-1], [-1], [-1]])
    # min_peak: hours below it are no peaks (an hour AT it is)
    assert _events(y, 4, 1, 1, min_peak=8) == ([[1], [8], [12], [-1]], [[3], [10], [14], [-1]])
    assert _events(y, 2, 1, 1, min_peak=9.5) == ([[-1], [-1]], [[-1], [-1]])


def test_flood_events_with_missing_hours_and_several_gages():
    #          0  1    2  3  4  5  6    7  8
    y = [1, 9, NAN, 1, 5, 1, 1, INF, 1]
    # hour 1's window [0, 2] holds a NaN and hour 7 is not finite: hour 4 is the one event above 2, hour 0 the next one
    assert _events(y, 2, 1, 1, min_peak=2) == ([[3], [-1]], [[5], [-1]])
    assert _events(y, 2, 1, 1) == ([[0], [3]], [[1], [5]])
    assert _events(y, 2, 0, 0) == ([[1], [4]], [[1], [4]])
    assert _events([NAN, NAN], 1, 0, 0) == ([[-1]], [[-1]])
    # gages are independent columns, [T,G,1] is taken like [T,G]
    two = torch.tensor([[1.0, 4.0], [5.0, 1.0], [1.0, 1.0], [1.0, 3.0], [2.0, 1.0]])
    s, f = flood_events(two, 2, 0, 1)
    assert s.tolist() == [[1, 0], [4, 3]] and f.tolist() == [[2, 1], [4, 4]]
    s3, f3 = flood_events(two.unsqueeze(-1).double(), 2, 0, 1)
    assert torch.equal(s3, s) and torch.equal(f3, f)
    again = flood_events(two, 2, 0, 1)
    assert torch.equal(again[0], s) and torch.equal(again[1], f)
    for bad in (dict(n_events=0), dict(before=-1), dict(after=-1), dict(n_events=1.5)):
        kw = dict(n_events=1, before=0, after=0)
        kw.update(bad)
        with pytest.raises(ValueError, match="flood_events"):
            flood_events(two, **kw)
    with pytest.raises(ValueError, match=r"target must be \[T,G\]"):
        flood_events(torch.zeros(5), 1, 0, 0)


def test_the_windows_of_flood_events_pass_the_front_ends_check():
    rng = np.random.default_rng(3)
    y = rng.gamma(2.0, 1.0, size=(300, 4)).astype(np.float32)
    y[40:60, 1] = np.nan
    y[:, 3] = np.nan
    s, f = flood_events(y, 5, 6, 12)
    sd, fd = he._check_events((s, f), 300, 4, torch.device("cpu"))
    assert torch.equal(sd, s) and torch.equal(fd, f)
    assert (s[:, 3] == -1).all() and (s[:, 0] >= 0).all()
    for g in range(3):
        for e in range(5):
            if s[e, g] >= 0:
                assert np.isfinite(y[s[e, g]:f[e, g] + 1, g]).all()


# ---------------------------------------------------------------------------------------------------------------------
# hourly_event_score
def _stats(peak, hour, volume, op, oh, ov, valid):
    t = lambda a, dt: torch.tensor(a, dtype=dt)      # noqa: E731
    return {"events": dict(peak=t(peak, torch.float32), peak_hour=t(hour, torch.int32), volume=t(volume, torch.float32),
                           obs_peak=t(op, torch.float32), obs_peak_hour=t(oh, torch.int32), obs_volume=t(ov, torch.float32),
                           valid=t(valid, torch.bool))}


def test_event_scores_against_textbook_float64():
    rng = np.random.default_rng(11)
    P, E, G = 4, 5, 3
    peak = rng.uniform(1, 9, (P, E, G)).astype(np.float32)
    hour = rng.integers(0, 200, (P, E, G)).astype(np.int32)
    vol = rng.uniform(10, 90, (P, E, G)).astype(np.float32)
    op = rng.uniform(1, 9, (E, G)).astype(np.float32)
    oh = rng.integers(0, 200, (E, G)).astype(np.int32)
    ov = rng.uniform(10, 90, (E, G)).astype(np.float32)
    valid = np.ones((E, G), bool)
    valid[3:, 1] = False                        # gage 1: three valid events
    valid[:, 2] = False                         # gage 2: none
    peak[:, 3:, 1] = np.nan                     # what an invalid slot holds does not matter
    hour[:, 3:, 1] = -1
    st = _stats(peak, hour, vol, op, oh, ov, valid)
    p8, h8, v8 = peak.astype(np.float64), hour.astype(np.float64), vol.astype(np.float64)
    o8, oh8, ov8 = op.astype(np.float64), oh.astype(np.float64), ov.astype(np.float64)
    want = {"peak_error": np.abs(p8 - o8) / o8, "peak_bias": (p8 - o8) / o8, "peak_timing": np.abs(h8 - oh8) / 24.0,
            "volume_error": np.abs(v8 - ov8) / ov8}
    for metric, terms in want.items():
        got = hourly_event_score(st, metric)
        assert got.dtype == torch.float64 and tuple(got.shape) == (P, G)
        for g, n in ((0, 5), (1, 3)):
            np.testing.assert_allclose(got[:, g].numpy(), terms[:, :n, g].mean(1), rtol=1e-14, atol=0)
        assert torch.isnan(got[:, 2]).all()
    assert (hourly_event_score(st, "peak_bias")[:, 0].abs() <= hourly_event_score(st, "peak_error")[:, 0] + 1e-15).all()
    np.testing.assert_allclose(hourly_event_score(st, "peak_timing", timing_scale=1.0)[:, 0].numpy(),
                               np.abs(h8 - oh8)[:, :, 0].mean(1), rtol=1e-14)
    with pytest.raises(ValueError, match="metric must be one of"):
        hourly_event_score(st, "kge")


def test_event_scores_nan_rules():
    one = lambda v: [[[v]]]       # noqa: E731
    base = dict(peak=one(2.0), hour=one(5), volume=one(8.0), op=[[4.0]], oh=[[3]], ov=[[16.0]], valid=[[True]])

    def score(metric, **over):
        return float(hourly_event_score(_stats(**{**base, **over}), metric)[0, 0])

    assert score("peak_error") == 0.5 and score("peak_bias") == -0.5 and score("volume_error") == 0.5
    assert score("peak_timing") == 2.0 / 24.0
    # a denominator that is not positive
    assert np.isnan(score("peak_error", op=[[0.0]])) and np.isnan(score("peak_bias", op=[[-1.0]]))
    assert np.isnan(score("volume_error", ov=[[0.0]])) and score("peak_error", ov=[[0.0]]) == 0.5
    assert np.isnan(float(hourly_event_score(_stats(**base), "peak_timing", timing_scale=0.0)[0, 0]))
    # a candidate without a finite flow in a valid window: NaN under every metric; the other candidate keeps its score
    two = _stats(peak=[[[2.0]], [[-INF]]], hour=[[[5]], [[-1]]], volume=[[[8.0]], [[NAN]]], op=[[4.0]], oh=[[3]], ov=[[16.0]],
                 valid=[[True]])
    for metric in he.EVENT_METRICS:
        got = hourly_event_score(two, metric)
        assert torch.isfinite(got[0, 0]) and torch.isnan(got[1, 0]), metric
    # a NaN volume (a NaN flow inside the window) leaves the peak metrics alone
    assert np.isnan(score("volume_error", volume=one(NAN))) and score("peak_error", volume=one(NAN)) == 0.5
    # no valid event
    assert np.isnan(score("peak_error", valid=[[False]]))


def test_the_observed_side_is_the_slots_rule():
    obs = np.array([[1, 3, 3, NAN, 2, 0, -0.0, 7]], np.float32).T
    starts = np.array([[0], [3], [4], [5], [-1]], np.int32)
    ends = np.array([[2], [4], [4], [6], [-1]], np.int32)
    peak, hour, vol, valid = he._observed_events(obs, starts, ends)
    assert hour[:, 0].tolist() == [1, 4, 4, 5, -1] and peak[:3, 0].tolist() == [3.0, 2.0, 2.0]
    assert peak[3, 0] == 0 and not np.signbit(peak[3, 0]) and np.isneginf(peak[4, 0])
    assert vol[0, 0] == 7.0 and np.isnan(vol[1, 0]) and vol[2, 0] == 2.0 and vol[4, 0] == 0.0
    assert valid[:, 0].tolist() == [True, False, True, True, False]
    assert peak.dtype == np.float32 and hour.dtype == np.int32 and vol.dtype == np.float32


# ---------------------------------------------------------------------------------------------------------------------
# refusals
def test_event_refusals_happen_before_anything_runs():
    """Host tensors and no library selected: a call that got as far as the module's forward would fail with the package's
    own 'no CPU path' error instead of the refusal under test."""
    T, U, G, P = 48, 4, 3, 3
    m, x, params, cand, dcand, n_pair = _problem(T, U, G, P)
    tgt = torch.rand(T, G, generator=torch.Generator().manual_seed(1)) + 0.5
    good = flood_events(tgt, 2, 2, 3)
    state = torch.get_rng_state()

    def stats(events=good, target=tgt, **kw):
        return hourly_population_event_stats(m, x, params, target, events, cand, dcand, **kw)

    i32 = lambda rows: torch.tensor(rows, dtype=torch.int32)        # noqa: E731
    none = [-1, -1, -1]
    # hourly_population_stats' own come first and are its own
    with pytest.raises(ValueError, match="needs candidates, distr_candidates or both"):
        hourly_population_event_stats(m, x, params, tgt, good)
    with pytest.raises(ValueError, match="target holds infinities"):
        stats(target=torch.full((T, G), INF))
    with pytest.raises(ValueError, match="max_candidates must be >= 1"):
        stats(max_candidates=0)
    with pytest.raises(ValueError, match="graph=True"):
        hourly_population_event_stats(_model(dyn=["parBETA"], graph=True), x, params, tgt, good, cand, dcand)
    # the pair itself
    for bad in (None, good[0], (good[0],), (good[0], good[1], good[1])):
        with pytest.raises(ValueError, match=r"events must be the pair \(starts, ends\)"):
            stats(events=bad)
    with pytest.raises(ValueError, match="starts must be an int32 or int64"):
        stats(events=(good[0].float(), good[1]))
    with pytest.raises(ValueError, match="ends must be an int32 or int64"):
        stats(events=(good[0], good[1].tolist()))
    with pytest.raises(ValueError, match="starts must be an int32 or int64"):
        stats(events=(good[0][0], good[1][0]))
    with pytest.raises(ValueError, match="starts is torch.int32 .* ends torch.int64"):
        stats(events=(good[0], good[1].long()))
    with pytest.raises(ValueError, match="starts is .* ends"):
        stats(events=(good[0], good[1][:1]))
    with pytest.raises(ValueError, match="lives on meta"):
        stats(events=(good[0].to("meta"), good[1].to("meta")))
    with pytest.raises(ValueError, match=r"must be \[E,3\]"):
        stats(events=(good[0][:, :2], good[1][:, :2]))
    with pytest.raises(ValueError, match=r"E < 1"):
        stats(events=(good[0][:0], good[1][:0]))
    with pytest.raises(ValueError, match="49 event rows on a record of 48 hours"):
        stats(events=(i32([none] * 49), i32([none] * 49)))
    # the windows
    for s, f in (([[5, 5, 5]], [[4, 9, 9]]), ([[5, 5, 5]], [[9, 9, T]]), ([[5, 5, T]], [[9, 9, T]])):
        with pytest.raises(ValueError, match=f"0 <= start <= end < {T}"):
            stats(events=(i32(s), i32(f)))
    for s, f in (([[5, 5, 5], [9, 20, 20]], [[9, 9, 9], [12, 25, 25]]),         # touching
                 ([[20, 5, 5], [5, 20, 20]], [[25, 9, 9], [9, 25, 25]]),        # descending
                 ([[5, 5, 5], [5, 20, 20]], [[9, 9, 9], [9, 25, 25]])):         # twice the same
        with pytest.raises(ValueError, match="strictly ascending and disjoint"):
            stats(events=(i32(s), i32(f)))
    with pytest.raises(ValueError, match="a present row after an absent one"):
        stats(events=(i32([[5, -1, 5], [20, 20, 20]]), i32([[9, -1, 9], [25, 25, 25]])))
    # event_target
    with pytest.raises(ValueError, match=r"event_target must be \[48,3\]"):
        stats(event_target=tgt[:40])
    with pytest.raises(ValueError, match=r"event_target must be \[T,G\]"):
        stats(event_target=tgt[:, 0])
    with pytest.raises(ValueError, match=r"give the observed HOURLY series as event_target \[48,3\]"):
        stats(target=tgt[:2], periods=24)
    with pytest.raises(ValueError, match=r"event_target must be \[48,3\]"):
        stats(target=tgt[:2], periods=24, event_target=tgt[:2])
    assert torch.equal(torch.get_rng_state(), state)
    # what passes every check reaches the model, and host tensors end there: int64, on the host, a one-hour window at
    # hour 0 and a window ending at T - 1, gages with different counts, a gage without events
    ok = (torch.tensor([[0, 3, -1], [40, -1, -1]]), torch.tensor([[0, 9, -1], [T - 1, -1, -1]]))
    for kw in (dict(events=ok), dict(events=good), dict(events=good, target=tgt[:2], periods=24, event_target=tgt),
               dict(events=good, event_target=tgt.unsqueeze(-1).double())):
        with pytest.raises(Exception) as err:
            stats(**kw)
        assert not isinstance(err.value, ValueError), err.value
    assert callable(m.population_event_stats)
    with pytest.raises(ValueError, match="strictly ascending and disjoint"):
        m.population_event_stats(x, params, tgt, (i32([[5, 5, 5], [5, 20, 20]]), i32([[9, 9, 9], [9, 25, 25]])), cand, dcand)


def test_search_refusals():
    T, U, G, P = 48, 4, 3, 3
    m, x, params, cand, dcand, n_pair = _problem(T, U, G, P, dyn=())
    tgt = torch.rand(T, G, generator=torch.Generator().manual_seed(1)) + 0.5
    good = flood_events(tgt, 2, 2, 3)

    def search(model=m, parameters=params, target=tgt, **kw):
        return hourly_routing_search(model, x, parameters, target, **kw)

    drop = _model(dy_drop=0.3)
    with pytest.raises(ValueError, match="dy_drop > 0"):
        search(model=drop)
    with pytest.raises(ValueError, match="n_candidates must be >= 2"):
        search(n_candidates=1)
    with pytest.raises(ValueError, match="n_rounds must be >= 1"):
        search(n_rounds=0)
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError, match="0 < shrink <= 1"):
            search(shrink=bad)
    for bad in ("rmse", "sse"):
        with pytest.raises(ValueError, match="objective must be one of"):
            search(objective=bad)
    for bad in (-0.1, 1.1, NAN):
        with pytest.raises(ValueError, match=r"event_share must lie in \[0, 1\]"):
            search(event_share=bad, events=good)
    with pytest.raises(ValueError, match="event_share > 0 needs events"):
        search(event_share=0.5)
    with pytest.raises(ValueError, match="event_metric must be one of"):
        search(event_share=0.5, events=good, event_metric="timing")
    with pytest.raises(ValueError, match="event_metric must be one of"):
        search(event_metric="timing")
    with pytest.raises(ValueError, match=rf"parameters\[2\] must be \[{n_pair},3\]"):
        search(parameters=(params[0], params[1], params[2][:-1]))
    # hourly_population_stats' own, and the event checks, before the model runs
    with pytest.raises(ValueError, match="target holds infinities"):
        search(target=torch.full((T, G), INF))
    with pytest.raises(ValueError, match="transform must be one of"):
        search(transform="cube")
    with pytest.raises(ValueError, match="strictly ascending and disjoint"):
        search(event_share=0.5, events=(torch.tensor([[5, 5, 5], [5, 20, 20]]), torch.tensor([[9, 9, 9], [9, 25, 25]])))
    with pytest.raises(ValueError, match="give the observed HOURLY series"):
        search(event_share=0.5, events=good, target=tgt[:2], periods=24)
    # event_share == 0 does not look at the events at all
    with pytest.raises(Exception) as err:
        search(events="not a pair")
    assert not isinstance(err.value, ValueError), err.value


def test_a_library_without_the_export_is_named_before_the_primal(monkeypatch):
    T, U, G, P = 48, 4, 3, 3
    m, x, params, cand, dcand, n_pair = _problem(T, U, G, P)
    tgt = torch.rand(T, G, generator=torch.Generator().manual_seed(1)) + 0.5
    import __graft_entry__ as ge
    from hydrodl2_amd import hourly_population as hp
    lib = _abi.Library(ge.build_hip())
    lib.missing.append("hbvx_gage_population_events")       # a library built before the export existed
    monkeypatch.setattr(hp, "get_library", lambda: lib)
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_gage_population_events"):
        hourly_population_event_stats(m, x, params, tgt, flood_events(tgt, 2, 2, 3), cand, dcand)
    # the parent's call does not ask for it
    with pytest.raises(Exception) as err:
        hydrodl2_amd.hourly_population_stats(m, x, params, tgt, cand, dcand)
    assert "hbvx_gage_population_events" not in str(err.value)


# ---------------------------------------------------------------------------------------------------------------------
# the search loop
PAIR_GAGE = torch.tensor([0, 0, 1, 1, 1, 1, 2, 2, 3, 5])       # gages 1 and 2 nested in a basin; gage 4 has no pair
N_GAGE = 6


def _synthetic(hidden, log=None):
    """cost[c, g]: the squared distance of g's rows to hidden ones; gage 3 is flat (every candidate ties), gage 4 has no
    pair and gage 5 no score: +inf."""
    def evaluate(dcands):
        if log is not None:
            log.append(dcands.clone())
        d = ((dcands.double() - hidden.double()) ** 2).sum(-1)                      # [P,n_pair]
        cost = torch.zeros(dcands.shape[0], N_GAGE, dtype=torch.float64).index_add_(1, PAIR_GAGE, d)
        cost[:, 3] = 0.25
        cost[:, 4:] = INF
        return cost, {"score": 1.0 - cost}
    return evaluate


def test_the_search_loop_on_a_synthetic_evaluate():
    n_pair = int(PAIR_GAGE.numel())
    hidden = torch.rand(n_pair, 3, generator=torch.Generator().manual_seed(5))
    start = torch.rand(n_pair, 3, generator=torch.Generator().manual_seed(6))
    log = []
    gen = torch.Generator().manual_seed(7)
    best, hist = he._routing_search(PAIR_GAGE, start, _synthetic(hidden, log), 16, 5, 0.5, gen, ("score",))
    assert tuple(best.shape) == (n_pair, 3) and best.dtype == torch.float32
    assert tuple(hist["cost"].shape) == (6, N_GAGE) and hist["cost"].dtype == torch.float64
    assert tuple(hist["score"].shape) == (6, N_GAGE) and tuple(hist["best_index"].shape) == (5, N_GAGE)
    # the held rows are candidate 0 of every round, the draws lie in the unit cube and, from round 1 on, in the box
    assert torch.equal(log[0][0], start)
    held = start
    for k, dc in enumerate(log):
        assert tuple(dc.shape) == (16, n_pair, 3) and float(dc.min()) >= 0 and float(dc.max()) <= 1
        assert torch.equal(dc[0], held)
        if k > 0:
            assert float((dc[1:] - held).abs().max()) <= 0.5 ** k / 2 + 1e-6
        # per-gage gather: gage g's pairs come from g's own winner, whatever the other gages chose
        idx = hist["best_index"][k]
        held = torch.stack([dc[idx[PAIR_GAGE[p]], p] for p in range(n_pair)])
    assert torch.equal(best, held)
    assert len({int(i) for i in hist["best_index"][0][:3]}) > 1, "the gages all chose one candidate: nothing is gathered"
    # the cost never rises, and gages 0..2 improve; the flat gage and the +inf gages keep candidate 0 and their start
    c = hist["cost"]
    assert bool((c[1:, :4] <= c[:-1, :4]).all()) and bool((c[-1, :3] < c[0, :3]).all())
    assert bool((hist["best_index"][:, 3:] == 0).all())
    assert bool(torch.isinf(c[:, 4:]).all()) and bool((c[:, 3] == 0.25).all())
    for p in (8, 9):
        assert torch.equal(best[p], start[p])
    assert torch.equal(hist["score"], 1.0 - c)
    # what is returned has the cost the history ends on
    final, _ = _synthetic(hidden)(best.unsqueeze(0))
    assert torch.equal(final[0], c[-1])
    # reproducible under a seeded generator; another seed draws something else
    again, hist2 = he._routing_search(PAIR_GAGE, start, _synthetic(hidden), 16, 5, 0.5, torch.Generator().manual_seed(7),
                                      ("score",))
    assert torch.equal(again, best) and all(torch.equal(hist[k], hist2[k]) for k in hist)
    other, _ = he._routing_search(PAIR_GAGE, start, _synthetic(hidden), 16, 5, 0.5, torch.Generator().manual_seed(8), ("score",))
    assert not torch.equal(other, best)
    # a start outside the unit cube is clipped into it
    wide, _ = he._routing_search(PAIR_GAGE, start * 3 - 1, _synthetic(hidden), 4, 1, 0.5, torch.Generator().manual_seed(7))
    assert float(wide.min()) >= 0 and float(wide.max()) <= 1


def test_a_tie_keeps_the_held_row_and_two_scores_are_kept():
    n_pair = int(PAIR_GAGE.numel())
    start = torch.full((n_pair, 3), 0.5)

    def evaluate(dcands):
        cost = torch.ones(dcands.shape[0], N_GAGE, dtype=torch.float64)
        cost[3, 1] = 0.5                                        # gage 1 alone has a better candidate
        cost[5, 2] = 1.0                                        # a tie with the held row: not taken
        return cost, {"score": 1 - cost, "score_event": cost * 2}

    best, hist = he._routing_search(PAIR_GAGE, start, evaluate, 8, 1, 1.0, torch.Generator().manual_seed(1),
                                    ("score", "score_event"))
    assert hist["best_index"].tolist() == [[0, 3, 0, 0, 0, 0]]
    moved = (best != start).any(1)
    assert moved.tolist() == (PAIR_GAGE == 1).tolist()
    assert hist["score_event"].tolist() == [[2.0] * 6, [2.0, 1.0, 2.0, 2.0, 2.0, 2.0]]
    assert hist["cost"][1].tolist() == [1.0, 0.5, 1.0, 1.0, 1.0, 1.0]


# ---------------------------------------------------------------------------------------------------------------------
# the header, the table and the entry point's own refusals
def _prototypes():
    with open(os.path.join(ROOT, "include", "hbvx_gage_events.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    found = {}
    for ret, name, args in re.findall(r"^(int|uint64_t)\s*(hbvx_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        assert name not in found, name
        found[name] = (ret, [a.strip() for a in " ".join(args.split()).split(",")])
    return found


def test_every_row_of_the_new_table_is_a_prototype_of_the_new_header():
    protos = _prototypes()
    returns = {"int": C.c_int, "uint64_t": C.c_uint64}
    assert sorted(protos) == sorted(row[0] for row in _abi.GAGE_EVENTS_SIGNATURES) and len(protos) == 2
    for name, required, restype, argtypes, layout in _abi.GAGE_EVENTS_SIGNATURES:
        ret, params = protos[name]
        assert len(params) == len(argtypes) and returns[ret] is restype and required is False, name
    assert protos["hbvx_gage_population_events"][1] == ["const hbvx_gage_events *ev", "void *stream"]
    assert _abi.GAGE_EVENTS_SIGNATURES[1][3][0] == C.POINTER(_abi.GageEvents)
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    for name in protos:
        assert name not in lib.missing and hasattr(lib.dll, name), name
    assert lib.dll.hbvx_gage_events_sizeof(0) == C.sizeof(_abi.GageEvents) == 24 + 6 * 8
    assert lib.dll.hbvx_gage_events_sizeof(1) == 0 and lib.dll.hbvx_gage_events_sizeof(-1) == 0
    # the neighbours are what they were
    assert lib.dll.hbvx_gage_pop_sizeof(0) == C.sizeof(_abi.PopRunoff) and lib.dll.hbvx_gage_pop_sizeof(2) == 0
    assert lib.dll.hbvx_version() == 10
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        assert "hbvx_gage_events.h" in f.read()                  # a change to the header rebuilds the library
    with open(os.path.join(ROOT, "include", "hbvx_gage_events.h")) as f:
        assert "#define HBVX_GAGE_EVENTS_ABI_VERSION 1" in f.read()


def _event_args(**kw):
    ev = _abi.GageEvents(abi_version=_abi.GAGE_EVENTS_ABI_VERSION, n_cand=4, T=100, G=3, n_events=5, series=64, start=64,
                         end=64, peak=64, peak_hour=64, volume=64)
    for k, v in kw.items():
        setattr(ev, k, v)
    return ev


def test_the_abi_refuses_bad_arguments_before_any_launch():
    """Host-side checks (no launch): runs without a GPU on the cross-compiled library."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    who = "hbvx_gage_population_events: "

    def refused(code, msg, ev):
        with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*{who}{msg}"):
            lib.gage_population_events(ev, 0)

    refused(-1, "ev is NULL", None)
    for v in (0, 2):
        refused(-4, "ev abi_version mismatch", _event_args(abi_version=v))
    for n in (0, -1, 65536):
        refused(-2, r"n_cand must be in 1\.\.65535", _event_args(n_cand=n))
    for bad in (dict(T=0), dict(G=0), dict(T=-5)):
        refused(-2, "bad T/G", _event_args(**bad))
    for n in (0, -1, 101):
        refused(-2, r"n_events must be in 1\.\.T", _event_args(n_events=n))
    refused(-1, "series is NULL", _event_args(series=None))
    for name in ("start", "end"):
        refused(-1, "start / end is NULL", _event_args(**{name: None}))
    for name in ("peak", "peak_hour", "volume"):
        refused(-1, "peak / peak_hour / volume is NULL", _event_args(**{name: None}))
    lib.missing.append("hbvx_gage_population_events")
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_gage_population_events"):
        lib.gage_population_events(_event_args(), 0)
