"""GPU tier: the flood-event statistics of the hourly population (hbvx_gage_population_events,
include/hbvx_gage_events.h; `hourly_population_event_stats`, `hourly_routing_search`) on the records 'tiles', 'short' and
'm16_muwts' of tests/test_hourly_population_gpu.py with its P = 5 candidates, and on one synthetic series handed to
`ops.gage_events` directly.

  series only   G = 70 (two gage groups, the second a partial wave), T = 40, no model: every slot against the host
                restatement (tests/hosttest/gageevents_host.cpp) bit for bit, NaN flows and a plateau inside windows, a slot
                with end >= T (clamped), one with end < start and one with start >= T (absent), a gage without events;
  own series    peak and peak_hour equal torch's max and first argmax over the call's own [P,T,G] series exactly, volume
                has the host restatement's bits, the gage without a pair gives peak 0 at its window's first hour, and the
                four sums and the period means have `hourly_population_stats`' bits, hourly and with periods=24 +
                event_target.  The windows are hand-made: one crossing hours 1023/1024, one crossing a multiple of 16, a
                one-hour window, windows [0, ..] and [.., T-1], a gage with zero events, gages with different counts;
  bit rules     two calls agree; a candidate alone or in another order; max_candidates 2 and 1; an event alone; the
                events permuted across slots (ops layer: the front end wants them ascending); return_series on or off;
  module route  against P module forwards with the candidate substituted, windows from `flood_events` on the primal
                streamflow (min_peak above zero: the gage without a pair has no flood).  A max is 1-Lipschitz in the
                series, so |peak - peak_module| <= tol := FLUX_ATOL + FLUX_RTOL |peak_module| (tests/abi_util.py, the
                series' own tolerance); the volume within n_hours x tol (every hour is within the tolerance at its own
                flow, which the peak bounds; the float32 rounding of the sum, <= n_hours 2^-24 of it, is three orders
                below); peak_hour equal wherever the module route's maximum exceeds every other hour of its window by
                more than 2 tol, the others skipped, and at most a quarter may be skipped.  Skipped share measured on an
                MI355X: 0.133 on 'tiles' (8 of 60 slots), 0.050 on 'short' (1 of 20), 0.178 on 'm16_muwts' (8 of 45);
                the peaks and volumes compared were the module route's to 1e-3 of the bound;
  search        'tiles', 8 candidates, 2 rounds, seeded: the history cost never rises, the returned p_distr evaluated by a
                plain `hourly_population_stats` call reproduces history['cost'][-1], stage 1 never launches,
                event_share=0 is the same search with and without `events`, and a search with event_share > 0 keeps both
                scores."""
import functools

import numpy as np
import pytest
import torch

from hydrodl2_amd import ops
from hydrodl2_amd.hourly_events import (flood_events, hourly_event_score, hourly_population_event_stats,
                                        hourly_routing_search)
from hydrodl2_amd.hourly_population import hourly_population_stats
from hydrodl2_amd.population import population_score

from . import abi_util as au
from .test_gage_events_host import load_eventlib
from .test_hourly_population_gpu import (DEV, KEYS, P, bits, call, case, hourly_target, kwargs_of, module_route, observations,
                                         staged)

pytestmark = pytest.mark.gpu

NAMES = ("tiles", "short", "m16_muwts")

@pytest.fixture(scope="module")
def eventlib():
    return load_eventlib()


def same(a, b):
    """torch.equal that takes a NaN for a NaN (an unobserved window's volume, an unobserved gage's score)."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


def host_events(dll, series, starts, ends):
    """(peak, hour, volume) [E,G] of tests/hosttest/gageevents_host.cpp on one candidate's [T,G] series (numpy)."""
    T, G = series.shape
    E = starts.shape[0]
    series = np.ascontiguousarray(series, dtype=np.float32)
    s, f = (np.ascontiguousarray(a, dtype=np.int32) for a in (starts, ends))
    peak, volume = (np.full((E, G), np.nan, np.float32) for _ in range(2))
    hour = np.full((E, G), -7, np.int32)
    assert dll.gageevents_host(T, G, E, series.ctypes.data, s.ctypes.data, f.ctypes.data, peak.ctypes.data, hour.ctypes.data,
                               volume.ctypes.data) == 0
    return peak, hour, volume


def check_against_host(dll, series, starts, ends, peak, hour, volume, what):
    s, f = starts.cpu().numpy(), ends.cpu().numpy()
    for c in range(series.shape[0]):
        wp, wh, wv = host_events(dll, series[c].cpu().numpy(), s, f)
        assert np.array_equal(peak[c].cpu().numpy().view(np.uint32), wp.view(np.uint32)), f"{what}: peak of candidate {c}"
        assert np.array_equal(hour[c].cpu().numpy(), wh), f"{what}: peak_hour of candidate {c}"
        assert np.array_equal(volume[c].cpu().numpy().view(np.uint32), wv.view(np.uint32)), f"{what}: volume of candidate {c}"


def test_a_series_alone_through_the_ops_layer(hip_backend, eventlib):
    assert ops._POISON, "the GPU tier runs with poisoned output buffers"
    Pn, T, G, E = 3, 40, 70, 5
    rng = np.random.default_rng(70)
    series = np.round(rng.gamma(2.0, 1.5, size=(Pn, T, G)) * 4).astype(np.float32) / np.float32(4)     # ties are common
    series[0, 12, :] = np.nan                       # a NaN flow inside windows
    series[1, 20:24, 5] = series[1, 20:24, 5].max() + 1                     # a plateau
    series[2, :, 66] = np.nan                       # a gage of the partial wave without a finite flow
    starts = np.full((E, G), -1, np.int32)
    ends = np.full((E, G), -1, np.int32)
    count = rng.integers(0, E + 1, size=G)          # gages with different counts, some with none
    count[[0, 5, 63, 64, 66, 69]] = E
    count[[1, 65]] = 0
    for g in range(G):
        cuts = np.sort(rng.choice(np.arange(1, T - 1), size=2 * count[g], replace=False)) if count[g] else []
        for e in range(count[g]):
            starts[e, g], ends[e, g] = cuts[2 * e], cuts[2 * e + 1] - 1        # disjoint, ascending; some one hour long
    starts[0, 0], ends[0, 0] = 0, 0                 # the one-hour window at hour 0
    starts[E - 1, 69], ends[E - 1, 69] = ends[E - 2, 69] + 1, T - 1         # a window ending at T - 1 in the last lane
    starts[E - 1, 64], ends[E - 1, 64] = ends[E - 2, 64] + 1, T + 25        # end >= T: clamped to T - 1
    starts[E - 1, 63], ends[E - 1, 63] = 30, 29                             # end < start: absent
    starts[:, 5], ends[:, 5] = [2, 10, 18, 30, T], [5, 14, 26, 33, T + 3]   # the plateau's window; a start past the record: absent
    st, en, ser = (torch.from_numpy(a).to(DEV) for a in (starts, ends, series))
    peak, hour, volume = ops.gage_events(ser, st, en)
    torch.cuda.synchronize()
    assert tuple(peak.shape) == (Pn, E, G) and peak.dtype == torch.float32 and hour.dtype == torch.int32
    assert int((hour < -1).sum()) == 0, "a slot was not written"
    check_against_host(eventlib, ser, st, en, peak, hour, volume, "series only")
    for e, g in ((E - 1, 63), (E - 1, 5), (0, 1), (2, 65)):                 # the absent rule
        assert bool(torch.isneginf(peak[:, e, g]).all()) and bool((hour[:, e, g] == -1).all())
        assert bool((volume[:, e, g] == 0).all()) and not bool(torch.signbit(volume[:, e, g]).any())
    s64 = int(starts[E - 1, 64])                                            # the clamp
    assert torch.equal(peak[1:, E - 1, 64], ser[1:, s64:, 64].max(1).values)
    assert int((hour[1, :, 5] != -1).sum()) == E - 1 and int(hour[1, 2, 5]) == 20              # the plateau's first hour
    assert bool((hour[2, :, 66] == -1).all()) and bool(torch.isnan(volume[2, :count[66], 66]).all())
    assert bool((hour[:, 0, 0] == 0).all()) and torch.equal(bits(peak[:, 0, 0]), bits(ser[:, 0, 0]))
    # bit rules at the ops layer: twice, a candidate alone, an event alone, the events permuted across slots
    again = ops.gage_events(ser, st, en)
    alone = ops.gage_events(ser[1:2].contiguous(), st, en)
    order = [3, 0, 4, 2, 1]
    perm = ops.gage_events(ser, st[order].contiguous(), en[order].contiguous())
    single = ops.gage_events(ser, st[2:3].contiguous(), en[2:3].contiguous())
    for k, base in enumerate((peak, hour, volume)):
        assert torch.equal(bits(again[k]), bits(base)), "two calls"
        assert torch.equal(bits(alone[k]), bits(base[1:2])), "a candidate alone"
        assert torch.equal(bits(perm[k]), bits(base[:, order])), "the events permuted across slots"
        assert torch.equal(bits(single[k]), bits(base[:, 2:3])), "an event alone"
    # the ops layer's own checks
    with pytest.raises(TypeError, match="starts must be an int32 tensor"):
        ops.gage_events(ser, st.long(), en)
    with pytest.raises(ValueError, match=r"ends must be a contiguous \[E,70\]"):
        ops.gage_events(ser, st, en[:, :69].contiguous())
    with pytest.raises(ValueError, match=r"starts must be a contiguous \[E,70\]"):
        ops.gage_events(ser, st.cpu(), en)
    with pytest.raises(ValueError, match=r"series must be a contiguous \[P,T,G\]"):
        ops.gage_events(ser.transpose(1, 2), st, en)
    with pytest.raises(TypeError, match="series must be float32"):
        ops.gage_events(ser.double(), st, en)


@functools.lru_cache(maxsize=None)
def hand_made(name):
    """(starts, ends) [E,G] int32 on the host: gage 0 a window [0, 5], a one-hour window and a window ending at T - 1;
    gage 1 a window crossing a multiple of 16 and, where the record has two tiles, one crossing hours 1023/1024 and a
    121-hour one; the last gage (on 'tiles' the gage without a pair) one window; on 'tiles' gage 2 two and gage 3 none."""
    cs = case(name)
    T, G = cs.T, cs.G
    rows = {0: [(0, 5), (T // 2, T // 2), (T - 8, T - 1)], 1: [(10, 20)]}
    if T > 1024:
        rows[1] += [(300, 420), (1000, 1060)]
    if G > 2:
        rows[G - 1] = [(30, 45)]
    if G > 3:
        rows[2] = [(7, 40), (1020, 1027)]
    E = max(len(r) for r in rows.values())
    starts, ends = (torch.full((E, G), -1, dtype=torch.int32) for _ in range(2))
    for g, wins in rows.items():
        for e, (s, f) in enumerate(wins):
            starts[e, g], ends[e, g] = s, f
    return starts, ends


def event_call(name, mode, cal, events, **kw):
    cs = case(name)
    tgt, w, _ = observations(name, cal)
    cs.prepare()
    args = kwargs_of(cs, mode)
    args.update(kw)
    args.setdefault("event_target", hourly_target(name))
    return hourly_population_event_stats(cs.model, cs.xd, cs.p, tgt, events, weights=w, periods=cal, transform="none", **args)


@pytest.mark.parametrize("name,mode", [(n, "both") for n in NAMES] + [("tiles", "routing")])
def test_the_events_of_the_calls_own_series(hip_backend, eventlib, name, mode):
    cs = case(name)
    starts, ends = hand_made(name)
    E = int(starts.shape[0])
    series = staged(name, mode, None, "none")[3]                    # [P,T,G]: the call's own hourly gage series
    got = event_call(name, mode, None, (starts, ends), return_series=True)
    ev = got["events"]
    assert tuple(ev["peak"].shape) == (P, E, cs.G) and ev["peak"].dtype == torch.float32
    assert ev["peak_hour"].dtype == torch.int32 and ev["volume"].dtype == torch.float32
    assert torch.equal(ev["start"].cpu(), starts) and torch.equal(ev["end"].cpu(), ends) and ev["start"].dtype == torch.int32
    n_present = 0
    for e in range(E):
        for g in range(cs.G):
            s, f = int(starts[e, g]), int(ends[e, g])
            if s < 0:
                assert bool(torch.isneginf(ev["peak"][:, e, g]).all()) and bool((ev["peak_hour"][:, e, g] == -1).all())
                assert bool((ev["volume"][:, e, g] == 0).all()) and not bool(ev["valid"][e, g])
                continue
            n_present += 1
            w = series[:, s:f + 1, g]
            top = w.max(1).values
            first = torch.stack([(w[c] == top[c]).nonzero()[0, 0] for c in range(P)]) + s
            assert torch.equal(bits(ev["peak"][:, e, g]), bits(top)), (e, g)
            assert torch.equal(ev["peak_hour"][:, e, g].long(), first), (e, g)
            assert torch.equal(first, w.argmax(1) + s)
    assert n_present == {"tiles": 9, "short": 4, "m16_muwts": 5}[name]
    check_against_host(eventlib, series, starts, ends, ev["peak"], ev["peak_hour"], ev["volume"], name)
    if name == "tiles":
        flat = cs.G - 1                                             # the gage without a pair: its series is 0
        assert bool((ev["peak"][:, 0, flat] == 0).all()) and bool((ev["peak_hour"][:, 0, flat] == 30).all())
        assert bool((ev["volume"][:, 0, flat] == 0).all())
        assert bool((starts[:, 3] == -1).all()) and not bool(ev["valid"][:, 3].any())
    # the observed side: the same rule on the hourly target (float32), valid where the window is observed throughout
    obs = hourly_target(name).float()
    for e in range(E):
        for g in range(cs.G):
            s, f = int(starts[e, g]), int(ends[e, g])
            if s < 0 or not bool(torch.isfinite(obs[s:f + 1, g]).all()):
                assert not bool(ev["valid"][e, g])
                continue
            assert bool(ev["valid"][e, g])
            assert float(ev["obs_peak"][e, g]) == float(obs[s:f + 1, g].max())
            assert int(ev["obs_peak_hour"][e, g]) == s + int((obs[s:f + 1, g] == obs[s:f + 1, g].max()).nonzero()[0, 0])
    assert int(ev["valid"].sum()) > 0
    for metric in ("peak_error", "peak_bias", "peak_timing", "volume_error"):
        score = hourly_event_score(got, metric)
        assert tuple(score.shape) == (P, cs.G) and score.dtype == torch.float64
        seen = ev["valid"].any(0)
        assert bool(torch.isfinite(score[:, seen]).all()) and bool(torch.isnan(score[:, ~seen]).all())
    # the rest of the dictionary has hourly_population_stats' bits, hourly and on the 24-hour calendar with event_target
    for cal in (None, 24):
        plain = call(name, mode, cal, "none", return_series=True)
        before = dict(ops.HOURLY_POP_LAUNCHES)
        with_events = got if cal is None else event_call(name, mode, cal, (starts, ends), return_series=True)
        if cal is not None:
            launched = {k: ops.HOURLY_POP_LAUNCHES[k] - before[k] for k in before}
            assert launched == {"runoff": 0 if mode == "routing" else 1, "gage": 1}, launched
            for k in ("peak", "peak_hour", "volume", "obs_peak", "obs_peak_hour", "obs_volume", "valid"):
                assert same(with_events["events"][k], ev[k]), f"{k} depends on the calendar"
        for k in KEYS + ("series",):
            assert torch.equal(bits(with_events[k]), bits(plain[k])), f"{k} under periods={cal}"
        assert sorted(set(with_events) - set(plain)) == ["events"]
        for k in plain["outputs"]:
            assert torch.equal(with_events["outputs"][k], plain["outputs"][k])


def test_the_bit_rules(hip_backend):
    name, mode = "tiles", "both"
    cs = case(name)
    events = hand_made(name)
    base = event_call(name, mode, 24, events, return_series=True)
    again = event_call(name, mode, 24, events)
    split = event_call(name, mode, 24, events, max_candidates=2)
    one = event_call(name, mode, 24, events, max_candidates=1)
    order = [3, 0, 4, 2, 1]
    shuffled = event_call(name, mode, 24, events, candidates=cs.cand[order].contiguous(),
                          distr_candidates=cs.dcand[order].contiguous())
    alone = event_call(name, mode, 24, events, candidates=cs.cand[2:3].contiguous(), distr_candidates=cs.dcand[2:3].contiguous())
    on_device = event_call(name, mode, 24, tuple(t.to(DEV).long() for t in events))
    assert "series" in base and "series" not in again
    for k in ("peak", "peak_hour", "volume"):
        b = base["events"][k]
        for other, what in ((again, "a second call, return_series off"), (split, "max_candidates=2"),
                            (one, "max_candidates=1"), (on_device, "int64 events on the device")):
            assert torch.equal(bits(other["events"][k]), bits(b)), f"{k}: {what}"
        assert torch.equal(bits(shuffled["events"][k]), bits(b[order])), f"{k}: another order"
        assert torch.equal(bits(alone["events"][k]), bits(b[2:3])), f"{k}: a candidate alone"
    for k in KEYS:
        for other in (again, split, one):
            assert torch.equal(bits(other[k]), bits(base[k])), k
        assert torch.equal(bits(shuffled[k]), bits(base[k][order])) and torch.equal(bits(alone[k]), bits(base[k][2:3]))
    # an event alone: every row of the windows by itself (E = 1) gives that row's bits
    for e in range(int(events[0].shape[0])):
        row = event_call(name, mode, 24, (events[0][e:e + 1], events[1][e:e + 1]))
        for k in ("peak", "peak_hour", "volume"):
            assert torch.equal(bits(row["events"][k]), bits(base["events"][k][:, e:e + 1])), f"{k}: event {e} alone"
    # the method is the function
    tgt, w, _ = observations(name, 24)
    cs.prepare()
    meth = cs.model.population_event_stats(cs.xd, cs.p, tgt, events, cs.cand, cs.dcand, names=cs.names, weights=w, periods=24,
                                           event_target=hourly_target(name))
    for k in ("peak", "peak_hour", "volume"):
        assert torch.equal(bits(meth["events"][k]), bits(base["events"][k]))


@pytest.mark.parametrize("name", NAMES)
def test_events_against_the_module_route(hip_backend, name):
    cs = case(name)
    _, flow_want = module_route(name, "both")                       # [P,T,G] from P module forwards
    _, primal = cs.forward(cs.p)
    starts, ends = flood_events(primal, 3, 6, 12, min_peak=1e-6)
    assert int((starts >= 0).sum()) >= 3, "the primal streamflow has no floods"
    got = event_call(name, "both", None, (starts, ends), event_target=primal)
    ev = got["events"]
    want = flow_want.double()
    compared = skipped = 0
    worst_peak = worst_vol = 0.0
    for e in range(int(starts.shape[0])):
        for g in range(cs.G):
            s, f = int(starts[e, g]), int(ends[e, g])
            if s < 0:
                continue
            n = f - s + 1
            for c in range(P):
                w = want[c, s:f + 1, g]
                top, at = w.max(0)
                tol = au.FLUX_ATOL + au.FLUX_RTOL * float(top.abs())
                d_peak = abs(float(ev["peak"][c, e, g]) - float(top))
                d_vol = abs(float(ev["volume"][c, e, g]) - float(w.sum()))
                worst_peak, worst_vol = max(worst_peak, d_peak / tol), max(worst_vol, d_vol / (n * tol))
                assert d_peak <= tol, (c, e, g, d_peak, tol)
                assert d_vol <= n * tol, (c, e, g, d_vol, n * tol)
                others = torch.cat([w[:at], w[at + 1:]])
                if n > 1 and float(top - others.max()) <= 2 * tol:
                    skipped += 1
                    continue
                compared += 1
                assert int(ev["peak_hour"][c, e, g]) == s + int(at), (c, e, g)
    share = skipped / (compared + skipped)
    print(f"{name}: {compared} hours of the peak compared, {skipped} skipped (share {share:.3f}); worst peak error / "
          f"tolerance {worst_peak:.3g}, worst volume error / tolerance {worst_vol:.3g}")
    assert share <= 0.25, f"{skipped} of {compared + skipped} peaks are not separated by twice the tolerance"


def test_the_routing_search(hip_backend):
    name = "tiles"
    cs = case(name)
    tgt, w, _ = observations(name, None)
    events = flood_events(hourly_target(name), 3, 6, 12)
    kw = dict(n_candidates=8, n_rounds=2, weights=w, objective="kge")
    before = dict(ops.HOURLY_POP_LAUNCHES)
    cs.prepare()
    kept = [t.clone() for t in cs.p]
    (p_dyn, p_sta, p_distr), hist = hourly_routing_search(cs.model, cs.xd, cs.p, tgt, generator=torch.Generator().manual_seed(3), **kw)
    assert ops.HOURLY_POP_LAUNCHES["runoff"] == before["runoff"], "stage 1 ran in a routing-only search"
    assert ops.HOURLY_POP_LAUNCHES["gage"] == before["gage"] + 2
    assert p_dyn is cs.p[0] and p_sta is cs.p[1] and tuple(p_distr.shape) == tuple(cs.p[2].shape)
    assert all(torch.equal(a, b) for a, b in zip(cs.p, kept))
    cost = hist["cost"]
    assert tuple(cost.shape) == (3, cs.G) and cost.dtype == torch.float64 and tuple(hist["best_index"].shape) == (2, cs.G)
    assert bool((cost[1:] <= cost[:-1]).all()), "a gage's cost rose"
    seen = cs.observed_gages().cpu()
    assert bool(torch.isfinite(cost[:, seen]).all()) and bool(torch.isinf(cost[:, ~seen]).all())
    assert bool((cost[-1, seen] < cost[0, seen]).any()), "eight candidates in two rounds improved no gage"
    assert float(p_distr.min()) >= 0 and float(p_distr.max()) <= 1 and not torch.equal(p_distr, cs.p[2])
    # the returned rows, evaluated by a plain call, have the cost the history ends on (a candidate's bits do not depend
    # on the others, and gage g's series reads g's pairs alone)
    cs.prepare()
    st = hourly_population_stats(cs.model, cs.xd, cs.p, tgt, distr_candidates=p_distr.unsqueeze(0).contiguous(), weights=w)
    final = 1.0 - population_score(st, "kge")[0].cpu()
    assert torch.equal(final[seen], cost[-1, seen])
    assert torch.equal(hist["score"][-1][seen], population_score(st, "kge")[0].cpu()[seen])
    # event_share = 0 does not touch the events: the same search
    cs.prepare()
    (_, _, p2), hist2 = hourly_routing_search(cs.model, cs.xd, cs.p, tgt, generator=torch.Generator().manual_seed(3),
                                              events=events, event_target=hourly_target(name), event_share=0.0, **kw)
    assert torch.equal(p2, p_distr) and all(same(hist[k], hist2[k]) for k in hist) and "score_event" not in hist2
    # event_share > 0: both scores are kept, the mixed cost never rises, stage 1 stays off
    cs.prepare()
    (_, _, p3), hist3 = hourly_routing_search(cs.model, cs.xd, cs.p, tgt, generator=torch.Generator().manual_seed(3),
                                              events=events, event_target=hourly_target(name), event_share=0.5,
                                              event_metric="peak_timing", **kw)
    assert ops.HOURLY_POP_LAUNCHES["runoff"] == before["runoff"]
    c3 = hist3["cost"]
    assert bool((c3[1:] <= c3[:-1]).all()) and bool(torch.isfinite(c3[:, seen]).all())
    mixed = 0.5 * (1.0 - hist3["score"]) + 0.5 * hist3["score_event"]
    assert torch.allclose(mixed[:, seen], c3[:, seen], rtol=1e-12, atol=0)
    assert same(hist3["score"][0], hist["score"][0])                        # the start is the start
