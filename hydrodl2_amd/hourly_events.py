"""Flood events of `Hbv_2_hourly` at its gages: event statistics of a population of candidates, scores on them, and the
routing-only search that can put those scores into its objective.

A KGE over a season of hours hardly moves when a flood peak comes four hours late, and it cannot tell that a candidate
halves the peak of the three storms that matter.  The routing parameters -- route_tau, a lag in hours; route_a / route_b,
the attenuation of the peak -- are exactly what such a moment score is blind to.  So the event windows are fixed on the
OBSERVED side (`flood_events`), and each candidate's peak, hour of the peak and volume in each window are a max, a
first-argmax and an ordered sum over a few dozen hours of the hourly gage series that stage 2 of
`hourly_population_stats` already holds (hbvx_gage_population_events, include/hbvx_gage_events.h states the arithmetic
line by line).  No series leaves the device.

  flood_events                   (starts, ends) [E,G]: the E highest separated peaks of the observed series per gage;
  hourly_population_event_stats  `hourly_population_stats`' dictionary, same bits, plus 'events';
  hourly_event_score             peak error, peak bias, peak timing and volume error per (candidate, gage);
  hourly_routing_search          shrinking random search over parameters[2], selected PER GAGE: every (gage, unit) pair
                                 belongs to one gage, so the gages' searches do not meet.  Its objective can also take a
                                 flow-duration term (hourly_fdc.py).

The daily models Hbv, Hbv_1_1p and Hbv_2 have the same statistics per basin in population_events.py, which reuses
`flood_events`, `_check_events`, `_observed_events` and the score of this file.

Not built: events for the implicit family, event detection on the simulated side, a search over unit
parameters (gages share units), Hbv_2_mts, gradients of event scores.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .hourly_fdc import HOURLY_FDC_METRICS, _FdcHook, _fdc_stats, hourly_fdc_score
from .hourly_population import _evaluate, hourly_population_stats
from .population import OBJECTIVES, _check_search, _mixed_cost, _objective_cost, population_score

WHAT = "hourly_population_event_stats"
EVENT_METRICS = ('peak_error', 'peak_bias', 'peak_timing', 'volume_error')
SEARCH_OBJECTIVES = tuple(o for o in OBJECTIVES if o != 'sse')        # 'nse', 'kge', 'kge12'


def _hourly(series, name, what) -> np.ndarray:
    """[T,G] float32 on the host of a [T,G] or [T,G,1] tensor or array."""
    a = series.detach().cpu().numpy() if torch.is_tensor(series) else np.asarray(series)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[..., 0]
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{what}: {name} must be [T,G] or [T,G,1], got {tuple(a.shape)}")
    return np.ascontiguousarray(a, dtype=np.float32)


def flood_events(target, n_events: int, before: int, after: int, min_peak: Optional[float] = None):
    """Event windows on the observed hourly series, per gage: (starts, ends), [E,G] int32 on the host, E = n_events.

    target   [T,G] or [T,G,1] observed hourly flow; NaN is a missing hour.
    Per gage, greedily: the highest finite hour not yet looked at (ties: the earliest; >= min_peak if that is given) is a
    peak, its window [peak - before, peak + after] clipped to the record.  The peak is rejected when its window overlaps
    an accepted window or holds a non-finite observation.  That repeats until n_events windows are accepted or no hour
    qualifies.  The gage's windows are then sorted ascending, and the rows it does not fill hold (-1, -1).
    Runs on the host and is deterministic."""
    what = "flood_events"
    obs = _hourly(target, "target", what)
    T, G = obs.shape
    if int(n_events) != n_events or n_events < 1:
        raise ValueError(f"{what}: n_events must be an integer >= 1, got {n_events!r}")
    if int(before) != before or int(after) != after or before < 0 or after < 0:
        raise ValueError(f"{what}: before and after must be integers >= 0, got {before!r}, {after!r}")
    E, before, after = int(n_events), int(before), int(after)
    starts = np.full((E, G), -1, np.int32)
    ends = np.full((E, G), -1, np.int32)
    for g in range(G):
        y = obs[:, g]
        ok = np.isfinite(y)
        bad = np.concatenate([[0], np.cumsum(~ok)])             # bad[f + 1] - bad[s]: non-finite hours of s .. f
        if min_peak is not None:
            ok = ok & (y >= np.float32(min_peak))
        hours = np.nonzero(ok)[0]
        hours = hours[np.argsort(-y[hours].astype(np.float64), kind="stable")]     # descending, ties: the earliest first
        taken = []
        for p in hours.tolist():
            if len(taken) == E:
                break
            s, f = max(0, p - before), min(T - 1, p + after)
            if bad[f + 1] - bad[s] or any(s <= f0 and s0 <= f for s0, f0 in taken):
                continue
            taken.append((s, f))
        for e, (s, f) in enumerate(sorted(taken)):
            starts[e, g], ends[e, g] = s, f
    return torch.from_numpy(starts), torch.from_numpy(ends)


def _check_events(events, T: int, G: int, dev, what: str = WHAT):
    """`events` = (starts, ends) as `hourly_population_event_stats` takes them -> the pair as contiguous int32 [E,G] on
    `dev`; ValueError for anything else."""
    if not isinstance(events, (tuple, list)) or len(events) != 2:
        raise ValueError(f"{what}: events must be the pair (starts, ends)")
    starts, ends = events
    for name, t in (("starts", starts), ("ends", ends)):
        if not torch.is_tensor(t) or t.dtype not in (torch.int32, torch.int64) or t.dim() != 2:
            raise ValueError(f"{what}: {name} must be an int32 or int64 [E,{G}] tensor, got "
                             f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
        if t.device.type != 'cpu' and t.device != dev:
            raise ValueError(f"{what}: {name} lives on {t.device}; the host or {dev}")
    if starts.dtype != ends.dtype or tuple(starts.shape) != tuple(ends.shape):
        raise ValueError(f"{what}: starts is {starts.dtype} {tuple(starts.shape)}, ends {ends.dtype} {tuple(ends.shape)}")
    E = int(starts.shape[0])
    if int(starts.shape[1]) != G:
        raise ValueError(f"{what}: starts and ends must be [E,{G}] (one column per gage), got {tuple(starts.shape)}")
    if E < 1:
        raise ValueError(f"{what}: no event rows (E < 1)")
    if E > T:
        raise ValueError(f"{what}: {E} event rows on a record of {T} hours")
    s, f = starts.detach().cpu().long(), ends.detach().cpu().long()
    present = s >= 0
    if bool((present & ((f < s) | (f >= T))).any()):
        raise ValueError(f"{what}: a present window must have 0 <= start <= end < {T} (start < 0 marks an absent slot)")
    if bool((present[1:] & ~present[:-1]).any()):
        raise ValueError(f"{what}: a present row after an absent one (a gage's windows come first, (-1, -1) pads)")
    if bool((present[1:] & (s[1:] <= f[:-1])).any()):
        raise ValueError(f"{what}: a gage's windows must be strictly ascending and disjoint")
    return (starts.detach().to(device=dev, dtype=torch.int32).contiguous(),
            ends.detach().to(device=dev, dtype=torch.int32).contiguous())


def _observed_events(obs: np.ndarray, starts: np.ndarray, ends: np.ndarray):
    """The kernel's rule (hbvx_popk::EventSlot) on the observed hourly series, float32 on the host: (peak, peak_hour,
    volume, valid) [E,G].  Valid: present, and every observed hour of the window finite."""
    E, G = starts.shape
    T = obs.shape[0]
    s, f = starts.astype(np.int64), np.minimum(ends.astype(np.int64), T - 1)
    present = (s >= 0) & (f >= s)
    W = int((f - s)[present].max()) + 1 if present.any() else 1
    hours = s[:, None, :] + np.arange(W).reshape(1, W, 1)                           # [E,W,G]
    inside = present[:, None, :] & (hours <= f[:, None, :])
    w = obs[np.clip(hours, 0, T - 1), np.arange(G).reshape(1, 1, G)]                # the windows, hour by hour
    ranked = np.where(inside & ~np.isnan(w), w, np.float32(-np.inf))
    first = ranked.argmax(1)                                                        # the first hour at the maximum
    found = ranked.max(1) > -np.inf
    # (the hour's own value: a maximum of zeros has either sign)
    peak = np.where(found, np.take_along_axis(w, first[:, None, :], 1)[:, 0, :], np.float32(-np.inf)).astype(np.float32)
    hour = np.where(found, s + first, -1).astype(np.int32)
    # one float32 addition per hour, ascending, from +0 (np.cumsum of float32 adds sequentially; the +0 of the hours
    # behind a shorter window changes nothing)
    volume = np.cumsum(np.where(inside, w, np.float32(0.0)), axis=1, dtype=np.float32)[:, -1, :]
    valid = present & (np.isfinite(w) | ~inside).all(1)
    return peak, hour, volume, valid


class _EventHook:
    """What `hourly_population._evaluate` calls for the event statistics of every chunk's series."""
    exports = ('hbvx_gage_population_events',)

    def __init__(self, events, event_target, target, periods):
        self.events, self.event_target, self.target, self.periods = events, event_target, target, periods
        self.parts = []
        self.bytes = 0

    def check(self, T, G, dev):
        self.starts, self.ends = _check_events(self.events, T, G, dev)
        src = self.event_target
        if src is None:
            if self.periods is not None:
                raise ValueError(f"{WHAT}: with a calendar `target` holds period rows; give the observed HOURLY series as "
                                 f"event_target [{T},{G}]")
            src = self.target
        obs = _hourly(src, "event_target", WHAT)
        if obs.shape != (T, G):
            raise ValueError(f"{WHAT}: event_target must be [{T},{G}] (the hourly record at the gages), got {obs.shape}")
        self.obs = _observed_events(obs, self.starts.cpu().numpy(), self.ends.cpu().numpy())
        self.dev = dev
        self.bytes = 12 * int(self.starts.shape[0]) * G

    def chunk(self, series):
        self.parts.append(ops.gage_events(series, self.starts, self.ends))

    def result(self) -> dict:
        peak, hour, volume = (self.parts[0][i] if len(self.parts) == 1 else torch.cat([p[i] for p in self.parts])
                              for i in range(3))
        op, oh, ov, valid = (torch.from_numpy(a).to(self.dev) for a in self.obs)
        return dict(start=self.starts, end=self.ends, peak=peak, peak_hour=hour, volume=volume, obs_peak=op,
                    obs_peak_hour=oh, obs_volume=ov, valid=valid)


def hourly_population_event_stats(model, x_dict: dict, parameters, target, events, candidates: Optional[torch.Tensor] = None,
                                  distr_candidates: Optional[torch.Tensor] = None, names: Optional[Sequence[str]] = None,
                                  weights=None, periods=None, transform: str = 'none', eps=None, return_series: bool = False,
                                  max_candidates: Optional[int] = None, event_target=None) -> dict:
    """`hourly_population_stats` (same arguments, same dictionary, same bits) plus the flood-event statistics of every
    candidate at the gages.

    events        (starts, ends): int32 or int64 [E,G] on the host or on the device, inclusive hours, 0-based, a gage's
                  windows strictly ascending and disjoint in its first rows, (-1, -1) in the rows it does not fill --
                  what `flood_events` returns.  Events are windows of HOURS on the hourly gage series whatever
                  `periods` is.
    event_target  [T,G] or [T,G,1]: the observed hourly series the observed side of the events is formed on.  Without a
                  calendar it defaults to `target`; with one, `target` holds period rows and it must be given.
    Returns the dictionary of `hourly_population_stats` and 'events':
      'start', 'end'        [E,G] int32, as given;
      'peak'                [P,E,G] float32, the highest flow of the candidate's hourly gage series in the window;
      'peak_hour'           [P,E,G] int32, the FIRST hour at that flow (-1: no hour of the window has a flow above -inf:
                            all NaN);
      'volume'              [P,E,G] float32, the float32 sum of the window's flows in hour order;
      'obs_peak', 'obs_peak_hour', 'obs_volume'   [E,G], the same rule in float32 on the observed series;
      'valid'               [E,G] bool: the event is present and every observed hour of its window is finite.
    An absent slot holds -inf, -1, +0 on either side.  Per chunk of candidates the call is stage 2 with its hourly series
    kept, then hbvx_gage_population_events on that series (include/hbvx_gage_events.h); memory and chunking are
    `hourly_population_stats`' own, and a candidate's bits depend on neither the split nor the other events.

    Refused before the model runs (ValueError): what `hourly_population_stats` refuses; starts / ends that are not both
    int32 or both int64 [E,G] on the host or on x_phy's device; E < 1 (or E > T); a present window outside
    0 <= start <= end < T; a gage's present windows not strictly ascending and disjoint; a present row after an absent
    one; an event_target of another shape than [T,G], or none with a calendar."""
    hook = _EventHook(events, event_target, target, periods)
    out = _evaluate(model, x_dict, parameters, target, candidates, distr_candidates, names, weights, periods, transform, eps,
                    return_series, max_candidates, hook)
    out['events'] = hook.result()
    return out


def hourly_event_score(stats: dict, metric: str, timing_scale: float = 24.0) -> torch.Tensor:
    """[P,G] float64 event score of every candidate from what `hourly_population_event_stats` returned: the mean over the
    gage's valid events of
      'peak_error'    |peak - obs_peak| / obs_peak          'peak_bias'     (peak - obs_peak) / obs_peak
      'peak_timing'   |peak_hour - obs_peak_hour| / timing_scale          (zero is perfect; in units of timing_scale hours)
      'volume_error'  |volume - obs_volume| / obs_volume
    NaN where the gage has no valid event, where a valid event's denominator (obs_peak, obs_volume, timing_scale) is not
    positive, and for a candidate with peak_hour == -1 in a valid event (no finite flow in the window)."""
    return _event_score(stats['events'], 'peak_hour', metric, timing_scale)


def _event_score(ev: dict, when: str, metric: str, timing_scale: float) -> torch.Tensor:
    """`hourly_event_score` on an 'events' dictionary whose time-of-peak keys are `when` and 'obs_' + `when` ('peak_hour';
    'peak_day' for the daily models' `population_event_score`)."""
    if metric not in EVENT_METRICS:
        raise ValueError(f"metric must be one of {list(EVENT_METRICS)}, got {metric!r}")
    dev = ev['peak'].device
    valid = ev['valid'].to(dev)                                                         # [E,G]
    if metric == 'peak_timing':
        num = (ev[when].to(torch.float64) - ev['obs_' + when].to(dev).to(torch.float64)).abs()
        den = torch.full(valid.shape, float(timing_scale), dtype=torch.float64, device=dev)
    else:
        key = 'volume' if metric == 'volume_error' else 'peak'
        den = ev['obs_' + key].to(dev).to(torch.float64)
        num = ev[key].to(torch.float64) - den
        if metric != 'peak_bias':
            num = num.abs()
    bad_den = valid & ~(den > 0)
    term = num / torch.where(den > 0, den, torch.ones_like(den))
    term = torch.where(valid.unsqueeze(0), term, torch.zeros_like(term))               # [P,E,G]
    n = valid.sum(0)                                                                   # [G]
    mean = term.sum(1) / n.clamp_min(1).to(torch.float64)
    empty = (valid.unsqueeze(0) & (ev[when] == -1)).any(1)                              # [P,G]
    undefined = empty | ((n == 0) | bad_den.any(0)).unsqueeze(0)
    return torch.where(undefined, torch.full_like(mean, float('nan')), mean)


def _routing_search(pair_gage: torch.Tensor, start: torch.Tensor, evaluate, n_candidates: int, n_rounds: int,
                    shrink: float, generator: Optional[torch.Generator], kept: Sequence[str] = ()):
    """The loop of `hourly_routing_search`.  pair_gage [n_pair] int: the gage of every (gage, unit) pair in
    GageTopology's CSR order; start [n_pair,3] unit-interval rows; evaluate(dcands [P,n_pair,3]) -> (cost [P,G],
    {name: [P,G]} for the names of `kept`).  Returns (best rows [n_pair,3], history)."""
    dev = start.device
    gdev = generator.device if generator is not None else torch.device('cpu')
    pg = pair_gage.to(device=dev, dtype=torch.long)
    n_pair = int(start.shape[0])
    best = start.detach().to(torch.float32).clamp(0.0, 1.0)
    pairs = torch.arange(n_pair, device=dev)
    hist = {'cost': [], 'best_index': [], **{name: [] for name in kept}}
    for k in range(n_rounds):
        draws = torch.rand((n_candidates - 1, n_pair, 3), generator=generator, device=gdev).to(dev)
        if k > 0:
            draws = (best.unsqueeze(0) + (draws - 0.5) * float(shrink) ** k).clamp(0.0, 1.0)
        dcands = torch.cat([best.unsqueeze(0), draws]).contiguous()
        cost, scores = evaluate(dcands)
        low, idx = cost.min(0)
        idx = torch.where(cost[0] <= low, torch.zeros_like(idx), idx)          # a tie keeps the row that is held
        if k == 0:
            hist['cost'].append(cost[0].double().cpu())
            for name in kept:
                hist[name].append(scores[name][0].cpu())
        best = dcands[idx.to(dev)[pg], pairs]                                   # gage g's pairs from g's own winner
        hist['cost'].append(cost.gather(0, idx.unsqueeze(0))[0].double().cpu())
        for name in kept:
            hist[name].append(scores[name].gather(0, idx.unsqueeze(0))[0].cpu())
        hist['best_index'].append(idx.cpu())
    return best, {name: torch.stack(rows) for name, rows in hist.items()}


def hourly_routing_search(model, x_dict: dict, parameters, target, n_candidates: int = 64, n_rounds: int = 4,
                          shrink: float = 0.5, weights=None, periods=None, transform: str = 'none', eps=None,
                          objective: str = 'kge', events=None, event_target=None, event_share: float = 0.0,
                          event_metric: str = 'peak_timing', timing_scale: float = 24.0,
                          generator: Optional[torch.Generator] = None, max_candidates: Optional[int] = None,
                          fdc_share: float = 0.0, fdc_probs=None, fdc_metric: str = 'fdc_freq', fdc_target=None):
    """Per-gage shrinking random search over the distributed routing parameters parameters[2] (unit-interval route_a,
    route_b, route_tau per (gage, unit) pair) of `Hbv_2_hourly`: `population_search`'s search in the unit cube,
    routing-only, so stage 1 never launches and every round is one `hourly_population_stats` call.

    Round 0 evaluates the held rows as candidate 0 and n_candidates - 1 uniform draws; round k >= 1 draws uniformly in a
    box of half-width shrink**k / 2 around each gage's best so far, clipped to [0, 1], and always re-includes that best
    as candidate 0.  Selection is PER GAGE: gage g takes the candidate with the lowest cost[:, g] (a tie keeps the held
    rows), and the rows of g's pairs are gathered from that candidate -- every pair belongs to one gage, so the gages do
    not meet and a gage's cost never rises.  A gage whose cost is +inf for every candidate keeps its start.

    cost = 1 - score under `objective` ('nse', 'kge' or 'kge12'; +inf where `population_score` gives NaN).  With
    event_share = S > 0 (then `events`, and with a calendar `event_target`, as `hourly_population_event_stats` takes
    them) the cost is (1 - S) * (1 - score) + S * hourly_event_score(stats, event_metric, timing_scale), +inf where
    either is undefined, and every round is one `hourly_population_event_stats` call.  With S == 0 (the default) the
    events are not touched and hbvx_gage_population_events is not required.

    With fdc_share = S > 0 (not together with event_share > 0) the cost is (1 - S) * (1 - score) + S *
    hourly_fdc_score(stats, fdc_metric), +inf where either is undefined, and every round is one
    `hourly_population_fdc_stats` call at the probabilities fdc_probs (None: its default fifteen; 'fdc_slope' needs 0.2
    and 0.7 among them) with fdc_target as that call takes it.  The observed curve is formed once, before the first
    round, not per round.  With S == 0 (the default) fdc_probs and fdc_target are not touched, the search is the one
    above bit for bit, and the exports of include/hbvx_gage_fdc.h are not required.

    Returns ((p_dyn, p_sta, new p_distr), history): history['cost'] [n_rounds+1,G] float64 (row 0: the start, row k+1:
    the best after round k), 'score' and with event_share > 0 'score_event', with fdc_share > 0 'score_fdc' likewise, 'best_index' [n_rounds,G] (the winning
    candidate of the round; 0: nothing better was drawn).  The inputs are not modified.  Deterministic for a given
    `generator` (default: torch's global CPU generator).

    Refused (ValueError): what `hourly_population_stats` refuses; dy_drop > 0, n_candidates < 2, n_rounds < 1, shrink
    outside (0, 1], an objective other than the three; event_share outside [0, 1] or NaN; event_share > 0 without
    `events`; an unknown event_metric; fdc_share outside [0, 1] or NaN; fdc_share > 0 together with event_share > 0; an
    unknown fdc_metric; what `hourly_population_fdc_stats` refuses of fdc_probs and fdc_target (a calendar without
    fdc_target among it)."""
    what = "hourly_routing_search"
    _check_search(model, n_candidates, n_rounds, shrink, objective, what)
    if objective not in SEARCH_OBJECTIVES:
        raise ValueError(f"{what}: objective must be one of {list(SEARCH_OBJECTIVES)}, got {objective!r}")
    if not 0.0 <= float(event_share) <= 1.0:            # (a NaN fails both comparisons)
        raise ValueError(f"{what}: event_share must lie in [0, 1], got {event_share!r}")
    share = float(event_share)
    if event_metric not in EVENT_METRICS:
        raise ValueError(f"{what}: event_metric must be one of {list(EVENT_METRICS)}, got {event_metric!r}")
    if share > 0 and events is None:
        raise ValueError(f"{what}: event_share > 0 needs events (see flood_events)")
    if not 0.0 <= float(fdc_share) <= 1.0:
        raise ValueError(f"{what}: fdc_share must lie in [0, 1], got {fdc_share!r}")
    fshare = float(fdc_share)
    if fdc_metric not in HOURLY_FDC_METRICS:
        raise ValueError(f"{what}: fdc_metric must be one of {list(HOURLY_FDC_METRICS)}, got {fdc_metric!r}")
    if fshare > 0 and share > 0:
        raise ValueError(f"{what}: fdc_share > 0 together with event_share > 0 (one extra term per search)")
    if fshare > 0 and periods is not None and fdc_target is None:
        raise ValueError(f"{what}: with a calendar `target` holds period rows; give the observed HOURLY series as fdc_target")
    p_distr = parameters[2]
    topo = x_dict['outlet_topo']
    pair_gage = (topo == 1).nonzero(as_tuple=False)[:, 0]           # GageTopology's pair order: by gage, then unit
    if not torch.is_tensor(p_distr) or p_distr.dim() != 2 or tuple(p_distr.shape) != (int(pair_gage.numel()), 3):
        raise ValueError(f"{what}: parameters[2] must be [{int(pair_gage.numel())},3] (the pairs of outlet_topo), got "
                         f"{tuple(p_distr.shape) if torch.is_tensor(p_distr) else type(p_distr).__name__}")
    common = dict(weights=weights, periods=periods, transform=transform, eps=eps, max_candidates=max_candidates)
    # one hook for every round: it forms the observed curve on its first check and keeps it
    fdc_hook = _FdcHook(x_dict, target, weights, periods, fdc_probs, None, fdc_target, what) if fshare > 0 else None

    def evaluate(dcands):
        if fshare > 0:
            st = _fdc_stats(fdc_hook, model, x_dict, parameters, target, None, dcands, None, weights, periods, transform,
                            eps, False, max_candidates)
            score = population_score(st, objective)
            score_fdc = hourly_fdc_score(st, fdc_metric)
            cost_fdc = torch.where(torch.isnan(score_fdc), torch.full_like(score_fdc, float('inf')), score_fdc)
            return _mixed_cost(_objective_cost(score, objective), cost_fdc, fshare), {'score': score, 'score_fdc': score_fdc}
        if share > 0:
            st = hourly_population_event_stats(model, x_dict, parameters, target, events, distr_candidates=dcands,
                                               event_target=event_target, **common)
        else:
            st = hourly_population_stats(model, x_dict, parameters, target, distr_candidates=dcands, **common)
        score = population_score(st, objective)
        cost = _objective_cost(score, objective)
        if share == 0:
            return cost, {'score': score}
        score_event = hourly_event_score(st, event_metric, timing_scale)
        cost_event = torch.where(torch.isnan(score_event), torch.full_like(score_event, float('inf')), score_event)
        return _mixed_cost(cost, cost_event, share), {'score': score, 'score_event': score_event}

    best, hist = _routing_search(pair_gage, p_distr.to(x_dict['x_phy'].device), evaluate, n_candidates, n_rounds, shrink,
                                 generator, ('score', 'score_fdc') if fshare > 0 else
                                 ('score', 'score_event') if share > 0 else ('score',))
    return (parameters[0], parameters[1], best.to(device=p_distr.device, dtype=p_distr.dtype)), hist
