"""Population flood-event scores of the daily models: the peak, the day of the peak and the volume of many candidate
parameter sets inside event windows fixed on the observed side, from the launch that forms their flow scores.

`population_stats` scores moments and `population_fdc_stats` exceedance counts; neither sees a flood as an event: a KGE
over twenty years hardly moves when the annual peak is 30 % low or a day late, and a flow-duration curve is blind to
the order of the days.  The windows are fixed on the OBSERVED side (`flood_events`, basins for gages and scored days for
hours), so a candidate's statistic in a window is a max, a first-argmax and an ordered float32 sum over the days of the
window.  `population_event_stats` is `population_stats` -- the same checks, the same observation side, the same four
chains bit for bit -- through hbvx_population_events (include/hbvx_pop_events.h), which adds [P,E,B] peaks, days and
volumes and still writes no series; `population_event_score` forms peak error, peak bias, peak timing and volume error
from them, and `population_search(events=..., event_share=...)` mixes one into its objective.

Hbv, Hbv_1_1p and Hbv_2, daily.  Not built: the implicit scheme (HbvAdj); events together with period calendars or an
aux term; event detection on the simulated side; moving-mean low-flow windows; gradients of event scores.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch

from . import ops
from ._lib import get_library
from .hourly_events import EVENT_METRICS, _check_events, _event_score, _hourly, _observed_events
from .population import EXPLICIT, _candidate_sources, _check, _daily_request, _primal, _sums

EXPORT = 'hbvx_population_events'


class Windows(NamedTuple):
    """The event windows of a call after their checks, and the observed half of its 'events' dictionary: formed once,
    before the model runs (once per search, not per round)."""
    starts: torch.Tensor        # [E,B] int32 on the device of x_phy
    ends: torch.Tensor
    observed: dict              # 'obs_peak', 'obs_peak_day', 'obs_volume', 'valid' [E,B] on the device of x_phy


def _event_request(what, model, x_dict, parameters, candidates, target, events, names, weights, transform, eps,
                   return_series=False):
    """Everything the call can refuse before the model runs -> (population.py's request of the stats form, Windows).
    candidates None: the search."""
    # the windows before the request: `_daily_request` ends by asking the library for hbvx_population_stats
    req = _check(EXPLICIT, model, x_dict, parameters, target, names, weights, what)
    dev = x_dict['x_phy'].device
    starts, ends = _check_events(events, req.T_out, req.B, dev, what)
    rq = _daily_request(EXPLICIT, what, 'stats', model, x_dict, parameters, candidates, target, names, weights, transform,
                        eps, return_series=return_series)
    get_library().require(EXPORT)
    obs = _hourly(target, "target", what)                       # [T_out,B] float32 on the host, NaN where missing
    peak, day, volume, valid = (torch.from_numpy(a).to(dev)
                                for a in _observed_events(obs, starts.cpu().numpy(), ends.cpu().numpy()))
    return rq, Windows(starts, ends, dict(obs_peak=peak, obs_peak_day=day, obs_volume=volume, valid=valid))


def _event_run(rq, win: Windows):
    """The module once at rq.parameters, then rq.candidates through ops.population_events: `population_stats`'
    dictionary and 'events'."""
    outputs, main, t_first = _primal(EXPLICIT, rq.model, rq.req, rq.x_dict, rq.parameters)
    sources, route = _candidate_sources(rq.model, rq.names, rq.candidates)
    ob = rq.ob
    flow = ops.PopTerm(ob['target'], ob['w'], ob['shift'], ob['eps'], rq.transform)
    flow_out, (peak, day, volume) = ops.population_events(main, sources, route, flow, win.starts, win.ends, t_first,
                                                          rq.return_series)
    out = _sums(flow_out, ob, rq.transform, rq, outputs)
    out['events'] = dict(win.observed, start=win.starts, end=win.ends, peak=peak, peak_day=day, volume=volume)
    return out


def population_event_stats(model, x_dict: dict, parameters, candidates: torch.Tensor, target, events,
                           names: Optional[Sequence[str]] = None, weights=None, transform: str = 'none', eps=None,
                           return_series: bool = False) -> dict:
    """`population_stats`, and each candidate's flood-event statistics per basin, from one launch that writes no series:
    the peak, the day of the peak and the volume of the routed streamflow inside E event windows per basin.

    candidates, target, names, weights, transform, eps, return_series: as `population_stats`.  Weights do not enter the
    event statistics: the window is the mask.
    events       (starts, ends): int32 or int64 [E,B] on the host or on the device, inclusive SCORED days (day 0 is the
                 first day after the warm-up, the first row of `target`), 0-based, a basin's windows strictly ascending
                 and disjoint in its first rows, (-1, -1) in the rows it does not fill -- what
                 `flood_events(target, n_events, before, after)` returns on the daily target.
    Returns `population_stats`' dictionary, the same keys and the same bits, and 'events':
      'start', 'end'        [E,B] int32, as given;
      'peak'                [P,E,B] float32, the highest streamflow of the candidate in the window;
      'peak_day'            [P,E,B] int32, the FIRST scored day at that flow (-1: no day of the window has a flow above
                            -inf: all NaN);
      'volume'              [P,E,B] float32, the float32 sum of the window's flows in day order;
      'obs_peak', 'obs_peak_day', 'obs_volume'   [E,B], the same rule in float32 on `target`;
      'valid'               [E,B] bool: the event is present and observed on every day of its window.
    An absent slot holds -inf, -1, +0 on either side.  The statistics are taken on the streamflow itself under every
    transform.  A slot depends on that candidate and on its basin's windows up to that row alone: not on E, the rows
    after it, the other candidates or return_series; two calls agree bit for bit, and the numbers are what
    `ops.gage_events` gives on the call's own return_series series.

    Refused before the model runs: everything `population_stats` refuses; starts / ends that are not both int32 or both
    int64 [E,B] on the host or on x_phy's device; E < 1 (or E > T_out); a present window outside 0 <= start <= end <
    T_out; a basin's present windows not strictly ascending and disjoint; a present row after an absent one
    (ValueError); HbvAdj, Hbv_2_hourly, Hbv_2_mts (NotImplementedError); a library without hbvx_population_events
    (HbvxError)."""
    return _event_run(*_event_request("population_event_stats", model, x_dict, parameters, candidates, target, events,
                                      names, weights, transform, eps, return_series))


def population_event_score(stats: dict, metric: str, timing_scale: float = 1.0) -> torch.Tensor:
    """[P,B] float64 event score of every candidate from what `population_event_stats` returned: the mean over the
    basin's valid events of
      'peak_error'    |peak - obs_peak| / obs_peak          'peak_bias'     (peak - obs_peak) / obs_peak
      'peak_timing'   |peak_day - obs_peak_day| / timing_scale          (zero is perfect; in units of timing_scale days)
      'volume_error'  |volume - obs_volume| / obs_volume
    with the NaN rules of `hourly_event_score`: NaN where the basin has no valid event, where a valid event's
    denominator (obs_peak, obs_volume, timing_scale) is not positive, and for a candidate with peak_day == -1 in a valid
    event (no finite flow in the window)."""
    return _event_score(stats['events'], 'peak_day', metric, timing_scale)


__all__ = ["EVENT_METRICS", "population_event_stats", "population_event_score"]
