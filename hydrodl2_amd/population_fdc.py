"""Population flow-duration scores: the simulated flow-duration curve of many candidate parameter sets, sampled at
thresholds fixed on the observed side, from the launch that forms their flow scores.

`population_stats` scores moments.  How often a river is above a flood level or below a low-flow level, and how much
volume passes above it, is the other half of what is calibrated on, and needs no sort once the thresholds are the
OBSERVED flows exceeded with probabilities p_1..p_K: the simulated curve at those levels is K counters per (candidate,
basin).  `population_fdc_stats` is `population_stats` -- the same checks, the same observation side, the same four
chains bit for bit -- through hbvx_population_fdc (include/hbvx_pop_fdc.h), which adds [P,K,B] exceedance counts and
volumes and still writes no series; `population_fdc_score` forms two distances between the simulated and the observed
curve from them, and `population_search(fdc_share=...)` mixes one into its objective.

Hbv, Hbv_1_1p and Hbv_2, daily.  The hourly model has the same counts at its gages, and the simulated quantiles that
need the series, in hourly_fdc.py, which reuses `_check_levels`, `fdc_thresholds`, `_fdc_observations` and the score's
body of this file.  Not built: the implicit scheme; period calendars; simulated quantiles here (k_pop keeps no series);
an FDC term in `calibrate` (a count has no derivative); more than 32 thresholds.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _abi, ops
from ._lib import get_library
from .population import EXPLICIT, _candidate_sources, _check, _daily_request, _primal, _sums

EXPORT = 'hbvx_population_fdc'
MAX_THRESHOLDS = _abi.POP_FDC_MAX_THR
DEFAULT_PROBS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98, 0.99)
FDC_METRICS = ('fdc_freq', 'fdc_vol')


def _check_levels(req, x_dict, probs, thresholds, what):
    """What can be refused about `probs` / `thresholds` without the observations: -> (probs as a tuple or None)."""
    if thresholds is not None:
        if probs is not None:
            raise ValueError(f"{what}: give probs or thresholds, not both")
        dev = x_dict['x_phy'].device
        if not torch.is_tensor(thresholds) or thresholds.dim() != 2 or int(thresholds.shape[1]) != req.B \
                or int(thresholds.shape[0]) < 1:
            raise ValueError(f"{what}: thresholds must be [K,{req.B}] (K >= 1 levels per basin), got "
                             f"{tuple(thresholds.shape) if torch.is_tensor(thresholds) else type(thresholds).__name__}")
        if int(thresholds.shape[0]) > MAX_THRESHOLDS:
            raise ValueError(f"{what}: {int(thresholds.shape[0])} thresholds, at most {MAX_THRESHOLDS} per call")
        if thresholds.dtype != torch.float32:
            raise ValueError(f"{what}: thresholds must be float32, got {thresholds.dtype}")
        if thresholds.device != dev:
            raise ValueError(f"{what}: thresholds live on {thresholds.device}, x_phy on {dev}")
        if not bool(torch.isfinite(thresholds).all()):
            raise ValueError(f"{what}: thresholds must be finite")
        return None
    probs = DEFAULT_PROBS if probs is None else probs
    try:
        probs = tuple(float(p) for p in (probs.tolist() if torch.is_tensor(probs) else probs))
    except TypeError as e:
        raise ValueError(f"{what}: probs must be a sequence of exceedance probabilities") from e
    if len(probs) < 1:
        raise ValueError(f"{what}: probs must hold at least one exceedance probability")
    if len(probs) > MAX_THRESHOLDS:
        raise ValueError(f"{what}: {len(probs)} probs, at most {MAX_THRESHOLDS} thresholds per call")
    if not all(0.0 < p < 1.0 for p in probs):           # (a NaN fails both comparisons)
        raise ValueError(f"{what}: probs must lie in (0, 1) (exceedance probabilities), got {list(probs)}")
    return probs


def _ranked(obs, scored):
    """[T,B]: each basin's scored observations sorted descending, -inf below them for the days that are not scored."""
    return torch.where(scored, obs, torch.full_like(obs, -math.inf)).sort(0, descending=True).values


def fdc_thresholds(obs: torch.Tensor, scored: torch.Tensor, probs: Sequence[float], ranked=None) -> torch.Tensor:
    """[K,B] float32: per basin the observed flow exceeded with probability p_k.  obs [T,B] float32, scored [T,B] bool.
    The n scored observations of a basin sorted descending, tau_k is the one at 0-based index min(floor(p_k n), n - 1)
    (the product in float64): without ties exactly floor(p_k n) observations lie above it.  n = 0: +inf."""
    T, B = obs.shape
    n = scored.sum(0, dtype=torch.int64)                                                    # [B]
    ranked = _ranked(obs, scored) if ranked is None else ranked
    p = torch.as_tensor(probs, dtype=torch.float64, device=obs.device).unsqueeze(1)         # [K,1]
    idx = torch.minimum(torch.floor(p * n.double().unsqueeze(0)).long(), (n - 1).unsqueeze(0)).clamp_min(0)
    thr = ranked.gather(0, idx) if T > 0 else obs.new_full((len(probs), B), math.inf)
    return torch.where((n > 0).unsqueeze(0), thr, torch.full_like(thr, math.inf)).contiguous()


def _fdc_observations(req, x_dict, target, weights, probs, thresholds):
    """The observed flow-duration curve at the thresholds: {'probs', 'thresholds' [K,B] float32, 'obs_count' [K,B] int64,
    'obs_volume' [K,B] float64, 'n_days' [B] int64} on the device of x_phy.  A scored day has a finite target and a
    weight > 0; the comparison is the kernel's, float32 `obs > tau`.  Nothing of size [K,T_out,B] is formed: the count
    is a binary search in the basin's sorted observations, the volume the float64 running sum of the sorted observations
    at that count (a sum over descending values)."""
    dev = x_dict['x_phy'].device
    obs = target.to(device=dev, dtype=torch.float32).reshape(req.T_out, req.B)
    scored = torch.isfinite(obs)
    if weights is not None:
        scored = scored & (weights.to(device=dev, dtype=torch.float32) > 0)
    obs = torch.where(scored, obs, torch.zeros_like(obs))
    ranked = _ranked(obs, scored)
    thr = fdc_thresholds(obs, scored, probs, ranked) if thresholds is None else thresholds.detach().contiguous()
    # ascending per basin: the observations <= tau come first (the -inf of the other days among them)
    at_most = torch.searchsorted(ranked.flip(0).t().contiguous(), thr.t().contiguous(), right=True).t()     # [K,B]
    count = req.T_out - at_most
    running = torch.where(torch.isinf(ranked), torch.zeros_like(ranked), ranked).double().cumsum(0)         # [T_out,B]
    volume = torch.where(count > 0, running.gather(0, (count - 1).clamp_min(0)), torch.zeros((), dtype=torch.float64, device=dev))
    return {'probs': None if probs is None else torch.tensor(probs, dtype=torch.float64), 'thresholds': thr,
            'obs_count': count, 'obs_volume': volume, 'n_days': scored.sum(0, dtype=torch.int64)}


def _fdc_request(what, model, x_dict, parameters, candidates, target, names, weights, transform, eps, probs, thresholds,
                 return_series=False):
    """Everything the call can refuse before the model runs -> (population.py's request of the stats form, the observed
    curve).  candidates None: the search."""
    # the levels before the request: `_daily_request` ends by asking the library for hbvx_population_stats
    probs = _check_levels(_check(EXPLICIT, model, x_dict, parameters, target, names, weights, what), x_dict, probs,
                          thresholds, what)
    rq = _daily_request(EXPLICIT, what, 'stats', model, x_dict, parameters, candidates, target, names, weights, transform,
                        eps, return_series=return_series)
    get_library().require(EXPORT)
    return rq, _fdc_observations(rq.req, x_dict, target, weights, probs, thresholds)


def _fdc_run(rq, curve):
    """The module once at rq.parameters, then rq.candidates through ops.population_fdc: `population_stats`' dictionary
    and 'fdc'."""
    outputs, main, t_first = _primal(EXPLICIT, rq.model, rq.req, rq.x_dict, rq.parameters)
    sources, route = _candidate_sources(rq.model, rq.names, rq.candidates)
    ob = rq.ob
    flow = ops.PopTerm(ob['target'], ob['w'], ob['shift'], ob['eps'], rq.transform)
    flow_out, (count, volume) = ops.population_fdc(main, sources, route, flow, curve['thresholds'], t_first, rq.return_series)
    out = _sums(flow_out, ob, rq.transform, rq, outputs)
    out['fdc'] = dict(curve, count=count, volume=volume)
    return out


def population_fdc_stats(model, x_dict: dict, parameters, candidates: torch.Tensor, target,
                         names: Optional[Sequence[str]] = None, weights=None, transform: str = 'none', eps=None,
                         probs: Optional[Sequence[float]] = None, thresholds: Optional[torch.Tensor] = None,
                         return_series: bool = False) -> dict:
    """`population_stats`, and each candidate's flow-duration curve sampled at K thresholds per basin, from one launch
    that writes no series: on how many scored days the routed streamflow was above each threshold, and the volume above.

    candidates, target, names, weights, transform, eps, return_series: as `population_stats`.  A weight is a mask here:
    a day with a finite target and a weight > 0 is a scored day and counts once.
    probs        exceedance probabilities in (0, 1), at most 32; None (without `thresholds`): 0.01, 0.02, 0.05, 0.1,
                 0.2 .. 0.9, 0.95, 0.98, 0.99.  Per basin the n scored observations are sorted descending and tau_k is the
                 one at 0-based index min(floor(p_k n), n - 1), float32: without ties exactly floor(p_k n) observations
                 lie above it.  A basin without a scored day gets +inf.
    thresholds   [K,B] float32 on the device of x_phy, finite, in any order, K <= 32: levels of the caller's own (a flood
                 stage) instead of `probs`.
    Returns `population_stats`' dictionary, the same keys and the same bits, and
      'fdc': {'probs': [K] float64 or None, 'thresholds': [K,B] float32,
              'count': [P,K,B] int32, 'volume': [P,K,B] float32 (a sum over ascending days of the flows above tau),
              'obs_count': [K,B] int64, 'obs_volume': [K,B] float64 (the same of the observations, `obs > tau` in
              float32), 'n_days': [B] int64 the scored days}.
    The comparison is on the streamflow itself under every transform.  A slot's count and volume depend on that
    candidate and that threshold alone: not on K, the order of the thresholds, the other candidates or return_series;
    two calls agree bit for bit.

    Refused before the model runs: everything `population_stats` refuses; probs and thresholds together; probs outside
    (0, 1) or empty; more than 32 of either; a wrong shape, dtype or device of thresholds, or non-finite ones
    (ValueError); HbvAdj, Hbv_2_hourly, Hbv_2_mts (NotImplementedError); a library without hbvx_population_fdc
    (HbvxError)."""
    return _fdc_run(*_fdc_request("population_fdc_stats", model, x_dict, parameters, candidates, target, names, weights,
                                  transform, eps, probs, thresholds, return_series))


def population_fdc_score(stats: dict, metric: str) -> torch.Tensor:
    """[P,B] float64 distance between each candidate's sampled flow-duration curve and the observed one, from what
    `population_fdc_stats` returned; zero is perfect, NaN where it is undefined.
      'fdc_freq'  mean_k |count_k - obs_count_k| / n_days: the mean distance between the two exceedance curves along the
                  probability axis.  NaN without a scored day.
      'fdc_vol'   the mean over the k with obs_volume_k > 0 of |volume_k - obs_volume_k| / obs_volume_k.  NaN where there
                  is no such k, or where one of the candidate's volumes is not finite."""
    if metric not in FDC_METRICS:
        raise ValueError(f"metric must be one of {list(FDC_METRICS)}, got {metric!r}")
    return _fdc_score(stats['fdc'], 'n_days', metric)


def _fdc_score(f: dict, scored: str, metric: str) -> torch.Tensor:
    """`population_fdc_score` on an 'fdc' dictionary whose count of scored steps is under the key `scored` ('n_days';
    'n_hours' for the hourly model's `hourly_fdc_score`); metric is one of FDC_METRICS."""
    count, volume = f['count'], f['volume'].double()
    dev = count.device
    nan = torch.full((count.shape[0], count.shape[2]), float('nan'), dtype=torch.float64, device=dev)
    if metric == 'fdc_freq':
        n = f[scored].to(dev).double()
        dist = (count.double() - f['obs_count'].to(dev).double().unsqueeze(0)).abs().mean(1)
        return torch.where(n > 0, dist / n.clamp_min(1.0), nan)
    ov = f['obs_volume'].to(device=dev, dtype=torch.float64).unsqueeze(0)      # [1,K,B]
    has = ov > 0
    rel = torch.where(has, (volume - ov).abs() / torch.where(has, ov, torch.ones_like(ov)), torch.zeros_like(volume))
    k = has.sum(1)
    ok = (k > 0) & torch.isfinite(volume).all(1)
    return torch.where(ok, rel.sum(1) / k.clamp_min(1).double(), nan)
