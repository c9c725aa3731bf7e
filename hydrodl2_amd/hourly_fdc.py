"""Flow-duration scores of `Hbv_2_hourly` at its gages: the flow-duration curve of every candidate of a population, in
the two forms the hourly gage series allows, and scores on them.

`population_fdc_stats` samples a daily candidate's curve at thresholds fixed on the observed side, because k_pop keeps
no series: a curve becomes K counters.  Stage 2 of `hourly_population_stats` DOES hold every candidate's hourly gage
series [p,T,G] on the device, so here both are possible (include/hbvx_gage_fdc.h states the arithmetic line by line):

  counts and volumes  on how many scored hours the series lies above each observed threshold, and the volume above it
                      -- the daily call's rule, one ordered pass (hbvx_gage_population_fdc);
  quantiles           the candidate's OWN curve at the probabilities: a sort per (candidate, gage) column in LDS and the
                      flows at K ranks (hbvx_gage_population_quantiles).  A sort does no arithmetic: a quantile is a value
                      of the series, bit for bit.

  hourly_population_fdc_stats  `hourly_population_stats`' dictionary, same bits, plus 'fdc';
  hourly_fdc_score             'fdc_freq' and 'fdc_vol' (`population_fdc_score`'s body), 'fdc_quantile' (the distance of
                               the two curves along the flow axis), 'fdc_slope' (the mid-segment log slope).
`hourly_routing_search(fdc_share=...)` (hourly_events.py) mixes one of them into its objective: route_a / route_b
reshape the curve and hardly move a KGE.

The observed side -- the sort of the observations, the thresholds, the observed counts and volumes -- stays on the host
side of the call (`population_fdc._fdc_observations`, with gages in the place of basins).

Not built: FDC for HbvAdj and Hbv_2_mts; segment volumes of the simulated curve (FHV / FLV); more than 32 levels per
call; quantiles of records longer than 16 384 hours (refused; the counts and volumes have no such limit); a device-side
observed half; gradients of any of these scores; a search over unit parameters.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _abi, ops
from .hourly_population import _Gages, _evaluate
from .population_fdc import FDC_METRICS, _check_levels, _fdc_observations, _fdc_score

WHAT = "hourly_population_fdc_stats"
HOURLY_FDC_METRICS = FDC_METRICS + ('fdc_quantile', 'fdc_slope')
QUANTILE_METRICS = ('fdc_quantile', 'fdc_slope')
SLOPE_PROBS = (0.2, 0.7)
MAX_QUANTILE_HOURS = _abi.GAGE_QUANT_MAX_T


def fdc_ranks(n: torch.Tensor, probs: Sequence[float]) -> torch.Tensor:
    """[K,G] int32: rank[k][g] = min(floor(p_k n_g), n_g - 1), the product in float64 -- the index `fdc_thresholds` reads
    the sorted observations at.  n [G] the scored hours per gage; a gage without one gets -1, which no column has."""
    p = torch.as_tensor(probs, dtype=torch.float64, device=n.device).unsqueeze(1)
    n = n.to(torch.int64)
    return torch.minimum(torch.floor(p * n.double().unsqueeze(0)).long(), (n - 1).unsqueeze(0)).to(torch.int32).contiguous()


class _FdcHook:
    """What `hourly_population._evaluate` calls for the flow-duration statistics of every chunk's series.  The observed
    half is formed on the first `check` and kept: a search hands one hook to every round."""

    def __init__(self, x_dict, target, weights, periods, probs, thresholds, fdc_target, what=WHAT):
        self.x_dict, self.target, self.weights, self.periods = x_dict, target, weights, periods
        self.probs, self.thresholds, self.fdc_target, self.what = probs, thresholds, fdc_target, what
        self.quantiles = thresholds is None
        self.exports = ('hbvx_gage_population_fdc',) + (
            ('hbvx_gage_population_quantiles', 'hbvx_gage_quantiles_workspace_bytes') if self.quantiles else ())
        self.curve = None
        self.parts = []
        self.bytes = 0

    def check(self, T, G, dev):
        self.parts = []
        if self.curve is not None:
            return
        what = self.what
        req = _Gages(T, G)
        probs = _check_levels(req, self.x_dict, self.probs, self.thresholds, what)
        if self.quantiles and T > MAX_QUANTILE_HOURS:
            raise ValueError(f"{what}: the simulated quantiles of `probs` are sorted in LDS, at most {MAX_QUANTILE_HOURS} "
                             f"hours per column; the record has {T} (`thresholds=` has no such limit)")
        src, weights = self.fdc_target, None
        if self.periods is None:
            weights = self.weights
            if src is None:
                src = self.target
        elif src is None:
            raise ValueError(f"{what}: with a calendar `target` holds period rows; give the observed HOURLY series as "
                             f"fdc_target [{T},{G}]")
        if not torch.is_tensor(src):
            src = torch.as_tensor(src)
        if tuple(src.shape) not in ((T, G), (T, G, 1)):
            raise ValueError(f"{what}: fdc_target must be [{T},{G}] or [{T},{G},1] (the hourly record at the gages), got "
                             f"{tuple(src.shape)}")
        obs = src.detach().to(device=dev, dtype=torch.float32).reshape(T, G)
        if weights is not None:
            weights = weights.detach().reshape(T, G)
        curve = _fdc_observations(req, self.x_dict, obs, weights, probs, self.thresholds)
        curve['n_hours'] = curve.pop('n_days')
        scored = torch.isfinite(obs)
        if weights is not None:
            scored = scored & (weights.to(device=dev, dtype=torch.float32) > 0)
        self.scored = scored.to(torch.uint8).contiguous()
        K = int(curve['thresholds'].shape[0])
        if self.quantiles:
            curve['rank'] = fdc_ranks(curve['n_hours'], probs)
        self.curve = curve
        # count and volume; with the quantiles those and the sort's workspace, one series' worth
        self.bytes = 8 * K * G + ((4 * K * G + 4 * T * G) if self.quantiles else 0)

    def chunk(self, series):
        got = ops.gage_fdc(series, self.scored, self.curve['thresholds'])
        if self.quantiles:
            got = got + (ops.gage_quantiles(series, self.scored, self.curve['rank']),)
        self.parts.append(got)

    def result(self) -> dict:
        got = [self.parts[0][i] if len(self.parts) == 1 else torch.cat([p[i] for p in self.parts])
               for i in range(len(self.parts[0]))]
        out = dict(self.curve, count=got[0], volume=got[1])
        if self.quantiles:
            out['quantile'] = got[2]
        return out


def _fdc_stats(hook, model, x_dict, parameters, target, candidates, distr_candidates, names, weights, periods, transform,
               eps, return_series, max_candidates) -> dict:
    out = _evaluate(model, x_dict, parameters, target, candidates, distr_candidates, names, weights, periods, transform, eps,
                    return_series, max_candidates, hook)
    out['fdc'] = hook.result()
    return out


def hourly_population_fdc_stats(model, x_dict: dict, parameters, target, candidates: Optional[torch.Tensor] = None,
                                distr_candidates: Optional[torch.Tensor] = None, names: Optional[Sequence[str]] = None,
                                weights=None, periods=None, transform: str = 'none', eps=None, return_series: bool = False,
                                max_candidates: Optional[int] = None, probs: Optional[Sequence[float]] = None,
                                thresholds: Optional[torch.Tensor] = None, fdc_target=None) -> dict:
    """`hourly_population_stats` (same arguments, same dictionary, same bits) plus every candidate's flow-duration curve at
    the gages, from the hourly gage series stage 2 holds.

    probs        exceedance probabilities in (0, 1), at most 32; None (without `thresholds`): `population_fdc_stats`'
                 fifteen.  Per gage the n scored observations are sorted descending (on the host side, as there) and
                 tau_k is the one at 0-based index rank_k = min(floor(p_k n), n - 1), float32; a gage without a scored
                 hour gets +inf and rank -1.  With `probs` the call also sorts every candidate's own column and returns
                 its flow at the same ranks: the record is then at most 16 384 hours long.
    thresholds   [K,G] float32 on the device of x_phy, finite, any order, K <= 32: levels of the caller's own (a flood
                 stage) instead of `probs`.  No quantiles then: hbvx_gage_population_quantiles is neither required nor
                 called, and the record may have any length.
    fdc_target   [T,G] or [T,G,1]: the observed HOURLY series the curve is formed on.  Without a calendar it defaults
                 to `target`, and a scored hour has a finite observation and a weight > 0 (a weight is a mask here).
                 With a calendar `target` holds period rows: fdc_target must be given, a scored hour has a finite
                 observation, and the weights, which belong to the periods, do not enter.
    Returns the dictionary of `hourly_population_stats` and
      'fdc': {'probs': [K] float64 or None, 'thresholds': [K,G] float32, 'obs_count': [K,G] int64, 'obs_volume': [K,G]
              float64 (`obs > tau` in float32), 'n_hours': [G] int64 the scored hours,
              'count': [P,K,G] int32 the scored hours with series > tau, 'volume': [P,K,G] float32 the float32 sum of
              those flows in hour order,
              with `probs` also 'rank': [K,G] int32 and 'quantile': [P,K,G] float32, the flow at index rank_k of the
              candidate's scored hours sorted descending -- NaN where the gage has no scored hour or a scored hour of
              the candidate is NaN}.
    A series equal to the observations has quantile == thresholds.  Per chunk of candidates the call is stage 2 with its
    hourly series kept, then the exports of include/hbvx_gage_fdc.h on that series; memory and chunking are
    `hourly_population_stats`' own (the sort's workspace, one more series, is counted).  A slot's bits depend on neither
    the split, the other candidates, K, the order of the levels nor return_series; two calls agree bit for bit.

    Refused before the model runs (ValueError): what `hourly_population_stats` refuses; probs and thresholds together;
    probs outside (0, 1) or empty; more than 32 of either; a wrong shape, dtype or device of thresholds, or non-finite
    ones; an fdc_target of another shape than [T,G], or none with a calendar; `probs` on more than 16 384 hours."""
    hook = _FdcHook(x_dict, target, weights, periods, probs, thresholds, fdc_target)
    return _fdc_stats(hook, model, x_dict, parameters, target, candidates, distr_candidates, names, weights, periods,
                      transform, eps, return_series, max_candidates)


def _check_metric(metric, what="hourly_fdc_score"):
    if metric not in HOURLY_FDC_METRICS:
        raise ValueError(f"{what}: metric must be one of {list(HOURLY_FDC_METRICS)}, got {metric!r}")


def hourly_fdc_score(stats: dict, metric: str, slope_probs: Sequence[float] = SLOPE_PROBS) -> torch.Tensor:
    """[P,G] float64 distance between each candidate's flow-duration curve and the observed one, from what
    `hourly_population_fdc_stats` returned; zero is perfect, NaN where it is undefined.
      'fdc_freq', 'fdc_vol'   `population_fdc_score`'s, on the counts and volumes above the observed thresholds;
      'fdc_quantile'  the mean over the k with tau_k > 0 (and finite) of |q_k - tau_k| / tau_k: the distance between the
                      two curves along the flow axis.  NaN without such a k, or where one of the candidate's q_k is not
                      finite;
      'fdc_slope'     |s - s_obs| / |s_obs| with s = log q_a - log q_b, s_obs the same of tau: the relative error of the
                      mid-segment slope of the curve in log flow, a, b = slope_probs (both must be among 'probs').  NaN
                      where one of the four flows is not positive and finite, or s_obs == 0.
    The last two need 'quantile' (a call with `probs`): ValueError without it."""
    _check_metric(metric)
    f = stats['fdc']
    if metric in FDC_METRICS:
        return _fdc_score(f, 'n_hours', metric)
    if 'quantile' not in f:
        raise ValueError(f"hourly_fdc_score: {metric!r} needs the simulated quantiles; call hourly_population_fdc_stats "
                         "with probs, not thresholds")
    q = f['quantile'].double()                                                      # [P,K,G]
    dev = q.device
    tau = f['thresholds'].to(device=dev, dtype=torch.float64).unsqueeze(0)          # [1,K,G]
    nan = torch.full((q.shape[0], q.shape[2]), float('nan'), dtype=torch.float64, device=dev)
    if metric == 'fdc_quantile':
        has = (tau > 0) & torch.isfinite(tau)
        rel = torch.where(has, (q - tau).abs() / torch.where(has, tau, torch.ones_like(tau)), torch.zeros_like(q))
        k = has.sum(1)                                                              # [1,G]
        ok = (k > 0) & torch.isfinite(q).all(1)
        return torch.where(ok, rel.sum(1) / k.clamp_min(1).double(), nan)
    probs = [float(p) for p in f['probs'].tolist()]
    try:
        a, b = (probs.index(float(p)) for p in slope_probs)
    except ValueError as e:
        raise ValueError(f"hourly_fdc_score: slope_probs {tuple(slope_probs)} must both be among probs {probs}") from e
    flows = torch.stack([q[:, a], q[:, b], tau[:, a].expand_as(q[:, a]), tau[:, b].expand_as(q[:, b])])    # [4,P,G]
    ok = ((flows > 0) & torch.isfinite(flows)).all(0)
    lg = torch.log(torch.where(ok.unsqueeze(0), flows, torch.ones_like(flows)))
    s, s_obs = lg[0] - lg[1], lg[2] - lg[3]
    ok = ok & (s_obs != 0)
    return torch.where(ok, (s - s_obs).abs() / torch.where(ok, s_obs.abs(), torch.ones_like(s_obs)), nan)
