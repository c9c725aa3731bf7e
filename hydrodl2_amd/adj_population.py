"""Population evaluation for `HbvAdj`: `adj_population_cost`, `adj_population_stats`, `adj_population_period_stats`,
`adj_population_search` (`HbvAdj.population_cost` / `.population_stats` / `.population_period_stats` /
`.population_search`).

What population.py does for Hbv, Hbv_1_1p and Hbv_2, for the implicit scheme: the module runs ONCE at `parameters` (its
warm-up pass, its dy_drop draws and the recorded descriptor of its main pass), then hbvx_adj_population_cost /
hbvx_adj_population_stats (include/hbvx.h) solve every candidate's days in registers -- the same day functions the
module's forward calls, under the module's Newton policy -- and write [P,B] numbers.  The route this replaces is P
forwards of the module, each with its [T,B] series, its routing launch and a float64 reduction.

Semantics are population.py's, with these differences:
  - the series scored is 'flow_sim';
  - candidates are in raw (pre-sigmoid) space, as HbvAdj takes its parameters;
  - the warm-up is a pass of its own whose end state the recorded main pass starts from, so every recorded day is
    scored (t_first = 0) and the candidates do not reach the warm-up (it reads row warm_up - 1, as in a plain call);
  - newton_stop='global' is refused: the batch-wide stopping rule votes over the 64 lanes of whichever kernel runs, and
    a candidate's cost must not depend on that.
`population_score` (population.py) turns what `adj_population_stats` returns into scores, unchanged.

`adj_population_period_stats` is `population_period_stats` for the model (hbvx_adj_population_period): the flow averaged
over the periods of a calendar -- 8-day composites, months -- and, from the same launch, one observed STORAGE on a
calendar of its own.  The implicit scheme solves for its five storages every day, so the second series is the ensemble
mean of SNOWPACK, MELTWATER, SM, SUZ or SLZ at the end of each day; fluxes are not offered.

The generic `population_*` keep refusing the model: these are explicit entry points, as `adj_jvp_batch` is.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _abi, ops
from ._lib import get_library
from .calibrate import _NO_TARGET, _check_request
from .population import (OBJECTIVES, _calendar, _candidate_sources, _check_aux, _check_candidates, _check_period_target,
                         _check_search, _mixed_cost, _objective_cost, _observations, _period_days, _search,
                         population_score)

AUX_KEYS = tuple(_abi.ADJ_POP_AUX_SERIES)       # 'SNOWPACK', 'MELTWATER', 'SM', 'SUZ', 'SLZ'


def _check(model, x_dict, parameters, target, names, weights, what):
    """Everything that can be refused without running the model."""
    if getattr(model, '_model_id', None) != _abi.MODEL_HBVADJ:
        raise NotImplementedError(f"{what} is for HbvAdj, not {type(model).__name__}: Hbv, Hbv_1_1p and Hbv_2 go through "
                                  f"hydrodl2_amd.{what[4:]}")
    req = _check_request(model, x_dict, parameters, target, names, 'flow_sim', weights, 1, what=what)
    if model.newton_stop == 'global':
        raise ValueError(f"{what}: newton_stop='global' (one stopping vote over the lanes of a wave) would make a "
                         "candidate's cost depend on the basins that share its wave; use newton_stop='lane'")
    if model.comprout:
        raise ValueError(f"{what}: comprout=True routes every member, not the ensemble mean; not supported")
    return req


def _primal(model, req, x_dict, parameters):
    """The one run of the module at `parameters`: (outputs, the recorded call of its main pass)."""
    with torch.no_grad(), ops.record_paths(want_traj=False) as records:     # the kernel solves every day itself
        outputs = model(x_dict, parameters)
    main = records[-1]
    cfg = main.cfg
    if cfg.T != req.T_out or cfg.B != req.B:
        raise RuntimeError(f"{type(model).__name__} ran {cfg.T} days on {cfg.B} basins, expected {req.T_out} on {req.B}")
    return outputs, main


def adj_population_cost(model, x_dict: dict, parameters, candidates: torch.Tensor, target,
                        names: Optional[Sequence[str]] = None, weights=None, return_series: bool = False) -> dict:
    """sum_t w (flow_sim - target)^2 per basin for each of P candidate static-parameter sets of `HbvAdj`.

    candidates  [P,B,C] float32 on the device of x_phy: raw (pre-sigmoid) values for the columns
                `jacobian_columns(model, names)` returns, in that order.  Candidate c stands in for
                parameters[T-1, b, columns]; everything else -- dynamic parameters, the other static columns, the
                forcings, the state the warm-up pass ends in -- is shared.
    target      [T_out,B] or [T_out,B,1], T_out = the days after the warm-up; a NaN is a missing observation (weight 0).
    weights     [T_out,B] >= 0 or None (ones).
    Returns {'cost': [P,B] float32, +inf where the sum is not finite, 'n_obs': [B] int64, 'columns': [C indices],
    'outputs': the primal dictionary at `parameters`, 'series': [P,T_out,B] each candidate's flow_sim (routed when the
    model routes), only with return_series}.

    The module runs once at `parameters`: that run does the warm-up, draws the dy_drop masks -- one set per lane,
    shared by all candidates -- and leaves the module as one plain call.  The cost is a float32 chain of fused
    multiply-adds over ascending days; two calls give the same bits, and a candidate's bits do not depend on the other
    candidates or on return_series.

    Refused before the model runs: any model but HbvAdj (NotImplementedError); graph=True, newton_stop='global',
    comprout=True, dynamic or unknown names, a wrong shape / dtype / device of candidates, target or weights, infinite
    targets, negative or non-finite weights (ValueError); a library without hbvx_adj_population_cost (HbvxError)."""
    req = _check(model, x_dict, parameters, target, names, weights, "adj_population_cost")
    _check_candidates(req, x_dict, candidates)
    get_library().require("hbvx_adj_population_cost")

    outputs, main = _primal(model, req, x_dict, parameters)
    dev = main.x.device
    tgt = target.to(device=dev, dtype=torch.float32).reshape(req.T_out, req.B)
    miss = torch.isnan(tgt)
    if weights is None and not bool(miss.any()):
        w = None
        n_obs = torch.full((req.B,), req.T_out, dtype=torch.int64, device=dev)
    else:
        w = torch.ones_like(tgt) if weights is None else weights.to(device=dev, dtype=torch.float32)
        w = torch.where(miss, torch.zeros_like(w), w).contiguous()
        tgt = torch.where(miss, torch.zeros_like(tgt), tgt)     # 0 * NaN would be NaN: the kernel multiplies what it gets
        n_obs = (w > 0).sum(0, dtype=torch.int64)

    sources, route = _candidate_sources(model, names, candidates)
    cost, series = ops.adj_population_cost(main, sources, route, tgt.contiguous(), w, 0, return_series)
    cost = torch.where(torch.isfinite(cost), cost, torch.full_like(cost, float('inf')))
    out = {'cost': cost, 'n_obs': n_obs, 'columns': list(req.cols), 'outputs': outputs}
    if return_series:
        out['series'] = series
    return out


def _stats(model, req, x_dict, parameters, candidates, names, ob, transform, return_series):
    outputs, main = _primal(model, req, x_dict, parameters)
    sources, route = _candidate_sources(model, names, candidates)
    sse, s1, s2, s3, series = ops.adj_population_stats(main, sources, route, ob['target'], ob['w'], ob['shift'],
                                                       ob['eps'], transform, 0, return_series)
    out = {'sse': sse, 's1': s1, 's2': s2, 's3': s3, 'shift': ob['shift'], 'obs': ob['obs'], 'transform': transform,
           'eps': ob['eps'], 'n_obs': ob['n_obs'], 'columns': list(req.cols), 'outputs': outputs}
    if return_series:
        out['series'] = series
    return out


def adj_population_stats(model, x_dict: dict, parameters, candidates: torch.Tensor, target,
                         names: Optional[Sequence[str]] = None, weights=None, transform: str = 'none', eps=None,
                         return_series: bool = False) -> dict:
    """The sums from which `population_score` forms NSE, KGE, correlation, variability and bias of each of P candidate
    static-parameter sets of `HbvAdj`, on flow_sim (transform 'none'), its square root ('sqrt') or log(flow + eps)
    ('log').  Arguments as `adj_population_cost`; transform, eps and the returned dictionary as
    `hydrodl2_amd.population_stats`.  Under 'none', 'sse' has the bits of `adj_population_cost`'s 'cost' (before its +inf
    rule), and 'series' has them under every transform.

    Refused before the model runs: everything `adj_population_cost` refuses; an unknown transform; eps <= 0 or
    non-finite; a negative target under 'sqrt'; a target <= -eps under 'log' (ValueError); a library without
    hbvx_adj_population_stats (HbvxError)."""
    req = _check(model, x_dict, parameters, target, names, weights, "adj_population_stats")
    _check_candidates(req, x_dict, candidates)
    ob = _observations(req, x_dict, target, weights, transform, eps, "adj_population_stats")
    get_library().require("hbvx_adj_population_stats")
    return _stats(model, req, x_dict, parameters, candidates, names, ob, transform, return_series)


def _period_request(model, x_dict, parameters, candidates, target, periods, aux_target, aux_key, aux_periods, names,
                    weights, aux_weights, transform, eps, what):
    """Everything `adj_population_period_stats` can refuse before the model runs, and what it works on: population.py's
    `_period_request` with this module's `_check` and the five storages as aux keys -> (req, ob, aux_ob or None, (flow
    closing days, aux closing days or None) as int64 CPU tensors)."""
    req = _check(model, x_dict, parameters, _NO_TARGET, names, None, what)
    if candidates is not None:
        _check_candidates(req, x_dict, candidates)
    ends_f = _calendar(periods, req.T_out, "periods", what)
    _check_period_target(req, x_dict, target, weights, int(ends_f.numel()), what)
    ends_a = aux_ob = None
    if aux_key is None and aux_target is None:
        if aux_periods is not None or aux_weights is not None:
            raise ValueError(f"{what}: {'aux_periods' if aux_periods is not None else 'aux_weights'} without aux_key")
    else:
        ends_a = _calendar(aux_periods, req.T_out, "aux_periods", what)
        _check_aux(req, x_dict, aux_target, aux_key, aux_weights, what, rows=int(ends_a.numel()), keys=AUX_KEYS)
    ob = _observations(req, x_dict, target, weights, transform, eps, what, rows=int(ends_f.numel()))
    if ends_a is not None:
        aux_ob = _observations(req, x_dict, aux_target, aux_weights, 'none', None, what, rows=int(ends_a.numel()))
    get_library().require("hbvx_adj_population_period")
    return req, ob, aux_ob, (ends_f, ends_a)


def _period(model, req, x_dict, parameters, candidates, names, ob, transform, aux_key, aux_ob, ends, return_series):
    outputs, main = _primal(model, req, x_dict, parameters)
    sources, route = _candidate_sources(model, names, candidates)
    dev = main.x.device
    end_f, end_a = (None if e is None else e.to(device=dev, dtype=torch.int32) for e in ends)
    if aux_ob is None:
        flow, aux = ops.adj_population_period(main, sources, route, ob['target'], ob['w'], ob['shift'], ob['eps'],
                                              transform, end_f, t_first=0, want_sim=return_series)
    else:
        flow, aux = ops.adj_population_period(main, sources, route, ob['target'], ob['w'], ob['shift'], ob['eps'],
                                              transform, end_f, _abi.ADJ_POP_AUX_SERIES[aux_key], aux_ob['target'],
                                              aux_ob['w'], aux_ob['shift'], end_a, 0, return_series)
    out = {'columns': list(req.cols), 'outputs': outputs}
    for name, got, o, tr, e in (('flow', flow, ob, transform, ends[0]), ('aux', aux, aux_ob, 'none', ends[1])):
        if got is None:
            continue
        sub = dict(zip(('sse', 's1', 's2', 's3'), got[:4]))
        sub.update(shift=o['shift'], obs=o['obs'], transform=tr, eps=o['eps'], n_obs=o['n_obs'], columns=list(req.cols),
                   outputs=outputs, period_ends=e.clone(), period_days=_period_days(e))
        if return_series:
            sub['series'] = got[4]
        out[name] = sub
    if aux is not None:
        out['aux']['key'] = aux_key
    return out


def adj_population_period_stats(model, x_dict: dict, parameters, candidates: torch.Tensor, target, periods=None,
                                aux_target=None, aux_key: Optional[str] = None, aux_periods=None,
                                names: Optional[Sequence[str]] = None, weights=None, aux_weights=None,
                                transform: str = 'none', eps=None, return_series: bool = False) -> dict:
    """`hydrodl2_amd.population_period_stats` for `HbvAdj`: each candidate's flow_sim, and optionally one of the
    model's five storages, is averaged over the periods of a calendar -- 8-day composites, months -- inside the kernel,
    and the period means are what meets the targets (hbvx_adj_population_period).  Nothing but [P,B] numbers is
    written; no daily series and no trajectory exists anywhere.

    periods, aux_periods, target, weights, aux_target, aux_weights, transform, eps, return_series and the returned
    dictionary {'flow', 'aux' (only with aux_key), 'columns', 'outputs'} -- each sub-dictionary with 'period_ends',
    'period_days', 'n_obs' counting periods and 'series' [P,K,B] period means -- are `population_period_stats`';
    `population_score` works on either sub-dictionary unchanged.  The differences are `adj_population_stats`': the flow
    is 'flow_sim', candidates are raw, every recorded day is scored (t_first = 0) and the module runs once.
    aux_key      'SNOWPACK', 'MELTWATER', 'SM', 'SUZ' or 'SLZ': the day's value is the ensemble mean over the members
                 of that storage at the END of the day, as the solve leaves it (not clamped at zero), never routed and
                 never transformed.  None (with aux_target None): no aux term; the flow numbers have the same bits
                 either way.
    With both calendars None and no aux term, 'sse', 's1', 's2', 's3' and 'series' have `adj_population_stats`' bits.

    Refused before the model runs: everything `adj_population_stats` refuses; everything `population_period_stats`
    refuses about calendars, period targets and aux arguments; an aux_key that is not one of the five storages
    (ValueError); any model but HbvAdj (NotImplementedError); a library without hbvx_adj_population_period
    (HbvxError)."""
    what = "adj_population_period_stats"
    req, ob, aux_ob, ends = _period_request(model, x_dict, parameters, candidates, target, periods, aux_target, aux_key,
                                            aux_periods, names, weights, aux_weights, transform, eps, what)
    return _period(model, req, x_dict, parameters, candidates, names, ob, transform, aux_key, aux_ob, ends, return_series)


def adj_population_search(model, x_dict: dict, parameters, target, names: Optional[Sequence[str]] = None,
                          n_candidates: int = 256, n_rounds: int = 1, shrink: float = 0.5, weights=None,
                          generator: Optional[torch.Generator] = None, objective: str = 'sse', transform: str = 'none',
                          eps=None, aux_target=None, aux_key: Optional[str] = None, aux_weights=None,
                          aux_objective: str = 'nse', aux_share: float = 0.5, periods=None, aux_periods=None):
    """`hydrodl2_amd.population_search` for `HbvAdj`: the same per-basin shrinking random search over the static row --
    the same draws from `generator`, the same rounds, the same tie rule, the same history -- with every round one
    `adj_population_cost` call (objective 'sse' with transform 'none') or one `adj_population_stats` call (anything
    else).  The row is raw: a draw is the logit of a unit-interval value clipped to [1e-4, 1 - 1e-4].

    periods / aux_periods / aux_target / aux_key / aux_weights / aux_objective / aux_share have `population_search`'s
    meaning, with aux_key one of the five storages: any of the first five makes every round one
    `adj_population_period_stats` call (a calendar left None is daily), the quantity minimised is 1 - score of the flow
    or, with an aux term, (1 - aux_share) * cost_flow + aux_share * cost_aux, +inf where either term has no score, and
    history['score'] / history['score_aux'] hold the scores.  With all of them at their defaults the function is the one
    above, bit for bit.

    Returns (best, history) as `population_search`; the inputs are not modified.  dy_drop > 0 makes the cost
    stochastic: ValueError."""
    what = "adj_population_search"
    _check_search(model, n_candidates, n_rounds, shrink, objective, what)
    joint = aux_target is not None or aux_key is not None or aux_weights is not None
    if joint or periods is not None or aux_periods is not None:
        if joint:
            if aux_objective not in OBJECTIVES:
                raise ValueError(f"{what}: aux_objective must be one of {list(OBJECTIVES)}, got {aux_objective!r}")
            if not 0.0 <= float(aux_share) <= 1.0:          # (a NaN fails both comparisons)
                raise ValueError(f"{what}: aux_share must lie in [0, 1], got {aux_share!r}")
            if aux_objective == 'sse' and objective != 'sse':
                raise ValueError(f"{what}: aux_objective 'sse' with objective {objective!r} would add a squared error to "
                                 "1 - score: two scales in one sum")
        req, ob, aux_ob, ends = _period_request(model, x_dict, parameters, None, target, periods, aux_target, aux_key,
                                                aux_periods, names, weights, aux_weights, transform, eps, what)

        def evaluate_periods(cands):
            st = _period(model, req, x_dict, parameters, cands, names, ob, transform, aux_key, aux_ob, ends, False)
            score = population_score(st['flow'], objective)
            if not joint:
                return _objective_cost(score, objective), score
            score_aux = population_score(st['aux'], aux_objective)
            return _mixed_cost(_objective_cost(score, objective), _objective_cost(score_aux, aux_objective),
                               float(aux_share)), (score, score_aux)

        return _search(req, x_dict, parameters, evaluate_periods, True, n_candidates, n_rounds, shrink, generator,
                       joint or objective != 'sse', joint)
    req = _check(model, x_dict, parameters, target, names, weights, "adj_population_search")
    by_stats = objective != 'sse' or transform != 'none'
    if by_stats:
        ob = _observations(req, x_dict, target, weights, transform, eps, "adj_population_search")
        get_library().require("hbvx_adj_population_stats")
    else:
        get_library().require("hbvx_adj_population_cost")       # before the first draw is made

    def evaluate(cands):
        """(cost, score or None) [P,B] of one round's candidates."""
        if not by_stats:
            return adj_population_cost(model, x_dict, parameters, cands, target, names, weights)['cost'], None
        st = _stats(model, req, x_dict, parameters, cands, names, ob, transform, False)
        score = population_score(st, objective)
        return _objective_cost(score, objective), score

    return _search(req, x_dict, parameters, evaluate, True, n_candidates, n_rounds, shrink, generator,
                   objective != 'sse')
