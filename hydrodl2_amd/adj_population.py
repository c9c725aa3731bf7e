"""Population evaluation for `HbvAdj`: `adj_population_cost`, `adj_population_stats`, `adj_population_search`
(`HbvAdj.population_cost` / `.population_stats` / `.population_search`).

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

The generic `population_*` keep refusing the model: these are explicit entry points, as `adj_jvp_batch` is.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _abi, ops
from ._lib import get_library
from .calibrate import _check_request
from .population import (_candidate_sources, _check_candidates, _check_search, _objective_cost, _observations, _search,
                         population_score)


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


def adj_population_search(model, x_dict: dict, parameters, target, names: Optional[Sequence[str]] = None,
                          n_candidates: int = 256, n_rounds: int = 1, shrink: float = 0.5, weights=None,
                          generator: Optional[torch.Generator] = None, objective: str = 'sse', transform: str = 'none',
                          eps=None):
    """`hydrodl2_amd.population_search` for `HbvAdj`: the same per-basin shrinking random search over the static row --
    the same draws from `generator`, the same rounds, the same tie rule, the same history -- with every round one
    `adj_population_cost` call (objective 'sse' with transform 'none') or one `adj_population_stats` call (anything
    else).  The row is raw: a draw is the logit of a unit-interval value clipped to [1e-4, 1 - 1e-4].

    Returns (best, history) as `population_search`; the inputs are not modified.  dy_drop > 0 makes the cost
    stochastic: ValueError."""
    _check_search(model, n_candidates, n_rounds, shrink, objective, "adj_population_search")
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
