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

from . import _abi
from .population import IMPLICIT, _front, _search_call

AUX_KEYS = tuple(_abi.ADJ_POP_AUX_SERIES)       # 'SNOWPACK', 'MELTWATER', 'SM', 'SUZ', 'SLZ'


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
    return _front(IMPLICIT, "adj_population_cost", 'cost', model, x_dict, parameters, candidates, target, names, weights,
                  return_series=return_series)


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
    return _front(IMPLICIT, "adj_population_stats", 'stats', model, x_dict, parameters, candidates, target, names, weights,
                  transform, eps, return_series=return_series)


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
    return _front(IMPLICIT, "adj_population_period_stats", 'period', model, x_dict, parameters, candidates, target, periods,
                  aux_target, aux_key, aux_periods, names, weights, aux_weights, transform, eps, return_series)


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
    return _search_call(IMPLICIT, "adj_population_search", model, x_dict, parameters, target, names, n_candidates,
                        n_rounds, shrink, weights, generator, objective, transform, eps, aux_target, aux_key, aux_weights,
                        aux_objective, aux_share, periods, aux_periods)
