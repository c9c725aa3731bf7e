"""Population evaluation: the cost of many candidate static-parameter sets per basin in one kernel launch.

`calibrate` is first order around one point and accepts a step only when the cost falls: on HBV's cost surface
(thresholds, clamps, equifinal parameter pairs) it stops in the first local basin it reaches.  Population steps --
random or Latin-hypercube starts, SCE-UA / DDS / DREAM-style searches -- evaluate hundreds of candidates per basin and
want one number back per candidate.  `population_cost` gives exactly that: the module runs ONCE at `parameters` (its
warm-up pass, its dy_drop draws and the recorded descriptor of its main pass), then hbvx_population_cost
(include/hbvx.h) runs the recurrence, the ensemble mean, the routing and the residual sum of every candidate in
registers and writes [P,B] costs -- no flux series, no trajectory, no [P,B,ny] copy of the parameters.
`population_search` is a per-basin shrinking random search on top, for a start that `calibrate` can refine.

Hbv, Hbv_1_1p and Hbv_2 only; the score is the weighted squared error of 'streamflow'.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _abi, ops
from ._lib import get_library
from .calibrate import _check_request, _static_tensor
from .sensitivity import jacobian_columns

_EDGE = 1e-4        # unit-space draws are kept in [_EDGE, 1 - _EDGE] where the module applies a sigmoid (finite logits)


def _check(model, x_dict, parameters, target, names, weights, what):
    """Everything that can be refused without running the model: calibrate's request checks for the key
    'streamflow', and what this path adds to them."""
    if getattr(model, '_model_id', None) == _abi.MODEL_HBVADJ:
        raise NotImplementedError(f"{what} is not implemented for {type(model).__name__}: the implicit scheme needs its "
                                  "Newton solve inside the day loop, which is not this kernel; Hbv, Hbv_1_1p and Hbv_2 only")
    req = _check_request(model, x_dict, parameters, target, names, 'streamflow', weights, 1, what=what)
    if model.comprout:
        raise ValueError(f"{what}: comprout=True routes every member, not the ensemble mean; not supported")
    return req


def _column_groups(model, names):
    """[(name, compact column, width)] in the order of `jacobian_columns(model, names)`: the nmul columns of each named
    physical parameter, one column per routing parameter."""
    if names is None:
        dyn = set(model.dynamic_params)
        names = [n for n in model.parameter_bounds if n not in dyn] + \
            (list(model.routing_parameter_bounds) if model.routing else [])
    groups, at = [], 0
    for n in names:
        width = 1 if n in model.routing_parameter_bounds else model.nmul
        groups.append((n, at, width))
        at += width
    return groups


def population_cost(model, x_dict: dict, parameters, candidates: torch.Tensor, target,
                    names: Optional[Sequence[str]] = None, weights=None, return_series: bool = False) -> dict:
    """sum_t w (streamflow - target)^2 per basin for each of P candidate static-parameter sets.

    candidates  [P,B,C] float32 on the device of x_phy: values for the columns `jacobian_columns(model, names)` returns,
                in that order, in the space the module takes them in (raw for Hbv / Hbv_1_1p, the unit interval for
                Hbv_2's p_sta).  Candidate c stands in for parameters[T-1, b, columns] (Hbv_2: p_sta[b, columns]);
                everything else -- dynamic parameters, the other static columns, forcings, muwts -- is shared.
    target      [T_out,B] or [T_out,B,1], T_out = the days after the warm-up; a NaN is a missing observation (weight 0).
    weights     [T_out,B] >= 0 or None (ones).
    Returns {'cost': [P,B] float32, +inf where the sum is not finite, 'n_obs': [B] int64, 'columns': [C indices],
    'outputs': the primal flux dictionary at `parameters`, 'series': [P,T_out,B] each candidate's streamflow (routed
    when the model routes), only with return_series}.

    The module runs once at `parameters`: that run does the warm-up (which reads row warm_up - 1, not the candidates'
    row), draws the dy_drop masks -- one set, shared by all candidates -- and leaves the module as one plain call.
    The cost is a float32 chain of fused multiply-adds over ascending days; two calls give the same bits, and a
    candidate's bits do not depend on the other candidates or on return_series.

    Refused before the model runs: HbvAdj, Hbv_2_hourly, Hbv_2_mts and anything else (NotImplementedError); graph=True,
    initialize mode, comprout=True, dynamic or unknown names, a wrong shape / dtype / device of candidates, target or
    weights, infinite targets, negative or non-finite weights (ValueError); a library without hbvx_population_cost
    (HbvxError)."""
    req = _check(model, x_dict, parameters, target, names, weights, "population_cost")
    x = x_dict['x_phy']
    C = len(req.cols)
    if not torch.is_tensor(candidates) or candidates.dim() != 3 or tuple(candidates.shape[1:]) != (req.B, C) \
            or candidates.shape[0] < 1:
        raise ValueError(f"candidates must be [P,{req.B},{C}] (P >= 1 sets for the {C} columns of `names`), got "
                         f"{tuple(candidates.shape) if torch.is_tensor(candidates) else type(candidates).__name__}")
    if candidates.dtype != torch.float32:
        raise ValueError(f"candidates must be float32, got {candidates.dtype}")
    if candidates.device != x.device:
        raise ValueError(f"candidates live on {candidates.device}, x_phy on {x.device}")
    get_library().require("hbvx_population_cost")

    with torch.no_grad(), ops.record_paths() as records:
        outputs = model(x_dict, parameters)
    main = records[-1]
    cfg = main.cfg
    t_first = cfg.T - req.T_out          # warm_up_states=False: the warm-up days are simulated, not scored
    if t_first < 0 or cfg.B != req.B:
        raise RuntimeError(f"{type(model).__name__} ran {cfg.T} days on {cfg.B} basins, expected at least {req.T_out} on {req.B}")
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

    cands = candidates.detach().contiguous()
    sources, route = {}, [None, None]
    for name, col, _ in _column_groups(model, names):
        if name in model.routing_parameter_bounds:
            route[list(model.routing_parameter_bounds).index(name)] = (cands, col)
        else:
            sources[_abi.PARAM_SLOTS.index(name)] = (cands, col)
    cost, series = ops.population_cost(main, sources, tuple(route), tgt.contiguous(), w, t_first, return_series)
    cost = torch.where(torch.isfinite(cost), cost, torch.full_like(cost, float('inf')))
    out = {'cost': cost, 'n_obs': n_obs, 'columns': list(req.cols), 'outputs': outputs}
    if return_series:
        out['series'] = series
    return out


def _to_input_space(u: torch.Tensor, raw: bool) -> torch.Tensor:
    """Unit-interval values -> the space the module takes them in (logit where it applies a sigmoid)."""
    if not raw:
        return u.clamp(0.0, 1.0)
    return torch.logit(u.clamp(_EDGE, 1.0 - _EDGE))


def population_search(model, x_dict: dict, parameters, target, names: Optional[Sequence[str]] = None,
                      n_candidates: int = 256, n_rounds: int = 1, shrink: float = 0.5, weights=None,
                      generator: Optional[torch.Generator] = None):
    """Per-basin shrinking random search over the static row, for a start that `calibrate` can refine.

    Round 0 evaluates the current row as candidate 0 and n_candidates - 1 uniform draws in the unit interval per
    column, mapped to the module's input space (logit of the draw clipped to [1e-4, 1 - 1e-4] for Hbv / Hbv_1_1p, which
    apply a sigmoid; Hbv_2 takes the unit interval itself).  Round k >= 1 draws uniformly in a box of half-width
    shrink**k / 2 around each basin's best so far, in unit space and clipped, and always re-includes that best as
    candidate 0 -- so a basin's cost never rises.  Every round is one `population_cost` call.

    Returns (best, history): `best` shaped like `parameters` with each basin's best row written (a new tensor; Hbv_2:
    (p_dyn, new p_sta)); history = {'cost': [n_rounds+1,B] float64 (row 0: the start, row k+1: the best after round k),
    'best_index': [n_rounds,B] int64 (the winning candidate of the round; 0: nothing better was drawn), 'columns'}.
    The inputs are not modified.  Deterministic for a given `generator` (default: torch's global CPU generator).
    dy_drop > 0 makes the cost stochastic: ValueError."""
    if float(getattr(model, 'dy_drop', 0.0)) > 0:
        raise ValueError("population_search: dy_drop > 0 draws new masks in every run, the cost is stochastic; set dy_drop = 0")
    if n_candidates < 2:
        raise ValueError("n_candidates must be >= 2 (the current row and at least one draw)")
    if n_rounds < 1:
        raise ValueError("n_rounds must be >= 1")
    if not 0 < shrink <= 1:
        raise ValueError("population_search wants 0 < shrink <= 1")
    req = _check(model, x_dict, parameters, target, names, weights, "population_search")
    two = req.tname == 'p_sta'
    raw = not two
    cur = _static_tensor(two, parameters).detach().clone()
    row = cur if two else cur[-1]           # [B,width] view of the row that moves
    dev = x_dict['x_phy'].device
    cols = torch.as_tensor(req.cols, dtype=torch.long, device=cur.device)
    C = len(req.cols)
    gdev = generator.device if generator is not None else torch.device('cpu')

    best = row[:, cols].to(device=dev, dtype=torch.float32)                     # [B,C], input space
    best_u = torch.sigmoid(best) if raw else best.clone()
    hist = {'cost': [], 'best_index': [], 'columns': list(req.cols)}
    for k in range(n_rounds):
        draws = torch.rand((n_candidates - 1, req.B, C), generator=generator, device=gdev).to(dev)
        if k > 0:
            draws = best_u.unsqueeze(0) + (draws - 0.5) * float(shrink) ** k
        cands = torch.cat([best.unsqueeze(0), _to_input_space(draws, raw)]).contiguous()
        cost = population_cost(model, x_dict, parameters, cands, target, names, weights)['cost']
        low, idx = cost.min(0)
        idx = torch.where(cost[0] <= low, torch.zeros_like(idx), idx)          # a tie keeps the row that is held
        if k == 0:
            hist['cost'].append(cost[0].double().cpu())
        pick = idx.view(1, req.B, 1).expand(1, req.B, C)
        best = cands.gather(0, pick)[0]
        best_u = torch.sigmoid(best) if raw else best.clone()
        hist['cost'].append(cost.gather(0, idx.unsqueeze(0))[0].double().cpu())
        hist['best_index'].append(idx.cpu())
    row[:, cols] = best.to(cur.device)
    hist['cost'] = torch.stack(hist['cost'])
    hist['best_index'] = torch.stack(hist['best_index'])
    return ((parameters[0], cur) if two else cur), hist
