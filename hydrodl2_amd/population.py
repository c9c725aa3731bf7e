"""Population evaluation: the cost of many candidate static-parameter sets per basin in one kernel launch.

`calibrate` is first order around one point and accepts a step only when the cost falls: on HBV's cost surface
(thresholds, clamps, equifinal parameter pairs) it stops in the first local basin it reaches.  Population steps --
random or Latin-hypercube starts, SCE-UA / DDS / DREAM-style searches -- evaluate hundreds of candidates per basin and
want one number back per candidate.  `population_cost` gives exactly that: the module runs ONCE at `parameters` (its
warm-up pass, its dy_drop draws and the recorded descriptor of its main pass), then hbvx_population_cost
(include/hbvx.h) runs the recurrence, the ensemble mean, the routing and the residual sum of every candidate in
registers and writes [P,B] costs -- no flux series, no trajectory, no [P,B,ny] copy of the parameters.
`population_search` is a per-basin shrinking random search on top, for a start that `calibrate` can refine.
`population_stats` is the same launch with three more sums per (candidate, basin), on the raw, the square-root or the
log flow (hbvx_population_stats), from which `population_score` forms NSE, KGE, correlation, variability and bias in
float64 -- so a search can run in the metric its result is reported in.
`population_joint_stats` is that launch with a second observed series beside streamflow -- evapotranspiration, snow-water
equivalent or one of the three un-routed runoff components (hbvx_population_joint): eight [P,B] numbers, still no
series -- and `population_search(aux_target=...)` minimises a weighted sum of the two scores.
`population_period_stats` is the joint launch against period MEANS -- 8-day composites, months -- on a calendar per
series (hbvx_population_period): each series is averaged over its periods inside the kernel, the chains take one step
per period, and `population_search(periods=..., aux_periods=...)` searches on those scores.
`population_fdc_stats` (population_fdc.py) is `population_stats` with each candidate's flow-duration curve sampled at
thresholds of the observations (hbvx_population_fdc: exceedance counts and volumes, [P,K,B], still no series), and
`population_search(fdc_share=...)` mixes a distance between the curves into its objective.
`population_event_stats` (population_events.py) is `population_stats` with each candidate's peak, day of the peak and
volume inside flood-event windows of the observations (hbvx_population_events: [P,E,B], still no series), and
`population_search(events=..., event_share=...)` mixes an event score into its objective.

Hbv, Hbv_1_1p and Hbv_2 only.  HbvAdj has the first three calls and a period call of its own in adj_population.py
(`adj_population_period_stats`: its second series is one of its five storages).  Hbv_2_hourly, whose scores live at
the gages, has `hourly_population_stats` in hourly_population.py (two stages: every candidate's unit runoff, then its
routing to the gages and the same four chains per gage); the calls here keep refusing it, and nothing is built for the
multi-timescale model.  The aux series is not transformed, there is one per launch, calendars are shared by all basins,
and there is no joint `calibrate`: two `normal_equations` calls can be summed by the caller.

Every call here and in adj_population.py is one front end over two `Family` records: checks, observations, requests and
results are written once, and `_run` is the one function that runs the module and reaches ops.population.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch

from . import _abi, ops
from ._lib import get_library
from .calibrate import _NO_TARGET, _check_request, _static_tensor

_EDGE = 1e-4        # unit-space draws are kept in [_EDGE, 1 - _EDGE] where the module applies a sigmoid (finite logits)


class Family(NamedTuple):
    """What differs between the front ends of the explicit models (Hbv, Hbv_1_1p, Hbv_2: the functions of this file) and
    those of the implicit scheme (HbvAdj: adj_population.py).  Everything else in this file is written once."""
    implicit: bool      # which models `_check` admits and what it refuses; how `_primal` records the run and finds t_first
    key: str            # the output that is scored
    aux_keys: dict      # aux_key -> the series index the family's kernels take
    prefix: str         # of the family's exports: prefix + 'cost' | 'stats' | 'joint' | 'period'
    has_joint: bool     # False: there is no prefix + 'joint'; an aux term without a calendar goes to prefix + 'period'


EXPLICIT = Family(False, 'streamflow', _abi.POP_AUX_SERIES, 'hbvx_population_', True)
IMPLICIT = Family(True, 'flow_sim', _abi.ADJ_POP_AUX_SERIES, 'hbvx_adj_population_', False)


def _check(family, model, x_dict, parameters, target, names, weights, what):
    """Everything that can be refused without running the model: calibrate's request checks for the family's key, and
    what this path adds to them."""
    adj = getattr(model, '_model_id', None) == _abi.MODEL_HBVADJ
    if adj and not family.implicit:
        raise NotImplementedError(f"{what} is not implemented for {type(model).__name__}: the implicit scheme needs its "
                                  "Newton solve inside the day loop, which is not this kernel; Hbv, Hbv_1_1p and Hbv_2 only "
                                  "-- HbvAdj goes through hydrodl2_amd.adj_population_cost / adj_population_stats / "
                                  "adj_population_search")
    if family.implicit and not adj:
        raise NotImplementedError(f"{what} is for HbvAdj, not {type(model).__name__}: Hbv, Hbv_1_1p and Hbv_2 go through "
                                  f"hydrodl2_amd.{what[4:]}")
    req = _check_request(model, x_dict, parameters, target, names, family.key, weights, 1, what=what)
    if family.implicit and model.newton_stop == 'global':
        raise ValueError(f"{what}: newton_stop='global' (one stopping vote over the lanes of a wave) would make a "
                         "candidate's cost depend on the basins that share its wave; use newton_stop='lane'")
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


def _check_candidates(req, x_dict, candidates):
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


def _primal(family, model, req, x_dict, parameters):
    """The one run of the module at `parameters`: (outputs, the recorded call of its main pass, t_first)."""
    with torch.no_grad(), ops.record_paths(want_traj=not family.implicit) as records:   # HbvAdj's kernel solves every day itself
        outputs = model(x_dict, parameters)
    main = records[-1]
    cfg = main.cfg
    t_first = 0 if family.implicit else cfg.T - req.T_out       # warm_up_states=False: the warm-up days are simulated, not scored
    if t_first < 0 or cfg.B != req.B or (family.implicit and cfg.T != req.T_out):
        raise RuntimeError(f"{type(model).__name__} ran {cfg.T} days on {cfg.B} basins, expected "
                           f"{'' if family.implicit else 'at least '}{req.T_out} on {req.B}")
    return outputs, main, t_first


class Request(NamedTuple):
    """A population call after its checks: what `_run` works on."""
    model: object
    x_dict: dict
    parameters: object
    names: Optional[Sequence[str]]
    req: object                     # calibrate's request: columns, T_out, B
    ob: dict                        # the flow's observations: `_cost_observations` (form 'cost') or `_observations`
    transform: str = 'none'
    aux_key: Optional[str] = None
    aux_ob: Optional[dict] = None   # `_observations` of the aux term, None without one
    ends: tuple = (None, None)      # form 'period': the closing days of the flow's and the aux calendar, int64 on the CPU
    candidates: Optional[torch.Tensor] = None
    return_series: bool = False


def _sums(got, ob, transform, rq, outputs, ends=None):
    """What `population_score` reads, for one scored series: the four chains `got[:4]` with the observation side `ob`."""
    out = dict(zip(('sse', 's1', 's2', 's3'), got[:4]))
    out.update(shift=ob['shift'], obs=ob['obs'], transform=transform, eps=ob['eps'], n_obs=ob['n_obs'],
               columns=list(rq.req.cols), outputs=outputs)
    if ends is not None:
        out.update(period_ends=ends.clone(), period_days=_period_days(ends))
    if rq.return_series:
        out['series'] = got[4]
    return out


def _run(family, form, rq):
    """The one route from every front end to the kernels: runs the module once at rq.parameters, then rq.candidates
    through ops.population on the export family.prefix + form, and returns the call's result dictionary."""
    outputs, main, t_first = _primal(family, rq.model, rq.req, rq.x_dict, rq.parameters)
    sources, route = _candidate_sources(rq.model, rq.names, rq.candidates)
    ob, aux_ob = rq.ob, rq.aux_ob
    ends = rq.ends if form == 'period' else (None, None)
    end_f, end_a = (None if e is None else e.to(device=main.x.device, dtype=torch.int32) for e in ends)
    flow = ops.PopTerm(ob['target'], ob['w'], ob.get('shift'), ob.get('eps'), None if form == 'cost' else rq.transform,
                       end_f)
    aux = None if aux_ob is None else ops.PopTerm(aux_ob['target'], aux_ob['w'], aux_ob['shift'], ends=end_a,
                                                  series=family.aux_keys[rq.aux_key])
    flow_out, aux_out = ops.population(main, family.prefix + form, sources, route, flow, aux, t_first, rq.return_series)
    if form == 'cost':
        cost = flow_out[0]
        out = {'cost': torch.where(torch.isfinite(cost), cost, torch.full_like(cost, float('inf'))), 'n_obs': ob['n_obs'],
               'columns': list(rq.req.cols), 'outputs': outputs}
        if rq.return_series:
            out['series'] = flow_out[4]
        return out
    if form == 'stats':
        return _sums(flow_out, ob, rq.transform, rq, outputs)
    out = {'columns': list(rq.req.cols), 'outputs': outputs, 'flow': _sums(flow_out, ob, rq.transform, rq, outputs, ends[0])}
    if aux_out is not None:
        out['aux'] = _sums(aux_out, aux_ob, 'none', rq, outputs, ends[1])
        out['aux']['key'] = rq.aux_key
    return out


def _candidate_sources(model, names, candidates):
    """({parameter slot: (cands, column)}, (route_a, route_b) each None or (cands, column)) as ops.population takes
    them."""
    cands = candidates.detach().contiguous()
    sources, route = {}, [None, None]
    for name, col, _ in _column_groups(model, names):
        if name in model.routing_parameter_bounds:
            route[list(model.routing_parameter_bounds).index(name)] = (cands, col)
        else:
            sources[_abi.PARAM_SLOTS.index(name)] = (cands, col)
    return sources, tuple(route)


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
    return _front(EXPLICIT, "population_cost", 'cost', model, x_dict, parameters, candidates, target, names, weights,
                  return_series=return_series)


def _cost_observations(req, x_dict, target, weights):
    """The observation side of the cost form: {'target' [T_out,B] float32 (0 where missing), 'w' [T_out,B] float32 or
    None, 'n_obs' [B] int64} on the device of x_phy."""
    dev = x_dict['x_phy'].device
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
    return {'target': tgt.contiguous(), 'w': w, 'n_obs': n_obs}


def _daily_request(family, what, form, model, x_dict, parameters, candidates, target, names, weights, transform='none',
                   eps=None, aux_target=None, aux_key=None, aux_weights=None, return_series=False, mix=None) -> Request:
    """Everything the forms 'cost', 'stats' and 'joint' can refuse before the model runs, and what they work on.
    candidates None: the search, which fills them in round by round; mix: its (objective, aux_objective, aux_share)."""
    req = _check(family, model, x_dict, parameters, target, names, weights, what)
    if candidates is not None:
        _check_candidates(req, x_dict, candidates)
    aux_ob = None
    if form == 'joint':
        _check_aux(req, x_dict, aux_target, aux_key, aux_weights, what, keys=tuple(family.aux_keys))
        if mix is not None:
            _check_mix(*mix, what)
    if form == 'cost':
        ob = _cost_observations(req, x_dict, target, weights)
    else:
        ob = _observations(req, x_dict, target, weights, transform, eps, what)
    if form == 'joint':
        aux_ob = _observations(req, x_dict, aux_target, aux_weights, 'none', None, what)
    get_library().require(family.prefix + form)
    return Request(model, x_dict, parameters, names, req, ob, transform, aux_key, aux_ob, candidates=candidates,
                   return_series=return_series)


def _front(family, what, form, *args, **kw):
    """A public call: the request of its form (`_period_request` / `_daily_request` take the arguments), then `_run`."""
    rq = _period_request(family, what, *args, **kw) if form == 'period' else _daily_request(family, what, form, *args, **kw)
    return _run(family, form, rq)


TRANSFORMS = tuple(_abi.POP_TRANSFORMS)                 # 'none', 'sqrt', 'log'
METRICS = ('sse', 'mse', 'nse', 'kge', 'kge12', 'r', 'alpha', 'beta', 'pbias')
OBJECTIVES = ('sse', 'nse', 'kge', 'kge12')
# A variance of float32 chains at or below this fraction of the mean square about the shift is rounding noise, not a
# variance (a constant series leaves about T_out * 2^-24 of it): the scores that divide by it are NaN there.
_VAR_FLOOR = 1e-6


def _observations(req, x_dict, target, weights, transform, eps, what, rows=None):
    """The observation side of `population_stats`, everything that can be refused about it, before the model runs.
    float64 on the device of x_phy -> {'target' [T_out,B] float32 transformed (0 where missing), 'w' [T_out,B] float32
    or None, 'shift' [B] float32, 'eps' [B] float32 or None, 'obs': {'W','e1','e2'} [B] float64, 'n_obs' [B] int64}.
    rows: the leading size of target and weights where it is not T_out -- the K periods of `population_period_stats`,
    whose observations are one value per period; everything above then reads K for T_out."""
    if transform not in _abi.POP_TRANSFORMS:
        raise ValueError(f"{what}: transform must be one of {list(TRANSFORMS)}, got {transform!r}")
    dev = x_dict['x_phy'].device
    tgt = target.to(device=dev, dtype=torch.float32).reshape(req.T_out if rows is None else rows, req.B)
    miss = torch.isnan(tgt)
    plain = weights is None and not bool(miss.any())
    w = torch.ones_like(tgt) if weights is None else weights.to(device=dev, dtype=torch.float32)
    w = torch.where(miss, torch.zeros_like(w), w).contiguous()
    w8 = w.double()
    W = w8.sum(0)
    some = W > 0
    o8 = torch.where(miss, torch.zeros_like(tgt), tgt).double()
    eps8 = None
    if eps is not None:                                 # checked under every transform, read under 'log'
        eps8 = torch.as_tensor(eps, dtype=torch.float64, device=dev)
        if eps8.dim() == 0:
            eps8 = eps8.expand(req.B)
        if tuple(eps8.shape) != (req.B,):
            raise ValueError(f"{what}: eps must be a scalar or [{req.B}], got {tuple(eps8.shape)}")
    elif transform == 'log':
        # a hundredth of the basin's weighted mean observed flow (1 where nothing is observed: never read)
        eps8 = torch.where(some, 0.01 * (w8 * o8).sum(0) / W.clamp_min(1e-300), torch.ones_like(W))
    if eps8 is not None:
        eps8 = eps8.float().double()                    # the float32 the kernel adds
        if not bool((torch.isfinite(eps8) & (eps8 > 0)).all()):
            raise ValueError(f"{what}: eps must be finite and > 0 in every basin (the default, a hundredth of the weighted "
                             "mean observed flow, needs a positive mean)")
    if transform != 'log':
        eps8 = None
    if transform == 'log':
        if bool(((o8 <= -eps8) & ~miss).any()):
            raise ValueError(f"{what}: a target <= -eps has no logarithm")
        o8 = torch.log(o8 + eps8)
    elif transform == 'sqrt':
        if bool(((o8 < 0) & ~miss).any()):
            raise ValueError(f"{what}: a negative target has no square root")
        o8 = torch.sqrt(o8)
    ot = torch.where(miss, torch.zeros_like(tgt), o8.float())     # o' as the kernel reads it
    shift = torch.where(some, (w8 * ot.double()).sum(0) / W.clamp_min(1e-300), torch.zeros_like(W)).float()
    e = ot.double() - shift.double()
    return {'target': ot.contiguous(), 'w': None if plain else w, 'shift': shift,
            'eps': None if eps8 is None else eps8.float(),
            'obs': {'W': W, 'e1': (w8 * e).sum(0), 'e2': (w8 * e * e).sum(0)},
            'n_obs': (w > 0).sum(0, dtype=torch.int64)}


def population_stats(model, x_dict: dict, parameters, candidates: torch.Tensor, target,
                     names: Optional[Sequence[str]] = None, weights=None, transform: str = 'none', eps=None,
                     return_series: bool = False) -> dict:
    """The sums from which `population_score` forms NSE, KGE, correlation, variability and bias of each of P candidate
    static-parameter sets, on the raw flow (transform 'none'), its square root ('sqrt') or log(flow + eps) ('log'):
    `population_cost`'s launch with three more chains per (candidate, basin) and still nothing but [P,B] numbers.

    candidates, target, names, weights: as `population_cost`.  eps: a scalar, [B] or None -- None is a hundredth of the
    basin's weighted mean observed flow under 'log'; unused otherwise.
    With y' the transformed streamflow, o' the transformed target, m = `shift` the float32 weighted mean of o' and
    d = y' - m, e = o' - m, returns
      {'sse': sum w (y' - o')^2, 's1': sum w d, 's2': sum w d^2, 's3': sum w d e   -- [P,B] float32 chains over
       ascending days (include/hbvx.h states them line by line), non-finite where a candidate's flow has no transform,
       'shift': [B] float32, 'obs': {'W': sum w, 'e1': sum w e, 'e2': sum w e^2} [B] float64, 'transform', 'eps': [B]
       float32 or None, 'n_obs': [B] int64, 'columns', 'outputs': the primal flux dictionary,
       'series': [P,T_out,B] the streamflow itself (NOT transformed), only with return_series}.
    Under 'none', 'sse' has the bits of `population_cost`'s 'cost' (before its +inf rule), and 'series' has them under
    every transform.  The moments are taken about m because raw float32 sums cancel: see DESIGN.md.

    Refused before the model runs: everything `population_cost` refuses; an unknown transform; eps <= 0 or non-finite;
    a negative target under 'sqrt'; a target <= -eps under 'log' (ValueError); a library without hbvx_population_stats
    (HbvxError)."""
    return _front(EXPLICIT, "population_stats", 'stats', model, x_dict, parameters, candidates, target, names, weights,
                  transform, eps, return_series=return_series)


AUX_KEYS = tuple(_abi.POP_AUX_SERIES)       # 'srflow_no_rout', 'ssflow_no_rout', 'gwflow_no_rout', 'AET_hydro', 'SWE'


def _check_aux(req, x_dict, aux_target, aux_key, aux_weights, what, rows=None, keys=AUX_KEYS):
    """What can be refused about the aux term without running the model.  rows: the leading size of aux_target and
    aux_weights where it is not T_out (the periods of its calendar).  keys: the aux keys the family's kernels offer."""
    if aux_target is None or aux_key is None:
        raise ValueError(f"{what}: aux_target and aux_key go together "
                         f"({'aux_target' if aux_target is None else 'aux_key'} is missing)")
    if aux_key not in keys:
        raise ValueError(f"{what}: aux_key must be one of {list(keys)}, got {aux_key!r}")
    n, of = (req.T_out, "days after the warm-up") if rows is None else (rows, "periods of its calendar")
    _check_rows(req, x_dict, aux_target, aux_weights, n, of, what, "aux_")


def _check_rows(req, x_dict, target, weights, rows, of, what, aux=""):
    """calibrate's checks of a target and its weights where their leading size is `rows` -- the `of` of the message --
    and not necessarily T_out; aux: 'aux_' for the aux term's pair, which the messages then name so."""
    dev = x_dict['x_phy'].device
    for name, t, shapes in ((aux + "target", target, ((rows, req.B), (rows, req.B, 1))),
                            (aux + "weights", weights, ((rows, req.B),))):
        if t is None and name.endswith("weights"):
            continue
        if not torch.is_tensor(t) or tuple(t.shape) not in shapes:
            raise ValueError(f"{what}: {name} must be {' or '.join(str(list(s)) for s in shapes)} (the {of}), "
                             f"got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if t.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{what}: {name} must be float32 or float64, got {t.dtype}")
        if t.device != dev:
            raise ValueError(f"{what}: {name} lives on {t.device}, x_phy on {dev}")
    if bool(torch.isinf(target).any()):
        raise ValueError(f"{what}: {aux}target holds infinities (a missing observation is a NaN)")
    if weights is not None:
        if not bool(torch.isfinite(weights).all()):
            raise ValueError(f"{what}: {aux}weights must be finite")
        if bool((weights < 0).any()):
            raise ValueError(f"{what}: {aux}weights must not be negative")


def population_joint_stats(model, x_dict: dict, parameters, candidates: torch.Tensor, target, aux_target, aux_key: str,
                           names: Optional[Sequence[str]] = None, weights=None, aux_weights=None,
                           transform: str = 'none', eps=None, return_series: bool = False) -> dict:
    """`population_stats` for streamflow and, from the same launch, the same four sums for a second observed series:
    outputs[aux_key] with aux_key one of 'AET_hydro', 'SWE', 'srflow_no_rout', 'ssflow_no_rout', 'gwflow_no_rout' -- the
    day's ensemble mean of that flux as the module returns it, never routed and never transformed.

    candidates, target, names, weights, transform, eps: as `population_stats`; they shape the flow term only.
    aux_target   [T_out,B] or [T_out,B,1], float32 or float64 on the device of x_phy; a NaN is a missing observation.
                 Sparse records -- an 8-day product given as NaN on the other days -- are the normal case.
    aux_weights  [T_out,B] >= 0 or None (ones).
    Returns {'flow': what `population_stats` returns, bit for bit, 'aux': the same layout for the aux series (transform
    'none', 'shift' the float32 weighted mean of aux_target, 'key': aux_key), 'columns', 'outputs'}; with return_series
    each of the two carries its 'series' [P,T_out,B].  `population_score(result['flow'], m)` and
    `population_score(result['aux'], m)` work as on `population_stats`' result.  include/hbvx.h states the aux chains
    line by line; the guarantees are `population_stats`' for all eight numbers.

    Refused before the model runs: everything `population_stats` refuses; an unknown aux_key; aux_key without aux_target
    or the reverse; a wrong shape, dtype or device of aux_target / aux_weights, infinite aux targets, negative or
    non-finite aux weights (ValueError); a library without hbvx_population_joint (HbvxError)."""
    return _front(EXPLICIT, "population_joint_stats", 'joint', model, x_dict, parameters, candidates, target, names, weights,
                  transform, eps, aux_target, aux_key, aux_weights, return_series)


def _calendar(periods, T_out: int, name: str, what: str) -> torch.Tensor:
    """The closing days of a calendar, 0-based in the scored days: a 1-D int64 CPU tensor.  periods None: every day its
    own period; an int n: blocks of n days from the first scored day, an incomplete last block dropped; a 1-D integer
    sequence or tensor: the closing days themselves, strictly ascending in 0..T_out-1."""
    if periods is None:
        return torch.arange(T_out, dtype=torch.int64)
    if isinstance(periods, bool):
        raise ValueError(f"{what}: {name} must be None, an int or a 1-D sequence of closing days, got a bool")
    if isinstance(periods, int):
        if not 1 <= periods <= T_out:
            raise ValueError(f"{what}: {name} = {periods} days per period, with {T_out} scored days it must be in 1..{T_out}")
        return torch.arange(periods - 1, T_out, periods, dtype=torch.int64)
    try:
        ends = periods.detach().cpu() if torch.is_tensor(periods) else torch.as_tensor(list(periods))
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"{what}: {name} must be None, an int or a 1-D sequence of closing days") from e
    if ends.dim() != 1 or ends.numel() < 1:
        raise ValueError(f"{what}: {name} must hold at least one closing day in one dimension, got shape {tuple(ends.shape)}")
    if ends.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"{what}: {name} must hold integers (closing days), got {ends.dtype}")
    ends = ends.to(torch.int64)
    if int(ends[0]) < 0 or int(ends[-1]) >= T_out or bool((ends[1:] <= ends[:-1]).any()):
        raise ValueError(f"{what}: {name} must be strictly ascending closing days in 0..{T_out - 1} (0-based in the "
                         "scored days)")
    return ends


def _period_days(ends: torch.Tensor) -> torch.Tensor:
    """The day count of each period of a calendar: period 0 starts at the first scored day."""
    return ends - torch.cat([ends.new_full((1,), -1), ends[:-1]])


def _period_request(family, what, model, x_dict, parameters, candidates, target, periods, aux_target, aux_key,
                    aux_periods, names, weights, aux_weights, transform, eps, return_series=False) -> Request:
    """Everything the period form can refuse before the model runs, and what it works on.  candidates None: the search,
    which fills them in round by round."""
    req = _check(family, model, x_dict, parameters, _NO_TARGET, names, None, what)
    if candidates is not None:
        _check_candidates(req, x_dict, candidates)
    ends_f = _calendar(periods, req.T_out, "periods", what)
    K = int(ends_f.numel())
    _check_rows(req, x_dict, target, weights, K, f"{K} periods of its calendar", what)
    ends_a = aux_ob = None
    if aux_key is None and aux_target is None:
        if aux_periods is not None or aux_weights is not None:
            raise ValueError(f"{what}: {'aux_periods' if aux_periods is not None else 'aux_weights'} without aux_key")
    else:
        ends_a = _calendar(aux_periods, req.T_out, "aux_periods", what)
        _check_aux(req, x_dict, aux_target, aux_key, aux_weights, what, rows=int(ends_a.numel()), keys=tuple(family.aux_keys))
    ob = _observations(req, x_dict, target, weights, transform, eps, what, rows=K)
    if ends_a is not None:
        aux_ob = _observations(req, x_dict, aux_target, aux_weights, 'none', None, what, rows=int(ends_a.numel()))
    get_library().require(family.prefix + 'period')
    return Request(model, x_dict, parameters, names, req, ob, transform, aux_key, aux_ob, (ends_f, ends_a), candidates,
                   return_series)


def population_period_stats(model, x_dict: dict, parameters, candidates: torch.Tensor, target, periods=None,
                            aux_target=None, aux_key: Optional[str] = None, aux_periods=None,
                            names: Optional[Sequence[str]] = None, weights=None, aux_weights=None,
                            transform: str = 'none', eps=None, return_series: bool = False) -> dict:
    """`population_joint_stats` against period MEANS: each candidate's streamflow, and optionally one second series, is
    averaged over the periods of a calendar -- 8-day composites, months -- inside the kernel, and the period means are
    what meets the targets (hbvx_population_period).  Still nothing but [P,B] numbers; no daily series exists anywhere.

    periods, aux_periods   the calendar of the flow and of the aux series, each one of
                 None: every scored day is its own period (with both None the numbers are `population_joint_stats`' bit
                       for bit);
                 an int n >= 1: blocks of n days from the first scored day, an incomplete last block is not scored;
                 a 1-D integer sequence or tensor of closing days: 0-based in the scored days, strictly ascending, all
                       below T_out.  Period k covers the days after closing day k - 1 up to and including closing day k;
                       days after the last closing day are simulated and not scored.
    target       [K,B] or [K,B,1], K the number of periods of `periods`: the period MEAN in the module's units (a caller
                 with sums divides by the lengths); a NaN is a missing period.  aux_target likewise on `aux_periods`.
    weights, aux_weights   [K,B] >= 0 per period, or None (ones).
    transform, eps   as `population_stats`, applied to the period mean of the flow; the default eps under 'log' is a
                 hundredth of the weighted mean of the period targets.  The aux series is never transformed.
    aux_key None (with aux_target None): there is no aux term; the flow numbers have the same bits either way.
    Returns `population_joint_stats`' layout, {'flow', 'aux' (only with aux_key), 'columns', 'outputs'}; each of the two
    also carries 'period_ends' and 'period_days' ([K] int64, CPU), 'n_obs' counts observed periods, and with
    return_series 'series' is [P,K,B]: the period means (the flow's before its transform).  `population_score` works on
    either unchanged.  include/hbvx.h states the arithmetic line by line: float32, the days of a period added in
    ascending order and divided once, fused multiply-add chains over ascending periods, no atomics; two calls agree bit
    for bit and a candidate's bits depend on nothing but its own values.

    Refused before the model runs: everything `population_joint_stats` refuses (its aux rules only with an aux term); a
    calendar that is empty, not integer, not strictly ascending, negative or >= T_out; n < 1 or n > T_out; a target or
    weights whose leading size is not K; aux_periods or aux_weights without aux_key (ValueError); HbvAdj, the hourly and
    multi-timescale models (NotImplementedError); a library without hbvx_population_period (HbvxError)."""
    return _front(EXPLICIT, "population_period_stats", 'period', model, x_dict, parameters, candidates, target, periods,
                  aux_target, aux_key, aux_periods, names, weights, aux_weights, transform, eps, return_series)


def population_score(stats: dict, metric: str) -> torch.Tensor:
    """[P,B] float64 score of every candidate from what `population_stats` returned.  Weighted population moments in the
    transformed space, W = sum w:
        mean_o = m + e1/W      var_o = e2/W - (e1/W)^2
        mean_s = m + s1/W      var_s = s2/W - (s1/W)^2      cov = s3/W - (s1/W)(e1/W)
      'sse'    sum w (y' - o')^2                 'mse'   sse / W
      'nse'    1 - sse / (e2 - e1^2 / W)
      'r'      cov / sqrt(var_s var_o)           'alpha' sqrt(var_s / var_o)
      'beta'   mean_s / mean_o                   'pbias' 100 (mean_s - mean_o) / mean_o
      'kge'    1 - sqrt((r-1)^2 + (alpha-1)^2 + (beta-1)^2)                    (Gupta et al. 2009)
      'kge12'  the same with the ratio of the coefficients of variation, (sd_s/mean_s) / (sd_o/mean_o), in place of
               alpha (Kling et al. 2012)
    A score is NaN where it is undefined: a non-finite chain (every metric); no observation ('mse'); fewer than two
    observations or no observed variance ('nse', 'r', 'alpha', 'kge', 'kge12'); no simulated variance -- at or below
    1e-6 of the mean square about m, the noise a float32 chain leaves of a constant series -- ('r', 'kge', 'kge12'); a
    zero observed mean ('beta', 'pbias', 'kge', 'kge12'); a zero simulated mean ('kge12').

    beta and pbias on a transformed flow compare the means of sqrt(Q) or log(Q + eps), not volumes: under 'sqrt' beta
    still reads as a bias of the mid-range flows; under 'log' the mean of the logarithms can lie anywhere around zero
    (it changes sign with the unit of Q), so beta, pbias, kge and kge12 on log flows seldom mean anything -- use 'nse',
    'r' and 'alpha' there."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {list(METRICS)}, got {metric!r}")
    sse, s1, s2, s3 = (stats[k].double() for k in ('sse', 's1', 's2', 's3'))
    dev = sse.device
    W, e1, e2 = (stats['obs'][k].to(device=dev, dtype=torch.float64) for k in ('W', 'e1', 'e2'))
    m = stats['shift'].to(device=dev, dtype=torch.float64)
    n_obs = stats['n_obs'].to(dev)
    nan = torch.full_like(sse, float('nan'))
    Ws = W.clamp_min(1e-300)
    finite = torch.isfinite(sse) & torch.isfinite(s1) & torch.isfinite(s2) & torch.isfinite(s3)
    if metric == 'sse':
        return torch.where(finite, sse, nan)
    if metric == 'mse':
        return torch.where(finite & (W > 0), sse / Ws, nan)
    var_o = e2 / Ws - (e1 / Ws) ** 2
    obs_ok = (n_obs >= 2) & (var_o > _VAR_FLOOR * e2 / Ws)
    if metric == 'nse':
        return torch.where(finite & obs_ok, 1.0 - sse / (e2 - e1 * e1 / Ws), nan)
    mean_o, mean_s = m + e1 / Ws, m + s1 / Ws
    var_s = s2 / Ws - (s1 / Ws) ** 2
    sim_ok = var_s > _VAR_FLOOR * s2 / Ws
    cov = s3 / Ws - (s1 / Ws) * (e1 / Ws)
    sd_o, sd_s = var_o.clamp_min(0).sqrt(), var_s.clamp_min(0).sqrt()
    if metric == 'beta':
        return torch.where(finite & (W > 0) & (mean_o != 0), mean_s / mean_o, nan)
    if metric == 'pbias':
        return torch.where(finite & (W > 0) & (mean_o != 0), 100.0 * (mean_s - mean_o) / mean_o, nan)
    if metric == 'alpha':
        return torch.where(finite & obs_ok, sd_s / sd_o, nan)
    r = cov / (sd_s * sd_o)
    if metric == 'r':
        return torch.where(finite & obs_ok & sim_ok, r, nan)
    ok = finite & obs_ok & sim_ok & (mean_o != 0)
    if metric == 'kge12':
        ok = ok & (mean_s != 0)
        ratio = (sd_s / mean_s) / (sd_o / mean_o)
    else:
        ratio = sd_s / sd_o
    kge = 1.0 - torch.sqrt((r - 1.0) ** 2 + (ratio - 1.0) ** 2 + (mean_s / mean_o - 1.0) ** 2)
    return torch.where(ok, kge, nan)


def _objective_cost(score: torch.Tensor, objective: str) -> torch.Tensor:
    """What `population_search` minimises: 1 - score (the squared error itself for 'sse'), +inf where the score is NaN."""
    cost = score if objective == 'sse' else 1.0 - score
    return torch.where(torch.isnan(cost), torch.full_like(cost, float('inf')), cost)


def _to_input_space(u: torch.Tensor, raw: bool) -> torch.Tensor:
    """Unit-interval values -> the space the module takes them in (logit where it applies a sigmoid)."""
    if not raw:
        return u.clamp(0.0, 1.0)
    return torch.logit(u.clamp(_EDGE, 1.0 - _EDGE))


def population_search(model, x_dict: dict, parameters, target, names: Optional[Sequence[str]] = None,
                      n_candidates: int = 256, n_rounds: int = 1, shrink: float = 0.5, weights=None,
                      generator: Optional[torch.Generator] = None, objective: str = 'sse', transform: str = 'none',
                      eps=None, aux_target=None, aux_key: Optional[str] = None, aux_weights=None,
                      aux_objective: str = 'nse', aux_share: float = 0.5, periods=None, aux_periods=None,
                      fdc_share: float = 0.0, fdc_probs=None, fdc_metric: str = 'fdc_freq', events=None,
                      event_share: float = 0.0, event_metric: str = 'peak_error', timing_scale: float = 1.0):
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
    dy_drop > 0 makes the cost stochastic: ValueError.

    objective 'sse' with transform 'none' (the defaults) is the search above, bit for bit.  objective 'nse', 'kge' or
    'kge12', or a transform 'sqrt' / 'log' (eps as `population_stats` takes it), makes every round one
    `population_stats` call: the quantity minimised, and what history['cost'] holds, is then 1 - score (the squared error
    of the transformed flow for 'sse'), +inf where `population_score` gives NaN, and history['score'] [n_rounds+1,B]
    holds the score itself ('nse', 'kge', 'kge12' only).  A basin whose observations admit no score keeps its row.

    aux_target / aux_key (both or neither; aux_weights as `population_joint_stats` takes them) add a second observed
    series: every round is then one `population_joint_stats` call, and the quantity minimised, and what history['cost']
    holds, is (1 - aux_share) * cost_flow + aux_share * cost_aux, each term 1 - score (the squared error for 'sse') of
    its own series under `objective` / `aux_objective`, +inf where either score is NaN; history['score'] (flow) and
    history['score_aux'] hold the two scores (for 'sse' the squared error itself).  aux_share in [0, 1]; aux_objective
    'sse' goes with objective 'sse' only -- a squared error and 1 - score are two scales in one sum.  Without aux_target
    the function is the one above, bit for bit.

    periods / aux_periods (as `population_period_stats` takes them; either may be given alone, the other is then daily)
    score period means: target, weights, aux_target and aux_weights then hold one row per period, and every round is one
    `population_period_stats` call, with or without an aux term; cost and history are formed as above.  With both None
    the function is the one above, bit for bit.

    fdc_share > 0 adds a flow-duration term (population_fdc.py): every round is one `population_fdc_stats` call at
    `fdc_probs` (None: its default probabilities), and the quantity minimised, and what history['cost'] holds, is
    (1 - fdc_share) * cost_flow + fdc_share * fdc_score, with cost_flow = 1 - score under `objective` and fdc_score
    `population_fdc_score(stats, fdc_metric)` ('fdc_freq' or 'fdc_vol': zero is perfect), +inf where either is
    undefined; history['score'] and history['score_fdc'] hold the two.  fdc_share in [0, 1].  It goes with objective
    'nse', 'kge' or 'kge12' on daily streamflow alone: with objective 'sse' the raw cost has no scale to mix with, and
    with aux_target or periods / aux_periods it is a ValueError.  With fdc_share == 0 (the default) the function is the
    one above, bit for bit, and hbvx_population_fdc is not touched.

    event_share > 0 adds a flood-event term (population_events.py): `events` = (starts, ends) as
    `population_event_stats` takes them (what `flood_events(target, ...)` returns), every round is one
    `population_event_stats` call, and the quantity minimised, and what history['cost'] holds, is
    (1 - event_share) * (1 - score) + event_share * event_score, with event_score
    `population_event_score(stats, event_metric, timing_scale)` ('peak_error', 'peak_bias', 'peak_timing' or
    'volume_error'), +inf where either is undefined; history['score'] and history['score_event'] hold the two.  The
    windows are checked and their observed half is formed once, before the first round.  event_share in [0, 1].  It goes
    with objective 'nse', 'kge' or 'kge12' on daily streamflow alone: with objective 'sse', with aux_target, periods /
    aux_periods or fdc_share > 0, and without `events`, it is a ValueError.  With event_share == 0 (the default) the
    function is the one above, bit for bit: `events` is not read and hbvx_population_events is not touched."""
    return _search_call(EXPLICIT, "population_search", model, x_dict, parameters, target, names, n_candidates, n_rounds,
                        shrink, weights, generator, objective, transform, eps, aux_target, aux_key, aux_weights,
                        aux_objective, aux_share, periods, aux_periods, fdc_share, fdc_probs, fdc_metric, events,
                        event_share, event_metric, timing_scale)


def _check_mix(objective, aux_objective, aux_share, what):
    """What the search refuses about the weighted sum of the two terms' costs."""
    if aux_objective not in OBJECTIVES:
        raise ValueError(f"{what}: aux_objective must be one of {list(OBJECTIVES)}, got {aux_objective!r}")
    if not 0.0 <= float(aux_share) <= 1.0:          # (a NaN fails both comparisons)
        raise ValueError(f"{what}: aux_share must lie in [0, 1], got {aux_share!r}")
    if aux_objective == 'sse' and objective != 'sse':
        raise ValueError(f"{what}: aux_objective 'sse' with objective {objective!r} would add a squared error to "
                         "1 - score: two scales in one sum")


def _search_call(family, what, model, x_dict, parameters, target, names, n_candidates, n_rounds, shrink, weights,
                 generator, objective, transform, eps, aux_target, aux_key, aux_weights, aux_objective, aux_share, periods,
                 aux_periods, fdc_share=0.0, fdc_probs=None, fdc_metric='fdc_freq', events=None, event_share=0.0,
                 event_metric='peak_error', timing_scale=1.0):
    """`population_search` / `adj_population_search`: the checks, the form every round is scored in ('period' with a
    calendar, or an aux term where there is no joint export) and the loop.  The export is required before the first draw."""
    _check_search(model, n_candidates, n_rounds, shrink, objective, what)
    joint = aux_target is not None or aux_key is not None or aux_weights is not None
    if not 0.0 <= float(fdc_share) <= 1.0:          # (a NaN fails both comparisons)
        raise ValueError(f"{what}: fdc_share must lie in [0, 1], got {fdc_share!r}")
    if not 0.0 <= float(event_share) <= 1.0:
        raise ValueError(f"{what}: event_share must lie in [0, 1], got {event_share!r}")
    if float(event_share) > 0:
        return _event_search(what, model, x_dict, parameters, target, names, n_candidates, n_rounds, shrink, weights,
                             generator, objective, transform, eps, joint, periods, aux_periods, float(fdc_share), events,
                             float(event_share), event_metric, timing_scale)
    if float(fdc_share) > 0:
        return _fdc_search(what, model, x_dict, parameters, target, names, n_candidates, n_rounds, shrink, weights,
                           generator, objective, transform, eps, joint, periods, aux_periods, float(fdc_share), fdc_probs,
                           fdc_metric)
    if periods is not None or aux_periods is not None or (joint and not family.has_joint):
        form = 'period'
        if joint:
            _check_mix(objective, aux_objective, aux_share, what)
        rq = _period_request(family, what, model, x_dict, parameters, None, target, periods, aux_target, aux_key,
                             aux_periods, names, weights, aux_weights, transform, eps)
    else:
        form = 'joint' if joint else 'stats' if objective != 'sse' or transform != 'none' else 'cost'
        rq = _daily_request(family, what, form, model, x_dict, parameters, None, target, names, weights, transform, eps,
                            aux_target, aux_key, aux_weights, mix=(objective, aux_objective, aux_share))

    def evaluate(cands):
        """(cost, score or None) [P,B] of one round's candidates; with the aux term the score is the pair."""
        st = _run(family, form, rq._replace(candidates=cands))
        if form == 'cost':
            return st['cost'], None
        score = population_score(st if form == 'stats' else st['flow'], objective)
        if not joint:
            return _objective_cost(score, objective), score
        score_aux = population_score(st['aux'], aux_objective)
        return _mixed_cost(_objective_cost(score, objective), _objective_cost(score_aux, aux_objective),
                           float(aux_share)), (score, score_aux)

    return _search(rq.req, x_dict, parameters, evaluate, rq.req.tname != 'p_sta', n_candidates, n_rounds, shrink, generator,
                   joint or objective != 'sse', joint)


def _fdc_search(what, model, x_dict, parameters, target, names, n_candidates, n_rounds, shrink, weights, generator,
                objective, transform, eps, joint, periods, aux_periods, fdc_share, fdc_probs, fdc_metric):
    """`population_search` with fdc_share > 0: its refusals, and the loop on `population_fdc_stats`' numbers."""
    from . import population_fdc as pf              # (it imports this module)
    if joint or periods is not None or aux_periods is not None:
        raise ValueError(f"{what}: fdc_share > 0 goes with daily streamflow alone, not with aux_target or periods / "
                         "aux_periods")
    if objective == 'sse':
        raise ValueError(f"{what}: fdc_share > 0 with objective 'sse' would add a distance between curves to a squared "
                         "error: the raw cost has no scale to mix with; use 'nse', 'kge' or 'kge12'")
    if fdc_metric not in pf.FDC_METRICS:
        raise ValueError(f"{what}: fdc_metric must be one of {list(pf.FDC_METRICS)}, got {fdc_metric!r}")
    rq, curve = pf._fdc_request(what, model, x_dict, parameters, None, target, names, weights, transform, eps, fdc_probs,
                                None)

    def evaluate(cands):
        st = pf._fdc_run(rq._replace(candidates=cands), curve)
        score = population_score(st, objective)
        score_fdc = pf.population_fdc_score(st, fdc_metric)
        cost_fdc = torch.where(torch.isnan(score_fdc), torch.full_like(score_fdc, float('inf')), score_fdc)
        return _mixed_cost(_objective_cost(score, objective), cost_fdc, fdc_share), (score, score_fdc)

    return _search(rq.req, x_dict, parameters, evaluate, rq.req.tname != 'p_sta', n_candidates, n_rounds, shrink, generator,
                   True, 'score_fdc')


def _event_search(what, model, x_dict, parameters, target, names, n_candidates, n_rounds, shrink, weights, generator,
                  objective, transform, eps, joint, periods, aux_periods, fdc_share, events, event_share, event_metric,
                  timing_scale):
    """`population_search` with event_share > 0: its refusals, the windows and their observed half once, and the loop on
    `population_event_stats`' numbers."""
    from . import population_events as pe           # (it imports this module)
    if joint or periods is not None or aux_periods is not None or fdc_share > 0:
        raise ValueError(f"{what}: event_share > 0 goes with daily streamflow alone, not with aux_target, periods / "
                         "aux_periods or fdc_share > 0")
    if objective == 'sse':
        raise ValueError(f"{what}: event_share > 0 with objective 'sse' would add an event score to a squared error: the "
                         "raw cost has no scale to mix with; use 'nse', 'kge' or 'kge12'")
    if event_metric not in pe.EVENT_METRICS:
        raise ValueError(f"{what}: event_metric must be one of {list(pe.EVENT_METRICS)}, got {event_metric!r}")
    if events is None:
        raise ValueError(f"{what}: event_share > 0 needs events (see flood_events)")
    rq, win = pe._event_request(what, model, x_dict, parameters, None, target, events, names, weights, transform, eps)

    def evaluate(cands):
        st = pe._event_run(rq._replace(candidates=cands), win)
        score = population_score(st, objective)
        score_event = pe.population_event_score(st, event_metric, timing_scale)
        cost_event = torch.where(torch.isnan(score_event), torch.full_like(score_event, float('inf')), score_event)
        return _mixed_cost(_objective_cost(score, objective), cost_event, event_share), (score, score_event)

    return _search(rq.req, x_dict, parameters, evaluate, rq.req.tname != 'p_sta', n_candidates, n_rounds, shrink, generator,
                   True, 'score_event')


def _mixed_cost(cost_flow: torch.Tensor, cost_aux: torch.Tensor, aux_share: float) -> torch.Tensor:
    """(1 - aux_share) * cost_flow + aux_share * cost_aux, +inf where either is +inf (a share of 0 does not hide a
    series that admits no score: 0 * inf would be NaN)."""
    mixed = (1.0 - aux_share) * torch.where(torch.isinf(cost_flow), torch.zeros_like(cost_flow), cost_flow) \
        + aux_share * torch.where(torch.isinf(cost_aux), torch.zeros_like(cost_aux), cost_aux)
    return torch.where(torch.isinf(cost_flow) | torch.isinf(cost_aux), torch.full_like(mixed, float('inf')), mixed)


def _check_search(model, n_candidates, n_rounds, shrink, objective, what):
    """The search's own refusals, before anything else."""
    if float(getattr(model, 'dy_drop', 0.0)) > 0:
        raise ValueError(f"{what}: dy_drop > 0 draws new masks in every run, the cost is stochastic; set dy_drop = 0")
    if n_candidates < 2:
        raise ValueError("n_candidates must be >= 2 (the current row and at least one draw)")
    if n_rounds < 1:
        raise ValueError("n_rounds must be >= 1")
    if not 0 < shrink <= 1:
        raise ValueError(f"{what} wants 0 < shrink <= 1")
    if objective not in OBJECTIVES:
        raise ValueError(f"{what}: objective must be one of {list(OBJECTIVES)}, got {objective!r}")


def _search(req, x_dict, parameters, evaluate, raw, n_candidates, n_rounds, shrink, generator, keep_score,
            two_scores=False):
    """The search loop of `population_search` and `adj_population_search`: `evaluate(cands)` -> (cost, score or None)
    [P,B] is the front end's route to one round's numbers; raw: the module applies a sigmoid to the row.  two_scores:
    `evaluate` returns the pair (score, score_aux), kept as history['score'] and history['score_aux'] -- or under the
    name two_scores itself where it is one ('score_fdc', 'score_event')."""
    two = req.tname == 'p_sta'
    cur = _static_tensor(two, parameters).detach().clone()
    row = cur if two else cur[-1]           # [B,width] view of the row that moves
    dev = x_dict['x_phy'].device
    cols = torch.as_tensor(req.cols, dtype=torch.long, device=cur.device)
    C = len(req.cols)
    gdev = generator.device if generator is not None else torch.device('cpu')

    best = row[:, cols].to(device=dev, dtype=torch.float32)                     # [B,C], input space
    best_u = torch.sigmoid(best) if raw else best.clone()
    kept = ['score'] * bool(keep_score) + [two_scores if isinstance(two_scores, str) else 'score_aux'] * bool(two_scores)
    hist = {'cost': [], 'best_index': [], 'columns': list(req.cols), **{name: [] for name in kept}}
    for k in range(n_rounds):
        draws = torch.rand((n_candidates - 1, req.B, C), generator=generator, device=gdev).to(dev)
        if k > 0:
            draws = best_u.unsqueeze(0) + (draws - 0.5) * float(shrink) ** k
        cands = torch.cat([best.unsqueeze(0), _to_input_space(draws, raw)]).contiguous()
        cost, score = evaluate(cands)
        scores = dict(zip(kept, score if two_scores else (score,)))
        low, idx = cost.min(0)
        idx = torch.where(cost[0] <= low, torch.zeros_like(idx), idx)          # a tie keeps the row that is held
        if k == 0:
            hist['cost'].append(cost[0].double().cpu())
            for name, sc in scores.items():
                hist[name].append(sc[0].cpu())
        pick = idx.view(1, req.B, 1).expand(1, req.B, C)
        best = cands.gather(0, pick)[0]
        best_u = torch.sigmoid(best) if raw else best.clone()
        hist['cost'].append(cost.gather(0, idx.unsqueeze(0))[0].double().cpu())
        for name, sc in scores.items():
            hist[name].append(sc.gather(0, idx.unsqueeze(0))[0].cpu())
        hist['best_index'].append(idx.cpu())
    row[:, cols] = best.to(cur.device)
    for name in ['cost', 'best_index'] + kept:
        hist[name] = torch.stack(hist[name])
    return ((parameters[0], cur) if two else cur), hist
