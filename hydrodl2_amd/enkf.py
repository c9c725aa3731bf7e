"""State estimation: an ensemble Kalman filter over the explicit models' storages, one analysis kernel per observation.

`particle_filter` (ensemble.py) can only choose among the storages its particles already have; an ensemble Kalman filter
MOVES them: per basin, every storage of every member and every entry of the routing history is regressed on the predicted
flow across the particles and shifted by gain x innovation.  hbvx_enkf_update (include/hbvx_enkf.h) is that analysis step
-- float32 in, float64 sums in particle order, one rounding at the store, a thread per element, no temporaries -- and on it

  `enkf_update`   analyses an `EnsembleState` (and any [P,k,B] arrays beside it) against ONE observation per basin, by
                  perturbed observations or by the serial square-root form of Whitaker and Hamill, with multiplicative
                  posterior inflation and a floor;
  `enkf_filter`   walks a record in windows as `particle_filter` does -- `ensemble_record` once, one
                  hbvx_population_ensemble launch per window, the same forcing noise in the same draw order -- and
                  assimilates a window's observations serially in day order; there is no ancestor index and there are
                  no weights: the next launch reads the updated state.

Hbv, Hbv_1_1p and Hbv_2, daily.  Not built: a full observation-error covariance (serial assimilation with a diagonal R
covers a window), localisation across basins (basins are independent by construction), adaptive inflation, an update of
candidate parameter columns, the implicit, hourly and multi-timescale models, graph=True capture.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _abi, ops
from ._lib import get_library
from .ensemble import (EnsembleState, HIST, _check_counts, _check_noise, _check_state, _launch, _randn, _refuse, _sigma,
                       _start_states, ensemble_record)
from .population import _check_rows, _observations

EXPORT = 'hbvx_enkf_update'
METHODS = tuple(_abi.ENKF_METHODS)       # 'perturbed', 'sqrt'


def _check_method(method, inflation, what):
    if method not in _abi.ENKF_METHODS:
        raise ValueError(f"{what}: method must be one of {list(METHODS)}, got {method!r}")
    try:
        rho = float(inflation)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: inflation must be a number, got {inflation!r}") from None
    if not (math.isfinite(rho) and rho > 0.0):
        raise ValueError(f"{what}: inflation must be finite and > 0, got {inflation!r}")
    return rho


def _analyse(states, history, y, obs, obs_var, method, rho, eps, floor, extras, extra_lo, active, inplace):
    """One hbvx_enkf_update call on checked tensors: (states, history, extras, status, stats)."""
    out = (lambda t: t) if inplace else (lambda t: None)
    arrays = [ops.EnkfArray(states, int(states.shape[3]), floor, out(states))]
    if history is not None:
        arrays.append(ops.EnkfArray(history, 1, 0.0, out(history)))
    arrays += [ops.EnkfArray(x, 1, extra_lo, out(x)) for x in extras]
    outs, status, stats = ops.enkf_update(y, obs, obs_var, arrays, _abi.ENKF_METHODS[method], rho, eps, active)
    k = 1 if history is None else 2
    return outs[0], None if history is None else outs[1], outs[k:], status, stats


def enkf_update(state: EnsembleState, predicted: torch.Tensor, observed: torch.Tensor, obs_sigma, *, method: str = 'sqrt',
                eps: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, inflation: float = 1.0,
                floor: float = 1e-5, extra: Sequence[torch.Tensor] = (), active: Optional[torch.Tensor] = None) -> dict:
    """The ensemble Kalman analysis of P particles against one observation per basin, in ONE call of hbvx_enkf_update.

    state        an `EnsembleState`: `states` [P,5,B,M] and `history` [P,14,B] or None are analysed; `day` is kept.
    predicted    [P,B] float32: what each particle predicts for the observation, in whatever (transformed) space the caller
                 scores in; observed [B] float32 or float64 in the same space, NaN where missing.
    obs_sigma    a scalar or [B], > 0: the standard deviation of the observation error in that space (R = sigma^2).
    method       'sqrt': the serial square-root filter of Whitaker and Hamill, deterministic; 'perturbed': every particle
                 sees observed + eps, eps [P,B] float32 given or drawn as obs_sigma * randn from `generator`.
    inflation    rho > 0: analysed anomalies about the analysis mean are multiplied by it; 1 is no operation at all.
    floor        the storages are floored at it after the update (the model's `nearzero`); the history is floored at 0.
    extra        up to two [P,k,B] float32 tensors analysed alongside with the same gain rule and no floor (the predicted
                 rows of the window that remain, for instance; `predicted` itself to get the analysed prediction).
    active       [B] bool or None: basins with False are not analysed.
    Per basin and element, with x_p the particles' values and y_p their predictions (float64, sums in particle order):
    K = cov(x, y) / (var(y) + R); 'perturbed': x_p += K (observed + eps_p - y_p); 'sqrt': the mean moves by
    K (observed - ybar) and the anomalies by -alpha K (y_p - ybar), alpha = 1 / (1 + sqrt(R / (var(y) + R))).
    Returns {'state': the analysed `EnsembleState` (new tensors, same day, weights None), 'extra': the analysed extras,
    'ybar', 'yvar', 'innovation': [B] float64 (the mean, the variance across particles and observed - ybar; NaN where not
    formed), 'status': [B] int32 -- 0 analysed, 1 inactive or missing (a bit copy), 2 a non-finite mean, variance or
    perturbation (a bit copy), 3 some element of the basin had a non-finite gain or result and was copied}.

    Two calls agree bit for bit; a basin's results depend on its own columns alone.

    Refused (ValueError): a state that is no `EnsembleState`, wrong shapes / dtypes / devices of state, predicted,
    observed, eps, extra or active, P < 2, more than two extras, obs_sigma <= 0 or not finite, inflation <= 0 or not
    finite, a floor that is not finite, an unknown method; a library without hbvx_enkf_update (HbvxError)."""
    what = "enkf_update"
    if not isinstance(state, EnsembleState):
        raise ValueError(f"{what}: state must be an EnsembleState, got {type(state).__name__}")
    if not torch.is_tensor(state.states):
        raise ValueError(f"{what}: state.states must be a float32 tensor, got {type(state.states).__name__}")
    anchor = {'x_phy': state.states}
    _check_state(anchor, state, what)
    P, _, B, M = (int(n) for n in state.states.shape)
    if P < 2:
        raise ValueError(f"{what}: an ensemble Kalman update needs at least 2 particles, got {P}")
    if state.history is not None and int(state.history.shape[2]) != B:
        raise ValueError(f"{what}: state.history must be [{P},{HIST},{B}], got {tuple(state.history.shape)}")
    rho = _check_method(method, inflation, what)
    if not (isinstance(floor, (int, float)) and math.isfinite(float(floor))):
        raise ValueError(f"{what}: floor must be finite, got {floor!r}")
    dev = state.states.device
    _check_noise(anchor, 'predicted', predicted, what)
    if predicted is None or tuple(predicted.shape) != (P, B):
        raise ValueError(f"{what}: predicted must be [{P},{B}], got {None if predicted is None else tuple(predicted.shape)}")
    if not torch.is_tensor(observed) or observed.dtype not in (torch.float32, torch.float64) or \
            tuple(observed.shape) != (B,):
        raise ValueError(f"{what}: observed must be a float32 or float64 [{B}] tensor, got "
                         f"{(observed.dtype, tuple(observed.shape)) if torch.is_tensor(observed) else type(observed).__name__}")
    if observed.device != dev:
        raise ValueError(f"{what}: observed lives on {observed.device}, the state on {dev}")
    if bool(torch.isinf(observed).any()):
        raise ValueError(f"{what}: observed holds infinities (a missing observation is a NaN)")
    sigma = _sigma(obs_sigma, B, dev, what)
    if method == 'perturbed' and eps is not None:
        _check_noise(anchor, 'eps', eps, what)
        if tuple(eps.shape) != (P, B):
            raise ValueError(f"{what}: eps must be [{P},{B}], got {tuple(eps.shape)}")
    extra = list(extra)
    if len(extra) > _abi.ENKF_MAX_ARRAYS - 2:
        raise ValueError(f"{what}: at most {_abi.ENKF_MAX_ARRAYS - 2} extra arrays, got {len(extra)}")
    for i, x in enumerate(extra):
        if x is None:
            raise ValueError(f"{what}: extra[{i}] must be a float32 tensor, got NoneType")
        _check_noise(anchor, f'extra[{i}]', x, what)
        if x.dim() != 3 or int(x.shape[0]) != P or int(x.shape[2]) != B or int(x.shape[1]) < 1:
            raise ValueError(f"{what}: extra[{i}] must be [{P},k,{B}], got {tuple(x.shape)}")
    if active is not None:
        if not torch.is_tensor(active) or active.dtype != torch.bool or tuple(active.shape) != (B,):
            raise ValueError(f"{what}: active must be a bool [{B}] tensor, got "
                             f"{(active.dtype, tuple(active.shape)) if torch.is_tensor(active) else type(active).__name__}")
        if active.device != dev:
            raise ValueError(f"{what}: active lives on {active.device}, the state on {dev}")
    get_library().require(EXPORT)
    sigma32 = sigma.float()
    if method == 'perturbed' and eps is None:
        eps = sigma32 * _randn((P, B), generator, dev)
    states, history, extras, status, stats = _analyse(
        state.states.contiguous(), None if state.history is None else state.history.contiguous(),
        predicted.contiguous(), observed.float().contiguous(), sigma.square().float().contiguous(), method, rho,
        None if method != 'perturbed' else eps.contiguous(), float(floor), [x.contiguous() for x in extra],
        -math.inf, None if active is None else active.contiguous(), False)
    return {'state': EnsembleState(states, history, state.day), 'extra': extras, 'ybar': stats[0], 'yvar': stats[1],
            'innovation': stats[2], 'status': status}


def _forward_transform(sim: torch.Tensor, transform: str, eps):
    """float32 [P,rows,B] -> the space `population_stats` scores in (a new tensor)."""
    if transform == 'sqrt':
        return torch.sqrt(sim)
    if transform == 'log':
        return torch.log(sim + eps)
    return sim.clone()


def _back_transform(z: torch.Tensor, transform: str, eps):
    """The flow of a transformed value, float64, never negative."""
    z = z.double()
    if transform == 'sqrt':
        return z.clamp_min(0.0).square()
    if transform == 'log':
        return (torch.exp(z) - eps.double()).clamp_min(0.0)
    return z.clamp_min(0.0)


def enkf_filter(model, x_dict: dict, parameters, target, n_particles: int, window: int = 1, *, obs_sigma,
                method: str = 'sqrt', prcp_sigma: float = 0.0, temp_sigma: float = 0.0, state_sigma: float = 0.0,
                state_add_sigma: float = 0.0, inflation: float = 1.0, transform: str = 'none', eps=None, weights=None,
                generator: Optional[torch.Generator] = None, return_series: bool = False) -> dict:
    """An ensemble Kalman filter of the storages and the routing history, per basin, over consecutive windows of `window`
    days: one hbvx_population_ensemble launch per window, one hbvx_enkf_update call per scored day.

    Initial particles: the module's start state times exp(state_sigma z) (`particle_filter`'s form), then plus
    state_add_sigma z millimetres, floored at the model's nearzero -- multiplicative noise on storages of 0.001 mm stays at
    0.001 mm, additive noise gives a dry start a spread the gain can work with.  Forcing noise per (particle, day, basin) as
    `particle_filter` draws it, in the same order: prcp_mul = exp(prcp_sigma z - prcp_sigma^2 / 2), temp_add =
    temp_sigma z.  After a window's launch its scored days are assimilated SERIALLY in day order: for day r, y is a copy
    of that day's current predicted row in the transformed space, and one `enkf_update` moves the storages at the window's
    end, the routing history and the window's predicted rows from r on ([P,k,B]) -- so later observations see earlier
    updates, and the analysed row comes back.  A basin is analysed on a day with a weight > 0 and a finite target; the
    mask goes to the kernel, nothing is decided on the host between launches.  With window=1 this is the classical
    daily EnKF.  A window longer than a day updates the END state from observations up to `window`-1 days old through
    the ensemble's own lagged covariances: it is another filter than window=1, not an approximation of it.

    target, weights, transform, eps   as `population_stats`; obs_sigma a scalar or [B], > 0, in the transformed space.
    method, inflation   as `enkf_update`; under 'perturbed' every scored day draws obs_sigma * randn [P,B] after the window's
                 forcing noise.
    generator    every draw comes from it, in a fixed order: two runs with equally seeded generators agree bit for bit.
    Returns {'forecast_mean': [T_out,B] float64 the ensemble mean of the simulated flow, before that day's observation is
    used (observations of EARLIER days have moved the state it started from); 'spread': [T_out,B] float64 its standard
    deviation across particles; 'analysis_mean': [T_out,B] float64 the mean of the analysed predicted row,
    back-transformed to a flow; 'innovation': [T_out,B] float64 observed - ybar in the transformed space, NaN where
    nothing was analysed; 'status': [T_out,B] int32 (`enkf_update`'s); 'state': the final `EnsembleState` (weights None;
    `ensemble_forecast` takes it as it is); 'windows': [n_windows,2] int64 descriptor days; 'outputs'; with return_series
    'series' [P,T_out,B] float32, the forecast series}.

    Refused before the model runs: what `particle_filter` refuses; n_particles < 2, an unknown method, inflation <= 0 or
    not finite, a negative state_add_sigma (ValueError); a library without hbvx_enkf_update (HbvxError)."""
    what = "enkf_filter"
    _check_counts(n_particles, what)
    if n_particles is None or n_particles < 2:
        raise ValueError(f"{what}: n_particles must be an integer >= 2, got {n_particles!r}")
    if isinstance(window, bool) or not isinstance(window, int) or window < 1:
        raise ValueError(f"{what}: window must be an integer >= 1 (days per launch), got {window!r}")
    for name, v in (('prcp_sigma', prcp_sigma), ('temp_sigma', temp_sigma), ('state_sigma', state_sigma),
                    ('state_add_sigma', state_add_sigma)):
        if not (float(v) >= 0.0 and math.isfinite(float(v))):
            raise ValueError(f"{what}: {name} must be finite and >= 0, got {v!r}")
    rho = _check_method(method, inflation, what)
    req = _refuse(model, x_dict, parameters, None, what)
    get_library().require(EXPORT)
    _check_rows(req, x_dict, target, weights, req.T_out, "days after the warm-up", what)
    dev = x_dict['x_phy'].device
    sigma = _sigma(obs_sigma, req.B, dev, what)
    ob = _observations(req, x_dict, target, weights, transform, eps, what)
    rec = ensemble_record(model, x_dict, parameters)
    cfg, t_first = rec.main.cfg, rec.t_first
    T, B, P = cfg.T, cfg.B, n_particles
    floor = float(cfg.nearzero)

    states = _start_states(rec).unsqueeze(0).expand(P, 5, B, cfg.M)
    if state_sigma > 0:
        states = states * torch.exp(float(state_sigma) * _randn((P, 5, B, cfg.M), generator, dev))
    if state_add_sigma > 0:
        states = (states + float(state_add_sigma) * _randn((P, 5, B, cfg.M), generator, dev)).clamp_min(floor)
    states = states.contiguous()
    history = None
    sigma32, var32 = sigma.float(), sigma.square().float().contiguous()
    active = (torch.ones_like(ob['target'], dtype=torch.bool) if ob['w'] is None else ob['w'] > 0).contiguous()
    extra_lo = -math.inf if transform == 'log' else 0.0        # a flow and its square root are not negative
    shape = (req.T_out, B)
    fmean = torch.zeros(shape, dtype=torch.float64, device=dev)
    spread, amean = torch.zeros_like(fmean), torch.zeros_like(fmean)
    innovation = torch.full(shape, math.nan, dtype=torch.float64, device=dev)
    status = torch.ones(shape, dtype=torch.int32, device=dev)
    series = torch.empty((P, req.T_out, B), dtype=torch.float32, device=dev) if return_series else None
    bounds = [(a, min(a + window, T)) for a in range(0, T, window)]
    for a, b in bounds:
        W = b - a
        pm = ta = None
        if prcp_sigma > 0:
            s = float(prcp_sigma)
            pm = torch.exp(s * _randn((P, W, B), generator, dev) - 0.5 * s * s).contiguous()
        if temp_sigma > 0:
            ta = (float(temp_sigma) * _randn((P, W, B), generator, dev)).contiguous()
        flow_out, _, states, history = _launch(rec, ob, transform, P, a, b, states, history, None, pm, ta, {},
                                               (None, None), True)
        r0, r1 = max(a, t_first) - t_first, max(b, t_first) - t_first
        if r1 == r0:                # a window of warm-up days: nothing is observed
            continue
        sim = flow_out[4]           # [P,rows,B]
        sim8 = sim.double()
        fmean[r0:r1] = sim8.mean(0)
        spread[r0:r1] = sim8.std(0)
        if return_series:
            series[:, r0:r1] = sim
        z = _forward_transform(sim, transform, ob['eps'])
        for r in range(r1 - r0):
            y = z[:, r].clone()
            tail = z[:, r:] if r == 0 else z[:, r:].contiguous()
            e = (sigma32 * _randn((P, B), generator, dev)).contiguous() if method == 'perturbed' else None
            states, history, _, st, stats = _analyse(states, history, y, ob['target'][r0 + r], var32, method, rho, e,
                                                     floor, [tail], extra_lo, active[r0 + r], True)
            if r > 0:
                z[:, r:] = tail
            amean[r0 + r] = _back_transform(tail[:, 0], transform, ob['eps']).mean(0)
            innovation[r0 + r] = stats[2]
            status[r0 + r] = st
    out = {'forecast_mean': fmean, 'analysis_mean': amean, 'spread': spread, 'innovation': innovation, 'status': status,
           'state': EnsembleState(states, history, T), 'windows': torch.tensor(bounds, dtype=torch.int64),
           'outputs': rec.outputs}
    if return_series:
        out['series'] = series
    return out
