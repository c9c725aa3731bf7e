"""State estimation: a particle filter over the explicit models' storages, one kernel launch per window.

The population calls answer which parameters fit a record.  The question after that -- given yesterday's observed flow,
what are the storages now, and what does an ensemble forecast from them look like -- needs an ensemble whose members
differ in their STATE and their forcings.  An element of that ensemble is a PARTICLE here (a basin's `nmul` members keep
the word member).  hbvx_population_ensemble (include/hbvx_pop_ens.h) is the stats form of the population kernel over a
window of the record's days with storages, routing history and forcing noise per particle, handed back for the next
window; on it,

  `ensemble_record`    runs the module once (its warm-up, its dy_drop draws, its descriptor) and keeps that call;
  `ensemble_step`      advances P particles over days t_begin .. t_end-1 in ONE launch: the four sums `population_score`
                       reads, the new `EnsembleState`, optionally the window's series;
  `particle_filter`    sequential importance resampling per basin over consecutive windows: multiplicative log-normal
                       precipitation noise, additive temperature noise, a Gaussian likelihood in the transformed space,
                       systematic resampling where the effective sample size falls below a threshold -- the resampling
                       is an `ancestor` index the next launch reads, nothing is gathered on the host between windows;
  `ensemble_forecast`  runs particles over a future record without observations and forms weighted quantiles.

Hbv, Hbv_1_1p and Hbv_2, daily.  Updates that MOVE the states by a gain instead of choosing among them -- the ensemble
Kalman filter on the same launches and the same `EnsembleState` -- are hydrodl2_amd/enkf.py (`enkf_update`,
`enkf_filter`).  Not built: noise on PET, the dynamic parameters or muwts; an aux series or period calendars;
the implicit, hourly and multi-timescale models; quantiles across particles inside the kernel; graph=True capture.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence

import torch

from . import _abi, ops
from ._lib import get_library
from .calibrate import _NO_TARGET
from .population import EXPLICIT, _candidate_sources, _check, _check_candidates, _check_rows, _observations, _primal

EXPORT = 'hbvx_population_ensemble'
HIST = _abi.POP_ENS_HIST


class EnsembleState(NamedTuple):
    """P particles at the start of descriptor day `day`: `states` [P,5,B,M] float32 (snowpack, meltwater, soil moisture,
    upper and lower zone), `history` [P,14,B] float32 or None (a model that does not route; or zeros: entry k is the
    un-routed ensemble-mean flow of day `day`-1-k), `weights` [P,B] float64 or None (uniform)."""
    states: torch.Tensor
    history: Optional[torch.Tensor]
    day: int
    weights: Optional[torch.Tensor] = None


class EnsembleRecord(NamedTuple):
    """One run of the module, kept: `ensemble_step` takes it in place of (model, x_dict, parameters)."""
    model: object
    x_dict: dict
    parameters: object
    req: object             # calibrate's request for every static column: T_out, B
    outputs: dict           # the primal flux dictionary
    main: object            # ops.PathRecord of the module's main pass
    t_first: int            # the first scored day of the descriptor (warm_up_states=False: the warm-up days)


def _refuse(model, x_dict, parameters, names, what):
    """Everything that can be refused about the model without running it, in the population calls' wording; and the
    export, named before the module runs."""
    req = _check(EXPLICIT, model, x_dict, parameters, _NO_TARGET, names, None, what)
    get_library().require(EXPORT)
    return req


def ensemble_record(model, x_dict: dict, parameters) -> EnsembleRecord:
    """Runs the module once at `parameters` -- its warm-up pass, its dy_drop draws, the descriptor of its main pass -- and
    returns the recorded call for `ensemble_step`.  The tensors of x_dict and parameters must stay alive and unchanged
    while the record is used.  Refusals: `ensemble_step`'s."""
    req = _refuse(model, x_dict, parameters, None, "ensemble_record")
    outputs, main, t_first = _primal(EXPLICIT, model, req, x_dict, parameters)
    return EnsembleRecord(model, x_dict, parameters, req, outputs, main, t_first)


def _start_states(rec: EnsembleRecord) -> torch.Tensor:
    """[5,B,M] float32: what the recorded call started from (0.001 everywhere without carried-in storages)."""
    cfg = rec.main.cfg
    if rec.main.state_in is not None:
        return rec.main.state_in.detach().reshape(5, cfg.B, cfg.M)
    return torch.full((5, cfg.B, cfg.M), 0.001, dtype=torch.float32, device=rec.main.x.device)


def _check_counts(n_particles, what):
    if n_particles is not None and (isinstance(n_particles, bool) or not isinstance(n_particles, int) or n_particles < 1):
        raise ValueError(f"{what}: n_particles must be an integer >= 1, got {n_particles!r}")


def _check_noise(x_dict, name, t, what):
    """What can be refused about prcp_mul / temp_add / ancestor / a state tensor before the window is known."""
    if t is None:
        return
    dev = x_dict['x_phy'].device
    want = torch.int32 if name == 'ancestor' else torch.float32
    if not torch.is_tensor(t) or t.dtype != want:
        raise ValueError(f"{what}: {name} must be a {str(want).replace('torch.', '')} tensor, got "
                         f"{t.dtype if torch.is_tensor(t) else type(t).__name__}")
    if t.device != dev:
        raise ValueError(f"{what}: {name} lives on {t.device}, x_phy on {dev}")


def _check_state(x_dict, state, what):
    if state is None:
        return
    if not isinstance(state, EnsembleState):
        raise ValueError(f"{what}: state must be an EnsembleState, got {type(state).__name__}")
    _check_noise(x_dict, 'state.states', state.states, what)
    _check_noise(x_dict, 'state.history', state.history, what)
    if state.states.dim() != 4 or int(state.states.shape[1]) != 5:
        raise ValueError(f"{what}: state.states must be [P,5,B,M], got {tuple(state.states.shape)}")
    if state.history is not None and (state.history.dim() != 3 or tuple(state.history.shape[:2]) !=
                                      (int(state.states.shape[0]), HIST)):
        raise ValueError(f"{what}: state.history must be [{int(state.states.shape[0])},{HIST},B], got "
                         f"{tuple(state.history.shape)}")


def _window_obs(ob: dict, r0: int, r1: int) -> dict:
    """Rows r0 .. r1-1 of the record's observation side (`_observations`): views of target / w, and the window's own
    float64 sums about the record's shift."""
    tgt = ob['target'][r0:r1]
    w = None if ob['w'] is None else ob['w'][r0:r1]
    w8 = torch.ones_like(tgt, dtype=torch.float64) if w is None else w.double()
    e = tgt.double() - ob['shift'].double()
    return {'target': tgt, 'w': w, 'shift': ob['shift'], 'eps': ob['eps'],
            'obs': {'W': w8.sum(0), 'e1': (w8 * e).sum(0), 'e2': (w8 * e * e).sum(0)},
            'n_obs': (w8 > 0).sum(0, dtype=torch.int64)}


def _launch(rec: EnsembleRecord, ob: dict, transform: str, P: int, t_begin: int, t_end: int, states, history, ancestor,
            prcp_mul, temp_add, sources, route, want_sim: bool):
    """One hbvx_population_ensemble launch over descriptor days t_begin .. t_end-1 with the record's observation side `ob`
    (rows are scored days of the RECORD): (flow_out, window observations, state_out, hist_out)."""
    t0 = max(t_begin, rec.t_first)
    wob = _window_obs(ob, max(t0 - rec.t_first, 0), max(t_end - rec.t_first, 0))
    flow = ops.PopTerm(wob['target'], wob['w'], wob['shift'], wob['eps'], transform)
    ens = ops.EnsTerm(P, t_begin, t_end, states, history, ancestor, prcp_mul, temp_add)
    flow_out, (state_out, hist_out) = ops.population_ensemble(rec.main, sources, route, flow, ens, rec.t_first, want_sim)
    return flow_out, wob, state_out, hist_out


def ensemble_step(model, x_dict: Optional[dict], parameters, target, state: Optional[EnsembleState] = None,
                  t_begin: Optional[int] = None, t_end: Optional[int] = None, n_particles: Optional[int] = None,
                  candidates: Optional[torch.Tensor] = None, names: Optional[Sequence[str]] = None, weights=None,
                  transform: str = 'none', eps=None, prcp_mul: Optional[torch.Tensor] = None,
                  temp_add: Optional[torch.Tensor] = None, ancestor: Optional[torch.Tensor] = None,
                  return_series: bool = False) -> dict:
    """Advances P particles over days t_begin .. t_end-1 of the record in one launch of hbvx_population_ensemble.

    model, x_dict, parameters   as `population_stats` takes them: the module runs once (`ensemble_record`); or an
                 `EnsembleRecord` as `model`, with x_dict and parameters None: nothing is re-run.
    target, weights, transform, eps   as `population_stats`: [T_out,B] over the scored days of the WHOLE record; the
                 window reads its own rows.  The sums are those of the window's scored days.
    state        where the particles stand (None: every particle at the module's start state, zero routing history, day
                 0); t_begin defaults to state.day, t_end to the record's last day + 1.  Days are the descriptor's: with
                 warm_up_states=False the first `warm_up` of them are simulated and not scored.
    n_particles  P; may be omitted when `state`, `candidates`, prcp_mul, temp_add or ancestor fixes it.
    candidates, names   optional [P,B,C] static values per particle, as `population_stats` takes them (joint
                 state-parameter particles); None: every particle has `parameters`.
    prcp_mul, temp_add   None, [P,B] or [P,t_end-t_begin,B] float32: P = P * prcp_mul, T = T + temp_add, one float32
                 operation each, PET untouched.  None is no operation at all.
    ancestor     [P,B] int32 or None: particle c of basin b starts from state particle ancestor[c,b] (values must lie in
                 0..len(state)-1; the kernel clamps anything else).
    Returns {'sse','s1','s2','s3' [P,B] float32, 'shift','obs','transform','eps','n_obs','columns','outputs'} as
    `population_stats` does -- `population_score` reads it; a window without a scored day has zero sums and n_obs 0 --
    and 'state': the `EnsembleState` at t_end; with return_series 'series' [P,rows,B], the window's scored days.

    Two calls agree bit for bit; a particle's bits depend on its own inputs alone; consecutive windows, each fed the
    previous 'state', give the bits of one window over the same days.

    Refused before the model runs: HbvAdj, Hbv_2_hourly, Hbv_2_mts and anything else (NotImplementedError); graph=True,
    initialize mode, comprout=True, dynamic or unknown names, a wrong shape / dtype / device of candidates, target,
    weights, state, prcp_mul, temp_add or ancestor, n_particles < 1 (ValueError); a library without
    hbvx_population_ensemble (HbvxError).  A window outside the record is refused once the record's length is known."""
    what = "ensemble_step"
    if isinstance(model, EnsembleRecord):
        if x_dict is not None or parameters is not None:
            raise ValueError(f"{what}: with an EnsembleRecord, x_dict and parameters must be None")
        rec = model
        model, x_dict, parameters = rec.model, rec.x_dict, rec.parameters
        get_library().require(EXPORT)
    else:
        rec = None
    _check_counts(n_particles, what)
    req = rec.req if rec is not None and names is None else _refuse(model, x_dict, parameters, names, what)
    _check_rows(req, x_dict, target, weights, req.T_out, "days after the warm-up", what)
    if candidates is not None:
        _check_candidates(req, x_dict, candidates)
    _check_state(x_dict, state, what)
    for name, t in (('prcp_mul', prcp_mul), ('temp_add', temp_add), ('ancestor', ancestor)):
        _check_noise(x_dict, name, t, what)
    sizes = {int(t.shape[0]) for t in (candidates, prcp_mul, temp_add, ancestor) if t is not None and t.dim() >= 1}
    if state is not None and ancestor is None:
        sizes.add(int(state.states.shape[0]))
    if n_particles is not None:
        sizes.add(n_particles)
    if len(sizes) != 1:
        raise ValueError(f"{what}: the particle count must be given once and consistently (n_particles, state, candidates, "
                         f"prcp_mul, temp_add, ancestor), got {sorted(sizes)}")
    P = sizes.pop()
    ob = _observations(req, x_dict, target, weights, transform, eps, what)
    if rec is None:
        rec = ensemble_record(model, x_dict, parameters)
    t_begin = (state.day if state is not None else 0) if t_begin is None else t_begin
    t_end = rec.main.cfg.T if t_end is None else t_end
    sources, route = ({}, (None, None)) if candidates is None else _candidate_sources(model, names, candidates)
    flow_out, wob, state_out, hist_out = _launch(
        rec, ob, transform, P, t_begin, t_end, None if state is None else state.states.contiguous(),
        None if state is None or state.history is None else state.history.contiguous(), ancestor, prcp_mul, temp_add,
        sources, route, return_series)
    out = dict(zip(('sse', 's1', 's2', 's3'), flow_out[:4]))
    out.update(shift=wob['shift'], obs=wob['obs'], transform=transform, eps=wob['eps'], n_obs=wob['n_obs'],
               columns=list(req.cols) if candidates is not None else [], outputs=rec.outputs,
               state=EnsembleState(state_out, hist_out, t_end))
    if return_series:
        out['series'] = flow_out[4]
    return out


# ---- the filter's arithmetic, on plain tensors (tests/test_ensemble_host.py) ----------------------------------------------

def update_log_weights(log_w: torch.Tensor, sse: torch.Tensor, obs_sigma: torch.Tensor):
    """The importance update of one window, float64 per basin: log_w [P,B] (normalised: logsumexp over particles is 0),
    sse [P,B] the window's squared error in the transformed space, obs_sigma [B] > 0.
        l = log_w - 0.5 * sse / obs_sigma^2        (a non-finite sse is a particle of weight zero: l = -inf)
        lse = logsumexp_c l                        (the window's log-likelihood increment without its constant)
    Returns (log_w' = l - lse, lse, degenerate [B] bool).  A basin whose l are all -inf (or whose lse is not finite) is
    degenerate: it keeps UNIFORM weights, its lse is reported as 0 and the caller reports the basin."""
    P = log_w.shape[0]
    s = sse.double()
    l = log_w.double() - 0.5 * s / obs_sigma.double().square()
    l = torch.where(torch.isfinite(s) & ~torch.isnan(l), l, torch.full_like(l, -math.inf))
    lse = torch.logsumexp(l, 0)
    degenerate = ~torch.isfinite(lse)
    uniform = torch.full_like(l, -math.log(P))
    new = torch.where(degenerate.unsqueeze(0), uniform, l - torch.where(degenerate, torch.zeros_like(lse), lse))
    return new, torch.where(degenerate, torch.zeros_like(lse), lse), degenerate


def effective_sample_size(log_w: torch.Tensor) -> torch.Tensor:
    """[B] float64: 1 / sum_c w^2 of normalised log-weights [P,B]."""
    return 1.0 / torch.exp(2.0 * log_w.double()).sum(0)


def systematic_resample(log_w: torch.Tensor, u: torch.Tensor, resample: torch.Tensor) -> torch.Tensor:
    """[P,B] int32 ancestors by systematic resampling, per basin: with w = exp(log_w) [P,B] float64 and ONE uniform u[b]
    in [0,1) per basin, the P points (u + i) / P, i = 0..P-1, are looked up in the running sum of w: ancestor i is the
    first particle whose running sum exceeds the point.  Every particle gets floor(P w) or ceil(P w) offspring, the
    ancestors ascend.  Basins where `resample` [B] is False get the identity row."""
    P, B = log_w.shape
    w = torch.exp(log_w.double())
    cum = torch.cumsum(w, 0)
    cum = cum / cum[-1:]                                                    # (the last running sum is 1 up to rounding)
    pts = (u.double().unsqueeze(0) + torch.arange(P, dtype=torch.float64, device=w.device).unsqueeze(1)) / P   # [P,B]
    anc = torch.searchsorted(cum.t().contiguous(), pts.t().contiguous(), right=True).t().clamp_max(P - 1)
    ident = torch.arange(P, device=w.device).unsqueeze(1).expand(P, B)
    return torch.where(resample.unsqueeze(0), anc, ident).to(torch.int32).contiguous()


def weighted_quantiles(values: torch.Tensor, weights: Optional[torch.Tensor], quantiles: Sequence[float]) -> torch.Tensor:
    """Quantiles across the leading axis of `values` [P,...] under `weights` [P,...] >= 0 (broadcastable; None: equal),
    by the inverted empirical distribution: the smallest value whose cumulative normalised weight reaches q.  Returns
    [len(quantiles),...] in the dtype of `values`; float64 inside."""
    v, order = values.sort(0)
    w = torch.ones_like(values, dtype=torch.float64) if weights is None else \
        weights.double().expand_as(values).gather(0, order)
    cum = torch.cumsum(w, 0)
    cum = cum / cum[-1:]
    out = []
    for q in quantiles:
        # (cum <= 0: the leading values of weight zero carry no mass, at q = 0 either)
        idx = ((cum < q) | (cum <= 0)).sum(0, keepdim=True).clamp_max(values.shape[0] - 1)
        out.append(v.gather(0, idx)[0])
    return torch.stack(out)


def _sigma(obs_sigma, B, dev, what):
    s = torch.as_tensor(obs_sigma, dtype=torch.float64, device=dev)
    if s.dim() == 0:
        s = s.expand(B)
    if tuple(s.shape) != (B,):
        raise ValueError(f"{what}: obs_sigma must be a scalar or [{B}], got {tuple(s.shape)}")
    if not bool((torch.isfinite(s) & (s > 0)).all()):
        raise ValueError(f"{what}: obs_sigma must be finite and > 0")
    return s


def _randn(shape, generator, dev):
    gdev = generator.device if generator is not None else torch.device('cpu')
    return torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32).to(dev)


def particle_filter(model, x_dict: dict, parameters, target, n_particles: int, window: int = 1, *, obs_sigma,
                    prcp_sigma: float = 0.0, temp_sigma: float = 0.0, state_sigma: float = 0.0,
                    ess_threshold: float = 0.5, transform: str = 'none', eps=None, weights=None,
                    generator: Optional[torch.Generator] = None, return_series: bool = False) -> dict:
    """Sequential importance resampling of the storages, per basin, over consecutive windows of `window` days; one launch
    per window.

    Initial particles: the module's start state times exp(state_sigma z), z ~ N(0,1) per (particle, storage, basin,
    member).  Per (particle, day, basin): prcp_mul = exp(prcp_sigma z - prcp_sigma^2 / 2) (mean one), temp_add =
    temp_sigma z; a sigma of 0 passes no perturbation at all.  After each window, in float64 per basin (`update_log_weights`):
    log w -= 0.5 sse / obs_sigma^2 with sse the window's weighted squared error in the transformed space, normalised by a
    log-sum-exp; ESS = 1 / sum w^2; where ESS < ess_threshold * P the basin is resampled by `systematic_resample` with one
    uniform per basin and window, its weights reset to 1/P, and the ancestors go to the next launch as an index (basins not
    resampled keep the identity).  A basin whose weights are all non-finite keeps uniform weights and is reported.

    target, weights, transform, eps   as `population_stats`; obs_sigma a scalar or [B], > 0, in the transformed space.
    generator    every draw comes from it, in a fixed order: two runs with equally seeded generators agree bit for bit.
    Returns {'mean': [T_out,B] float64 the filtered mean flow, each day weighted with the weights in force after its
    window's update; 'ess': [n_windows,B] float64 (before resampling); 'resampled', 'degenerate': [n_windows,B] bool;
    'log_likelihood': [B] float64, the sum of the windows' log-sum-exp increments (without the Gaussian constant; nothing
    from degenerate windows); 'state': the final `EnsembleState`, resampling applied, with its 'weights' [P,B] float64;
    'windows': [n_windows,2] int64 descriptor days; 'outputs'; with return_series 'series' [P,T_out,B] float32 (particle
    slots, not lineages)}.

    Refused before the model runs: what `ensemble_step` refuses; window < 1, n_particles < 1, obs_sigma <= 0 or not
    finite, negative sigmas, ess_threshold outside [0, 1] (ValueError)."""
    what = "particle_filter"
    _check_counts(n_particles, what)
    if n_particles is None:
        raise ValueError(f"{what}: n_particles must be an integer >= 1, got None")
    if isinstance(window, bool) or not isinstance(window, int) or window < 1:
        raise ValueError(f"{what}: window must be an integer >= 1 (days per launch), got {window!r}")
    for name, v in (('prcp_sigma', prcp_sigma), ('temp_sigma', temp_sigma), ('state_sigma', state_sigma)):
        if not (float(v) >= 0.0 and math.isfinite(float(v))):
            raise ValueError(f"{what}: {name} must be finite and >= 0, got {v!r}")
    if not 0.0 <= float(ess_threshold) <= 1.0:
        raise ValueError(f"{what}: ess_threshold must lie in [0, 1], got {ess_threshold!r}")
    req = _refuse(model, x_dict, parameters, None, what)
    _check_rows(req, x_dict, target, weights, req.T_out, "days after the warm-up", what)
    dev = x_dict['x_phy'].device
    sigma = _sigma(obs_sigma, req.B, dev, what)
    ob = _observations(req, x_dict, target, weights, transform, eps, what)
    rec = ensemble_record(model, x_dict, parameters)
    cfg, t_first = rec.main.cfg, rec.t_first
    T, B, P = cfg.T, cfg.B, n_particles

    states = _start_states(rec).unsqueeze(0).expand(P, 5, B, cfg.M)
    if state_sigma > 0:
        states = states * torch.exp(float(state_sigma) * _randn((P, 5, B, cfg.M), generator, dev))
    states = states.contiguous()
    history, ancestor = None, None
    log_w = torch.full((P, B), -math.log(P), dtype=torch.float64, device=dev)
    mean = torch.zeros((req.T_out, B), dtype=torch.float64, device=dev)
    series = torch.empty((P, req.T_out, B), dtype=torch.float32, device=dev) if return_series else None
    ess_all, res_all, deg_all, log_lik = [], [], [], torch.zeros(B, dtype=torch.float64, device=dev)
    bounds = [(a, min(a + window, T)) for a in range(0, T, window)]
    gdev = generator.device if generator is not None else torch.device('cpu')
    for a, b in bounds:
        W = b - a
        pm = ta = None
        if prcp_sigma > 0:
            s = float(prcp_sigma)
            pm = torch.exp(s * _randn((P, W, B), generator, dev) - 0.5 * s * s).contiguous()
        if temp_sigma > 0:
            ta = (float(temp_sigma) * _randn((P, W, B), generator, dev)).contiguous()
        flow_out, wob, states, history = _launch(rec, ob, transform, P, a, b, states, history, ancestor, pm, ta, {},
                                                 (None, None), True)
        u = torch.rand((B,), generator=generator, device=gdev, dtype=torch.float64).to(dev)      # one per basin and window
        if b > t_first:
            log_w, lse, degenerate = update_log_weights(log_w, flow_out[0], sigma)
            log_lik = log_lik + lse
        else:                       # a window of warm-up days: nothing is observed, the weights stand
            degenerate = torch.zeros(B, dtype=torch.bool, device=dev)
        ess = effective_sample_size(log_w)
        r0, r1 = max(a, t_first) - t_first, max(b, t_first) - t_first
        if r1 > r0:
            mean[r0:r1] = (torch.exp(log_w).unsqueeze(1) * flow_out[4].double()).sum(0)
            if return_series:
                series[:, r0:r1] = flow_out[4]
        resample = ess < float(ess_threshold) * P
        ancestor = systematic_resample(log_w, u, resample) if bool(resample.any()) else None
        log_w = torch.where(resample.unsqueeze(0), torch.full_like(log_w, -math.log(P)), log_w)
        ess_all.append(ess)
        res_all.append(resample)
        deg_all.append(degenerate)
    if ancestor is not None:        # the last window's resampling, applied here: the state that is returned is consistent
        idx = ancestor.long()
        states = states.gather(0, idx.view(P, 1, B, 1).expand(P, 5, B, cfg.M))
        if history is not None:
            history = history.gather(0, idx.view(P, 1, B).expand(P, HIST, B))
    out = {'mean': mean, 'ess': torch.stack(ess_all), 'resampled': torch.stack(res_all), 'degenerate': torch.stack(deg_all),
           'log_likelihood': log_lik, 'state': EnsembleState(states, history, T, torch.exp(log_w)),
           'windows': torch.tensor(bounds, dtype=torch.int64), 'outputs': rec.outputs}
    if return_series:
        out['series'] = series
    return out


def ensemble_forecast(model, x_dict: dict, parameters, state: EnsembleState, particle_weights: Optional[torch.Tensor] = None,
                      quantiles: Sequence[float] = (0.05, 0.5, 0.95), prcp_mul: Optional[torch.Tensor] = None,
                      temp_add: Optional[torch.Tensor] = None) -> dict:
    """Runs the particles of `state` over the future record `x_dict` without observations: one launch with a zero target
    and zero weights (the kernel multiplies what it is given; zeros are safe), then weighted quantiles across particles
    per day in torch (`weighted_quantiles`; forecast horizons are short).

    state        an `EnsembleState` (from `particle_filter` or `ensemble_step`); its `day` is not read: the future record
                 starts at its own day 0, and its own warm-up state is replaced by the particles'.
    particle_weights   [P,B] >= 0 or None: state.weights, or equal weights without them.
    prcp_mul, temp_add   as `ensemble_step` takes them, for forcing uncertainty over the horizon.
    Returns {'series': [P,T_out,B] float32 streamflow per particle, 'quantiles': [Q,T_out,B] float32, 'mean': [T_out,B]
    float64 weighted mean, 'levels': the quantiles asked for, 'state': the `EnsembleState` at the horizon's end,
    'outputs'}.  Refusals: `ensemble_step`'s; quantiles outside [0, 1]; a wrong shape of particle_weights."""
    what = "ensemble_forecast"
    levels = tuple(float(q) for q in quantiles)
    if not levels or not all(0.0 <= q <= 1.0 for q in levels):
        raise ValueError(f"{what}: quantiles must lie in [0, 1], got {list(quantiles)}")
    req = _refuse(model, x_dict, parameters, None, what)
    if state is None:
        raise ValueError(f"{what}: state must be an EnsembleState, got NoneType")
    _check_state(x_dict, state, what)
    for name, t in (('prcp_mul', prcp_mul), ('temp_add', temp_add)):
        _check_noise(x_dict, name, t, what)
    P = int(state.states.shape[0])
    pw = state.weights if particle_weights is None else particle_weights
    if pw is not None and (not torch.is_tensor(pw) or tuple(pw.shape) != (P, req.B)):
        raise ValueError(f"{what}: particle_weights must be [{P},{req.B}], got "
                         f"{tuple(pw.shape) if torch.is_tensor(pw) else type(pw).__name__}")
    dev = x_dict['x_phy'].device
    zeros = torch.zeros((req.T_out, req.B), dtype=torch.float32, device=dev)
    ob = {'target': zeros, 'w': zeros, 'shift': torch.zeros(req.B, dtype=torch.float32, device=dev), 'eps': None}
    rec = ensemble_record(model, x_dict, parameters)
    flow_out, _, state_out, hist_out = _launch(rec, ob, 'none', P, 0, rec.main.cfg.T, state.states.contiguous(),
                                               None if state.history is None else state.history.contiguous(), None,
                                               prcp_mul, temp_add, {}, (None, None), True)
    series = flow_out[4]
    w = torch.full((P, req.B), 1.0 / P, dtype=torch.float64, device=dev) if pw is None else pw.to(dev).double()
    w = w / w.sum(0, keepdim=True)
    wq = weighted_quantiles(series, w.unsqueeze(1), levels)
    return {'series': series, 'quantiles': wq, 'mean': (w.unsqueeze(1) * series.double()).sum(0), 'levels': levels,
            'state': EnsembleState(state_out, hist_out, rec.main.cfg.T, None if pw is None else w), 'outputs': rec.outputs}
