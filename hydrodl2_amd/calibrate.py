"""Per-basin normal equations and Levenberg-Marquardt calibration of the static parameters.

`parameter_jacobian` / `adj_parameter_jacobian` return the per-basin Jacobian J [T_out,B,C] as a permuted copy of the
tangent series.  A Gauss-Newton or Levenberg-Marquardt step never wants J itself: it wants J^T W J [B,C,C], J^T W r
[B,C] and the cost per basin.  `normal_equations` forms them straight from the direction-major series the tangent
kernels write ([C,T_out,B], the basin as the unit-stride axis) with one hbvx_gram call (include/hbvx.h) -- the
permuted Jacobian is never built; `lm_step` solves the damped systems; `calibrate` is the per-basin LM loop on top.

Basins are independent in Hbv, Hbv_1_1p, Hbv_2 and HbvAdj, so one compact one-hot direction per column serves every
basin's own Jacobian.  Hbv_2_hourly and Hbv_2_mts route to gages, which couple the units: refused.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch

from . import _abi, adj_jvp, ops, sensitivity
from ._lib import get_library
from .core.hbv_module import HbvModule
from .sensitivity import direction_chunks, jacobian_columns, one_hot_directions


class _Request(NamedTuple):
    adj: bool               # HbvAdj (adj_jvp internals) or Hbv / Hbv_1_1p / Hbv_2 (sensitivity internals)
    key: str
    tname: str              # 'parameters' or 'p_sta'
    cols: list
    T_out: int
    B: int
    width: int              # columns of the tensor the static row lives in


def _static_tensor(req_or_two, parameters):
    return parameters[1] if req_or_two else parameters


_NO_TARGET = object()     # predictive_variance (uncertainty.py) fits nothing: the same refusals without a target


def _check_request(model, x_dict, parameters, target, names, key, weights, max_directions,
                   what: str = "normal_equations") -> _Request:
    """Everything that can be refused without running the model; what the call works on.  `what` names the caller in
    the messages; target = _NO_TARGET skips the checks of target and weights."""
    adj = getattr(model, '_model_id', None) == _abi.MODEL_HBVADJ
    explicit = isinstance(model, HbvModule) and model._model_id in sensitivity._TANGENT_MODELS
    if not (adj or explicit):
        raise NotImplementedError(f"{what} is not implemented for {type(model).__name__}: Hbv, Hbv_1_1p, Hbv_2 "
                                  "and HbvAdj only (the hourly and multi-timescale models route to gages, which couple "
                                  "the units: their Jacobian is not one block per basin)")
    if model.graph:
        raise ValueError(f"{type(model).__name__}(graph=True) does not support forward-mode AD (batched directions); "
                         "use graph=False")
    if getattr(model, 'initialize', False):
        raise ValueError(f"{what}: the module is in initialize mode (it returns states, no flux dictionary)")
    if key is None:
        key = 'flow_sim' if adj else 'streamflow'
    if key == 'BFI':
        raise ValueError(f"{what}: 'BFI' is one number per basin, not a series")
    if adj:
        if key != 'flow_sim':
            raise KeyError(f"HbvAdj has no flux key {key!r}")
    else:
        sensitivity._check_keys(model, [key])
    if max_directions < 1:
        raise ValueError("max_directions must be >= 1")
    tname, cols = jacobian_columns(model, names)
    if not cols:
        raise ValueError(f"{what} needs at least one column")
    two = tname == 'p_sta'
    ptensor = _static_tensor(two, parameters)
    x = x_dict['x_phy']
    B, width = int(ptensor.shape[-2]), int(ptensor.shape[-1])
    if int(x.shape[1]) != B:
        raise ValueError(f"x_phy has {int(x.shape[1])} basins, the parameters {B}")
    # Hbv_2 has no warm-up pass of its own: every day of the record is an output day
    T_out = int(x.shape[0]) - (0 if two else int(model.warm_up))
    if T_out < 1:
        raise ValueError(f"{what}: no day is left after the warm-up")
    if target is _NO_TARGET:
        return _Request(adj, key, tname, list(cols), T_out, B, width)
    if not torch.is_tensor(target) or tuple(target.shape) not in ((T_out, B), (T_out, B, 1)):
        raise ValueError(f"target must be [{T_out},{B}] or [{T_out},{B},1] (the days after the warm-up), got "
                         f"{tuple(target.shape) if torch.is_tensor(target) else type(target).__name__}")
    if bool(torch.isinf(target).any()):
        raise ValueError("target holds infinities (a missing observation is a NaN)")
    if weights is not None:
        if not torch.is_tensor(weights) or tuple(weights.shape) != (T_out, B):
            raise ValueError(f"weights must be [{T_out},{B}]")
        if not bool(torch.isfinite(weights).all()):
            raise ValueError("weights must be finite")
        if bool((weights < 0).any()):
            raise ValueError("weights must not be negative")
    return _Request(adj, key, tname, list(cols), T_out, B, width)


def _residual(req: _Request, sim: torch.Tensor, target, weights):
    """(w, r) as the kernel sees them: float32 [T_out,B] on sim's device, a NaN target made a zero weight AND a zero
    residual (the kernel multiplies what it is given: 0 * NaN would be NaN).  w is None when nothing weighs."""
    if not bool(torch.isfinite(sim).all()):
        raise ValueError(f"the simulated {req.key} holds non-finite values")
    tgt = target.to(device=sim.device, dtype=torch.float32).reshape(req.T_out, req.B)
    miss = torch.isnan(tgt)
    r = torch.where(miss, torch.zeros_like(sim), sim - tgt)
    if weights is None and not bool(miss.any()):
        return None, r
    w = torch.ones_like(sim) if weights is None else weights.to(device=sim.device, dtype=torch.float32)
    return torch.where(miss, torch.zeros_like(w), w).contiguous(), r


def _primal_and_series(model, req: _Request, x_dict, parameters, max_directions: int):
    """ONE run of the module, then its one-hot directions through the tangent kernels `max_directions` at a time into a
    single direction-major buffer.  Returns (outputs, sim [T_out,B], series [C,T_out,B] float32)."""
    with ops.record_paths() as records:
        outputs = model(x_dict, parameters)
    sim = outputs[req.key].detach()[..., 0]
    if tuple(sim.shape) != (req.T_out, req.B):
        raise RuntimeError(f"{type(model).__name__} returned {req.key} of shape {tuple(sim.shape)}, expected "
                           f"({req.T_out}, {req.B})")
    dev = sim.device
    C = len(req.cols)
    series = torch.empty((C, req.T_out, req.B), dtype=torch.float32, device=dev)
    for c0, c1 in direction_chunks(C, max_directions):
        tangents = {req.tname: one_hot_directions(req.cols[c0:c1], req.B, req.width, dev)}
        if req.adj:
            tan = adj_jvp._directional(model, records, tangents, None)
        else:
            tan = sensitivity._directional(model, records, tangents, [req.key])[req.key]
        series[c0:c1].copy_(tan[..., 0])
    return outputs, sim, series


def normal_equations(model, x_dict: dict, parameters, target, names: Optional[Sequence[str]] = None,
                     key: Optional[str] = None, weights=None, max_directions: int = 64) -> dict:
    """Per-basin normal equations of a least-squares fit of one output series to `target`.

    With r = outputs[key][..., 0] - target and J as `parameter_jacobian` (HbvAdj: `adj_parameter_jacobian`) defines it,
        {'JtJ': J^T W J [B,C,C], 'Jtr': J^T W r [B,C], 'cost': sum_t w r^2 [B], 'n_obs': [B] int64, the number of
         (t, b) with a positive weight once NaN targets are masked, 'columns': [C indices],
         'outputs': the primal flux dictionary}.
    model     Hbv, Hbv_1_1p, Hbv_2 (key default 'streamflow', any series key) or HbvAdj (key 'flow_sim').
    names     as in `jacobian_columns`: static physical parameters (their nmul columns each) and routing parameters;
              default all of them.  The columns are those of parameters[T-1] (Hbv_2: p_sta).
    target    [T_out,B] or [T_out,B,1], T_out = the days after the warm-up.  A NaN is a missing observation: its weight
              and its residual are set to 0 before the kernel sees them.
    weights   [T_out,B] >= 0 or None (ones).
    The module runs ONCE (its dy_drop masks are drawn once, for the primal and all columns).  The one-hot directions go
    through the tangent kernels `max_directions` at a time and are written one after the other into a single
    [C,T_out,B] float32 buffer, which one hbvx_gram call reduces: that buffer is the size of J (B * T_out * C * 4 bytes,
    3.8 GB at 671 basins x 7300 days x 194 columns) -- what is saved is the permuted copy and the user's own
    contraction, not the series.  Results are bit-reproducible and do not depend on max_directions.

    Refused before the model runs: Hbv_2_hourly, Hbv_2_mts and anything else (NotImplementedError); graph=True,
    initialize mode, 'BFI', unknown or dynamic names, a wrong target / weights shape, infinite targets, negative or
    non-finite weights (ValueError); an unknown key (KeyError); a library without hbvx_gram (HbvxError).  A non-finite
    simulated value raises ValueError after it."""
    req = _check_request(model, x_dict, parameters, target, names, key, weights, max_directions)
    get_library().require("hbvx_gram")
    outputs, sim, series = _primal_and_series(model, req, x_dict, parameters, max_directions)
    w, r = _residual(req, sim, target, weights)
    n_obs = (torch.full((req.B,), req.T_out, dtype=torch.int64, device=sim.device) if w is None
             else (w > 0).sum(0, dtype=torch.int64))
    JtJ, Jtr, cost = ops.gram(series, w, r.contiguous())
    return {'JtJ': JtJ, 'Jtr': Jtr, 'cost': cost, 'n_obs': n_obs, 'columns': list(req.cols), 'outputs': outputs}


def lm_step(neq: dict, damping, eps: float = 1e-12):
    """The damped Gauss-Newton step of every basin: delta [B,C] (float32) solving
        (JtJ + damping[b] * diag(JtJ) + eps * I) delta = -Jtr
    in float64 by Cholesky factorisation.  damping: a number or [B].  Returns (delta, info) with info['failed'] [B]
    bool: basins whose matrix is not positive definite (or not finite) -- their delta is 0 -- and info['info'] the
    factorisation's own status."""
    JtJ, Jtr = neq['JtJ'], neq['Jtr']
    B, C = Jtr.shape
    A = JtJ.to(torch.float64)
    g = Jtr.to(torch.float64)
    lam = torch.as_tensor(damping, dtype=torch.float64, device=A.device)
    if lam.dim() == 0:
        lam = lam.expand(B)
    if tuple(lam.shape) != (B,):
        raise ValueError(f"damping must be a number or [{B}], got {tuple(lam.shape)}")
    if bool((lam < 0).any()):
        raise ValueError("damping must not be negative")
    diag = torch.diagonal(A, dim1=1, dim2=2)
    A = A + torch.diag_embed(lam[:, None] * diag + eps)
    finite = torch.isfinite(A).all(-1).all(-1) & torch.isfinite(g).all(-1)
    eye = torch.eye(C, dtype=torch.float64, device=A.device)
    A = torch.where(finite[:, None, None], A, eye)
    L, status = torch.linalg.cholesky_ex(A)
    failed = (status != 0) | ~finite
    L = torch.where(failed[:, None, None], eye, L)
    delta = torch.cholesky_solve(-g.unsqueeze(-1), L).squeeze(-1)
    delta = torch.where(failed[:, None] | ~torch.isfinite(delta), torch.zeros_like(delta), delta)
    return delta.to(torch.float32), {'failed': failed, 'info': status}


def _series_cost(req: _Request, outputs: dict, target, weights) -> torch.Tensor:
    """sum_t w (sim - target)^2 per basin in float64, missing observations skipped; inf where the run is not finite."""
    sim = outputs[req.key].detach()[..., 0].to(torch.float64)
    tgt = target.to(device=sim.device, dtype=torch.float64).reshape(req.T_out, req.B)
    miss = torch.isnan(tgt)
    d = torch.where(miss, torch.zeros_like(sim), sim - tgt)
    if weights is not None:
        d = d * torch.sqrt(weights.to(device=sim.device, dtype=torch.float64))
    cost = (d * d).sum(0)
    return torch.where(torch.isfinite(cost), cost, torch.full_like(cost, float('inf')))


def calibrate(model, x_dict: dict, parameters, target, names: Optional[Sequence[str]] = None, n_iter: int = 10,
              damping: float = 1e-2, up: float = 10.0, down: float = 0.1, weights=None, max_directions: int = 64,
              key: Optional[str] = None):
    """Per-basin Levenberg-Marquardt on the static row `parameter_jacobian` differentiates: parameters[T-1, b, columns]
    (Hbv_2: p_sta[b, columns]), in the space the module takes them in (raw for Hbv / Hbv_1_1p / HbvAdj).

    Every iteration makes one `normal_equations` call at the current parameters and one trial forward under no_grad at
    parameters + delta.  A basin accepts the step only if its cost fell; its damping is then multiplied by `down`,
    otherwise it keeps its parameters and its damping is multiplied by `up`.  Current and trial cost are computed by
    the same float64 sum over the module's own output, so "fell" compares like with like.

    Returns (calibrated, history): `calibrated` shaped like `parameters` (a new tensor; Hbv_2: (p_dyn, new p_sta));
    history = {'cost': [n_iter+1,B] float64 (the cost the basin holds before iteration i; the last row is the final one),
    'damping': [n_iter,B] (used in iteration i), 'accepted': [n_iter,B] bool, 'failed': [n_iter,B] bool (`lm_step`),
    'columns'}.  The inputs are not modified.  dy_drop > 0 makes the cost stochastic: ValueError."""
    if float(getattr(model, 'dy_drop', 0.0)) > 0:
        raise ValueError("calibrate: dy_drop > 0 draws new masks in every run, the cost is stochastic; set dy_drop = 0")
    if n_iter < 1:
        raise ValueError("n_iter must be >= 1")
    if not (damping >= 0 and up > 1 and 0 < down <= 1):
        raise ValueError("calibrate wants damping >= 0, up > 1 and 0 < down <= 1")
    req = _check_request(model, x_dict, parameters, target, names, key, weights, max_directions)
    two = req.tname == 'p_sta'
    cur = _static_tensor(two, parameters).detach().clone()
    row = cur if two else cur[-1]           # [B,width] view of the row that moves
    cols = torch.as_tensor(req.cols, dtype=torch.long, device=cur.device)

    def pack(t):
        return (parameters[0], t) if two else t

    lam = torch.full((req.B,), float(damping), dtype=torch.float64, device=cur.device)
    hist = {'cost': [], 'damping': [], 'accepted': [], 'failed': [], 'columns': list(req.cols)}
    cost = None
    for _ in range(n_iter):
        neq = normal_equations(model, x_dict, pack(cur), target, names, req.key, weights, max_directions)
        if cost is None:
            cost = _series_cost(req, neq['outputs'], target, weights)
        dev = neq['JtJ'].device
        delta, info = lm_step(neq, lam.to(dev))
        trial = cur.clone()
        trow = trial if two else trial[-1]
        trow[:, cols] = row[:, cols] + delta.to(cur.device)
        with torch.no_grad():
            trial_cost = _series_cost(req, model(x_dict, pack(trial)), target, weights)
        accept = (trial_cost < cost) & ~info['failed']
        hist['cost'].append(cost.cpu())
        hist['damping'].append(lam.cpu().clone())
        hist['accepted'].append(accept.cpu())
        hist['failed'].append(info['failed'].cpu())
        acc = accept.to(cur.device)
        row[acc] = trow[acc]
        cost = torch.where(accept, trial_cost, cost)
        lam = torch.where(acc, lam * down, lam * up)
    hist['cost'].append(cost.cpu())
    for k in ('cost', 'damping', 'accepted', 'failed'):
        hist[k] = torch.stack(hist[k])
    return pack(cur), hist
