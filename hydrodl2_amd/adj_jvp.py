"""Forward-mode AD of `HbvAdj` over many directions at once: `adj_jvp_batch` (`HbvAdj.jvp_batch`) and the per-basin
`adj_parameter_jacobian` (`HbvAdj.parameter_jacobian`).

The implicit scheme is the model whose purpose is sensitivities: a Gauss-Newton or Levenberg-Marquardt calibration of
it wants its per-basin Jacobian, which reverse mode gives one row per backward call and forward mode one column per
direction, for all days at once.  The derivative is the implicit-function one at the SOLVED state of every day -- the
transpose of the module's backward -- so a tangent never runs Newton: the module's forward runs ONCE, keeping the
trajectory of solved states, and hbvx_adj_tangent_batch (include/hbvx.h) then walks it with one evaluation of the
analytic Jacobian per lane-day and one forward substitution per direction.  With the reference Newton policy (gtol
1e-3) the VALUE is an inexact iterate and the derivative the exact one at it: finite differences of the module are not
a reference for this (they differ by about 3e-3 of the tangent), the float64 autograd oracle's JVP is.

The dual-tensor path (`torch.autograd.forward_ad` through `HbvAdj.forward`) and the generic `hydrodl2_amd.jvp_batch`
/ `parameter_jacobian` keep refusing the model: this is an explicit entry point, as `hourly_jvp_batch` is.
"""
from __future__ import annotations

import contextlib
from typing import Optional, Sequence

import torch

from . import _abi, ops
from .sensitivity import _leading, direction_chunks, jacobian_columns, one_hot_directions

TANGENT_NAMES = ('parameters', 'x_phy')


def _check_model(model) -> None:
    if getattr(model, '_model_id', None) != _abi.MODEL_HBVADJ:
        raise NotImplementedError(f"adj_jvp_batch is for HbvAdj, not {type(model).__name__}: Hbv, Hbv_1_1p and Hbv_2 go "
                                  "through hydrodl2_amd.jvp_batch, Hbv_2_hourly through hydrodl2_amd.hourly_jvp_batch")
    if model.graph:
        raise ValueError("HbvAdj(graph=True) does not support forward-mode AD (batched directions); use graph=False")


def _check_request(model, x_dict: dict, parameters, tangents: dict, max_directions) -> int:
    """Refuse what the path cannot differentiate, before the primal runs; the number of directions."""
    _check_model(model)
    unknown = sorted(set(tangents) - set(TANGENT_NAMES))
    if unknown:
        raise ValueError(f"unknown tangent names {unknown}; HbvAdj takes {sorted(TANGENT_NAMES)}")
    if not tangents:
        raise ValueError("jvp_batch needs at least one tangent")
    D = _leading(tangents)
    if max_directions is not None and max_directions < 1:
        raise ValueError("max_directions must be >= 1")
    x, p = x_dict['x_phy'], parameters
    t = tangents.get('x_phy')
    if t is not None and tuple(t.shape[1:]) != tuple(x.shape):
        raise ValueError(f"tangent of x_phy must be [D, {', '.join(map(str, x.shape))}], got {tuple(t.shape)}")
    t = tangents.get('parameters')
    if t is not None and tuple(t.shape[1:]) not in (tuple(p.shape), tuple(p.shape[1:])):
        raise ValueError(f"tangent of parameters must be [D, {', '.join(map(str, p.shape))}] (full) or "
                         f"[D, {', '.join(map(str, p.shape[1:]))}] (compact: zero except row T-1), got {tuple(t.shape)}")
    return D


def _directional(model, records, tangents: dict, max_directions: Optional[int]) -> torch.Tensor:
    """[D,T_out,B,1]: the tangents of flow_sim of the recorded primal run.  Touches nothing of the module: any number
    of direction sets may follow one primal run."""
    main = records[-1]
    x = main.x
    D = _leading(tangents)

    def f32(name):
        t = tangents.get(name)
        return None if t is None else t.to(device=x.device, dtype=torch.float32)

    x_t, p_t = f32('x_phy'), f32('parameters')

    def piece(t, c0, c1):
        return None if t is None else t[c0:c1]

    out = []
    guard = torch.cuda.device(x.device) if x.is_cuda else contextlib.nullcontext()
    with guard:
        for c0, c1 in direction_chunks(D, max_directions or D):
            s_t = None
            for rec in records:         # the warm-up (no series), then the main pass on its state tangent
                # (a compact tangent reaches the warm-up record too: fine because HbvAdj's warm-up configuration has no
                # dynamic parameters -- hbv_tangent_batch refuses compact dynamic rows on a call that ends before row T-1)
                last = rec is main
                res = ops.hbv_tangent_batch(rec, c1 - c0, piece(x_t, c0, c1), None, s_t, [piece(p_t, c0, c1)],
                                            flux_mask=1 if last else 0,
                                            n_routed=1 if (last and rec.cfg.route is not None) else 0)
                s_t = res.state_out
            out.append((res.routed if res.routed is not None else res.flux)[:, 0].unsqueeze(-1))
    return out[0] if len(out) == 1 else torch.cat(out, dim=0)


def adj_jvp_batch(model, x_dict: dict, parameters, tangents: dict, max_directions: Optional[int] = None):
    """Implicit-function forward-mode derivatives of `HbvAdj(x_dict, parameters)` along D directions on one primal run.

    tangents  input name -> tensor with a leading direction axis D; missing names are zero tangents.
              'parameters'  full [D,T,B,ny], or compact [D,B,ny], DEFINED (as in `hydrodl2_amd.jvp_batch`) as the full
                            tensor that is zero everywhere except row T-1: columns of dynamic parameters then carry
                            their last-row tangent only, and with warm_up > 0 the warm-up pass, which reads row
                            warm_up - 1, sees a zero parameter tangent.
              'x_phy'       [D,T,B,nvar]: all three forcings (precipitation through snowfall / rainfall, temperature
                            through melt and refreezing, zero slope of the T < TT threshold; PET through evaporation).
    max_directions   at most so many directions per tangent launch (bounds the scratch); the primal is never split.

    Returns (outputs, {'flow_sim': [D,T_out,B,1]}): `outputs` is the plain primal dictionary from ONE run of the
    module's forward (the dy_drop masks are drawn once, for the primal and all directions; the generator advances as in
    one plain call).  The warm-up pass is differentiated through, as the module's backward does: its state tangent
    enters the main pass.  A direction's result does not depend on the others it was batched with.

    Refused with ValueError: graph=True, unknown names, no tangents, mismatched leading axes, wrong shapes,
    max_directions < 1; with NotImplementedError: any other model.  A library without hbvx_adj_tangent_batch raises
    the error naming it after the primal ran."""
    _check_request(model, x_dict, parameters, tangents, max_directions)
    with ops.record_paths() as records:
        outputs = model(x_dict, parameters)
    return outputs, {'flow_sim': _directional(model, records, tangents, max_directions)}


def adj_parameter_jacobian(model, x_dict: dict, parameters, names: Optional[Sequence[str]] = None,
                           max_directions: int = 64) -> dict:
    """Per-basin Jacobian of flow_sim with respect to the static parameters.

    Returns {'flow_sim': J [T_out, B, C], 'columns': [C column indices]} with
    J[t, b, c] = d flow_sim[t, b] / d parameters[T-1, b, columns[c]].  `names`: static physical parameters (their nmul
    columns each, in table order) and 'rout_a' / 'rout_b'; default all of them.  A dynamic parameter's Jacobian is not
    one row per basin: naming one raises ValueError.  Compact one-hot directions, `max_directions` at a time, all on
    ONE run of the module's forward."""
    _check_model(model)
    if max_directions < 1:
        raise ValueError("max_directions must be >= 1")
    _, cols = jacobian_columns(model, names)
    B, width = parameters.shape[-2], parameters.shape[-1]
    with ops.record_paths() as records:
        model(x_dict, parameters)
    dev = records[-1].x.device
    tan = _directional(model, records, {'parameters': one_hot_directions(cols, B, width, dev)}, max_directions)
    return {'flow_sim': tan[..., 0].permute(1, 2, 0).contiguous(), 'columns': list(cols)}
