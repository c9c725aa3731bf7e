"""Forward-mode AD of `Hbv_2_hourly` over many directions at once: `hourly_jvp_batch` (`Hbv_2_hourly.jvp_batch`).

The hourly model is the one model whose output is gage streamflow, and gages couple the units: there is no per-basin
Jacobian, and the dual-tensor path (`torch.autograd.forward_ad` through `forward`) and the generic
`hydrodl2_amd.jvp_batch` keep refusing it.  This explicit entry point runs the module's forward ONCE and then, on
what that run worked on, the tangent-linear kernels of the sub-daily recurrence (hbvx_hourly_tangent_batch) and of the
gage routing (hbvx_gage_route_tangent_batch; the optional 72-tap per-unit routing is the same call with the identity
topology), many directions per launch.
"""
from __future__ import annotations

import contextlib
from typing import Optional, Sequence

import torch

from . import _abi, ops
from .sensitivity import _leading, direction_chunks

KEYS = ('Qs', 'streamflow')
TANGENT_NAMES = ('p_dyn', 'p_sta', 'p_distr', 'x_phy', 'muwts', 'states')
_FIXED_INPUTS = ('ac_all', 'elev_all', 'outlet_topo', 'areas')


def _check_request(model, tangents: dict, keys, max_directions) -> list:
    """Refuse what the path cannot differentiate, before the primal runs; the wanted keys without repeats."""
    if model._model_id != _abi.MODEL_HOURLY:
        raise NotImplementedError(f"hourly_jvp_batch is for Hbv_2_hourly, not {type(model).__name__}: "
                                  "Hbv, Hbv_1_1p and Hbv_2 go through hydrodl2_amd.jvp_batch")
    if model.graph:
        raise ValueError("Hbv_2_hourly(graph=True) does not support forward-mode AD (batched directions); "
                         "use graph=False")
    if model.initialize:
        raise ValueError("forward-mode AD: the module is in initialize mode (it returns states, no flux dictionary)")
    fixed = [n for n in _FIXED_INPUTS if n in tangents]
    if fixed:
        raise ValueError(f"forward-mode AD: tangents of {' / '.join(fixed)} are not supported")
    unknown = sorted(set(tangents) - set(TANGENT_NAMES))
    if unknown:
        raise ValueError(f"unknown tangent names {unknown}; Hbv_2_hourly takes {sorted(TANGENT_NAMES)}")
    if not tangents:
        raise ValueError("jvp_batch needs at least one tangent")
    _leading(tangents)
    if max_directions is not None and max_directions < 1:
        raise ValueError("max_directions must be >= 1")
    keys = list(dict.fromkeys(KEYS if keys is None else keys))
    for k in keys:
        if k not in KEYS:
            raise KeyError(f"Hbv_2_hourly has no output key {k!r}")
    return keys


def _shaped(name: str, t: Optional[torch.Tensor], shape: tuple) -> Optional[torch.Tensor]:
    if t is not None and tuple(t.shape[1:]) != tuple(shape):
        raise ValueError(f"tangent of {name} must be [D, {', '.join(map(str, shape))}] (the full form), "
                         f"got {tuple(t.shape)}")
    return t


def hourly_jvp_batch(model, x_dict: dict, parameters, tangents: dict, keys: Optional[Sequence[str]] = None,
                     max_directions: Optional[int] = None):
    """Forward-mode derivatives of `Hbv_2_hourly(x_dict, parameters)` along D directions on one primal run.

    tangents  input name -> tensor with a leading direction axis D.  Names: 'p_dyn' [D,T,B,.], 'p_sta' [D,B,.],
              'p_distr' [D,n_pairs,3], 'x_phy' [D,T,B,.], 'muwts' (shaped like x_dict['muwts']) and 'states'
              [D,5,B,nmul] (the storages the run starts from, used when the module starts from cached states).
              Only the full form is taken; missing names are zero tangents.
    keys      'Qs' and / or 'streamflow' (default: both).  Only flux row 0 of the recurrence is computed.
    max_directions   at most so many directions per tangent launch (bounds the scratch); the primal is never split.

    Returns (outputs, tangents_out): `outputs` is the plain primal dictionary from ONE run of the module's forward
    (drop masks drawn once; the state cache and the runoff history move as in one plain call); `tangents_out[key][d]`
    is the derivative along direction d -- [D,T,B,1] for 'Qs', [D,T,G,1] for 'streamflow' -- with the module's
    scaling by dt and its pred_cutoff slice applied.  With cache_states the routed history is detached, as in the
    reference: the streamflow tangent is the last row and carries the 'p_distr' term only.

    Refused with ValueError: graph=True, initialize mode, tangents on ac_all / elev_all / outlet_topo / areas, unknown
    names, mismatched leading axes.  A library without the tangent exports raises the error naming the missing one."""
    keys = _check_request(model, tangents, keys, max_directions)
    D = _leading(tangents)
    with ops.record_paths() as records, ops.record_gage_routes() as routes:
        outputs = model(x_dict, parameters)
    main = records[-1]
    cfg, x = main.cfg, main.x
    T, B, M = cfg.T, cfg.B, cfg.M

    def f32(name):
        t = tangents.get(name)
        return None if t is None else t.to(device=x.device, dtype=torch.float32)

    x_t = _shaped('x_phy', f32('x_phy'), x.shape)
    p_dyn_t = _shaped('p_dyn', f32('p_dyn'), main.ptensors[0].shape)
    p_sta_t = _shaped('p_sta', f32('p_sta'), main.ptensors[1].shape)
    distr = routes[-1]                              # the gage routing is the run's last routing call
    p_distr_t = _shaped('p_distr', f32('p_distr'), distr.dp.shape)
    s_t = _shaped('states', f32('states'), (5, B, M))
    mu_t = f32('muwts')
    if mu_t is not None and main.muwts is not None:
        _shaped('muwts', mu_t, x_dict['muwts'].shape)
        mu_t = mu_t.expand(D, *main.muwts.shape) if mu_t.dim() == 4 else mu_t.unsqueeze(1).expand(D, *main.muwts.shape)
    unit = routes[0] if model.routing else None     # the optional per-unit routing: the identity topology
    n_sta = len(model.parameter_bounds) - len(model.dynamic_params)
    want_qs = 'Qs' in keys or not model.cache_states

    def piece(t, c0, c1):
        return None if t is None else t[c0:c1]

    out = {k: [] for k in keys}
    guard = torch.cuda.device(x.device) if x.is_cuda else contextlib.nullcontext()
    with guard:
        for c0, c1 in direction_chunks(D, max_directions or D):
            d = c1 - c0
            qs_t = None
            if want_qs:
                res = ops.hbv_tangent_batch(main, d, piece(x_t, c0, c1), piece(mu_t, c0, c1), piece(s_t, c0, c1),
                                            [piece(p_dyn_t, c0, c1), piece(p_sta_t, c0, c1)], flux_mask=1)
                qs_t = res.flux[:, 0]                                             # [d,T,B], rate per day
                if unit is not None:
                    dp_t = None
                    if p_sta_t is not None:
                        ab = p_sta_t[c0:c1, :, n_sta * M:n_sta * M + 2]
                        dp_t = torch.cat([ab, torch.zeros_like(ab[:, :, :1])], dim=2)
                    qs_t = ops.gage_route_tangent_batch(unit, d, qs_t, dp_t)
                qs_t = qs_t * model.dt                                             # hbv_2_hourly.py:741
            if 'Qs' in keys:
                v = qs_t.unsqueeze(-1)
                out['Qs'].append(v if model.warm_up_states else v[:, model.pred_cutoff:])
            if 'streamflow' in keys:
                v = ops.gage_route_tangent_batch(distr, d, None if model.cache_states else qs_t,
                                                 piece(p_distr_t, c0, c1)).unsqueeze(-1)
                out['streamflow'].append(v[:, -1:] if model.cache_states else v)
    return outputs, {k: (v[0] if len(v) == 1 else torch.cat(v, dim=0)) for k, v in out.items()}
