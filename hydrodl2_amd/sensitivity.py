"""Forward-mode AD over many directions at once: `jvp_batch` and the per-basin `parameter_jacobian`.

`torch.autograd.forward_ad` on `Hbv`, `Hbv_1_1p` and `Hbv_2` carries one direction per call, and each call recomputes
the primal day by day beside its one tangent.  A sensitivity series, the Jacobian of a Gauss-Newton / Levenberg-
Marquardt calibration or the columns of an assimilation step want tens to hundreds of directions on the same primal:
here they share one primal run and one launch of each tangent kernel (hbvx_forward_tangent_batch,
hbvx_route_tangent_batch, hbvx_bfi_tangent_batch in include/hbvx.h).

Directions that start upstream of the model -- on the inputs or weights of the parameter network -- come through
`SeqLSTM.jvp_batch` (hydrodl2_amd/lstm.py), whose `[D,T,B,ny]` output is a full-form 'parameters' tangent here
(examples/input_sensitivity.py).

The hourly model has an entry point of its own, `hydrodl2_amd.hourly_jvp_batch` / `Hbv_2_hourly.jvp_batch`
(hydrodl2_amd/hourly_jvp.py): its output is gage streamflow, gages couple the units, so `jvp_batch` and
`parameter_jacobian` here keep refusing it.  So has the implicit scheme, `hydrodl2_amd.adj_jvp_batch` /
`HbvAdj.jvp_batch` and `adj_parameter_jacobian` (hydrodl2_amd/adj_jvp.py): its tangent is the implicit-function
derivative at the solved states of a saved trajectory, a different kernel and call.

Out of scope: `torch.func.jvp` / `jacfwd` / vmap over `make_dual`, and the multi-timescale model.
"""
from __future__ import annotations

import contextlib
from typing import Optional, Sequence

import torch

from . import _abi, ops
from .core.hbv_module import HbvModule

_F = _abi
# flux key -> index of the routed runoff series / of the flux series (core.hbv_module.HbvModule._assemble)
ROUTED_KEYS = {'streamflow': 0, 'srflow': 1, 'ssflow': 2, 'gwflow': 3}
FLUX_KEYS = {'AET_hydro': _F.F_AET, 'SWE': _F.F_SWE, 'streamflow_no_rout': _F.F_QSIM, 'srflow_no_rout': _F.F_Q0,
             'ssflow_no_rout': _F.F_Q1, 'gwflow_no_rout': _F.F_Q2, 'recharge': _F.F_RECHARGE, 'excs': _F.F_EXCS,
             'evapfactor': _F.F_EVAPFACTOR, 'tosoil': _F.F_TOSOIL, 'percolation': _F.F_PERC,
             'capillary': _F.F_CAPILLARY}
_TANGENT_MODELS = (_abi.MODEL_HBV10, _abi.MODEL_HBV11P, _abi.MODEL_HBV20)


def _check_model(model) -> None:
    if not (isinstance(model, HbvModule) and model._model_id in _TANGENT_MODELS):
        raise NotImplementedError(f"forward-mode AD (batched directions) is not implemented for {type(model).__name__}: "
                                  "Hbv, Hbv_1_1p and Hbv_2 only")
    if model.graph:
        raise ValueError(f"{type(model).__name__}(graph=True) does not support forward-mode AD (batched directions); "
                         "use graph=False")


def _is_two_tensor(model) -> bool:
    return model._model_id == _abi.MODEL_HBV20


def series_plan(keys: Sequence[str], routed: bool, n_flux: int):
    """(flux_mask, n_routed, want_bfi): the flux series, the number of leading routed runoff series and whether the
    BFI tangent is needed to serve `keys`; `routed`: the model routes its runoff."""
    mask, n_routed, want_bfi = 0, 0, False
    for k in keys:
        if k in ROUTED_KEYS:
            if routed:
                n_routed = max(n_routed, ROUTED_KEYS[k] + 1)
            else:
                mask |= 1 << ROUTED_KEYS[k]
        elif k in FLUX_KEYS and FLUX_KEYS[k] < n_flux:
            mask |= 1 << FLUX_KEYS[k]
        elif k == 'BFI':
            want_bfi = True
            if routed:
                n_routed = 4
            else:
                mask |= (1 << _F.F_QSIM) | (1 << _F.F_Q2)
        elif k != 'PET_hydro':
            raise KeyError(f"unknown flux key {k!r}")
    mask |= (1 << n_routed) - 1
    return mask, n_routed, want_bfi


def _leading(tangents: dict) -> int:
    sizes = {int(t.shape[0]) for t in tangents.values()}
    if len(sizes) != 1:
        raise ValueError(f"tangents must share their leading direction axis, got sizes {sorted(sizes)}")
    return sizes.pop()


def jvp_batch(model, x_dict: dict, parameters, tangents: dict, keys: Optional[Sequence[str]] = None):
    """Forward-mode derivatives of `model(x_dict, parameters)` along D directions in one call.

    tangents  input name -> tensor with a leading direction axis D.  Names: 'parameters' (Hbv, Hbv_1_1p) or 'p_dyn' /
              'p_sta' (Hbv_2), 'x_phy', 'muwts' (shaped like x_dict['muwts']) and 'states' ([D,5,B,nmul]: the storages
              the run starts from, used when the module starts from cached states).  Missing names are zero.
              'parameters' (and 'p_dyn') come in two forms:
                full     [D,T,B,ny];
                compact  [D,B,ny], DEFINED as the full tensor that is zero everywhere except row T-1.  Columns of
                         dynamic parameters then carry their last-row tangent only, exactly as that full tensor would.
                         With warm_up > 0 and warm_up_states=True the warm-up pass reads row warm_up - 1, which the
                         compact form leaves at zero: the warm-up then contributes no parameter tangent.
    keys      the flux keys wanted (default: all of the model's).  Only the series they need are computed and stored.

    Returns (outputs, tangents_out): `outputs` is the plain primal dictionary, from ONE run of the module's normal
    forward (its dy_drop masks are drawn once, for the primal and all directions, and the generator advances as in
    one plain call); `tangents_out[key][d]` is what one torch.autograd.forward_ad call with direction d returns for
    `key`: [D,T,B,1] series, [D,B] for BFI.

    Refused like the one-direction path: graph=True and tangents on ac_all / elev_all (ValueError); HbvAdj,
    Hbv_2_hourly and Hbv_2_mts (NotImplementedError)."""
    keys = _check_request(model, tangents, keys)
    outputs, records = _primal(model, x_dict, parameters)
    return outputs, _directional(model, records, tangents, keys)


def _check_request(model, tangents: dict, keys) -> list:
    """Refuse what the path cannot differentiate; the wanted flux keys as a list without repeats."""
    _check_model(model)
    if 'ac_all' in tangents or 'elev_all' in tangents:
        raise ValueError("forward-mode AD: tangents of ac_all / elev_all are not supported")
    allowed = ({'p_dyn', 'p_sta'} if _is_two_tensor(model) else {'parameters'}) | {'x_phy', 'muwts', 'states'}
    if set(tangents) - allowed:
        raise ValueError(f"unknown tangent names {sorted(set(tangents) - allowed)}; {type(model).__name__} takes "
                         f"{sorted(allowed)}")
    if not tangents:
        raise ValueError("jvp_batch needs at least one tangent")
    _leading(tangents)
    return _check_keys(model, keys)


def _check_keys(model, keys) -> list:
    if model.initialize:
        raise ValueError("forward-mode AD: the module is in initialize mode (it returns states, no flux dictionary)")
    flux_keys = list(model.flux_names)
    keys = list(dict.fromkeys(flux_keys if keys is None else keys))
    for k in keys:
        if k not in flux_keys:
            raise KeyError(f"{type(model).__name__} has no flux key {k!r}")
    return keys


def _primal(model, x_dict: dict, parameters):
    """(outputs, records): ONE run of the module's normal forward -- its dy_drop draws, its warm-up pass, its state
    cache all move as in a plain call -- and what each call of the path inside it worked on (ops.PathRecord)."""
    with ops.record_paths() as records:
        outputs = model(x_dict, parameters)
    return outputs, records


def _directional(model, records, tangents: dict, keys) -> dict:
    """The output tangents of the recorded primal run along the D directions of `tangents`.  Touches nothing of the
    module's state: any number of direction sets may follow one primal run (parameter_jacobian)."""
    main = records[-1]
    x = main.x
    D = _leading(tangents)
    mask, n_routed, want_bfi = series_plan(keys, main.cfg.route is not None, main.cfg.n_flux)

    def f32(name):
        t = tangents.get(name)
        return None if t is None else t.to(device=x.device, dtype=torch.float32)

    x_t = f32('x_phy')
    if x_t is not None and tuple(x_t.shape[1:]) != tuple(x.shape):
        raise ValueError(f"tangent of x_phy must be [D, {', '.join(map(str, x.shape))}]")
    p_t = [f32('p_dyn'), f32('p_sta')] if _is_two_tensor(model) else [f32('parameters')]
    for p, t in zip(main.ptensors, p_t):
        if t is not None and tuple(t.shape[1:]) not in (tuple(p.shape), tuple(p.shape[1:]) if p.dim() == 3 else None):
            raise ValueError(f"parameter tangent of shape {tuple(t.shape)} fits neither [D, *{tuple(p.shape)}] nor the "
                             "compact [D,B,ny]")
    mu_t = f32('muwts')
    if mu_t is not None and main.muwts is not None:
        T, T_total = main.cfg.T, x.shape[0]
        if mu_t.dim() == 3:
            mu_t = mu_t.unsqueeze(1)
        if mu_t.shape[1] == T_total and T_total != T:       # rows aligned with x_phy: cut at warm_up, as the module
            mu_t = mu_t[:, T_total - T:]
        mu_t = mu_t.expand(D, T, main.cfg.B, main.cfg.M)
    s_t = f32('states')
    if s_t is not None and tuple(s_t.shape) != (D, 5, main.cfg.B, main.cfg.M):
        raise ValueError(f"tangent of states must be [D, 5, {main.cfg.B}, {main.cfg.M}]")

    guard = torch.cuda.device(x.device) if x.is_cuda else contextlib.nullcontext()
    with guard:
        for rec in records:
            last = rec is main
            res = ops.hbv_tangent_batch(rec, D, x_t, mu_t if last else None, s_t, p_t,
                                        mask if last else 0, n_routed if last else 0, want_bfi and last)
            s_t = res.state_out         # the warm-up's state tangent enters the main pass
    return _assemble_tangents(model, keys, res, mask, x_t, main, D)


def _assemble_tangents(model, keys, res, mask, x_t, main, D) -> dict:
    """HbvModule._assemble over a leading direction axis, for the wanted keys only."""
    cfg = main.cfg
    pos = {k: bin(mask & ((1 << k) - 1)).count("1") for k in range(cfg.n_flux) if (mask >> k) & 1}
    out = {}
    for key in keys:
        if key in ROUTED_KEYS and res.routed is not None:
            v = res.routed[:, ROUTED_KEYS[key]].unsqueeze(-1)
        elif key in ROUTED_KEYS:
            v = res.flux[:, pos[ROUTED_KEYS[key]]].unsqueeze(-1)
        elif key in FLUX_KEYS:
            v = res.flux[:, pos[FLUX_KEYS[key]]].unsqueeze(-1)
        elif key == 'BFI':
            out[key] = res.bfi
            continue
        else:   # PET_hydro is a slice of the forcings
            if x_t is None:
                v = torch.zeros((D, cfg.T, cfg.B, 1), dtype=torch.float32, device=main.x.device)
            else:
                v = x_t[:, cfg.t0:, :, model.variables.index('pet')].unsqueeze(-1)
        if not model.warm_up_states:
            v = v[:, model.pred_cutoff:]
        out[key] = v
    return out


# -- per-basin Jacobians ------------------------------------------------------------------------------------------
def jacobian_columns(model, names: Optional[Sequence[str]] = None):
    """(tangent name, column indices): the columns of the static-parameter row a Jacobian over `names` runs through --
    the nmul columns of each named physical parameter, in table order, then the routing columns for 'route_a' /
    'route_b'.  Default: every static parameter (and both routing columns when the model routes).  The row is
    parameters[T-1] for Hbv / Hbv_1_1p and p_sta for Hbv_2.  A dynamic parameter's Jacobian is not per-basin-row:
    naming one raises ValueError."""
    M = model.nmul
    phys = list(model.parameter_bounds.keys())
    dyn = [n for n in phys if n in model.dynamic_params]
    routing = list(model.routing_parameter_bounds.keys()) if model.routing else []
    if names is None:
        names = [n for n in phys if n not in dyn] + routing
    two = _is_two_tensor(model)
    table = [n for n in phys if n not in dyn] if two else phys      # p_sta holds the static ones only
    cols = []
    for n in names:
        if n in dyn:
            raise ValueError(f"{n} is a dynamic parameter: its Jacobian is not one row per basin")
        if n in table:
            i = table.index(n)
            cols += list(range(i * M, (i + 1) * M))
        elif n in routing:
            cols.append(len(table) * M + routing.index(n))
        else:
            raise ValueError(f"{type(model).__name__} has no static parameter {n!r}"
                             + (" (routing is off)" if n in model.routing_parameter_bounds else ""))
    return ('p_sta' if two else 'parameters'), cols


def one_hot_directions(cols: Sequence[int], B: int, width: int, device=None) -> torch.Tensor:
    """Compact directions [len(cols), B, width]: direction c is one in column cols[c] of EVERY basin.  Basins are
    independent, so its tangent is column cols[c] of every basin's own Jacobian: ny directions, not B * ny."""
    d = torch.zeros((len(cols), B, width), dtype=torch.float32, device=device)
    d[torch.arange(len(cols), device=device), :, torch.as_tensor(list(cols), dtype=torch.long, device=device)] = 1.0
    return d


def direction_chunks(n: int, max_directions: int):
    """[(c0, c1), ...] covering range(n) in pieces of at most max_directions."""
    if max_directions < 1:
        raise ValueError("max_directions must be >= 1")
    return [(c0, min(n, c0 + max_directions)) for c0 in range(0, n, max_directions)]


def parameter_jacobian(model, x_dict: dict, parameters, names: Optional[Sequence[str]] = None,
                       keys: Sequence[str] = ('streamflow',), max_directions: int = 64) -> dict:
    """Per-basin Jacobian of the output series with respect to the static parameters.

    Returns {key: J [T_out, B, C] for key in keys, 'columns': [C column indices]} with
    J[t, b, c] = d out[key][t, b] / d parameters[T-1, b, columns[c]]  (Hbv_2: d p_sta[b, columns[c]]); `names` as in
    `jacobian_columns`; BFI gives [B, C].  Compact one-hot directions, `max_directions` at a time, all on ONE run of
    the module's forward (`jvp_batch`'s primal): every piece differentiates the same function, and the module --
    generator, cached states -- is left as by one plain call."""
    _check_model(model)
    keys = _check_keys(model, keys)
    tname, cols = jacobian_columns(model, names)
    ptensor = parameters[1] if _is_two_tensor(model) else parameters
    B, width = ptensor.shape[-2], ptensor.shape[-1]
    _, records = _primal(model, x_dict, parameters)
    main = records[-1]
    dev = main.x.device
    T_out = main.cfg.T - (0 if model.warm_up_states else model.pred_cutoff)
    J = {k: torch.empty(((B,) if k == 'BFI' else (T_out, B)) + (len(cols),), dtype=torch.float32, device=dev)
         for k in keys}
    for c0, c1 in direction_chunks(len(cols), max_directions):
        tan = _directional(model, records, {tname: one_hot_directions(cols[c0:c1], B, width, dev)}, keys)
        for k in keys:
            t = tan[k]
            J[k][..., c0:c1] = t[..., 0].permute(1, 2, 0) if t.dim() == 4 else t.permute(1, 0)
    J['columns'] = list(cols)
    return J
