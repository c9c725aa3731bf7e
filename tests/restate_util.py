"""Golden cases through oracle/hbv_restate64.py, the float64 restatement of Hbv, Hbv_1_1p and Hbv_2
(tests/test_restate64.py pins it to the reference's fixtures; tests/test_jvp_f64_gpu.py measures the HIP tangents
against it)."""
from __future__ import annotations

import importlib.util
import os

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

from . import golden_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MOD = None


def restate():
    """The module oracle/hbv_restate64.py (loaded once)."""
    global _MOD
    if _MOD is None:
        spec = importlib.util.spec_from_file_location("hbv_restate64", os.path.join(ROOT, "oracle", "hbv_restate64.py"))
        _MOD = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_MOD)
    return _MOD


def config_kwargs(model: str, cfg) -> dict:
    """Keyword arguments of hbv_restate64.run for a module config (None = the module defaults)."""
    cfg = cfg or {}
    kw = dict(nmul=cfg.get("nmul", 1), dynamic=tuple((cfg.get("dynamic_params") or {}).get(model, ())),
              warm_up=cfg.get("warm_up", 0), warm_up_states=cfg.get("warm_up_states", True),
              variables=tuple(cfg.get("variables", ("prcp", "tmean", "pet"))), comprout=cfg.get("comprout", False),
              nearzero=cfg.get("nearzero", 1e-5))
    if "routing" in cfg:
        kw["routing"] = cfg["routing"]
    return kw


def masks_for(model: str, cfg, B: int, torch_seed=None) -> dict:
    """The dy_drop masks one module call draws (after torch.manual_seed(torch_seed) when given)."""
    kw = config_kwargs(model, cfg)
    if torch_seed is not None:
        torch.manual_seed(torch_seed)
    m = restate().drop_masks(model, kw["dynamic"], B, float((cfg or {}).get("dy_drop", 0.0)))
    return m if (cfg or {}).get("dy_drop", 0.0) > 0 else {}


def run_inputs(model: str, cfg, inp: dict, masks: dict, dtype=torch.float64, device="cpu", dirs=None,
               grad_leaves=(), states=None, aux=None, events=None):
    """hbv_restate64.run on the numpy inputs `inp` (golden_cases.build_inputs form) cast to `dtype`.  `dirs`: input
    name -> tangent (those inputs become duals of the caller's forward-AD level); `grad_leaves`: input names that
    require grad.  Returns (outputs, states, leaves by name)."""
    def arg(k):
        t = torch.as_tensor(np.asarray(inp[k])).to(device=device, dtype=dtype)
        if k in grad_leaves:
            t.requires_grad_(True)
        leaves[k] = t
        if dirs is not None and k in dirs:
            return fwAD.make_dual(t, torch.as_tensor(np.asarray(dirs[k])).to(device=device, dtype=dtype))
        return t
    leaves = {}
    kw = config_kwargs(model, cfg)
    extra = {}
    if model == "Hbv_2":
        params = (arg("p_dyn"), arg("p_sta"))
        extra = dict(ac_all=arg("ac_all"), elev_all=arg("elev_all"))
    else:
        params = arg("parameters")
    mu = arg("muwts") if "muwts" in inp else None
    if states is None and "states0" in inp:      # storages loaded into a cache_states module before the call
        states = tuple(torch.as_tensor(np.asarray(inp["states0"])).to(device=device, dtype=dtype))
    out, st = restate().run(model, arg("x_phy"), params, masks=masks, muwts=mu, states=states, aux=aux, events=events,
                            **kw, **extra)
    return out, st, leaves


def case_reverse(name: str, dtype=torch.float64, events=None) -> dict:
    """Outputs, storages and (for a case with a loss) the loss gradients of golden case `name`, keyed as the fixture
    tests/golden/<name>.npz is.  `events`: see hbv_restate64._pbm / pbm_hourly (a two-call case records none)."""
    spec = gc.CASES[name]
    model, cfg = spec["model"], spec["config"]
    if model == "Hbv_2_hourly":
        return hourly_case_reverse(name, dtype, events)
    inp = gc.build_inputs(name)
    res = {}
    if spec.get("two_call"):          # cache_states: the second call starts from the storages the first one left
        T, h = spec["T"], spec["T"] // 2
        with torch.no_grad():
            i1 = dict(inp, x_phy=inp["x_phy"][:h], parameters=np.concatenate([inp["parameters"][:h - 1],
                                                                              inp["parameters"][-1:]], 0))
            out1, st1, _ = run_inputs(model, cfg, i1, {}, dtype)
            i2 = dict(inp, x_phy=inp["x_phy"][h:], parameters=inp["parameters"][h:])
            out2, st2, _ = run_inputs(model, cfg, i2, {}, dtype, states=st1)
        for tag, out, st in (("1", out1, st1), ("2", out2, st2)):
            res.update({f"out{tag}/{k}": v.numpy() for k, v in out.items()})
            res[f"states{tag}"] = torch.stack(st).numpy()
        return res
    masks = masks_for(model, cfg, spec["B"], spec.get("torch_seed"))
    leaves = ["p_dyn", "p_sta"] if model == "Hbv_2" else ["parameters"]
    if spec.get("x_grad"):
        leaves.append("x_phy")
    keys = gc.loss_keys(name)
    out, st, lv = run_inputs(model, cfg, inp, masks, dtype, grad_leaves=leaves if keys else (), events=events)
    res.update({f"out/{k}": v.detach().numpy() for k, v in out.items()})
    res["states"] = torch.stack([s.detach() for s in st]).numpy()
    if keys:
        loss = sum((torch.from_numpy(gc.loss_weight(name, k, out[k].shape)).to(dtype) * out[k]).sum() for k in keys)
        loss.backward()
        for k in leaves:
            g = lv[k].grad
            res[f"grad/{k}"] = (torch.zeros_like(lv[k]) if g is None else g).numpy()
    return res


def hourly_case_reverse(name: str, dtype=torch.float64, events=None) -> dict:
    """case_reverse for a golden case of Hbv_2_hourly: Qs, streamflow, the five state series and the loss gradients of
    p_dyn, p_sta, p_distr (and x_phy where the case asks), keyed as the fixture is.  A case with `states0` is one
    cache_states call from loaded storages: its gage routing reads the detached history and returns the last row
    (hbv_2_hourly.py:770-794)."""
    spec = gc.CASES[name]
    cfg = spec["config"]
    inp = gc.build_inputs(name)
    kw = config_kwargs("Hbv_2_hourly", cfg)
    masks = masks_for("Hbv_2_hourly", cfg, spec["B"], spec.get("torch_seed"))
    t = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in inp.items()}
    leaves = ["p_dyn", "p_sta", "p_distr"] + (["x_phy"] if spec.get("x_grad") else [])
    for k in leaves:
        t[k].requires_grad_(True)
    states = tuple(t["states0"]) if "states0" in t else None
    out, ser = restate().run_hourly(
        t["x_phy"], (t["p_dyn"], t["p_sta"], t["p_distr"]), nmul=kw["nmul"], dynamic=kw["dynamic"], masks=masks,
        variables=kw["variables"], routing=kw.get("routing", False), nearzero=kw["nearzero"], muwts=t.get("muwts"),
        ac_all=t["ac_all"], elev_all=t["elev_all"], outlet_topo=t["outlet_topo"], areas=t["areas"], states=states,
        warm_up_states=kw["warm_up_states"], cache_states=bool((cfg or {}).get("cache_states", False)), events=events)
    res = {f"out/{k}": v.detach().numpy() for k, v in out.items()}
    res["states"] = torch.stack([s.detach() for s in ser]).numpy()
    loss = sum((torch.from_numpy(gc.loss_weight(name, k, out[k].shape)).to(dtype) * out[k]).sum()
               for k in gc.loss_keys(name))
    loss.backward()
    for k in leaves:
        res[f"grad/{k}"] = (torch.zeros_like(t[k]) if t[k].grad is None else t[k].grad).numpy()
    return res


def abi_hourly(prob: dict, dtype=torch.float64, x_grad: bool = True, backward: bool = True, events=None) -> dict:
    """An abi_util.make_problem dict of model Hbv_2_hourly through the restatement at the level of the C ABI, in
    `dtype`: raw parameters [T,B,ny] through the sigmoid (static value = row T-1, dynamic rows where the parameter is
    dynamic and its basin not dropped), the twelve flux rows (means over the members; Qsim weighted by muwts where
    given), the loss sum(flux * gflux) as abi_util.run_problem forms it, storages carried in from prob["state_in"].
    Returns run_problem's keys: flux [12,T,B], traj [5,T+1,B*M], state_out [5,B,M], g_params, g_x, g_muwts (float64
    numpy).  `events`: see hbv_restate64.pbm_hourly."""
    from .abi_util import BOUNDS
    R = restate()
    T, B, M, names = prob["T"], prob["B"], prob["M"], prob["names"]
    x = torch.from_numpy(prob["x"]).to(dtype).requires_grad_(x_grad and backward)
    raw = torch.from_numpy(prob["params"]).to(dtype).requires_grad_(backward)
    mu = torch.from_numpy(prob["muwts"]).to(dtype).requires_grad_(backward) if "muwts" in prob else None
    ac = torch.from_numpy(prob["ac"]).to(dtype)
    elev = torch.from_numpy(prob["elev"]).to(dtype)
    unit = torch.sigmoid(raw[:, :, :len(names) * M]).reshape(T, B, len(names), M)
    par = {}
    for i, nm in enumerate(names):
        lo, hi = BOUNDS[nm]
        v = unit[-1, :, i, :]
        if nm in prob["dyn"]:
            dyn = unit[:, :, i, :]
            if "drop" in prob:
                m = torch.from_numpy(prob["drop"][prob["dyn"].index(nm)].astype(np.float64)).to(dtype).view(1, B, 1)
                dyn = dyn * (1 - m) + v.unsqueeze(0) * m
            v = dyn
        par[nm] = v * (hi - lo) + lo
    if "state_in" in prob:
        st = tuple(torch.from_numpy(prob["state_in"][k]).to(dtype) for k in range(5))
    else:
        st = tuple(torch.full((B, M), 0.001, dtype=dtype) for _ in range(5))
    ch = prob.get("channels", (0, 1, 2))
    s, ser = R.pbm_hourly(x[:, :, ch[0]], x[:, :, ch[1]], x[:, :, ch[2]], par, st, 1e-5, ac, elev, events)
    rows = [s[k].mean(-1) for k in R.HOURLY_SERIES]
    if mu is not None:
        rows[0] = (s["Qsim"] * mu).sum(-1)
    flux = torch.stack(rows)
    traj = torch.stack([torch.cat([st[k].unsqueeze(0), ser[k].detach()]).reshape(T + 1, B * M) for k in range(5)])
    res = {"flux": flux.detach().numpy(), "traj": traj.numpy(),
           "state_out": (torch.stack([ser[k][-1].detach() for k in range(5)]) if T else torch.stack(st)).numpy()}
    if backward:
        (flux * torch.from_numpy(prob["gflux"]).to(dtype)).sum().backward()
        res["g_params"] = raw.grad.numpy()
        if x_grad:
            res["g_x"] = x.grad.numpy()
        if mu is not None:
            res["g_muwts"] = mu.grad.numpy()
    return res


def daily_forward(prob: dict, x, raw, mu, st, dtype=torch.float64, events=None):
    """The forward of abi_daily on tensors the caller made (leaves of a backward pass, or duals of a forward-AD
    level): x [T,B,C], raw parameters [T,B,ny], mu [T,B,M] or None, st the five storages [B,M] carried in.  Returns
    (flux [11 or 12,T,B], routed [4,T,B] or None, the five final storages, the five storage series [T,B,M])."""
    from .abi_util import BOUNDS
    R = restate()
    model, T, B, M, names = prob["model"], prob["T"], prob["B"], prob["M"], prob["names"]
    assert model in R.MODELS, model
    ac = torch.from_numpy(prob["ac"]).to(dtype) if "ac" in prob else None
    elev = torch.from_numpy(prob["elev"]).to(dtype) if "elev" in prob else None
    unit = torch.sigmoid(raw[:, :, :len(names) * M]).reshape(T, B, len(names), M)
    par = {}
    for i, nm in enumerate(names):
        lo, hi = BOUNDS[nm]
        v = unit[-1, :, i, :].unsqueeze(0).expand(T, B, M)
        if nm in prob["dyn"]:
            dyn = unit[:, :, i, :]
            if "drop" in prob:
                m = torch.from_numpy(prob["drop"][prob["dyn"].index(nm)].astype(np.float64)).to(dtype).view(1, B, 1)
                dyn = dyn * (1 - m) + v * m
            v = dyn
        par[nm] = v * (hi - lo) + lo
    ch = prob.get("channels", (0, 1, 2))
    s, st_out, ser = R._pbm(model, x[:, :, ch[0]], x[:, :, ch[1]], x[:, :, ch[2]], par, st, 1e-5, ac, elev, events,
                            want_series=True)
    order = ["Qsim", "Q0", "Q1", "Q2", "AET", "SWE", "recharge", "excs", "evapfactor", "tosoil", "PERC"]
    if model != "Hbv":
        order.append("capillary")
    rows = [s[k].mean(-1) for k in order]
    if mu is not None:
        rows[0] = (s["Qsim"] * mu).sum(-1)
    flux = torch.stack(rows)
    routed = None
    if prob["routing"]:
        n = len(names)
        ab = torch.sigmoid(raw[-1, :, n * M:n * M + 2])
        uh = R.gamma_uh(ab[:, 0] * 2.9, ab[:, 1] * 6.5, min(T, 15))
        routed = torch.stack([R.route(flux[k], uh) for k in range(4)])
    return flux, routed, st_out, ser


def abi_daily(prob: dict, dtype=torch.float64, x_grad: bool = True, backward: bool = True, events=None) -> dict:
    """An abi_util.make_problem dict of a daily model (Hbv, Hbv_1_1p, Hbv_2) through the restatement at the level of the
    C ABI, in `dtype`: raw parameters [T,B,ny] through the sigmoid (static value = row T-1, dynamic rows where the
    parameter is dynamic and its basin not dropped), forcing channels prob["channels"], storages carried in from
    prob["state_in"], the 11 / 12 flux rows (means over the members; Qsim weighted by muwts where given), with
    prob["routing"] the four 15-tap routed rows (Qsim, Q0, Q1, Q2 through hbv_restate64.gamma_uh / route, routing
    columns from row T-1 with run_problem's RouteSource bounds), and the loss sum(flux * gflux) + sum(routed * grouted)
    as abi_util.run_problem forms it.  Returns run_problem's keys: flux, routed, traj [5,T+1,B*M], state_out [5,B,M],
    g_params, g_x, g_muwts (float64 numpy).  `events`: see hbv_restate64._pbm."""
    T, B, M = prob["T"], prob["B"], prob["M"]
    x = torch.from_numpy(prob["x"]).to(dtype).requires_grad_(x_grad and backward)
    raw = torch.from_numpy(prob["params"]).to(dtype).requires_grad_(backward)
    mu = torch.from_numpy(prob["muwts"]).to(dtype).requires_grad_(backward) if "muwts" in prob else None
    if "state_in" in prob:
        st = tuple(torch.from_numpy(prob["state_in"][k]).to(dtype) for k in range(5))
    else:
        st = tuple(torch.full((B, M), 0.001, dtype=dtype) for _ in range(5))
    flux, routed, st_out, ser = daily_forward(prob, x, raw, mu, st, dtype, events)
    traj = torch.stack([torch.cat([st[k].unsqueeze(0), ser[k].detach()]).reshape(T + 1, B * M) for k in range(5)])
    res = {"flux": flux.detach().numpy(), "traj": traj.numpy(),
           "state_out": torch.stack([v.detach() for v in st_out]).numpy()}
    loss = (flux * torch.from_numpy(prob["gflux"]).to(dtype)).sum()
    if routed is not None:
        res["routed"] = routed.detach().numpy()
        loss = loss + (routed * torch.from_numpy(prob["grouted"]).to(dtype)).sum()
    if backward:
        loss.backward()
        res["g_params"] = raw.grad.numpy()
        if x_grad:
            res["g_x"] = x.grad.numpy()
        if mu is not None:
            res["g_muwts"] = mu.grad.numpy()
    return res


def bfi_term_scale(aux: dict) -> np.ndarray:
    """Per basin, the size of the two terms whose difference is BFI's tangent, 100 (|dS2| + S2 |dS0'|/S0') / S0'
    (S2 = sum of the routed Q2, S0' = sum of the routed Qs + nearzero, d = their tangents), from run(aux=...)
    under forward AD: where they cancel, float32 rounds each of them, not their small difference."""
    (s2, ds2), (s0, ds0) = (fwAD.unpack_dual(v) for v in aux["bfi_sums"])
    ds2 = torch.zeros_like(s2) if ds2 is None else ds2
    ds0 = torch.zeros_like(s0) if ds0 is None else ds0
    return (100 * (ds2.abs() + s2.abs() * ds0.abs() / s0.abs()) / s0.abs()).detach().cpu().double().numpy()


def tangents(out: dict, keys) -> dict:
    """Output tangents (float64 numpy, zeros where none flows) of `keys` from duals of the current level."""
    res = {}
    for k in keys:
        p, t = fwAD.unpack_dual(out[k])
        res[k] = (torch.zeros_like(p) if t is None else t).detach().cpu().double().numpy()
    return res
