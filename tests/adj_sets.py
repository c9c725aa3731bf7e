"""Problem set, branch counts and the float64 comparison protocol of the implicit model's float64 tests
(tests/test_adj_f64.py on the CPU, tests/test_adj_f64_gpu.py on the GPU).  The protocol -- `admit`, the cap -- is
tests/hourly_sets.py's, used as it is; the tolerances are tests/test_hbv_adj.py's converged ones.  No test lives here.

A problem is a run of the HbvAdj module: forcing synth.forcing(T, B, 7, day0) with the precipitation scaled, raw
parameters synth.raw_parameters(T, B, ny, 7, 2.0) (spread over their ranges), loss weights synth.loss_weights, and a
start: zeros (the module's own, `state=None`) or synth.wet_states(B, M, 7) handed to HbvAdj._forward_eager as `state`
and to the oracle as `y0`.  The float64 reference is oracle/hbv_adj_oracle.py with a converged Newton iteration (gtol
1e-11, 40 updates: the root itself); the product runs its tight policy (gtol 1e-6, 12 updates) as in test_hbv_adj.py.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from . import abi_util as au
from . import hourly_sets as hs
from . import synth
from .test_hbv_adj import adj_oracle

SEED = 7
PROBLEMS = {
    # 80 lanes: a full wave and a ragged one
    "wet120": dict(T=120, B=5, M=16, dyn=("parBETAET",), wet=True),
    "storm120": dict(T=120, B=5, M=16, dyn=("parBETA", "parBETAET"), pscale=4.0),
    "storm120-wet": dict(T=120, B=5, M=16, dyn=("parBETA", "parBETAET"), pscale=4.0, wet=True),
    # five dynamic parameters with drops: the generic parameter fetch
    "wet64-list": dict(T=64, B=3, M=4, dyn=("parK0", "parFC", "parUZL", "parPERC", "parBETAET"), dy_drop=0.3, wet=True),
    # exactly one wave, three dynamic parameters (the slot list), one day past a tile
    "wet65-three": dict(T=65, B=4, M=16, dyn=("parK0", "parFC", "parBETAET"), wet=True),
    # one day past an 8-day tile and an HBVX_CHUNK=8 chunk; exactly one of each; the prologue / epilogue edges
    "wet9": dict(T=9, B=6, M=3, dyn=(), wet=True),
    "wet8": dict(T=8, B=6, M=3, dyn=(), wet=True),
    "wet2": dict(T=2, B=6, M=3, dyn=(), wet=True),
    "wet1": dict(T=1, B=6, M=3, dyn=(), wet=True),
    # the flux-less pipelined warm-up, differentiated through
    "storm90-warmup": dict(T=90, B=5, M=16, dyn=("parCFMAX",), warm_up=40, pscale=4.0),
    # the same from filled storages: the start and its tangent enter the warm-up pass (from zeros every storage sits ON
    # its clamp, where the derivative to the start is a convention float32 and float64 do not share)
    "storm90-warmup-wet": dict(T=90, B=5, M=16, dyn=("parCFMAX",), warm_up=40, pscale=4.0, wet=True),
    # a winter and a melt season on filled storages
    "wet400": dict(T=400, B=4, M=4, dyn=("parBETA",), wet=True, day0=120.0),
}
SOLVERS = ("staged", "joint")
TIGHT = dict(newton_gtol=1e-6, newton_max_iter=12)      # test_hbv_adj._run_case's converged policy of the product
ROOT_POLICY = dict(gtol=1e-11, max_iter=40)             # the oracle: the root itself


@functools.lru_cache(maxsize=None)
def inputs(name: str, zero_state: bool = False) -> dict:
    """x [T,B,3], p [T,B,ny], w [T',B,1], state [5,B,M] or None, and the module's settings.  `zero_state`: a problem
    with the zero start carries it as a tensor of zeros (so that the start has a gradient and a tangent)."""
    k = PROBLEMS[name]
    T, B, M = k["T"], k["B"], k["M"]
    n = 13 if "parBETAET" in k["dyn"] else 12
    x = synth.forcing(T, B, SEED, day0=k.get("day0", 60.0))
    x[..., 0] *= np.float32(k.get("pscale", 1.0))
    p = synth.raw_parameters(T, B, n * M + 2, SEED, 2.0)
    wu = k.get("warm_up", 0)
    w = synth.loss_weights((T, B, 1), SEED, 70)[wu:]
    state = synth.wet_states(B, M, SEED) if k.get("wet") else (np.zeros((5, B, M), np.float32) if zero_state else None)
    cfg = dict(nmul=M, warm_up=wu, dy_drop=k.get("dy_drop", 0.0), dynamic_params={"HbvAdj": list(k["dyn"])})
    return dict(name=name, T=T, B=B, M=M, x=torch.from_numpy(x), p=torch.from_numpy(p), w=torch.from_numpy(w),
                state=None if state is None else torch.from_numpy(state), cfg=cfg)


def to_lanes(state: torch.Tensor) -> torch.Tensor:
    """[...,5,B,M] (the module's) -> [...,N,5] in the oracle's member-major lane order (lane j*B + b)."""
    lead = state.shape[:-3]
    return state.movedim(-3, -1).transpose(-3, -2).reshape(*lead, -1, 5)


def from_lanes(y: torch.Tensor, B: int, M: int) -> torch.Tensor:
    """The inverse of to_lanes."""
    lead = y.shape[:-2]
    return y.reshape(*lead, M, B, 5).transpose(-3, -2).movedim(-1, -3)


F32_POLICY = dict(gtol=1e-6, max_iter=12)               # the float32 evaluation: what float32 can converge to


def oracle_kw(prob: dict, **policy) -> dict:
    cfg = prob["cfg"]
    return dict(nmul=cfg["nmul"], warm_up=cfg["warm_up"], dynamic_params=cfg["dynamic_params"]["HbvAdj"],
                dy_drop=cfg["dy_drop"], **(policy or ROOT_POLICY))


@functools.lru_cache(maxsize=None)
def oracle_run(name: str, dtype: str = "float64", zero_state: bool = False) -> dict:
    """The oracle at the root: flow [T',B,1], g_params [T,B,ny], g_state [5,B,M] (with a start), the update counts and
    (float64) the branches taken.  Computed once per problem and shared; nobody writes into it."""
    prob = inputs(name, zero_state)
    dt = getattr(torch, dtype)
    pp = prob["p"].clone().to(dt).requires_grad_(True)
    y0 = None if prob["state"] is None else to_lanes(prob["state"]).to(dt).requires_grad_(True)
    events = {} if dtype == "float64" else None
    torch.manual_seed(5)
    out, its = adj_oracle.hbv_adj_forward(prob["x"], pp, y0=y0, events=events, dtype=dt,
                                          **oracle_kw(prob, **(F32_POLICY if dtype == "float32" else {})))
    (out * prob["w"].to(dt)).sum().backward()
    res = dict(flow=out.detach().numpy(), g_params=pp.grad.numpy(), its=its, events=events)
    if y0 is not None:
        res["g_state"] = from_lanes(y0.grad, prob["B"], prob["M"]).contiguous().numpy()
    return res


# ---- tangents ---------------------------------------------------------------------------------------------------------
TAN_PROBLEMS = ("wet120", "wet64-list", "storm90-warmup", "storm90-warmup-wet", "wet9")


def tan_inputs(name: str):
    """The problem (a zero start as a tensor) and three directions: parameters [T,B,ny], x_phy [T,B,3], start [5,B,M]."""
    prob = inputs(name, True)
    g = torch.Generator().manual_seed(3000 + TAN_PROBLEMS.index(name))
    vp = torch.randn(prob["p"].shape, generator=g) * 0.3
    vx = torch.randn(prob["x"].shape, generator=g)
    vs = torch.randn(prob["state"].shape, generator=g)
    return prob, vp, vx, vs


@functools.lru_cache(maxsize=None)
def tangent_reference(name: str, dtype: str = "float64", routing: bool = True):
    """[3,T',B,1]: the oracle's JVP at the root along the three directions of tan_inputs (parameters, x_phy, start),
    by double backward on ONE forward run."""
    prob, vp, vx, vs = tan_inputs(name)
    dt = getattr(torch, dtype)
    x = prob["x"].to(dt).clone().requires_grad_(True)
    p = prob["p"].to(dt).clone().requires_grad_(True)
    y0 = to_lanes(prob["state"]).to(dt).clone().requires_grad_(True)
    torch.manual_seed(5)
    out = adj_oracle.hbv_adj_forward(x, p, y0=y0, dtype=dt, routing=routing,
                                     **oracle_kw(prob, **(F32_POLICY if dtype == "float32" else {})))[0]
    v = torch.zeros_like(out, requires_grad=True)
    gx, gp, gy = torch.autograd.grad(out, (x, p, y0), v, create_graph=True)
    res = []
    for g, t in ((gp, vp), (gx, vx), (gy, to_lanes(vs))):
        res.append(torch.autograd.grad((g * t.to(dt)).sum(), v, retain_graph=True)[0].numpy())
    return np.stack(res)


def model(device, prob: dict, solver: str = "staged", tight: bool = True, **extra):
    import hydrodl2_amd
    cfg = dict(prob["cfg"], newton_solver=solver, **(TIGHT if tight else {}), **extra)
    return hydrodl2_amd.load_model("hbv_adj", "HbvAdj")(cfg, torch.device(device))


def product_run(device, name: str, solver: str = "staged", tight: bool = True, zero_state: bool = False) -> dict:
    """The module on `device`: flow, g_params and (with a start) g_state, as oracle_run names them."""
    prob = inputs(name, zero_state)
    m = model(device, prob, solver, tight)
    pp = prob["p"].to(device).clone().requires_grad_(True)
    st = None if prob["state"] is None else prob["state"].to(device).clone().requires_grad_(True)
    torch.manual_seed(5)
    out = m._forward_eager({"x_phy": prob["x"].to(device)}, pp, state=st)["flow_sim"]
    (out * prob["w"].to(device)).sum().backward()
    res = dict(flow=out.detach().cpu().numpy(), g_params=pp.grad.cpu().numpy())
    if st is not None:
        res["g_state"] = st.grad.cpu().numpy()
    return res


# ---- comparison against float64 --------------------------------------------------------------------------------------
VALUE_TOL = (2e-4, 2e-5)      # test_hbv_adj._close's converged ones: rtol, atol relative to the array's largest value
GRAD_TOL = (2e-3, 2e-4)       # gradients and tangents


def tol_fn(rtol, atol_rel):
    """test_hbv_adj._close's tolerance as a function of the reference array, for hourly_sets.admit."""
    return lambda b: atol_rel * max(float(np.abs(b).max()), 1e-30) + rtol * np.abs(b)


def close_f64(label, got, want64, f32_eval, tol):
    """`got` against float64 under hourly_sets.admit (`f32_eval`: a callable returning the float32 oracle's array); the
    worst error / tolerance of what was not admitted goes to abi_util.REPORT and is returned."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    f = tol_fn(*tol)
    kept = hs.admit(label, got, want64, [f32_eval], f)
    err = np.abs(kept - want64)
    ratio = float((err / f(want64)).max()) if err.size else 0.0
    au.REPORT.append((label, float(err.max()) if err.size else 0.0, ratio, int((kept != got).sum()), got.size))
    print(f"{label}: worst error / tolerance {ratio:.4f}")
    return ratio


def compare_f64(label, name, got, zero_state=False):
    """A product_run result against oracle_run(name): values, parameter gradient and start gradient.  Every array is
    compared before anything is raised."""
    want = oracle_run(name, "float64", zero_state)
    bad = []
    for key, tol in (("flow", VALUE_TOL), ("g_params", GRAD_TOL), ("g_state", GRAD_TOL)):
        if key not in want:
            continue
        try:
            close_f64(f"adj-f64 {label} {key}", got[key], want[key],
                      lambda key=key: oracle_run(name, "float32", zero_state)[key], tol)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, " | ".join(bad)


# ---- branch coverage -------------------------------------------------------------------------------------------------
# Asserted: taken in at least COVER_MIN of the lane-days of at least one problem, at the float64 root
EVENTS = ("rain", "snow", "melt_pack_limited", "melt_potential", "refr_mw_limited", "refr_potential", "isnow_warm",
          "isnow_cold", "sm_above_fc", "sm_below_fc", "ef_clamped", "ef_free", "et_sm_limited", "et_pet_limited",
          "sm_floor", "perc_suz", "perc_par", "q0_active", "q0_idle", "gw_suz_idle", "gw_suz_q0", "gw_par_idle",
          "gw_par_q0")
COVER_MIN = hs.COVER_MIN


def coverage(name: str) -> dict:
    return {k: float(v.double().mean()) for k, v in oracle_run(name)["events"].items()}


def format_coverage(rows: dict) -> str:
    names = list(rows)
    out = [f"{'branch':18s} " + " ".join(f"{n[:10]:>10s}" for n in names)]
    for k in EVENTS:
        out.append(f"{k:18s} " + " ".join(f"{rows[n][k]:10.5f}" for n in names))
    return "\n".join(out)


def assert_covered(rows: dict, never=()):
    print(format_coverage(rows))
    missing = [k for k in EVENTS if k not in never and max(c[k] for c in rows.values()) < COVER_MIN]
    assert not missing, f"branches not covered: {missing}"
    taken = [(n, k) for n, c in rows.items() for k in never if c[k] != 0.0]
    assert not taken, f"a branch argued unreachable was taken: {taken}"


# ---- the acceptance test of the staged solve -------------------------------------------------------------------------
# |G_k| <= K_ROUND * 2^-23 * scale for the four closed forms and |G_2| <= gtol + the same allowance for the soil-
# moisture equation, where scale is, per lane-day, the largest of the equation's fluxes and of the storages it reads
# (the product holds its parameters in float32, the residual is evaluated with float64 ones: ex = SM - FC differs by
# the rounding of FC, a flux at its potential by that of TT).  Measured on the host build, wet120 and storm120 under the
# reference policy: 2.30 / 2.88 / 1.62 / 1.51 (wet120) and 1.35 / 1.75 / 2.35 / 1.40 (storm120) for G0, G1, G3, G4, and
# |G2| <= 9.995e-4 < gtol on every lane-day.  Committed: 4 x the largest, 2.88.
K_ROUND = 11.5
# per equation: its fluxes, and the storages it reads (hbv_adj.py:425-429: Isnow reads SNOWPACK and MELTWATER, Peff and
# ex read SM -- ex = SM - FC is a small difference of large numbers --, perc reads SUZ)
_EQ_TERMS = (("sf", "refr", "melt", "SNOWPACK", "MELTWATER"), ("melt", "refr", "Isnow", "SNOWPACK", "MELTWATER"),
             ("Isnow", "rf", "Peff", "ex", "et", "SNOWPACK", "MELTWATER", "SM"),
             ("Peff", "ex", "perc", "q0", "q1", "SNOWPACK", "MELTWATER", "SM", "SUZ"), ("perc", "q2", "SUZ", "SLZ"))


def accepted_state_residuals(name: str, traj: torch.Tensor, gtol: float = 1e-3):
    """The product's solved trajectory `traj` [5,T+1,B*M] (a PathRecord's, main pass without a warm-up) put into the
    oracle's float64 residual G = (x - x_t)/dt - f(x): per equation, the largest over the lane-days of
    (|G_k| - gtol [k = 2 only]) / (2^-23 * the largest of the equation's fluxes and of the storages it reads there),
    and the largest |G_k|."""
    prob = inputs(name)
    T, B, M = prob["T"], prob["B"], prob["M"]
    assert prob["cfg"]["warm_up"] == 0 and tuple(traj.shape) == (5, T + 1, B * M)
    y = to_lanes(traj.detach().cpu().double().view(5, T + 1, B, M).permute(1, 0, 2, 3))      # [T+1,N,5]
    torch.manual_seed(5)
    names, _, pr, clim, _ = adj_oracle.lane_inputs(prob["x"], prob["p"], **{k: v for k, v in oracle_kw(prob).items()
                                                                             if k not in ROOT_POLICY})
    ks, gs = np.zeros(5), np.zeros(5)
    for t in range(T):
        g = adj_oracle._G(y[t + 1], pr[t], y[t], clim[t], names).abs()
        fl = adj_oracle.fluxes(y[t + 1], pr[t], clim[t], names)
        # a flux at its potential CFMAX (T - TT) or CFR CFMAX (TT - T) carries the rounding of the larger of T and TT
        tmax = torch.maximum(fl["T"].abs(), fl["TT"].abs())
        pot = torch.maximum(fl["CFMAX"] * tmax * ((fl["melt"] > 0) & (fl["melt"] == fl["mpot"])),
                            fl["CFR"] * fl["CFMAX"] * tmax * ((fl["refr"] > 0) & (fl["refr"] == fl["rpot"])))
        for k in range(5):
            scale = torch.stack([y[t + 1][:, k].abs(), y[t][:, k].abs()] + [fl[n].abs() for n in _EQ_TERMS[k]]
                                + ([pot] if k < 2 else [])).amax(0)
            over = g[:, k] - (gtol if k == 2 else 0.0)
            ks[k] = max(ks[k], float((over / (2.0 ** -23 * scale.clamp(min=1e-30))).max()))
            gs[k] = max(gs[k], float(g[:, k].max()))
    return ks, gs
