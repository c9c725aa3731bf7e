"""Shared pieces of the hourly model's forward-mode tests (tests/test_hourly_jvp_abi_gpu.py, test_gage_route_jvp_gpu.py,
test_hourly_jvp_gpu.py): the tolerance, the directions and float64 / float32 forward AD of oracle/hbv_restate64.py at
the level of the C ABI, of the gage routing and of the module.  No test lives here."""
from __future__ import annotations

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

from . import golden_cases as gc
from . import hourly_sets as hs
from . import restate_util as ru
from . import synth
from .test_jvp_gpu import TAN_ATOL_REL, TAN_FLOOR, TAN_RTOL

HOURLY_CASES = [n for n, s in gc.CASES.items() if s["model"] == "Hbv_2_hourly"]


def tan_tol(top: float, axis: int = 0):
    """tol_fn for hourly_sets.admit: TAN_RTOL |b| + TAN_ATOL_REL x max|b over the series|, a series being one index of
    `axis`; a series below TAN_FLOOR of `top` (the call's largest float64 tangent) is priced at `top`."""
    def fn(b):
        b = np.asarray(b, np.float64)
        m = np.abs(np.moveaxis(b, axis, 0)).reshape(b.shape[axis], -1).max(1)
        scale = np.where(m >= TAN_FLOOR * top, m, top)
        shape = [1] * b.ndim
        shape[axis] = -1
        return TAN_ATOL_REL * np.maximum(scale, 1e-300).reshape(shape) + TAN_RTOL * np.abs(b)
    return fn


def compare(label, got, want64, f32_eval, top=None, axis=0):
    """`got` against float64 under hourly_sets.admit at tan_tol; returns the worst error / tolerance ratio."""
    want64 = np.asarray(want64, np.float64)
    top = float(np.abs(want64).max()) if top is None else top
    fn = tan_tol(max(top, 1e-300), axis)
    ratio = float((np.abs(np.asarray(got, np.float64) - want64) / fn(want64)).max()) if want64.size else 0.0
    print(f"{label}: worst error / tolerance against float64 {ratio:.3g}")
    assert np.isfinite(np.asarray(got)).all(), f"{label}: non-finite tangents"
    hs.admit(label, got, want64, [f32_eval], fn)
    return ratio


# ---- C ABI level --------------------------------------------------------------------------------------------------
def abi_directions(prob: dict, seed: int = 31) -> dict:
    """One direction over everything hbvx_hourly_tangent_batch differentiates along."""
    B, M = prob["B"], prob["M"]
    d = {"x": synth.normalish(prob["x"].shape, seed, 1) * 0.05,
         "params": synth.normalish(prob["params"].shape, seed, 2) * 0.3,
         "state_in": synth.normalish((5, B, M), seed, 4) * 1.0}
    if "muwts" in prob:
        d["muwts"] = synth.normalish(prob["muwts"].shape, seed, 3) * 0.05
    return {k: np.ascontiguousarray(v, np.float32) for k, v in d.items()}


def with_explicit_start(prob: dict) -> dict:
    """The problem with its initial storages spelled out (the default 0.001 where none are carried in), so that a
    state_in tangent has a state_in to go with: the same run."""
    if "state_in" in prob:
        return prob
    return dict(prob, state_in=np.full((5, prob["B"], prob["M"]), 0.001, np.float32))


def abi_forward_ad(prob: dict, dirs: dict, dtype=torch.float64) -> dict:
    """restate_util.abi_hourly's forward under forward AD along `dirs`: tangents of the twelve flux rows [12,T,B] and
    of the final storages [5,B,M] (float64 numpy)."""
    from .abi_util import BOUNDS
    R = ru.restate()
    T, B, M, names = prob["T"], prob["B"], prob["M"], prob["names"]

    def dual(a, d):
        a = torch.from_numpy(np.asarray(a)).to(dtype)
        return a if d is None else fwAD.make_dual(a, torch.from_numpy(np.asarray(d)).to(dtype))
    with fwAD.dual_level():
        x = dual(prob["x"], dirs.get("x"))
        raw = dual(prob["params"], dirs.get("params"))
        mu = dual(prob["muwts"], dirs.get("muwts")) if "muwts" in prob else None
        ac, elev = torch.from_numpy(prob["ac"]).to(dtype), torch.from_numpy(prob["elev"]).to(dtype)
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
        st = tuple(dual(prob["state_in"], dirs.get("state_in")).unbind(0))
        ch = prob.get("channels", (0, 1, 2))
        s, ser = R.pbm_hourly(x[:, :, ch[0]], x[:, :, ch[1]], x[:, :, ch[2]], par, st, 1e-5, ac, elev)
        rows = [s[k].mean(-1) for k in R.HOURLY_SERIES]
        if mu is not None:
            rows[0] = (s["Qsim"] * mu).sum(-1)
        out = {"flux": torch.stack(rows), "state_out": torch.stack([ser[k][-1] for k in range(5)])}
        return ru.tangents(out, ("flux", "state_out"))


# ---- gage routing -------------------------------------------------------------------------------------------------
def gage_forward_ad(qs, dp, topo, areas, lag_uh, bounds, qs_dot, dp_dot, dtype=torch.float64) -> np.ndarray:
    """Tangent of hbv_restate64.gage_route along (qs_dot, dp_dot) (None: zero), [T,G] float64 numpy."""
    R = ru.restate()

    def dual(a, d):
        a = torch.from_numpy(np.asarray(a)).to(dtype)
        return a if d is None else fwAD.make_dual(a, torch.from_numpy(np.asarray(d)).to(dtype))
    with fwAD.dual_level():
        out = R.gage_route(dual(qs, qs_dot), dual(dp, dp_dot), torch.from_numpy(np.asarray(topo)).to(dtype),
                           torch.from_numpy(np.asarray(areas)).to(dtype), lag_uh=lag_uh, bounds=bounds)
        return ru.tangents({"out": out}, ("out",))["out"]


# ---- module level -------------------------------------------------------------------------------------------------
SCALES = (("x_phy", 0.05), ("p_dyn", 0.1), ("p_sta", 0.1), ("p_distr", 0.1), ("muwts", 0.05), ("states0", 1.0))


def module_directions(inp: dict, seed: int = 41) -> dict:
    """One direction over every input of golden_cases.build_inputs form that jvp_batch differentiates along."""
    return {k: np.ascontiguousarray(synth.normalish(np.asarray(inp[k]).shape, seed, i) * s, np.float32)
            for i, (k, s) in enumerate(SCALES) if k in inp}


def module_forward_ad(name: str, inp: dict, dirs: dict, dtype=torch.float64) -> dict:
    """Tangents of 'Qs' and 'streamflow' of golden case `name` along `dirs`: forward AD of hbv_restate64.run_hourly,
    as restate_util.hourly_case_reverse runs it (float64 numpy)."""
    spec = gc.CASES[name]
    cfg = spec["config"]
    kw = ru.config_kwargs("Hbv_2_hourly", cfg)
    masks = ru.masks_for("Hbv_2_hourly", cfg, spec["B"], spec.get("torch_seed"))
    with fwAD.dual_level():
        t = {}
        for k, v in inp.items():
            a = torch.as_tensor(np.asarray(v)).to(dtype)
            t[k] = fwAD.make_dual(a, torch.from_numpy(dirs[k]).to(dtype)) if k in dirs else a
        states = tuple(t["states0"].unbind(0)) if "states0" in t else None
        out, _ = ru.restate().run_hourly(
            t["x_phy"], (t["p_dyn"], t["p_sta"], t["p_distr"]), nmul=kw["nmul"], dynamic=kw["dynamic"], masks=masks,
            variables=kw["variables"], routing=kw.get("routing", False), nearzero=kw["nearzero"], muwts=t.get("muwts"),
            ac_all=t["ac_all"], elev_all=t["elev_all"], outlet_topo=t["outlet_topo"], areas=t["areas"], states=states,
            warm_up_states=kw["warm_up_states"], cache_states=bool((cfg or {}).get("cache_states", False)))
        return ru.tangents(out, ("Qs", "streamflow"))
