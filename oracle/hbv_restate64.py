"""Dtype-agnostic pure-torch restatement of the reference's daily HBV models Hbv, Hbv_1_1p and Hbv_2 with their
module-level orchestration.  TEST INFRASTRUCTURE ONLY (tests/ and tools/ import it; the product never does).

Why it exists: the reference hard-codes float32, so no float64 run of it can be made.  This file restates the same
equations in whatever dtype its inputs carry; run in float64 under torch.autograd.forward_ad (or reverse mode) it is
the high-precision yardstick for the HIP tangent and adjoint kernels.  It is pinned to the reference's own fixtures
(tests/golden/<case>.npz, jvp_<case>.npz) by tests/test_restate64.py.

What it follows (file:line in the reference's src/hydrodl2):
  * parameter prep   Hbv / Hbv_1_1p: sigmoid of the raw NN output viewed [T,B,n,M], static value = last row, dynamic
                     values = per-day rows, `p*(hi-lo)+lo` (models/hbv/hbv.py:182-283, hbv_1_1p.py:181-282,
                     core/calc/utils.py:24); routing columns from the last row (hbv.py:212-214).
                     Hbv_2: no sigmoid; dynamic parameters in the ORDER OF THE CONFIG LIST from p_dyn, static ones in
                     table order from p_sta, routing columns after them (hbv_2.py:190-323).
  * dy_drop          per dynamic parameter one Bernoulli mask per basin, comPar = dyn*(1-m) + sta*m (hbv.py:236-246,
                     hbv_2.py:254-263).  The masks are an explicit argument; `drop_masks` draws them from the global
                     CPU generator in the order the module consumes it.
  * daily step       snow, soil, evaporation, groundwater (hbv.py:428-505); BETAET always and capillary rise for
                     Hbv_1_1p (hbv_1_1p.py:472-491); Hbv_2's elevation switch of parTT and its `ac` leakage term
                     (hbv_2.py:464-575).  parBETAET acts in Hbv only when it is dynamic (hbv.py:124-125,473-476).
  * warm-up          warm_up_states: a states-only call on days [0, warm_up) with every parameter static from row
                     warm_up-1 (hbv.py:314-346), under no_grad as there: reverse-mode gradients stop at it, forward-
                     mode tangents flow through it (no_grad does not stop forward AD).  Without warm_up_states the
                     whole record runs and the series are cut at pred_cutoff = warm_up afterwards, BFI over the whole record (hbv.py:314-319,591-594).  Hbv_2 has
                     no warm-up (hbv_2.py:324-390).
  * ensemble         mean over members, or sum weighted by muwts for the Qsim series only (hbv.py:507-511).
  * routing          gamma unit hydrograph of length min(T', 15) and a causal per-basin convolution
                     (core/calc/uh_routing.py:5-57, via oracle/hbv_torch_eager.py's gamma_uh / route).  routing=False
                     follows Hbv_2 (hbv_2.py:620-626) for every model: the reference's Hbv crashes there
                     (hbv.py:550-567) and the package follows Hbv_2 too.
  * BFI / outputs    hbv.py:555-596, hbv_1_1p.py:600, hbv_2.py:628-668.
  * states           final storages for Hbv / Hbv_1_1p (hbv.py:356-359); the full series for Hbv_2
                     (hbv_2.py:571-575).  `states` in: the storages a cache_states caller carries into the next call
                     (hbv.py:321-324); default 0.001 everywhere (hbv.py:128-136).

Not restated (the tests never request them):
  * comprout with nmul > 1 or with muwts: the reference's grouped convolution is inconsistent there (the package
    refuses it).  comprout with nmul == 1 and no weights routes the one member, which is the mean path: accepted.
  * the module's extension of accepting muwts with T_total rows under a state warm-up: not in the reference.
  * initialize=True, graph=True, adjoint_checkpoint, check_finite, grad_buffer: package settings with no effect on
    the values (or, for initialize, returning states only).
"""
from __future__ import annotations

import importlib.util
import os

import torch

_spec = importlib.util.spec_from_file_location(
    "_hbv_torch_eager", os.path.join(os.path.dirname(os.path.abspath(__file__)), "hbv_torch_eager.py"))
_eager = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_eager)
gamma_uh, route = _eager.gamma_uh, _eager.route

# (name, lo, hi) in table order (hbv.py:88-101, hbv_1_1p.py:87-106, hbv_2.py:90-107)
BASE = [("parBETA", 1.0, 6.0), ("parFC", 50, 1000), ("parK0", 0.05, 0.9), ("parK1", 0.01, 0.5),
        ("parK2", 0.001, 0.2), ("parLP", 0.2, 1), ("parPERC", 0, 10), ("parUZL", 0, 100),
        ("parTT", -2.5, 2.5), ("parCFMAX", 0.5, 10), ("parCFR", 0, 0.1), ("parCWH", 0, 0.2)]
EXTRA = {"Hbv": [], "Hbv_1_1p": [("parBETAET", 0.3, 5), ("parC", 0, 1)],
         "Hbv_2": [("parBETAET", 0.3, 5), ("parC", 0, 1), ("parRT", 0, 20), ("parAC", 0, 2500)]}
ROUTE = [("route_a", 0, 2.9), ("route_b", 0, 6.5)]
MODELS = tuple(EXTRA)


def table(model: str, dynamic=()) -> list:
    """(name, lo, hi) of the model's physical parameters in table order; Hbv gains parBETAET iff it is dynamic."""
    t = BASE + EXTRA[model]
    if model == "Hbv" and "parBETAET" in dynamic:
        t = t + [("parBETAET", 0.3, 5)]
    return t


def drop_order(model: str, dynamic) -> list:
    """Names of the dynamic parameters in the order the reference draws their drop masks: table order for Hbv /
    Hbv_1_1p (hbv.py:236-246), config-list order for Hbv_2 (hbv_2.py:254-258)."""
    if model == "Hbv_2":
        return list(dynamic)
    return [n for n, _, _ in table(model, dynamic) if n in dynamic]


def drop_masks(model: str, dynamic, B: int, dy_drop: float) -> dict:
    """name -> [B] 0/1 float mask of one forward call, drawn from the global CPU generator as the module draws them
    (one Bernoulli(dy_drop) value per basin and dynamic parameter, also when dy_drop == 0)."""
    names = drop_order(model, dynamic)
    if not names:
        return {}
    m = torch.bernoulli(torch.full((len(names), B), float(dy_drop)))
    return {n: m[k] for k, n in enumerate(names)}


def _rescale(u, lo, hi):
    return u * (hi - lo) + lo


def _step_params(model, unit_dyn, unit_sta, dynamic, masks, T):
    """Descaled per-day parameters: name -> [T,B,M].  unit_dyn: name -> [T,B,M] in [0,1] (dynamic ones);
    unit_sta: name -> [B,M] in [0,1] (every parameter's static value)."""
    par = {}
    for name, lo, hi in table(model, dynamic):
        sta = unit_sta[name]
        if name in dynamic:
            dyn = unit_dyn[name]
            m = masks.get(name)
            if m is not None:
                m = m.to(dyn.dtype).view(1, -1, 1)
                dyn = dyn * (1 - m) + sta.unsqueeze(0) * m
            par[name] = _rescale(dyn, lo, hi)
        else:
            par[name] = _rescale(sta, lo, hi).unsqueeze(0).expand(T, *sta.shape)
    return par


def _pbm(model, P, Tm, PET, par, states, nearzero, ac=None, elev=None):
    """The daily recurrence over T days.  P / Tm / PET: [T,B] forcing series; par: name -> [T,B,M]; states: the five
    storages [B,M].  Returns (series name -> [T,B,M], states after the last day, the states series or None)."""
    SP, MW, SM, SUZ, SLZ = states
    T = P.shape[0]
    names = ["Qsim", "Q0", "Q1", "Q2", "AET", "SWE", "recharge", "excs", "evapfactor", "tosoil", "PERC", "capillary"]
    rows = {k: [] for k in names}
    series = [] if model == "Hbv_2" else None
    for t in range(T):
        p = {k: v[t] for k, v in par.items()}
        Pt, Tt, Et = P[t].unsqueeze(-1), Tm[t].unsqueeze(-1), PET[t].unsqueeze(-1)
        tt = p["parTT"]
        if model == "Hbv_2":                                             # hbv_2.py:469-471
            hi = (elev >= 2000).to(Pt.dtype).unsqueeze(-1)
            tt = hi * 4.0 + (1 - hi) * tt
        rain = Pt * (Tt >= tt).to(Pt.dtype)
        snow = Pt * (Tt < tt).to(Pt.dtype)
        # snow (hbv.py:440-466)
        SP = SP + snow
        melt = torch.min(torch.clamp(p["parCFMAX"] * (Tt - tt), min=0.0), SP)
        MW = MW + melt
        SP = SP - melt
        refr = torch.min(torch.clamp(p["parCFR"] * p["parCFMAX"] * (tt - Tt), min=0.0), MW)
        SP = SP + refr
        MW = MW - refr
        tosoil = torch.clamp(MW - p["parCWH"] * SP, min=0.0)
        MW = MW - tosoil
        # soil and evaporation (hbv.py:468-480, hbv_1_1p.py:472-479)
        wet = torch.clamp((SM / p["parFC"]) ** p["parBETA"], min=0.0, max=1.0)
        rech = (rain + tosoil) * wet
        SM = SM + rain + tosoil - rech
        exc = torch.clamp(SM - p["parFC"], min=0.0)
        SM = SM - exc
        ef = SM / (p["parLP"] * p["parFC"])
        if "parBETAET" in p:
            ef = ef ** p["parBETAET"]
        ef = torch.clamp(ef, min=0.0, max=1.0)
        et = torch.min(SM, Et * ef)
        SM = torch.clamp(SM - et, min=nearzero)
        # capillary rise (hbv_1_1p.py:481-490, hbv_2.py:518-527)
        if model != "Hbv":
            cap = torch.min(SLZ, p["parC"] * SLZ * (1.0 - torch.clamp(SM / p["parFC"], max=1.0)))
            SM = torch.clamp(SM + cap, min=nearzero)
            SLZ = torch.clamp(SLZ - cap, min=nearzero)
        else:
            cap = None
        # groundwater (hbv.py:482-492, hbv_2.py:529-546)
        SUZ = SUZ + rech + exc
        perc = torch.min(SUZ, p["parPERC"])
        SUZ = SUZ - perc
        q0 = p["parK0"] * torch.clamp(SUZ - p["parUZL"], min=0.0)
        SUZ = SUZ - q0
        q1 = p["parK1"] * SUZ
        SUZ = SUZ - q1
        SLZ = SLZ + perc
        if model == "Hbv_2":
            a = ac.unsqueeze(-1)
            low = (a < 2500).to(a.dtype)
            lf = (torch.clamp((a - p["parAC"]) / 1000, min=-1, max=1) * p["parRT"] * low
                  + torch.exp(torch.clamp(-(a - 2500) / 50, min=-10.0, max=0.0)) * p["parRT"] * (1 - low))
            SLZ = torch.clamp(SLZ + lf, min=0.0)
        q2 = p["parK2"] * SLZ
        SLZ = SLZ - q2
        for k, v in zip(names, (q0 + q1 + q2, q0, q1, q2, et, SP, rech, exc, ef, tosoil, perc, cap)):
            if v is not None:
                rows[k].append(v)
        if series is not None:
            series.append((SP, MW, SM, SUZ, SLZ))
    out = {k: torch.stack(v) for k, v in rows.items() if v}
    ser = None if series is None else tuple(torch.stack([s[i] for s in series]) for i in range(5))
    return out, (SP, MW, SM, SUZ, SLZ), ser


def run(model: str, x_phy, parameters, *, nmul: int = 1, dynamic=(), warm_up: int = 0, warm_up_states: bool = True,
        masks=None, variables=("prcp", "tmean", "pet"), routing=None, comprout: bool = False, nearzero: float = 1e-5,
        muwts=None, ac_all=None, elev_all=None, states=None, aux=None) -> tuple:
    """One forward call of `model` ("Hbv", "Hbv_1_1p" or "Hbv_2") as the reference module runs it.

    x_phy [T,B,3] in `variables` order; parameters: raw [T,B,ny] (Hbv, Hbv_1_1p) or the tuple (p_dyn [T,B,n_dy*M],
    p_sta [B,n_st*M(+2)]) in [0,1] (Hbv_2); masks: dynamic name -> [B] drop mask (None: nothing dropped); muwts
    broadcastable to [T',B,M] (T' = the simulated days after a state warm-up); states: five [B,M] storages or None.
    Every tensor is used in its own dtype and on its own device.  `aux` (a dict, optional) receives "bfi_sums":
    (sum over days of the routed Q2, of the routed Qs + nearzero), BFI's numerator and denominator.  Returns (flux dict as the module returns it,
    states: the five final [B,M] storages, or for Hbv_2 the five [T,B,M] series)."""
    if model not in MODELS:
        raise ValueError(f"not restated: {model}")
    M = nmul
    dynamic = tuple(dynamic)
    masks = masks or {}
    routing = (model != "Hbv_2") if routing is None else routing
    if comprout and (M != 1 or muwts is not None):
        raise ValueError("comprout is restated for nmul == 1 without muwts only")
    T_total, B = x_phy.shape[0], x_phy.shape[1]
    dt, dev = x_phy.dtype, x_phy.device
    tab = table(model, dynamic)
    n = len(tab)
    if model == "Hbv_2":
        p_dyn, p_sta = parameters
        stat = [nm for nm, _, _ in tab if nm not in dynamic]
        dview = p_dyn.reshape(T_total, B, len(dynamic), M)
        unit_dyn = {nm: dview[:, :, i, :] for i, nm in enumerate(dynamic)}
        unit_sta = {nm: dview[-1, :, i, :] for i, nm in enumerate(dynamic)}
        unit_sta.update({nm: p_sta[:, i * M:(i + 1) * M] for i, nm in enumerate(stat)})
        route_ab = p_sta[:, len(stat) * M:len(stat) * M + 2] if routing else None
    else:
        unit = torch.sigmoid(parameters[:, :, :n * M]).reshape(T_total, B, n, M)
        route_ab = torch.sigmoid(parameters[-1, :, n * M:n * M + 2]) if routing else None

    if states is None:
        states = tuple(torch.full((B, M), 0.001, dtype=dt, device=dev) for _ in range(5))
    ch = [list(variables).index(v) for v in ("prcp", "tmean", "pet")]

    def forcing(x):
        return x[:, :, ch[0]], x[:, :, ch[1]], x[:, :, ch[2]]

    w = warm_up if (warm_up_states and model != "Hbv_2") else 0
    cutoff = warm_up if (not warm_up_states and model != "Hbv_2") else 0
    if w > 0:                                                            # hbv.py:327-346
        # every parameter of the table static from row w-1 (parBETAET of Hbv too, when the table has it), under
        # no_grad like the reference: reverse mode stops here, forward mode does not
        with torch.no_grad():
            sta_w = {nm: unit[w - 1, :, i, :] for i, (nm, _, _) in enumerate(tab)}
            par_w = {nm: _rescale(sta_w[nm], lo, hi).unsqueeze(0).expand(w, B, M) for nm, lo, hi in tab}
            _, states, _ = _pbm(model, *forcing(x_phy[:w]), par_w, states, nearzero, ac_all, elev_all)
    T = T_total - w
    if model != "Hbv_2":
        unit_dyn = {nm: unit[w:, :, i, :] for i, (nm, _, _) in enumerate(tab) if nm in dynamic}
        unit_sta = {nm: unit[-1, :, i, :] for i, (nm, _, _) in enumerate(tab)}
    par = _step_params(model, unit_dyn, unit_sta, dynamic, masks, T)
    P, Tm, PET = forcing(x_phy[w:])
    s, st_out, st_ser = _pbm(model, P, Tm, PET, par, states, nearzero, ac_all, elev_all)

    mean = {k: v.mean(-1) for k, v in s.items()}
    qsim = mean["Qsim"] if muwts is None else (s["Qsim"] * muwts).sum(-1)      # hbv.py:507-511
    if routing:
        ra = _rescale(route_ab[:, 0], ROUTE[0][1], ROUTE[0][2])
        rb = _rescale(route_ab[:, 1], ROUTE[1][1], ROUTE[1][2])
        with torch.device(dev):
            uh = gamma_uh(ra, rb, min(T, 15))
        qs, q0r, q1r, q2r = (route(v, uh) for v in (qsim, mean["Q0"], mean["Q1"], mean["Q2"]))
    else:
        qs, q0r, q1r, q2r = qsim, mean["Q0"], mean["Q1"], mean["Q2"]
    col = lambda v: v.unsqueeze(-1)  # noqa: E731
    out = {"streamflow": col(qs), "srflow": col(q0r), "ssflow": col(q1r), "gwflow": col(q2r),
           "AET_hydro": col(mean["AET"]), "PET_hydro": col(PET), "SWE": col(mean["SWE"]),
           "streamflow_no_rout": col(qsim), "srflow_no_rout": col(mean["Q0"]), "ssflow_no_rout": col(mean["Q1"]),
           "gwflow_no_rout": col(mean["Q2"]), "recharge": col(mean["recharge"]), "excs": col(mean["excs"]),
           "evapfactor": col(mean["evapfactor"]), "tosoil": col(mean["tosoil"]), "percolation": col(mean["PERC"])}
    if model != "Hbv":
        out["capillary"] = col(mean["capillary"])
    out["BFI"] = 100 * q2r.sum(0) / (qs.sum(0) + nearzero)
    if aux is not None:
        aux["bfi_sums"] = (q2r.sum(0), qs.sum(0) + nearzero)
    if cutoff:
        out = {k: (v if k == "BFI" else v[cutoff:]) for k, v in out.items()}
    return out, (st_ser if model == "Hbv_2" else st_out)
