"""Dtype-agnostic pure-torch restatement of the reference's daily HBV models Hbv, Hbv_1_1p and Hbv_2 and of the hourly
model Hbv_2_hourly (second half of this file: `run_hourly`, `pbm_hourly`, `gage_route`) with their module-level
orchestration.  TEST INFRASTRUCTURE ONLY (tests/ and tools/ import it; the product never does).

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


# the branches `_pbm` records on request (name -> [T,B,M] bool): every model's, the capillary models', Hbv_2's
DAILY_EVENTS = ("rain", "snow", "melt_pack_limited", "melt_potential", "refr_mw_limited", "refr_potential", "tosoil",
                "wet_clamped", "excs", "ef_clamped", "et_sm_limited", "et_pet_limited", "sm_floor", "perc_suz", "perc_par",
                "Q0")
CAP_EVENTS = ("cap_slz_limited", "cap_unlimited", "sm_floor_cap", "slz_floor")
HBV2_EVENTS = ("elev_hi", "elev_lo", "ac_lo", "ac_hi", "ac_clamp_hi", "ac_clamp_lo", "ac_free", "exp_clamped", "exp_free",
               "slz_lf_clamped")


def table(model: str, dynamic=()) -> list:
    """(name, lo, hi) of the model's physical parameters in table order; Hbv gains parBETAET iff it is dynamic."""
    t = BASE + EXTRA[model]
    if model == "Hbv" and "parBETAET" in dynamic:
        t = t + [("parBETAET", 0.3, 5)]
    return t


def drop_order(model: str, dynamic) -> list:
    """Names of the dynamic parameters in the order the reference draws their drop masks: table order for Hbv /
    Hbv_1_1p (hbv.py:236-246), config-list order for Hbv_2 and Hbv_2_hourly (hbv_2.py:254-258)."""
    if model in ("Hbv_2", "Hbv_2_hourly"):                              # (hbv_2_hourly.py:283-288: the same loop)
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


def _pbm(model, P, Tm, PET, par, states, nearzero, ac=None, elev=None, events=None, want_series=False):
    """The daily recurrence over T days.  P / Tm / PET: [T,B] forcing series; par: name -> [T,B,M]; states: the five
    storages [B,M].  Returns (series name -> [T,B,M], states after the last day, the states series or None: Hbv_2's
    always, every model's with `want_series`).  `events` (a dict, optional) receives name -> [T,B,M] bool tensors of
    the branches taken (DAILY_EVENTS; for Hbv_2 also HBV2_EVENTS) and the snowpack before and after the melt;
    recording changes no value."""
    SP, MW, SM, SUZ, SLZ = states
    T = P.shape[0]
    names = ["Qsim", "Q0", "Q1", "Q2", "AET", "SWE", "recharge", "excs", "evapfactor", "tosoil", "PERC", "capillary"]
    rows = {k: [] for k in names}
    series = [] if (model == "Hbv_2" or want_series) else None
    ev = {} if events is not None else None

    def mark(k, v):
        if ev is not None:
            ev.setdefault(k, []).append(v.detach())

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
        if ev is not None:
            full = torch.ones_like(SP, dtype=torch.bool)
            pot, rpot = p["parCFMAX"] * (Tt - tt), p["parCFR"] * p["parCFMAX"] * (tt - Tt)
            mark("rain", ((Tt >= tt) & (Pt > 0)) & full); mark("snow", ((Tt < tt) & (Pt > 0)) & full)
            mark("melt_pack_limited", (pot > 0) & (SP < pot) & (SP > 0)); mark("melt_potential", (pot > 0) & (SP >= pot))
            mark("SP_before", SP)
        melt = torch.min(torch.clamp(p["parCFMAX"] * (Tt - tt), min=0.0), SP)
        MW = MW + melt
        SP = SP - melt
        if ev is not None:
            mark("refr_mw_limited", (rpot > 0) & (MW < rpot) & (MW > 0)); mark("refr_potential", (rpot > 0) & (MW >= rpot))
            mark("SP_after", SP)
        refr = torch.min(torch.clamp(p["parCFR"] * p["parCFMAX"] * (tt - Tt), min=0.0), MW)
        SP = SP + refr
        MW = MW - refr
        tosoil = torch.clamp(MW - p["parCWH"] * SP, min=0.0)
        MW = MW - tosoil
        if ev is not None:
            mark("tosoil", tosoil > 0); mark("wet_clamped", (SM / p["parFC"]) ** p["parBETA"] > 1.0)
        # soil and evaporation (hbv.py:468-480, hbv_1_1p.py:472-479)
        wet = torch.clamp((SM / p["parFC"]) ** p["parBETA"], min=0.0, max=1.0)
        rech = (rain + tosoil) * wet
        SM = SM + rain + tosoil - rech
        exc = torch.clamp(SM - p["parFC"], min=0.0)
        SM = SM - exc
        ef = SM / (p["parLP"] * p["parFC"])
        if "parBETAET" in p:
            ef = ef ** p["parBETAET"]
        if ev is not None:
            mark("excs", exc > 0); mark("ef_clamped", ef > 1.0)
        ef = torch.clamp(ef, min=0.0, max=1.0)
        et = torch.min(SM, Et * ef)
        if ev is not None:
            mark("et_sm_limited", (SM < Et * ef) & (Et > 0)); mark("et_pet_limited", (SM >= Et * ef) & (Et > 0))
            mark("sm_floor", SM - et < nearzero)
        SM = torch.clamp(SM - et, min=nearzero)
        # capillary rise (hbv_1_1p.py:481-490, hbv_2.py:518-527)
        if model != "Hbv":
            capp = p["parC"] * SLZ * (1.0 - torch.clamp(SM / p["parFC"], max=1.0))
            cap = torch.min(SLZ, capp)
            if ev is not None:
                mark("cap_slz_limited", SLZ < capp); mark("cap_unlimited", (SLZ >= capp) & (capp > 0))
                mark("sm_floor_cap", SM + cap < nearzero); mark("slz_floor", SLZ - cap < nearzero)
            SM = torch.clamp(SM + cap, min=nearzero)
            SLZ = torch.clamp(SLZ - cap, min=nearzero)
        else:
            cap = None
        # groundwater (hbv.py:482-492, hbv_2.py:529-546)
        SUZ = SUZ + rech + exc
        if ev is not None:
            mark("perc_suz", SUZ < p["parPERC"]); mark("perc_par", SUZ >= p["parPERC"])
        perc = torch.min(SUZ, p["parPERC"])
        SUZ = SUZ - perc
        q0 = p["parK0"] * torch.clamp(SUZ - p["parUZL"], min=0.0)
        SUZ = SUZ - q0
        q1 = p["parK1"] * SUZ
        SUZ = SUZ - q1
        SLZ = SLZ + perc
        if ev is not None:
            mark("Q0", q0 > 0)
        if model == "Hbv_2":
            a = ac.unsqueeze(-1)
            low = (a < 2500).to(a.dtype)
            lf = (torch.clamp((a - p["parAC"]) / 1000, min=-1, max=1) * p["parRT"] * low
                  + torch.exp(torch.clamp(-(a - 2500) / 50, min=-10.0, max=0.0)) * p["parRT"] * (1 - low))
            if ev is not None:
                full = torch.ones_like(SLZ, dtype=torch.bool)
                d = (a - p["parAC"]) / 1000
                mark("elev_hi", (elev.unsqueeze(-1) >= 2000) & full); mark("elev_lo", (elev.unsqueeze(-1) < 2000) & full)
                mark("ac_lo", (a < 2500) & full); mark("ac_hi", (a >= 2500) & full)
                mark("ac_clamp_hi", (a < 2500) & (d > 1)); mark("ac_clamp_lo", (a < 2500) & (d < -1))
                mark("ac_free", (a < 2500) & (d >= -1) & (d <= 1))
                mark("exp_clamped", (a >= 2500) & (-(a - 2500) / 50 < -10.0)); mark("exp_free", (a >= 2500) & (-(a - 2500) / 50 >= -10.0))
                mark("slz_lf_clamped", SLZ + lf < 0.0)
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
    if events is not None:
        events.update({k: torch.stack(v) for k, v in ev.items()})
    return out, (SP, MW, SM, SUZ, SLZ), ser


def run(model: str, x_phy, parameters, *, nmul: int = 1, dynamic=(), warm_up: int = 0, warm_up_states: bool = True,
        masks=None, variables=("prcp", "tmean", "pet"), routing=None, comprout: bool = False, nearzero: float = 1e-5,
        muwts=None, ac_all=None, elev_all=None, states=None, aux=None, events=None) -> tuple:
    """One forward call of `model` ("Hbv", "Hbv_1_1p" or "Hbv_2") as the reference module runs it.

    x_phy [T,B,3] in `variables` order; parameters: raw [T,B,ny] (Hbv, Hbv_1_1p) or the tuple (p_dyn [T,B,n_dy*M],
    p_sta [B,n_st*M(+2)]) in [0,1] (Hbv_2); masks: dynamic name -> [B] drop mask (None: nothing dropped); muwts
    broadcastable to [T',B,M] (T' = the simulated days after a state warm-up); states: five [B,M] storages or None.
    Every tensor is used in its own dtype and on its own device.  `aux` (a dict, optional) receives "bfi_sums":
    (sum over days of the routed Q2, of the routed Qs + nearzero), BFI's numerator and denominator; `events`: see `_pbm`
    (the days after a state warm-up).  Returns (flux dict as the module returns it,
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
    s, st_out, st_ser = _pbm(model, P, Tm, PET, par, states, nearzero, ac_all, elev_all, events)

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


# ---------------------------------------------------------------------------------------------------------------------
# Hbv_2_hourly (models/hbv/hbv_2_hourly.py): HBV 2.0 in rate form with dt = 1/24 day.
#   * parameter table   19 parameters (hbv_2_hourly.py:91-115); parF0's bounds are (5/dt, 120/dt) = (120, 2880) mm/d.
#                       Tuple parameters (p_dyn, p_sta, p_distr) without sigmoid; dynamic ones in the ORDER OF THE
#                       CONFIG LIST, one drop mask each drawn in that order (:277-295); static ones in table order,
#                       the two per-unit routing columns after them (:229-256).
#   * recurrence        :527-675 -- guard rails at the top of every step (:529-533), P and PET divided by dt first
#                       (:485-487), every `/ dt` and `* dt` where the reference has it, Hortonian infiltration excess
#                       (:575-595), Qsim = Q0 + Q1 + Q2 + IE (:652).
#   * ensemble          mean, or the muwts-weighted sum of Qsim (:678-681).
#   * per-unit routing  optional, 72 taps (:684-700, lenF :45); `Qs * dt` (:741); pred_cutoff (:761-764).
#   * gage routing      lagged-UH, area-weighted, per (gage, unit) pair (:800-897): `gage_route`.
#   * states            the five [T,B,M] series (:670-675,725); initial storages as an argument (the storages a
#                       cache_states caller carries in, :424-427), default 0.001 (:152-160).
HOURLY = BASE + EXTRA["Hbv_2"] + [("parF0", 5.0 * 24, 120.0 * 24), ("parFMIN", 0.0, 1.0), ("parALPHA", 0.5, 5.0)]
HOURLY_ROUTE = [("route_a", 0, 5.0), ("route_b", 0, 12.0)]                      # :116-119
HOURLY_DISTR = [("route_a", 0, 5.0), ("route_b", 0, 12.0), ("route_tau", 0, 48.0)]   # :120-124
HOURLY_LENF = 72                                                                 # :45
HOURLY_SERIES = ["Qsim", "Q0", "Q1", "Q2", "AET", "SWE", "recharge", "excs", "evapfactor", "tosoil", "PERC", "capillary"]


def pbm_hourly(P, Tm, PET, par, states, nearzero, ac, elev, events=None):
    """The hourly recurrence (hbv_2_hourly.py:527-675).  P / Tm / PET: [T,B] forcing as given (depth per step);
    par: name -> [T,B,M] or [B,M] (static); states: the five storages [B,M] entering hour 0; ac / elev [B].
    Returns (series name -> [T,B,M] in HOURLY_SERIES order -- rates per day, as the loop stores them --, the five state
    series [T,B,M]).  `events` (a dict, optional) receives name -> [T,B,M] bool tensors of the branches taken."""
    dt = 1.0 / 24                                                        # :58
    SP, MW, SM, SUZ, SLZ = states
    T = P.shape[0]
    Pr, PETr = P / dt, PET / dt                                          # :485-487
    Ac, El = ac.unsqueeze(-1), elev.unsqueeze(-1)
    hi = (El >= 2000).to(P.dtype)
    lo = (El < 2000).to(P.dtype)
    rows = {k: [] for k in HOURLY_SERIES}
    ser = [[] for _ in range(5)]
    ev = {} if events is not None else None

    def mark(k, v):
        if ev is not None:
            ev.setdefault(k, []).append(v.detach() if torch.is_tensor(v) else v)

    for t in range(T):
        p = {k: (v[t] if v.dim() == 3 else v) for k, v in par.items()}
        if ev is not None:
            mark("rail", (SP < 0) | (MW < 0) | (SM < nearzero) | (SUZ < nearzero) | (SLZ < nearzero))
        SP = torch.clamp(SP, min=0.0)                                    # :529-533
        MW = torch.clamp(MW, min=0.0)
        SM = torch.clamp(SM, min=nearzero)
        SUZ = torch.clamp(SUZ, min=nearzero)
        SLZ = torch.clamp(SLZ, min=nearzero)
        Pt, Tt, Et = Pr[t].unsqueeze(-1), Tm[t].unsqueeze(-1), PETr[t].unsqueeze(-1)
        tt = hi * 4.0 + lo * p["parTT"]                                  # :544-546
        rain = Pt * (Tt >= tt).to(Pt.dtype)
        snow = Pt * (Tt < tt).to(Pt.dtype)
        # snow (:551-572)
        SP = SP + snow * dt
        SP_before = SP
        melt = torch.clamp(p["parCFMAX"] * (Tt - tt), min=0.0)
        melt = torch.min(melt * dt, SP)
        MW = MW + melt
        SP = SP - melt
        refr = torch.clamp(p["parCFR"] * p["parCFMAX"] * (tt - Tt), min=0.0)
        refr = torch.min(refr * dt, MW)
        SP = SP + refr
        MW = MW - refr
        tosoil = torch.clamp((MW - p["parCWH"] * SP) / dt, min=0.0)
        MW = MW - tosoil * dt
        # Hortonian infiltration excess (:577-595)
        W = rain + tosoil
        r = SM / p["parFC"]
        s = torch.clamp(r, 0.0, 1.0 - 0.01)
        fmin = p["parFMIN"] * p["parF0"]
        fcap = fmin + (p["parF0"] - fmin) * torch.pow(1.0 - s, p["parALPHA"])
        infil = torch.minimum(W, fcap)
        IE = torch.clamp(W - fcap, min=0.0)
        wet = torch.clamp(r ** p["parBETA"], 0.0, 1.0)
        rech = infil * wet
        SM = SM + (infil - rech) * dt
        # excess, evaporation (:603-613)
        exc = torch.clamp((SM - p["parFC"]) / dt, min=0.0)
        SM = SM - exc * dt
        ef0 = (SM / (p["parLP"] * p["parFC"])) ** p["parBETAET"]
        ef = torch.clamp(ef0, min=0.0, max=1.0)
        pet_dt = Et * ef * dt
        et = torch.min(SM, pet_dt) / dt
        if ev is not None:
            mark("IE", IE > 0); mark("excess", exc > 0); mark("s_clamped", r > 1.0 - 0.01)
            mark("ef_clamped", ef0 > 1.0); mark("et_sm_limited", (SM < pet_dt) & (Et > 0))
            mark("et_pet_limited", (SM >= pet_dt) & (Et > 0)); mark("refreeze", refr > 0)
            mark("SP_before", SP_before); mark("SP_after", SP)
        SM = torch.clamp(SM - et * dt, min=nearzero)
        # capillary rise (:616-628)
        capp = p["parC"] * SLZ * (1.0 - torch.clamp(SM / p["parFC"], max=1.0)) * dt
        cap = torch.min(SLZ, capp) / dt
        if ev is not None:
            mark("cap_slz_limited", SLZ < capp); mark("cap_unlimited", (SLZ >= capp) & (capp > 0))
        SM = torch.clamp(SM + cap * dt, min=nearzero)
        SLZ = torch.clamp(SLZ - cap * dt, min=nearzero)
        # groundwater boxes (:631-648)
        SUZ = SUZ + (rech + exc) * dt
        perc = torch.min(SUZ, p["parPERC"] * dt) / dt
        SUZ = SUZ - perc * dt
        q0 = p["parK0"] * torch.clamp(SUZ - p["parUZL"], min=0.0)
        SUZ = SUZ - q0 * dt
        q1 = p["parK1"] * SUZ
        SUZ = SUZ - q1 * dt
        SLZ = SLZ + perc * dt
        lf = (torch.clamp((Ac - p["parAC"]) / 1000, min=-1, max=1) * p["parRT"] * (Ac < 2500)
              + torch.exp(torch.clamp(-(Ac - 2500) / 50, min=-10.0, max=0.0)) * p["parRT"] * (Ac >= 2500))
        SLZ = torch.clamp(SLZ + lf * dt, min=0.0)
        q2 = p["parK2"] * SLZ
        SLZ = SLZ - q2 * dt
        if ev is not None:
            mark("Q0", q0 > 0)
        for k, v in zip(HOURLY_SERIES, (q0 + q1 + q2 + IE, q0, q1, q2, et, SP, rech, exc, ef, tosoil, perc, cap)):
            rows[k].append(v)
        for i, v in enumerate((SP, MW, SM, SUZ, SLZ)):
            ser[i].append(v)
    if events is not None:
        events.update({k: torch.stack(v) for k, v in ev.items()})
    return {k: torch.stack(v) for k, v in rows.items()}, tuple(torch.stack(v) for v in ser)


def hourly_uh(a, b, length, tau=None):
    """uh_gamma (core/calc/uh_routing.py:5-22) of `length` taps for a / b [n], then, with `tau` [n], the fractional
    shift _frac_shift1d (hbv_2_hourly.py:857-897).  Returns [length, n]."""
    dt = a.dtype
    aa, theta = torch.relu(a) + 0.1, torch.relu(b) + 0.5
    t = torch.arange(0.5, length * 1.0, dtype=dt, device=a.device).unsqueeze(1)
    w = 1 / (aa.lgamma().exp() * theta ** aa) * t ** (aa - 1) * torch.exp(-t / theta)
    w = w / w.sum(0)
    if tau is not None:
        L = length
        k = torch.floor(tau).unsqueeze(0)
        f = tau.unsqueeze(0) - k
        tt = torch.arange(L, dtype=dt, device=a.device).unsqueeze(1)
        i0, i1 = tt - k, tt - (k + 1)
        w0 = torch.gather(w, 0, i0.clamp(0, L - 1).long()) * ((i0 >= 0) & (i0 <= L - 1)).to(dt)
        w1 = torch.gather(w, 0, i1.clamp(0, L - 1).long()) * ((i1 >= 0) & (i1 <= L - 1)).to(dt)
        w = (1.0 - f) * w0 + f * w1
    return w


def gage_route(qs, dp, topo, areas, lag_uh=True, bounds=None):
    """distr_routing (hbv_2_hourly.py:800-855): unit runoff qs [T,U] -> gage streamflow [T,G].  dp [n_pairs,3] in
    [0,1] (route_a, route_b, route_tau), pairs in the row-major order of `topo == 1` [G,U]; areas [U]."""
    bounds = bounds or [(lo, hi) for _, lo, hi in HOURLY_DISTR]
    T = qs.shape[0]
    L = min(T, HOURLY_LENF)
    a, b, tau = (_rescale(dp[:, i], bounds[i][0], bounds[i][1]) for i in range(3))
    w = hourly_uh(a, b, L, tau if lag_uh else None)
    pairs = (topo == 1).nonzero()
    rows, cols = pairs[:, 0], pairs[:, 1]
    y = route((qs * areas[None, :])[:, cols], w)
    acc = torch.zeros((T, topo.shape[0]), dtype=qs.dtype, device=qs.device).index_add(1, rows, y)
    return acc / (topo * areas[None, :]).sum(1).clamp(min=1e-6)[None, :]


def run_hourly(x_phy, parameters, *, nmul: int = 1, dynamic=(), masks=None, variables=("prcp", "tmean", "pet"),
               routing: bool = False, nearzero: float = 1e-5, muwts=None, ac_all=None, elev_all=None,
               outlet_topo=None, areas=None, states=None, pred_cutoff: int = 0, warm_up_states: bool = True,
               cache_states: bool = False, events=None) -> tuple:
    """One forward call of Hbv_2_hourly as the reference module runs it (hbv_2_hourly.py:376-798; `cache_states`: the
    first such call after load_states(`states`)).  parameters: (p_dyn [T,B,n_dy*M], p_sta
    [B,n_st*M(+2)], p_distr [n_pairs,3]) in [0,1].  Returns ({"Qs": [T,B,1], "streamflow": [T,G,1]}, the five
    [T,B,M] state series).  `pred_cutoff` is the module attribute of that name (0: no config key sets it, :39)."""
    M = nmul
    dynamic = tuple(dynamic)
    masks = masks or {}
    T, B = x_phy.shape[0], x_phy.shape[1]
    dt_, dev = x_phy.dtype, x_phy.device
    p_dyn, p_sta, p_distr = parameters
    stat = [nm for nm, _, _ in HOURLY if nm not in dynamic]
    dview = p_dyn.reshape(T, B, len(dynamic), M)
    par = {}
    for nm, lo, hi in HOURLY:
        if nm in dynamic:
            i = dynamic.index(nm)
            dyn, sta = dview[:, :, i, :], dview[-1, :, i, :]
            m = masks.get(nm)
            if m is not None:
                m = m.to(dt_).view(1, -1, 1)
                dyn = dyn * (1 - m) + sta.unsqueeze(0) * m                # :285-290
            par[nm] = _rescale(dyn, lo, hi)
        else:
            i = stat.index(nm)
            par[nm] = _rescale(p_sta[:, i * M:(i + 1) * M], lo, hi)
    if states is None:
        states = tuple(torch.full((B, M), 0.001, dtype=dt_, device=dev) for _ in range(5))
    ch = [list(variables).index(v) for v in ("prcp", "tmean", "pet")]
    s, ser = pbm_hourly(x_phy[:, :, ch[0]], x_phy[:, :, ch[1]], x_phy[:, :, ch[2]], par, states, nearzero,
                        ac_all, elev_all, events)
    qsim = s["Qsim"].mean(-1) if muwts is None else (s["Qsim"] * muwts).sum(-1)  # :678-681
    if routing:                                                                   # :684-700
        ab = p_sta[:, len(stat) * M:len(stat) * M + 2]
        uh = hourly_uh(_rescale(ab[:, 0], *HOURLY_ROUTE[0][1:]), _rescale(ab[:, 1], *HOURLY_ROUTE[1][1:]),
                       min(T, HOURLY_LENF))
        qsim = route(qsim, uh)
    qs = qsim * (1.0 / 24)                                                        # :741
    out = {"Qs": qs.unsqueeze(-1)}
    if not warm_up_states:                                                        # :761-764 (pred_cutoff)
        out["Qs"] = out["Qs"][pred_cutoff:]
    # :766-796 -- a cache_states call routes its DETACHED history (here: this call alone, the first one after
    # load_states) and returns the last row only
    routed = gage_route(qs.detach() if cache_states else qs, p_distr, outlet_topo, areas).unsqueeze(-1)
    out["streamflow"] = routed[-1:] if cache_states else routed
    return out, ser
