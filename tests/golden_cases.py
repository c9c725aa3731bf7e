"""Golden-case catalogue shared by tests/golden/make_golden.py and the tests.

A case names a reference model class, its config, the synthetic input recipe
(tests/synth.py) and the scalar loss whose gradient is recorded.  The
generator runs the *reference* on these inputs (authoring container only) and
stores outputs + gradients in tests/golden/<name>.npz; the tests rebuild the
same inputs bit-for-bit and compare the oracle / the HIP path against the
stored arrays.  (SURVEY.md §8c lists the cases this catalogue covers.)
"""
from __future__ import annotations

import numpy as np

from . import synth

PHY_NAMES = {
    "Hbv": ["parBETA", "parFC", "parK0", "parK1", "parK2", "parLP", "parPERC",
            "parUZL", "parTT", "parCFMAX", "parCFR", "parCWH"],
    "Hbv_1_1p": ["parBETA", "parFC", "parK0", "parK1", "parK2", "parLP", "parPERC",
                 "parUZL", "parTT", "parCFMAX", "parCFR", "parCWH", "parBETAET", "parC"],
    "Hbv_2": ["parBETA", "parFC", "parK0", "parK1", "parK2", "parLP", "parPERC",
              "parUZL", "parTT", "parCFMAX", "parCFR", "parCWH", "parBETAET", "parC",
              "parRT", "parAC"],
    "Hbv_2_hourly": ["parBETA", "parFC", "parK0", "parK1", "parK2", "parLP", "parPERC",
                     "parUZL", "parTT", "parCFMAX", "parCFR", "parCWH", "parBETAET", "parC",
                     "parRT", "parAC", "parF0", "parFMIN", "parALPHA"],
}


def _cfg(cls, nmul=1, dyn=(), **kw):
    c = {"nmul": nmul, "dynamic_params": {cls: list(dyn)}}
    c.update(kw)
    return c


# name -> spec.  T/B are kept small: the fixtures are committed.
CASES = {
    # BASELINE config 1 exactly: Hbv(None), 10 basins x 365 d x 1 member, forward only.
    "cfg1_hbv_default": dict(model="Hbv", config=None, T=365, B=10, seed=11, loss="none"),
    # static parameters, 16 members, every flux key in the loss.
    "hbv_static_m16": dict(model="Hbv", config=_cfg("Hbv", 16), T=96, B=6, seed=12, loss="all"),
    "hbv_static_m16_sf": dict(model="Hbv", config=_cfg("Hbv", 16), T=96, B=6, seed=13,
                              loss="streamflow"),
    # warm-up variants.
    "hbv_warmup_states": dict(model="Hbv", config=_cfg("Hbv", 16, warm_up=30), T=96, B=6,
                              seed=14, loss="all"),
    "hbv_warmup_nostates": dict(model="Hbv",
                                config=_cfg("Hbv", 16, warm_up=30, warm_up_states=False),
                                T=96, B=6, seed=15, loss="all"),
    # dynamic parBETA + parBETAET (the common dMG setting, tests/config.yaml:48-49).
    "hbv_dyn2": dict(model="Hbv", config=_cfg("Hbv", 16, ("parBETA", "parBETAET"), warm_up=20),
                     T=80, B=5, seed=16, loss="all"),
    "hbv_dyn2_drop": dict(model="Hbv",
                          config=_cfg("Hbv", 16, ("parBETA", "parBETAET"), dy_drop=0.5),
                          T=64, B=12, seed=17, loss="all", torch_seed=1234),
    # non power-of-two ensemble, gradient w.r.t. the forcings too.
    "hbv_m3_xgrad": dict(model="Hbv", config=_cfg("Hbv", 3, ("parK0",)), T=64, B=7, seed=18,
                         loss="all", x_grad=True),
    # learned ensemble weights.
    "hbv_muwts": dict(model="Hbv", config=_cfg("Hbv", 4), T=64, B=5, seed=19, loss="all",
                      muwts=True),
    # weights with a state warm-up.  The reference multiplies muwts against the series of the
    # call at hand -- also in the warm-up call (hbv.py:497-511 runs before the `initialize`
    # return) -- so only shapes that broadcast over time ([B,nmul], [1,B,nmul]) run there.
    "hbv_muwts_warmup": dict(model="Hbv", config=_cfg("Hbv", 4, ("parBETA",), warm_up=12), T=60, B=5,
                             seed=32, loss="all", muwts="bcast"),
    # comprout=True (hbv.py:516-518,540-546): route every member, then average.  Self-consistent upstream for one member
    # only (the grouped convolution has `ngrid` groups): accepted here for nmul == 1, refused otherwise like the reference.
    # grad_atol_rel: a one-member "group" is a single column, and its smallest entries are sums over T with cancellation
    # -- in float64 (oracle/hbv_torch_eager.py) parK2's gradient of basin 2 is 0.00182629; the reference's float32 tape
    # gives 0.00182280 (-1.4e-5 of the column's largest entry, 0.241), the GPU 0.00182910 (+1.2e-5): both sides of the
    # truth, 2.6e-5 apart.  The stated 2e-6 of the group's largest holds for ensembles (every other fixture); here 2e-5.
    "hbv_comprout_m1": dict(model="Hbv", config=_cfg("Hbv", 1, ("parBETA",), comprout=True), T=64, B=6, seed=56,
                            loss="all", grad_atol_rel=2e-5),
    # cold dry start: melt = SNOWPACK = 0 ties, SM hitting FC, SUZ < PERC.
    "hbv_ties": dict(model="Hbv", config=_cfg("Hbv", 2), T=48, B=9, seed=20, loss="all",
                     cold=True, raw_scale=2.5),
    # forcing channels remapped.
    "hbv_variables": dict(model="Hbv", config=_cfg("Hbv", 2, variables=["tmean", "pet", "prcp"]),
                          T=40, B=4, seed=21, loss="streamflow"),
    # T' < 15 shortens the unit hydrograph.
    "hbv_short": dict(model="Hbv", config=_cfg("Hbv", 2), T=9, B=3, seed=22, loss="all"),
    # state continuation across two calls.
    "hbv_cache_states": dict(model="Hbv", config=_cfg("Hbv", 4, cache_states=True), T=60, B=4,
                             seed=23, loss="none", two_call=True),
    # HBV 1.1p, all 14 parameters dynamic (BASELINE config 3 shape).
    "hbv11p_dyn_all": dict(model="Hbv_1_1p",
                           config=_cfg("Hbv_1_1p", 16, PHY_NAMES["Hbv_1_1p"]), T=64, B=5,
                           seed=24, loss="all"),
    "hbv11p_static": dict(model="Hbv_1_1p", config=_cfg("Hbv_1_1p", 4, warm_up=10), T=72, B=6,
                          seed=25, loss="all", cold=True),
    # HBV 2.0 tuple parameters, elevation / area switches on both sides.
    "hbv2_dyn3": dict(model="Hbv_2",
                      config=_cfg("Hbv_2", 16, ("parBETA", "parK0", "parBETAET")), T=64, B=8,
                      seed=26, loss="all"),
    "hbv2_dyn3_routing": dict(model="Hbv_2",
                              config=_cfg("Hbv_2", 4, ("parBETA", "parK0", "parBETAET"),
                                          routing=True, dy_drop=0.3),
                              T=64, B=8, seed=27, loss="all", torch_seed=77),
    "hbv2_static": dict(model="Hbv_2", config=_cfg("Hbv_2", 2), T=48, B=6, seed=28, loss="all",
                        cold=True),
    # HBV 2.0 hourly: rate form with dt = 1/24, Hortonian infiltration,
    # lagged-UH gage routing; units -> gages through `outlet_topo`.
    "hourly_dyn3": dict(model="Hbv_2_hourly",
                        config=_cfg("Hbv_2_hourly", 4, ("parBETA", "parK0", "parBETAET")),
                        T=120, B=7, G=3, seed=29, loss="all"),
    "hourly_routing_drop": dict(model="Hbv_2_hourly",
                                config=_cfg("Hbv_2_hourly", 16, ("parBETA", "parF0"), routing=True,
                                            dy_drop=0.4),
                                T=100, B=6, G=2, seed=30, loss="all", torch_seed=5),
    "hourly_static_cold": dict(model="Hbv_2_hourly", config=_cfg("Hbv_2_hourly", 2), T=60, B=5, G=2,
                               seed=31, loss="all", cold=True),
    # --- long records (T >= 256) with a loss: the time-parallel adjoint (64-day chunks, T >= 128), the streaming
    # adjoint and the checkpointed adjoint meet the reference's own autograd tape, not only the oracle.
    "hbv_long_static": dict(model="Hbv", config=_cfg("Hbv", 16), T=400, B=6, seed=41, loss="all"),
    "hbv_long_dyn2": dict(model="Hbv", config=_cfg("Hbv", 16, ("parBETA", "parBETAET"), warm_up=40), T=400, B=6,
                          seed=42, loss="all"),
    "hbv_long_m4_xgrad": dict(model="Hbv", config=_cfg("Hbv", 4, ("parK0",)), T=300, B=9, seed=43, loss="all",
                              x_grad=True),
    "hbv11p_long_dyn_all": dict(model="Hbv_1_1p", config=_cfg("Hbv_1_1p", 16, PHY_NAMES["Hbv_1_1p"]), T=256, B=5,
                                seed=44, loss="all"),
    "hbv2_long_dyn3": dict(model="Hbv_2", config=_cfg("Hbv_2", 16, ("parBETA", "parK0", "parBETAET")), T=256, B=8,
                           seed=45, loss="all"),
    "hbv2_long_routing": dict(model="Hbv_2", config=_cfg("Hbv_2", 4, ("parBETA", "parBETAET"), routing=True), T=300,
                              B=7, seed=46, loss="streamflow"),
    # five dynamic parameters with dy_drop masks (the streaming kernels' six-slot run-time lists, the time-parallel
    # adjoint's generic mode); forcing channels in another order with one dynamic parameter (channel picks + slot list)
    "hbv_long_dyn5_drop": dict(model="Hbv", config=_cfg("Hbv", 16, ("parBETA", "parFC", "parK0", "parK1", "parLP"),
                                                         dy_drop=0.3), T=256, B=7, seed=51, loss="all", torch_seed=13),
    "hbv_long_variables": dict(model="Hbv", config=_cfg("Hbv", 8, ("parBETA",), variables=["tmean", "pet", "prcp"]),
                               T=300, B=5, seed=52, loss="streamflow"),
    # a capillary model with a short dynamic list (slot lists outside the compiled sets), HBV 2.0 all static from a cold
    # start, and the tie conventions (cold dry start, wide raw parameters) through the long adjoints
    "hbv11p_long_dyn2": dict(model="Hbv_1_1p", config=_cfg("Hbv_1_1p", 16, ("parBETA", "parC")), T=256, B=6, seed=53,
                             loss="all"),
    "hbv2_long_static_cold": dict(model="Hbv_2", config=_cfg("Hbv_2", 8), T=256, B=7, seed=54, loss="all", cold=True),
    "hbv_long_ties": dict(model="Hbv", config=_cfg("Hbv", 2), T=256, B=9, seed=55, loss="all", cold=True, raw_scale=2.5),
    # learned ensemble weights over a long record: the pipelined forward's staged weight row and the `MU` instances of the
    # time-parallel adjoint (static and slot-list modes) against hbv.py:508-511 taped
    "hbv_long_muwts": dict(model="Hbv", config=_cfg("Hbv", 16), T=300, B=6, seed=49, loss="all", muwts=True),
    "hbv_long_muwts_dyn2": dict(model="Hbv", config=_cfg("Hbv", 4, ("parBETA", "parBETAET")), T=256, B=9, seed=50,
                                loss="all", muwts=True),
    # the hourly model's production adjoints (hbv_2_hourly.py:527-675 taped): 300 hours, three dynamic parameters; and
    # with the lagged-UH gage routing, dy_drop and a 16-member ensemble
    "hourly_long_dyn3": dict(model="Hbv_2_hourly",
                             config=_cfg("Hbv_2_hourly", 4, ("parBETA", "parK0", "parBETAET")),
                             T=300, B=7, G=3, seed=47, loss="all"),
    "hourly_long_routing": dict(model="Hbv_2_hourly",
                                config=_cfg("Hbv_2_hourly", 16, ("parBETA", "parF0"), routing=True, dy_drop=0.3),
                                T=256, B=6, G=2, seed=48, loss="all", torch_seed=9),
    # --- the hourly model's wet regime: storages carried in wet (synth.wet_states, through load_states + cache_states,
    # hbv_2_hourly.py:424-427; `streamflow` is then the last row only, :792-794), hourly storm forcing
    # (synth.forcing_hourly), unit parameters spread towards the ends of their ranges, and the forcing gradient.  On
    # these the Hortonian excess (IE > 0), the soil excess and the fast-runoff box (Q0 > 0) are active in the
    # reference's own tape (tests/test_hourly_f64.py counts them).
    "hourly_wet_routing": dict(model="Hbv_2_hourly", config=_cfg("Hbv_2_hourly", 2, routing=True, cache_states=True),
                               T=240, B=8, G=3, seed=61, loss="all", x_grad=True, forcing="hourly", storm=6.0,
                               day0=100.25, wet_start=True, unit_spread=True),
    "hourly_wet_dyn3_drop": dict(model="Hbv_2_hourly",
                                 config=_cfg("Hbv_2_hourly", 16, ("parF0", "parBETA", "parK0"), dy_drop=0.3,
                                             cache_states=True),
                                 T=200, B=5, G=2, seed=62, loss="all", x_grad=True, torch_seed=21, forcing="hourly",
                                 storm=6.0, day0=130.25, wet_start=True, unit_spread=True),
    "hourly_wet_muwts": dict(model="Hbv_2_hourly", config=_cfg("Hbv_2_hourly", 4, ("parALPHA",), cache_states=True),
                             T=300, B=6, G=2, seed=63, loss="all", x_grad=True, muwts=True, forcing="hourly", storm=5.0,
                             day0=75.25, wet_start=True, unit_spread=True),
    # --- the daily models' wet regime: storages carried in wet (synth.wet_states through load_states + cache_states,
    # hbv.py:148-168,321-324), raw parameters spread over their ranges, a record from a spring day (day 120: PET > 0
    # while the carried-in soil is saturated) into late autumn, and the forcing gradient.  On these the soil excess, the
    # fast-runoff box (Q0 > 0), PERC = parPERC and evaporation limited by the soil moisture (the dry lanes of
    # wet_states) are active in the reference's own tape (tests/test_daily_f64.py counts them).
    "hbv_wet_dyn3": dict(model="Hbv", config=_cfg("Hbv", 4, ("parBETA", "parK0", "parBETAET"), cache_states=True),
                         T=200, B=6, seed=78, loss="all", x_grad=True, day0=120.0, wet_start=True, raw_scale=2.5),
    "hbv11p_wet_list_drop": dict(model="Hbv_1_1p",
                                 config=_cfg("Hbv_1_1p", 4, ("parK0", "parTT", "parFC", "parC"), dy_drop=0.3,
                                             cache_states=True),
                                 T=200, B=6, seed=84, loss="all", x_grad=True, torch_seed=31, day0=120.0, wet_start=True,
                                 raw_scale=2.0),
    "hbv2_wet_muwts_routing": dict(model="Hbv_2",
                                   config=_cfg("Hbv_2", 4, ("parBETA", "parK0", "parBETAET"), routing=True,
                                               cache_states=True),
                                   T=200, B=8, seed=90, loss="all", x_grad=True, muwts=True, day0=120.0, wet_start=True,
                                   unit_spread=True),
}

LONG_CASES = [n for n, c in CASES.items() if "_long_" in n]

# Randomly drawn cases (tests/test_live_reference.py): a fixed seed list, each seed one configuration -- model class,
# ensemble size, dynamic-parameter set, warm-up, dy_drop, routing, cold start, parameter spread.  The reference's
# outputs for every draw are stored in tests/golden/live_draws.npz (make_golden.py live).
LIVE_SEEDS = list(range(40))


def live_case(seed: int) -> dict:
    """Spec of draw `seed` (same form as a CASES entry)."""
    import random
    rng = random.Random(seed)
    model = rng.choice(["Hbv", "Hbv", "Hbv_1_1p", "Hbv_2", "Hbv_2_hourly"])
    names = list(PHY_NAMES[model]) + (["parBETAET"] if model == "Hbv" else [])
    mode = rng.choice(["static", "few", "few", "all"])
    dyn = [] if mode == "static" else (list(names) if mode == "all" else rng.sample(names, rng.randint(1, 3)))
    if model == "Hbv" and "parBETAET" not in dyn and rng.random() < 0.5:
        names.remove("parBETAET")
    dyn = tuple(n for n in names if n in dyn)
    kw = {}
    if model in ("Hbv", "Hbv_1_1p") and rng.random() < 0.4:
        kw["warm_up"] = rng.choice([5, 12])
        kw["warm_up_states"] = rng.random() < 0.7
    if dyn and rng.random() < 0.4:
        kw["dy_drop"] = 0.3
    if model in ("Hbv_2", "Hbv_2_hourly"):
        kw["routing"] = rng.random() < 0.5       # (routing=False on Hbv / Hbv_1_1p crashes upstream: hbv.py:550-567)
    spec = dict(model=model, config=_cfg(model, rng.choice([2, 3, 4, 16]), dyn, **kw),
                T=rng.choice([24, 40, 64]), B=rng.choice([3, 5, 7]), seed=1000 + seed, loss="all",
                torch_seed=seed, cold=rng.random() < 0.3, raw_scale=rng.choice([1.0, 1.0, 2.5]))
    if model == "Hbv_2_hourly":
        spec["G"] = rng.choice([2, 3])
        # a day or two of hours from a cold start moves no water: every gradient is a 1e-12 rounding residue.  Not a case
        spec["cold"] = False
        spec["T"] = max(spec["T"], 64)
    return spec

FLUX_KEYS_BASE = [
    "streamflow", "srflow", "ssflow", "gwflow", "AET_hydro", "PET_hydro", "SWE",
    "streamflow_no_rout", "srflow_no_rout", "ssflow_no_rout", "gwflow_no_rout",
    "recharge", "excs", "evapfactor", "tosoil", "percolation",
]


def flux_keys(model: str):
    if model == "Hbv_2_hourly":
        return ["Qs", "streamflow"]  # hbv_2_hourly.py:740-741,790-796
    keys = list(FLUX_KEYS_BASE)
    if model in ("Hbv_1_1p", "Hbv_2"):
        keys.append("capillary")
    keys.append("BFI")
    return keys


def n_phy(spec) -> int:
    model = spec["model"]
    n = len(PHY_NAMES[model])
    if model == "Hbv" and spec["config"] is not None:
        if "parBETAET" in spec["config"]["dynamic_params"].get("Hbv", []):
            n += 1
    return n


def build_inputs(name: str) -> dict:
    """All numpy inputs of a case (float32), bit-reproducible."""
    spec = CASES[name]
    cfg = spec["config"] or {}
    model = spec["model"]
    T, B, seed = spec["T"], spec["B"], spec["seed"]
    nmul = cfg.get("nmul", 1)
    out = {}
    if spec.get("forcing") == "hourly":       # hourly depths already
        x = synth.forcing_hourly(T, B, seed, storm=spec.get("storm", 4.0), day0=spec.get("day0", 0.0))
    else:
        x = synth.forcing(T, B, seed, cold=spec.get("cold", False), day0=spec.get("day0", 0.0))
    variables = cfg.get("variables", ["prcp", "tmean", "pet"])
    order = [["prcp", "tmean", "pet"].index(v) for v in variables]
    out["x_phy"] = np.ascontiguousarray(x[:, :, order])
    n = n_phy(spec)
    routing = cfg.get("routing", model not in ("Hbv_2", "Hbv_2_hourly"))
    if model in ("Hbv_2", "Hbv_2_hourly"):
        dyn = cfg["dynamic_params"].get(model, [])
        n_dy = len(dyn)
        out["p_dyn"] = synth.unit_parameters((T, B, n_dy * nmul), seed, 4)
        out["p_sta"] = synth.unit_parameters((B, (n - n_dy) * nmul + (2 if routing else 0)),
                                             seed, 6)
        out["ac_all"] = (synth.uniform((B,), seed, 7) * np.float32(5000.0)).astype(np.float32)
        out["elev_all"] = (synth.uniform((B,), seed, 8) * np.float32(3000.0)).astype(np.float32)
        if model == "Hbv_2_hourly":
            G = spec["G"]
            topo = (synth.uniform((G, B), seed, 13) < np.float32(0.45)).astype(np.float32)
            topo[np.arange(B) % G, np.arange(B)] = 1.0  # every unit drains to at least one gage
            out["outlet_topo"] = topo
            out["areas"] = (synth.uniform((B,), seed, 14) * np.float32(90.0) + np.float32(5.0)).astype(np.float32)
            out["p_distr"] = synth.unit_parameters((int(topo.sum()), 3), seed, 15)
            if spec.get("forcing") != "hourly":
                out["x_phy"] = out["x_phy"] * np.array([1.0 / 8.0, 1.0, 1.0 / 24.0], np.float32)[order]
        if spec.get("unit_spread"):           # unit parameters pushed towards the ends of (0,1): u -> smoothstep(u)
            for k in ("p_dyn", "p_sta"):
                u = out[k].astype(np.float64)
                out[k] = (u * u * (3.0 - 2.0 * u)).astype(np.float32)
    else:
        ny = n * nmul + 2
        out["parameters"] = synth.raw_parameters(T, B, ny, seed, spec.get("raw_scale", 1.0))
    if spec.get("wet_start"):                 # storages carried into the call, [5,B,nmul]
        out["states0"] = synth.wet_states(B, nmul, seed)
    if spec.get("muwts"):
        Tmu = 1 if spec["muwts"] == "bcast" else T
        u = synth.uniform((Tmu, B, nmul), seed, 9).astype(np.float64) + 0.25
        out["muwts"] = (u / u.sum(-1, keepdims=True)).astype(np.float32)
    return out


def loss_weight(name: str, key: str, shape) -> np.ndarray:
    spec = CASES[name]
    k = flux_keys(spec["model"]).index(key)
    return synth.loss_weights(tuple(shape), spec["seed"], 20 + k)


def loss_keys(name: str):
    spec = CASES[name]
    if spec["loss"] == "none":
        return []
    if spec["loss"] == "streamflow":
        return ["streamflow"]
    return flux_keys(spec["model"])
