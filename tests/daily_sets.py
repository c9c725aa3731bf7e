"""Problem sets, branch counts and the float64 comparison protocol of the daily models' float64 tests
(tests/test_daily_f64.py on the CPU, tests/test_daily_f64_gpu.py on the GPU).  The protocol itself -- `admit`, the
tolerance functions, the cap -- is tests/hourly_sets.py's, used as it is.  No test lives here."""
from __future__ import annotations

import numpy as np

from . import abi_util as au
from . import golden_cases as gc
from . import hourly_sets as hs
from . import restate_util as ru

MODELS = ("Hbv", "Hbv_1_1p", "Hbv_2")
D2 = ("parBETA", "parBETAET")                          # the delta-MG pair
D3 = ("parBETA", "parK0", "parBETAET")                 # the compiled three-slot set
DLIST = {"Hbv": ("parBETA", "parFC", "parK0", "parLP", "parBETAET"),            # four to six slots: run-time lists
         "Hbv_1_1p": ("parK0", "parTT", "parFC", "parC"),
         "Hbv_2": ("parBETA", "parK0", "parBETAET", "parRT", "parAC", "parUZL")}
DALL = {"Hbv": tuple(gc.PHY_NAMES["Hbv"]) + ("parBETAET",), "Hbv_1_1p": tuple(gc.PHY_NAMES["Hbv_1_1p"]),
        "Hbv_2": tuple(gc.PHY_NAMES["Hbv_2"])}
# a wet start: storages synth.wet_states handed in as state_in, raw parameters spread over their ranges
# from a spring day, so that PET > 0 while the carried-in soil is saturated (the class "PET = 0 on saturated soil" of
# tests/test_daily_f64.py's docstring); snow still falls and melts on the cold basins, and the long records run through
# their winters
WET = dict(wet=True, raw_scale=2.0, day0=120.0, routing=False)
WETR = dict(wet=True, raw_scale=2.0, day0=120.0, routing=True)
# the default start (0.001 mm everywhere) with parameters spread wide: a soil that stays dry, where evaporation is
# limited by the soil moisture (with parBETAET in the table)
DRY = dict(raw_scale=2.5, routing=False)

# ABI-level problems (abi_util.make_problem keywords, seed 7), per model.  Over the three sets T covers {1, 2, 15, 16,
# 17, 63, 64, 65, 129, 400, 1460}, B {1, 17, 67, 130}, M {1, 2, 4, 16, 64}; the dynamic sets none, the delta-MG pair, the
# compiled three-slot set, a four-to-six-slot list and all-dynamic with drop masks; ensemble weights, permuted forcing
# channels, routing on and off, wet and default starts.  "wet400" is the problem every adjoint family runs: at most
# three dynamic parameters and no ensemble weights, so that every family holds it -- the delta-MG pair for Hbv and
# Hbv_1_1p, the three-slot set for Hbv_2: the sets the pipelined and streaming kernels have compiled instances of.
ABI_PROBLEMS = {
    "Hbv": {
        "wet400": dict(T=400, B=17, M=4, dyn=D2, **WET),
        "wet400-d3": dict(T=400, B=17, M=4, dyn=D3, **WET),
        "wet400-static": dict(T=400, B=9, M=16, dyn=(), **WETR),
        "dry300-betaet": dict(T=300, B=9, M=4, dyn=(), betaet=True, **DRY),
        "wet1460": dict(T=1460, B=8, M=4, dyn=("parBETA",), **WET),
        "wet129-muwts": dict(T=129, B=67, M=2, dyn=D2, muwts=True, **WETR),
        "wet65-channels": dict(T=65, B=130, M=1, dyn=D3, channels=(2, 0, 1), **WETR),
        "wet64-m64": dict(T=64, B=1, M=64, dyn=(), **WET),
        "wet63-all-drop": dict(T=63, B=17, M=16, dyn=DALL["Hbv"], drop_frac=0.3, **WETR),
        "dry17-list": dict(T=17, B=17, M=4, dyn=DLIST["Hbv"], drop_frac=0.3, raw_scale=2.5, routing=True),
        "wet16": dict(T=16, B=67, M=2, dyn=(), **WETR),
        "dry15": dict(T=15, B=1, M=16, dyn=D2, raw_scale=2.5, routing=True),
        "wet2-all-drop": dict(T=2, B=130, M=4, dyn=DALL["Hbv"], drop_frac=0.3, **WETR),
        "wet1": dict(T=1, B=17, M=64, dyn=(), **WETR),
    },
    "Hbv_1_1p": {
        "wet400": dict(T=400, B=17, M=4, dyn=D2, **WET),
        "wet400-all-drop": dict(T=400, B=17, M=4, dyn=DALL["Hbv_1_1p"], drop_frac=0.3, **WET),
        "wet400-list": dict(T=400, B=17, M=4, dyn=DLIST["Hbv_1_1p"], **WETR),
        "dry300": dict(T=300, B=9, M=4, dyn=(), **DRY),
        "wet129-muwts": dict(T=129, B=67, M=2, dyn=D3, muwts=True, **WETR),
        "wet65-channels": dict(T=65, B=130, M=1, dyn=D2, channels=(1, 2, 0), **WET),
        "wet64-m64": dict(T=64, B=1, M=64, dyn=(), **WETR),
        "dry63": dict(T=63, B=17, M=16, dyn=D2, raw_scale=2.5, routing=True),
        "wet17": dict(T=17, B=67, M=2, dyn=(), **WETR),
        "wet15-list": dict(T=15, B=17, M=4, dyn=DLIST["Hbv_1_1p"], drop_frac=0.3, **WETR),
        "wet2": dict(T=2, B=130, M=1, dyn=D3, **WETR),
        "wet1": dict(T=1, B=17, M=16, dyn=(), **WET),
    },
    "Hbv_2": {
        "wet400": dict(T=400, B=17, M=4, dyn=D3, **WET),
        "wet400-muwts": dict(T=400, B=17, M=4, dyn=D3, muwts=True, **WET),
        "wet400-list": dict(T=400, B=17, M=4, dyn=DLIST["Hbv_2"], drop_frac=0.3, **WETR),
        "dry300": dict(T=300, B=9, M=4, dyn=(), **DRY),
        "wet129-static": dict(T=129, B=67, M=2, dyn=(), **WETR),
        "wet65-channels": dict(T=65, B=130, M=1, dyn=D2, channels=(2, 0, 1), **WETR),
        "wet64-m64": dict(T=64, B=1, M=64, dyn=D3, **WET),
        "wet63-all-drop": dict(T=63, B=17, M=16, dyn=DALL["Hbv_2"], drop_frac=0.3, **WETR),
        "dry16": dict(T=16, B=17, M=4, dyn=D3, raw_scale=2.5, routing=True),
        "wet15-muwts": dict(T=15, B=67, M=2, dyn=(), muwts=True, **WETR),
        "wet2-all-drop": dict(T=2, B=130, M=4, dyn=DALL["Hbv_2"], drop_frac=0.3, **WET),
        "wet1": dict(T=1, B=17, M=64, dyn=(), **WETR),
    },
}
# records of production length: four years per model where the set has none, and one of 7300 days (the benchmark's
# record length) on few basins and members
LONG_RECORDS = {
    "Hbv": {"wet1460": ABI_PROBLEMS["Hbv"]["wet1460"], "wet7300": dict(T=7300, B=4, M=2, dyn=("parBETA",), **WETR)},
    "Hbv_1_1p": {"wet1460": dict(T=1460, B=8, M=4, dyn=D2, **WETR)},
    "Hbv_2": {"wet1460": dict(T=1460, B=8, M=4, dyn=("parBETA",), **WET)},
}


def problems(model: str) -> dict:
    """name -> make_problem keywords of every problem of `model`: its ABI set and its long records."""
    return {**ABI_PROBLEMS[model], **LONG_RECORDS[model]}


def make(model: str, kw: dict, seed: int = 7) -> dict:
    return au.make_problem(model=model, seed=seed, **kw)


# ---- branch coverage -------------------------------------------------------------------------------------------------
# Branches asserted per model: taken in at least COVER_MIN of the lane-days of at least one problem of the model's set
# (LANE_EVENTS: of the lanes).  `et_sm_limited` and the SM floor it leads to are asserted for Hbv too: its set has
# problems with parBETAET in the table.
EVENTS = ("rain", "snow", "melt_pack_limited", "melt_potential", "refr_mw_limited", "refr_potential", "tosoil",
          "wet_clamped", "wet_free", "excs", "ef_clamped", "ef_free", "et_sm_limited", "et_pet_limited", "sm_floor",
          "perc_suz", "perc_par", "Q0")
CAP_EVENTS = ("cap_unlimited", "slz_floor")
HBV2_EVENTS = ("elev_hi", "elev_lo", "ac_lo", "ac_hi", "ac_clamp_hi", "ac_clamp_lo", "ac_free", "exp_clamped", "exp_free",
               "slz_lf_clamped")
LANE_EVENTS = ("meltout",)
# Branches that cannot be taken (argued in tests/test_daily_f64.py's docstring) and are asserted never to be
NEVER = ("cap_slz_limited", "sm_floor_cap")
COVER_MIN = hs.COVER_MIN


def events_of(model: str) -> tuple:
    return EVENTS + (CAP_EVENTS if model != "Hbv" else ()) + (HBV2_EVENTS if model == "Hbv_2" else ()) + LANE_EVENTS


def coverage(ev: dict) -> dict:
    """Share of lane-days taking each branch (meltout: share of lanes whose pack exceeded 1 mm and later was exactly
    0), from the `events` a float64 run of hbv_restate64._pbm recorded."""
    c = {k: float(v.double().mean()) for k, v in ev.items() if k not in ("SP_before", "SP_after")}
    c["ef_free"], c["wet_free"] = 1.0 - c["ef_clamped"], 1.0 - c["wet_clamped"]
    had_pack = (ev["SP_before"] > 1.0).cumsum(0) > 0
    c["meltout"] = float((had_pack & (ev["SP_after"] == 0)).any(0).double().mean())
    for k in NEVER:
        c.setdefault(k, 0.0)
    return c


TABLE_KEYS = ("Q0", "excs", "perc_par", "ef_clamped", "et_sm_limited", "wet_clamped", "refr_potential", "meltout")


def format_coverage(rows: dict, keys=TABLE_KEYS) -> str:
    out = [f"{'problem':30s} " + " ".join(f"{k[:9]:>9s}" for k in keys)]
    for name, c in rows.items():
        out.append(f"{name:30s} " + " ".join(f"{c.get(k, float('nan')):9.5f}" for k in keys))
    return "\n".join(out)


def assert_covered(model: str, rows: dict, what: str):
    """Every branch of events_of(model) is taken in at least COVER_MIN of the lane-days (lanes) of at least one
    problem; the branches of NEVER in none."""
    print(format_coverage(rows))
    missing = [k for k in events_of(model) if max(c[k] for c in rows.values()) < COVER_MIN]
    assert not missing, f"{what}: branches not covered: {missing}"
    never = [(n, k) for n, c in rows.items() for k in NEVER if c[k] != 0.0]
    assert not never, f"{what}: a branch argued unreachable was taken: {never}"


def hbv_without_betaet(prob: dict) -> bool:
    return prob["model"] == "Hbv" and "parBETAET" not in prob["names"]


# ---- comparison against float64 --------------------------------------------------------------------------------------
# No element of these problems had to be named (hourly_sets.PRECISION_ONLY / TIES have no daily entry).
def compare_f64(prob, got, want64, f32_evals, label):
    """A run_problem result against the float64 restatement (ru.abi_daily) at abi_util's tolerances: g_params (the
    routing columns at ROUTE_ATOL_REL), g_muwts and the routed rows whole, flux / traj / state_out / g_x under
    hourly_sets.admit."""
    hs.compare_f64(prob, got, want64, f32_evals, label)


def compare_case_f64(name, res, want64, f32_eval, precision_only=()):
    """A helpers.run_case result of a daily golden case against the module-level restatement in float64
    (ru.case_reverse) at helpers.compare's tolerances: outputs and parameter gradients whole, `states` and
    `grad/x_phy` under `admit` against the restatement run in float32.  `precision_only`: the case's entries of
    test_restate64.PRECISION_ONLY -- a storage element is held to its bound there (x the member's largest value of
    that storage, in float64), a tie (bound ("jump", j)) within the jump of the float64 value across it, and a gradient
    block (bound None: a tie float32 and float64 resolve differently) is held to the float32 restatement instead of the
    float64 one, at the same tolerances."""
    res, want64 = dict(res), dict(want64)
    f32 = {}
    for key, idx, bound in precision_only:
        if key not in want64:
            continue
        a = np.array(res[key], np.float64)
        if isinstance(bound, tuple):       # a tie: within the jump of the float64 value across it, either side
            assert abs(float(a[idx]) - float(want64[key][idx])) <= bound[1] * (1 + 1e-3), (name, key, idx, a[idx], bound)
            a[idx] = want64[key][idx]
            res[key] = a
        elif bound is None:
            if not f32:
                f32.update(f32_eval())
            w = np.array(want64[key], np.float64)
            w[idx] = f32[key][idx]
            want64[key] = w
        else:
            scale = float(np.abs(want64[key][(idx[0], slice(None)) + tuple(idx[2:])]).max())
            assert abs(float(a[idx]) - float(want64[key][idx])) <= bound * scale, (name, key, idx, a[idx], want64[key][idx])
            a[idx] = want64[key][idx]
            res[key] = a
    hs.compare_case_f64(name, res, want64, (lambda: f32) if f32 else f32_eval)
