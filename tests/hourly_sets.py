"""Problem sets, branch counts and the float64 comparison protocol of the hourly model's float64 tests
(tests/test_hourly_f64.py on the CPU, tests/test_hourly_f64_gpu.py on the GPU).  No test lives here."""
from __future__ import annotations

import numpy as np

from . import abi_util as au
from . import golden_cases as gc
from . import restate_util as ru

D3 = ("parBETA", "parK0", "parBETAET")
DF4 = ("parF0", "parALPHA", "parFMIN", "parBETA")
DALL = tuple(n for n in gc.PHY_NAMES["Hbv_2_hourly"] if n != "parCFMAX")
# a wet start under storm forcing: storages synth.wet_states, synth.forcing_hourly from noon of a spring day (the
# snowpack melts out), storm bursts of up to 18 mm/h, raw parameters spread over their ranges
WET = dict(forcing="hourly", wet=True, storm=6.0, day0=100.5, raw_scale=2.0)

# ABI-level problems (abi_util.make_problem keywords, model Hbv_2_hourly, seed 7).  T covers {1, 2, 23, 24, 25, 63, 64,
# 65, 129, 400, 2200}, B {1, 17, 67, 130}, M {1, 2, 4, 16, 64}, the four dynamic sets, muwts, permuted channels, wet
# and default starts.  "wet400" and "wet400-f4" are the problems every adjoint family runs.
ABI_PROBLEMS = {
    "wet400": dict(T=400, B=17, M=4, dyn=D3, **WET),
    "wet400-f4": dict(T=400, B=17, M=4, dyn=DF4, **WET),
    "wet2200": dict(T=2200, B=8, M=4, dyn=(), **WET),
    "wet129-muwts": dict(T=129, B=67, M=2, dyn=DF4, muwts=True, **WET),
    "wet65-channels": dict(T=65, B=130, M=1, dyn=D3, channels=(2, 0, 1), **WET),
    "wet64-m64": dict(T=64, B=1, M=64, dyn=(), **WET),
    "wet63-all-drop": dict(T=63, B=17, M=16, dyn=DALL, drop_frac=0.3, **WET),
    "dry25": dict(T=25, B=17, M=4, dyn=DF4, forcing="hourly", day0=180.0),
    "wet24": dict(T=24, B=67, M=2, dyn=(), **WET),
    "dry23": dict(T=23, B=1, M=16, dyn=D3, forcing="hourly", day0=180.0),
    "wet2-all-drop": dict(T=2, B=130, M=4, dyn=DALL, drop_frac=0.3, **WET),
    "wet1": dict(T=1, B=17, M=64, dyn=(), **WET),
    # the suite's older recipe (daily series scaled to hourly depths, default start) with parameters spread wide: a soil
    # that stays dry, where evaporation is limited by the soil moisture
    "dry300": dict(T=300, B=9, M=4, dyn=(), raw_scale=2.5),
}
# records of production length: a month, a season and a water year of hours (midwinter start: the snowpack
# accumulates and melts out inside the year)
LONG_RECORDS = {
    "month720": dict(T=720, B=17, M=4, dyn=D3, **WET),
    "season2200": ABI_PROBLEMS["wet2200"],
    "year8760": dict(T=8760, B=4, M=2, dyn=("parBETA",), forcing="hourly", wet=True, storm=6.0, day0=0.0, raw_scale=2.0),
}

EVENTS = ("IE", "excess", "Q0", "cap_unlimited", "et_sm_limited", "et_pet_limited", "ef_clamped", "ef_free", "refreeze",
          "s_clamped", "s_free", "rail")
LANE_EVENTS = ("meltout", "elev_hi", "elev_lo", "ac_hi", "ac_lo")
COVER_MIN = 1e-3      # of the lane-hours (EVENTS) or lanes (LANE_EVENTS) of at least one problem of a set


def make(kw: dict, seed: int = 7) -> dict:
    return au.make_problem(model="Hbv_2_hourly", seed=seed, **kw)


def coverage(ev: dict, elev, ac) -> dict:
    """Share of lane-hours (EVENTS) and of lanes (LANE_EVENTS) taking each branch, from the `events` a float64 run of
    hbv_restate64.pbm_hourly recorded.  `cap_slz_limited` is counted too: it cannot happen (see test_hourly_f64.py)."""
    c = {k: float(ev[k].double().mean()) for k in ("IE", "excess", "Q0", "cap_slz_limited", "cap_unlimited",
                                                   "et_sm_limited", "et_pet_limited", "ef_clamped", "refreeze",
                                                   "s_clamped", "rail")}
    c["ef_free"], c["s_free"] = 1.0 - c["ef_clamped"], 1.0 - c["s_clamped"]
    had_pack = (ev["SP_before"] > 1.0).cumsum(0) > 0                    # a pack above 1 mm, at this hour or before
    c["meltout"] = float((had_pack & (ev["SP_after"] == 0)).any(0).double().mean())
    elev, ac = np.asarray(elev), np.asarray(ac)
    c["elev_hi"], c["elev_lo"] = float((elev >= 2000).mean()), float((elev < 2000).mean())
    c["ac_hi"], c["ac_lo"] = float((ac >= 2500).mean()), float((ac < 2500).mean())
    return c


def format_coverage(rows: dict) -> str:
    keys = ("IE", "excess", "Q0", "et_sm_limited", "ef_clamped", "s_clamped", "refreeze", "rail", "meltout")
    out = [f"{'problem':24s} " + " ".join(f"{k[:9]:>9s}" for k in keys)]
    for name, c in rows.items():
        out.append(f"{name:24s} " + " ".join(f"{c[k]:9.5f}" for k in keys))
    return "\n".join(out)


def assert_covered(rows: dict, what: str):
    """Every listed branch is taken in at least COVER_MIN of the lane-hours (lanes) of at least one problem."""
    print(format_coverage(rows))
    missing = [k for k in EVENTS + LANE_EVENTS if max(c[k] for c in rows.values()) < COVER_MIN]
    assert not missing, f"{what}: branches not covered: {missing}"


# ---- comparison against float64 -------------------------------------------------------------------------------------
ADMIT_CAP = 2e-3      # of an array's elements (the issue's condition; the problem lists are chosen so that it holds)
ADMITTED = []         # (name, admitted, size) of every admitting comparison of the session


def _flux_tol(b):
    return au.FLUX_ATOL + au.FLUX_RTOL * np.abs(b)


def _grad_tol(b, groups, floor_abs=1e-30, atol_rel=au.GRAD_ATOL_REL):
    """abi_util.assert_grad_close's tolerance (helpers.compare's with floor_abs = 1e-5)."""
    w = b.shape[-1]
    groups = np.zeros(w, int) if groups is None else np.asarray(groups)
    colmax = np.abs(b).reshape(-1, w).max(0)
    floor = max(au.GROUP_FLOOR * float(colmax.max()), floor_abs)
    scale = np.empty(w)
    for g in np.unique(groups):
        scale[groups == g] = max(float(colmax[groups == g].max()), floor) * (
            au.ROUTE_ATOL_REL / au.GRAD_ATOL_REL if g < 0 else 1.0)
    return atol_rel * scale + au.GRAD_RTOL * np.abs(b)


def admit(name, got, want64, f32_evals, tol_fn):
    """`got` with the elements admitted under the protocol replaced by float64's: an element outside tolerance against
    float64 is admitted only if `got` agrees there, at the same tolerance, with one of `f32_evals` (arrays, or callables
    returning one: float32 evaluations of the same equations).  At most ADMIT_CAP of the array; an element outside that
    agrees with none of them is a finding and fails here."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    assert got.shape == want64.shape, f"{name}: {got.shape} vs {want64.shape}"
    if got.size == 0:
        return got
    out = np.abs(got - want64) > tol_fn(want64)
    if not out.any():
        return got
    ok = np.zeros_like(out)
    for ev in f32_evals:
        alt = np.asarray(ev() if callable(ev) else ev, np.float64)
        ok |= out & (np.abs(got - alt) <= tol_fn(alt))
        if not (out & ~ok).any():
            break
    n = int(ok.sum())
    ADMITTED.append((name, n, got.size))
    print(f"{name}: {int(out.sum())} of {got.size} outside tolerance against float64, {n} admitted "
          f"(they agree with a float32 evaluation); cap {int(ADMIT_CAP * got.size)}")
    left = out & ~ok
    if left.any():
        i = tuple(np.argwhere(left)[0])
        raise AssertionError(f"{name}: {int(left.sum())} elements agree neither with float64 nor with a float32 evaluation; "
                             f"first at {i}: {got[i]!r} vs float64 {want64[i]!r}")
    assert n <= ADMIT_CAP * got.size, f"{name}: {n} admitted elements of {got.size}, above the cap of {ADMIT_CAP:g}"
    res = got.copy()
    res[ok] = want64[ok]
    return res


# Elements that no float32 evaluation can be held to, by problem name: (key, index, the largest content in mm that the
# storage behind the element reached).  A groundwater box that runs empty hands over its last remainder in its last
# hour: that remainder carries the rounding float32 accumulated while the box held tens to hundreds of mm (an ulp of
# 293.5 is 3e-5 mm), it is the storage's value in `traj`, and as PERC = min(SUZ, parPERC * dt) / dt it is a rate 24 x as
# large in `flux`.  Float32 evaluations (oracle, float32 restatement, kernel) differ from float64 there by more than
# the tolerance and, their rounding being their own, not always alike.  Bound, the one tests/test_restate64.py
# commits for the same thing on the fixtures: 1e-5 x the member's largest content for a storage, 24 / M x that for
# the ensemble-mean flux row it drains into.  The measured values are in tests/test_hourly_f64.py's docstring.
PRECISION_ONLY = {
    "wet2200": [("flux", (10, 331, 0), 293.51), ("traj", (3, 38, 26), 39.69)],
    "year8760": [("flux", (10, 2031, 2), 212.63)],
}


# Ties, by problem name: (key, index, the jump of the float64 value across the tie).  d loss / d P of an hour without
# precipitation on a basin with snow-free members: SNOWPACK = MELTWATER = 0 exactly (float64), so melt = min(melt
# potential, SNOWPACK) is min(0, 0) in a cold hour and splits its gradient 0.5 / 0.5, tosoil's (MW - CWH * SP) / dt >= 0
# holds with equality, and whether MELTWATER's remainder of `MW - tosoil * dt` is 0 or +-1e-10 (which the next hour's
# guard rail masks or not) is decided by the last bit.  With P = 0 nothing of the forward run depends on it; only this
# gradient does.  Two float32 evaluations usually resolve it alike (those elements are admitted above), the kernel's own
# rounding may not.  "wet63-all-drop" g_x[21, 11, 0]: members 0, 10, 14 of basin 11 are snow-free; float64 gives
# -9.0598 with the ties, -9.8254 with P nudged to 1e-7 (all three resolved to one side), oracle and float32
# restatement -9.0598, the kernel -8.7700.  Bound: the jump, 0.7657.
TIES = {
    "wet63-all-drop": [("g_x", (21, 11, 0), 0.7657)],
}


def _named(name, got, want64, M):
    got = dict(got)
    for key, idx, jump in TIES.get(name, ()):
        if key in got and key in want64:
            a = np.array(got[key], np.float64)
            assert abs(a[idx] - want64[key][idx]) <= jump, (name, key, idx, a[idx], want64[key][idx], jump)
            a[idx] = want64[key][idx]
            got[key] = a
    for key, idx, content in PRECISION_ONLY.get(name, ()):
        if key in got and key in want64:
            bound = 1e-5 * content * (24.0 / M if key == "flux" else 1.0)
            a = np.array(got[key], np.float64)
            assert abs(a[idx] - want64[key][idx]) <= bound, (name, key, idx, a[idx], want64[key][idx], bound)
            a[idx] = want64[key][idx]
            got[key] = a
    return got


def compare_f64(prob, got, want64, f32_evals, label, name=None):
    """A run_problem result against the float64 restatement (ru.abi_hourly) at abi_util's tolerances: g_params and
    g_muwts whole, flux / traj / state_out / g_x under `admit` (the elements PRECISION_ONLY names for problem `name`
    are held to their own bound first).  f32_evals: run_problem-shaped dicts or callables
    returning one.  Everything lands in abi_util.REPORT through compare_runs."""
    cache = {}

    def alt(i, k):
        def f():
            if i not in cache:
                cache[i] = f32_evals[i]() if callable(f32_evals[i]) else f32_evals[i]
            return cache[i][k]
        return f
    got = _named(name, got, want64, prob["M"])
    bad, popped = [], []          # every array is compared before anything is raised
    for k in ("flux", "traj", "state_out", "g_x"):
        if k in got and k in want64:
            tol = _flux_tol if k != "g_x" else (lambda b: _grad_tol(b, np.arange(b.shape[-1])))
            try:
                got[k] = admit(f"{label} {k}", got[k], want64[k], [alt(i, k) for i in range(len(f32_evals))], tol)
            except AssertionError as e:
                bad.append(str(e))
                got.pop(k)
                popped.append(k)
    try:       # (an array that failed under `admit` is reported by that failure, not compared again)
        au.compare_runs(prob, got, {k: v for k, v in want64.items() if k not in popped}, label=label)
    except AssertionError as e:
        bad.append(str(e))
    assert not bad, " | ".join(bad)


def compare_case_f64(name, res, want64, f32_eval):
    """A helpers.run_case result of an hourly golden case against the module-level restatement in float64
    (ru.hourly_case_reverse) at helpers.compare's tolerances: outputs and parameter gradients whole, the state series
    and the forcing gradient under `admit` against the restatement run in float32."""
    from .helpers import compare
    cache = {}

    def alt(k):
        def f():
            if not cache:
                cache.update(f32_eval())
            return cache[k]
        return f
    res = dict(res)
    for k in ("states", "grad/x_phy"):
        if k in want64:
            tol = _flux_tol if k == "states" else (lambda b: _grad_tol(b, np.arange(b.shape[-1]), 1e-5))
            res[k] = admit(f"{name}:{k} (float64)", res[k], want64[k], [alt(k)], tol)

    class _Ref(dict):
        files = property(lambda self: list(self))
    compare(name, res, _Ref({k: v for k, v in want64.items()}))
