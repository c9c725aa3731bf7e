"""CPU tier: the C oracle's hourly step (oracle/hbv_oracle.c: hstep_fwd / hstep_bwd, which every GPU parity test of
Step<MODEL_HOURLY> trusts) against the float64 restatement of Hbv_2_hourly (oracle/hbv_restate64.py, pinned to the
reference's fixtures by tests/test_restate64.py), at the level of the C ABI: twelve flux rows with their own loss
weights, the storage trajectory, the gradients of the raw parameters, the forcings and the ensemble weights.

Inputs (tests/hourly_sets.py): problems that start wet (synth.wet_states) under hourly storm forcing
(synth.forcing_hourly), so that the branches the older hourly problems never take are taken, and records of 720, 2200
and 8760 hours.  Every set asserts its own branch coverage on the float64 run before anything is compared.

Branch coverage, share of lane-hours in float64 (meltout: share of lanes whose pack exceeded 1 mm and later was exactly
0), measured by test_new_problem_sets_take_the_branches / test_wet_fixtures_take_the_branches_and_the_older_inputs_do_not:

problem                         IE    excess        Q0 et_sm_lim ef_clampe s_clamped  refreeze      rail   meltout
--- existing suite (as found) ---
hourly_dyn3                0.00000   0.00000   0.00000   0.00000   0.00000   0.00000   0.23393   0.98601   0.60714
hourly_routing_drop        0.00000   0.00000   0.00000   0.00000   0.00635   0.00000   0.16521   0.98885   0.75000
hourly_static_cold         0.00000   0.00000   0.00000   0.00000   0.00000   0.00000   0.08833   0.98333   0.20000
hourly_long_dyn3           0.00000   0.00000   0.00000   0.00000   0.03952   0.00000   0.17690   0.96488   0.82143
hourly_long_routing        0.00000   0.00000   0.00000   0.00244   0.02165   0.00000   0.14779   0.98490   0.79167
ORACLE T300 B21 3dyn       0.00000   0.00000   0.00000   0.00000   0.01073   0.00000   0.14428   0.98798   0.83929
ORACLE T200 B9 0dyn        0.00000   0.00000   0.00000   0.00000   0.00847   0.00000   0.13639   0.98917   0.91667
STREAM2 T100 B19 3dyn      0.00000   0.00000   0.00000   0.00000   0.00000   0.00000   0.20263   0.98934   0.53947
STREAM2 T100 B19 2dyn      0.00000   0.00000   0.00000   0.00000   0.00000   0.00000   0.20263   0.99000   0.53947
STREAM2 T100 B19 4dyn      0.00000   0.00000   0.00000   0.00000   0.00000   0.00000   0.20263   0.98934   0.53947
--- new fixtures ---
hourly_wet_routing         0.02109   0.00208   0.46484   0.00000   0.75000   0.04974   0.26693   0.26276   0.37500
hourly_wet_dyn3_drop       0.01188   0.00337   0.52481   0.00006   0.62131   0.05975   0.22262   0.16294   0.40000
hourly_wet_muwts           0.00889   0.00167   0.25278   0.00028   0.51944   0.04792   0.23972   0.29306   0.33333
--- new ABI-level problems and long records (tests/hourly_sets.py) ---
wet400                     0.01033   0.00129   0.29478   0.00004   0.68195   0.03445   0.13926   0.31864   0.48529
wet400-f4                  0.01099   0.00129   0.30121   0.00007   0.68357   0.03449   0.13926   0.31085   0.48529
wet2200 (= season2200)     0.01271   0.00026   0.20581   0.00000   0.77129   0.00892   0.04842   0.40889   0.68750
wet129-muwts               0.00978   0.00382   0.55611   0.00000   0.65244   0.11732   0.17344   0.12449   0.38060
wet65-channels             0.00675   0.00710   0.70095   0.00047   0.63811   0.20698   0.18367   0.03231   0.25385
wet64-m64                  0.00220   0.00781   0.66528   0.00000   0.66772   0.19531   0.00000   0.02905   0.40625
wet63-all-drop             0.00677   0.05655   0.83438   0.00006   0.29791   0.10621   0.14542   0.02048   0.43015
dry25                      0.00000   0.00000   0.00000   0.00000   0.00000   0.00000   0.00000   0.96000   0.00000
wet24                      0.00342   0.01928   0.75404   0.00031   0.61318   0.32027   0.17879   0.03420   0.13433
dry23                      0.00000   0.00000   0.00000   0.00000   0.00000   0.00000   0.00000   0.95652   0.00000
wet2-all-drop              0.02308   0.35192   0.86154   0.00288   0.59038   0.41635   0.17212   0.07212   0.01154
wet1                       0.02665   0.46232   0.80055   0.00643   0.63419   0.46783   0.09467   0.14246   0.01471
dry300                     0.00491   0.00000   0.00000   0.00704   0.13546   0.00000   0.13500   0.94852   0.86111
month720                   0.02138   0.00069   0.17600   0.00002   0.66003   0.02006   0.11281   0.43723   0.50000
year8760                   0.01585   0.00037   0.16567   0.00000   0.84553   0.01390   0.13763   0.37451   1.00000
(ef / s "not clamped", evaporation limited by PET, capillary not limited, both sides of elevation 2000 and of ac 2500
are asserted too and are everywhere far above 0.1 %.)
Capillary rise limited by SLZ cannot happen and is asserted never to: cap = min(SLZ, parC * SLZ * (1 - min(SM / FC,
1)) * dt) with parC <= 1, dt = 1/24 and SLZ >= nearzero > 0 after the guard rail, so the second argument is at most
SLZ / 24.  (The reference's min() is dead code there; its adjoint branch `wa` of minw_(SLZc, capp) is unreachable.)

Protocol (tests/hourly_sets.py::compare_f64): abi_util's committed tolerances.  g_params and g_muwts are compared
whole, with no exclusion.  An element of flux, traj, state_out or g_x outside tolerance against float64 is admitted
only if the oracle agrees there, at the same tolerance, with the restatement run in float32 (the same equations, the
same precision as the oracle, different code); admitted elements are counted, printed and capped at 2e-3 of the array.
The problem lists were chosen so that this holds here, on the CPU.

What the admitted elements are (oracle against float64; the float32 restatement shares every one of them):
 * forcing gradient -- d loss / d P (that channel only) of hours with P = 0 on a basin with snow-free members, where
   SNOWPACK = MELTWATER = 0 exactly: ties of min(melt potential, SNOWPACK) and of tosoil's `>= 0` that float32 and
   float64 resolve by the last bit of MELTWATER's remainder (hourly_sets.TIES has the details).  With a night PET of
   exactly 0 a second class appears, d loss / d PET on saturated soil: the hour that sheds the excess leaves SM = FC to
   an ulp (SM / FC - 1 in {0, +-2.2e-16, -3.3e-16} in float64, {0, +-8e-8, 2.6e-7, -4.7e-7} in float32), it stays there
   while nothing evaporates, and the masks SM / FC <= 1, (SM / FC) ** BETA <= 1, excess >= 0 fall by the last bit: 35 of
   9600 elements on a 400-hour wet problem, above the cap.  synth.forcing_hourly therefore keeps a small PET at night,
   which dries the soil below FC within the hour, and the class is gone from these problems.
 * flux rows -- the `excs` row and those downstream of it in such hours (24 x an ulp of SM is 1e-3 mm/d beside a
   tolerance of 1e-5), and PERC / Q1 / Q2 in the last hours of a box running empty.
 * storages -- the last hours of a box running empty, where float32's accumulated rounding of a 40-500 mm storage
   (1e-5 .. 1e-4 mm) is the value's third or fourth digit (hourly_sets.PRECISION_ONLY; test_restate64.py names the
   same thing on the fixtures).  Measured: wet2200 PERC[331, basin 0] oracle 0.0706816, float32 restatement 0.0706629,
   float64 0.0706616 (member 3's SUZ held 293.5 mm, its last 0.0117 mm leave); wet2200 SUZ[38, basin 6, member 2]
   oracle = float32 restatement 0.0776904, float64 0.0776578, kernel 0.0776203 (39.7 mm); year8760 PERC[2031, basin 2]
   oracle = float32 restatement 0.199784, float64 0.198232, kernel 0.199738 (member 1's SUZ held 212.6 mm 900 hours
   earlier).

Admitted elements, oracle against float64 (outside = admitted in every row; cap = 2e-3 of the array); g_params and
g_muwts: none outside in any problem:

problem          flux            traj            g_x
wet400           6 / 81600       18 / 136340     1 / 20400
wet400-f4        4 / 81600       11 / 136340     1 / 20400
wet2200          49 / 211200     164 / 352160    0
wet129-muwts     12 / 103716     2 / 87100       0
wet65-channels   4 / 101400      0               0
wet63-all-drop   0               0               1 / 3213
dry300           1 / 32400       0               2 / 8100
month720         27 / 146880     43 / 245140     7 / 36720
year8760         124 / 420480    166 / 350440    2 / 105120
(wet64-m64, dry25, wet24, dry23, wet2-all-drop, wet1: nothing outside.)

float64 cost on 8 host threads: 0.1-1.8 s per problem up to 400 hours, 4 s (720), 10 s (2200), 42 s (8760).
"""
import time

import numpy as np
import pytest
import torch

from . import abi_util as au
from . import golden_cases as gc
from . import hourly_sets as hs
from . import restate_util as ru

_CACHE = {}


def f64_run(kw_name, kw):
    """(problem, float64 result, coverage) of a problem of the sets, computed once per session."""
    if kw_name not in _CACHE:
        prob = hs.make(kw)
        ev = {}
        t = time.time()
        res = ru.abi_hourly(prob, torch.float64, events=ev)
        cov = hs.coverage(ev, prob["elev"], prob["ac"])
        print(f"{kw_name}: float64 forward + backward {time.time() - t:.1f} s on {torch.get_num_threads()} threads")
        _CACHE[kw_name] = (prob, res, cov)
    return _CACHE[kw_name]


def test_new_problem_sets_take_the_branches():
    """The ABI-level set (long records included) takes every listed branch in at least 0.1 % of the lane-hours (or
    lanes) of one of its problems; each long record takes the infiltration excess and the fast-runoff box at that rate
    and the soil excess at all; capillary rise limited by SLZ never happens (module docstring)."""
    rows = {n: f64_run(n, kw)[2] for n, kw in {**hs.ABI_PROBLEMS, **hs.LONG_RECORDS}.items()}
    hs.assert_covered(rows, "ABI_PROBLEMS + LONG_RECORDS")
    for n in hs.LONG_RECORDS:
        assert min(rows[n]["IE"], rows[n]["Q0"]) >= hs.COVER_MIN and rows[n]["excess"] > 0 and rows[n]["meltout"] > 0, n
    assert all(c["cap_slz_limited"] == 0.0 for c in rows.values())


def _fixture_coverage(name):
    ev = {}
    ru.hourly_case_reverse(name, torch.float64, events=ev)
    inp = gc.build_inputs(name)
    return hs.coverage(ev, inp["elev_all"], inp["ac_all"])


def test_wet_fixtures_take_the_branches_and_the_older_inputs_do_not():
    """The three wet fixtures take IE > 0, excess > 0 and Q0 > 0 in the reference's own tape, each of them; the five
    older hourly fixtures and the hourly problems of test_gpu_parity.py take none of the three (the table of the module
    docstring).  The eight hourly fixtures together take every listed branch (evaporation limited by the soil moisture
    is the older, dry ones' part: capillary rise keeps a wet column's soil above PET * dt)."""
    from .test_gpu_parity import ORACLE_CASES, STREAM2_CASES
    hourly = [n for n, s in gc.CASES.items() if s["model"] == "Hbv_2_hourly"]
    rows = {n: _fixture_coverage(n) for n in hourly}
    wet = {n: c for n, c in rows.items() if gc.CASES[n].get("wet_start")}
    hs.assert_covered(rows, "hourly fixtures")
    for tag, cases, seed in (("ORACLE", ORACLE_CASES, 7), ("STREAM2", STREAM2_CASES, 21)):
        for kw in cases:
            if kw["model"] == "Hbv_2_hourly" and kw["T"] >= 100:
                prob = au.make_problem(seed=seed, **kw)
                ev = {}
                ru.abi_hourly(prob, torch.float64, backward=False, events=ev)
                rows[f"{tag} T{kw['T']} B{kw['B']} {len(kw['dyn'])}dyn"] = hs.coverage(ev, prob["elev"], prob["ac"])
    print(hs.format_coverage(rows))
    for n, c in rows.items():
        if n not in wet:
            assert c["IE"] == c["excess"] == c["Q0"] == 0.0, (n, c)
    assert len(wet) == 3 and all(min(c["IE"], c["excess"], c["Q0"]) >= hs.COVER_MIN for c in wet.values())


@pytest.mark.parametrize("name", list(hs.ABI_PROBLEMS) + [n for n in hs.LONG_RECORDS if n != "season2200"])
def test_oracle_matches_float64(name, oracle_path):
    kw = hs.ABI_PROBLEMS.get(name) or hs.LONG_RECORDS[name]
    prob, want, _ = f64_run(name, kw)
    got = au.run_problem(prob, oracle_path, device="cpu", x_grad=True)
    hs.compare_f64(prob, got, want, [lambda: ru.abi_hourly(prob, torch.float32)], f"oracle-f64 {name}", name)
