"""CPU tier: the C oracle's daily step (oracle/hbv_oracle.c, which every GPU parity test of Hbv, Hbv_1_1p and Hbv_2
trusts) against the float64 restatement of the daily models (oracle/hbv_restate64.py, pinned to the reference's fixtures
by tests/test_restate64.py), at the level of the C ABI: the 11 / 12 flux rows and the four routed rows with their own
loss weights, the storage trajectory, the gradients of the raw parameters (routing columns included), the forcings and
the ensemble weights. 

Inputs (tests/daily_sets.py): problems that start wet (synth.wet_states handed in as state_in, raw parameters spread
over their ranges, a record from day 120 of the year) and problems from the default start with parameters spread wider
still, so that the branches the older daily inputs take rarely or never are taken; records of 1460 days per model and one
of 7300 days, the benchmark's record length.  Every set asserts its own branch coverage on the float64 run.

Branch coverage, share of lane-days in float64 (perc_par: PERC = parPERC, i.e. Q1 fed at the full rate; et_sm_lim:
AET = SM < PET * ef; meltout: share of lanes whose pack exceeded 1 mm and later was exactly 0), measured by
test_new_problem_sets_take_the_branches / test_wet_fixtures_take_the_branches_and_the_older_inputs_do_not:

problem                               Q0      excs  perc_par ef_clampe et_sm_lim wet_clamp refr_pote   meltout
--- existing suite (as found): the 32 older single-call fixtures ---
cfg1_hbv_default                 0.00164   0.00000   0.01041   0.09507   0.00000   0.00000   0.06521   1.00000
hbv_static_m16                   0.00000   0.00000   0.00109   0.01063   0.00000   0.00000   0.10026   0.20833
hbv_static_m16_sf                0.00000   0.00000   0.00781   0.03982   0.00000   0.00000   0.11285   0.60417
hbv_warmup_states                0.00000   0.00016   0.02241   0.16146   0.00000   0.00000   0.12405   0.60417
hbv_warmup_nostates              0.00000   0.00000   0.00477   0.01584   0.00000   0.00000   0.02062   0.50000
hbv_dyn2                         0.00000   0.00000   0.00187   0.02937   0.00104   0.00000   0.04333   0.60000
hbv_dyn2_drop                    0.00000   0.00000   0.00065   0.01562   0.00016   0.00000   0.06982   0.54167
hbv_m3_xgrad                     0.00000   0.00000   0.00000   0.00223   0.00000   0.00000   0.05655   0.52381
hbv_muwts                        0.00000   0.00000   0.00000   0.00703   0.00000   0.00000   0.09375   0.20000
hbv_muwts_warmup                 0.00000   0.00000   0.00313   0.02083   0.00000   0.00000   0.01979   0.35000
hbv_comprout_m1                  0.00000   0.00000   0.00000   0.00000   0.00000   0.00000   0.08333   0.33333
hbv_ties                         0.00116   0.00231   0.00579   0.00926   0.00000   0.00000   0.00926   0.33333
hbv_variables                    0.00000   0.00000   0.00000   0.00000   0.00000   0.00000   0.06563   0.37500
hbv_short                        0.00000   0.00000   0.00000   0.00000   0.00000   0.00000   0.00000   0.00000
hbv11p_dyn_all                   0.00059   0.00352   0.01016   0.04336   0.00000   0.00352   0.05840   0.60000
hbv11p_static                    0.00000   0.00000   0.00000   0.00336   0.00000   0.00000   0.12903   0.33333
hbv2_dyn3                        0.00000   0.00879   0.02136   0.12219   0.00415   0.00854   0.09961   0.33594
hbv2_dyn3_routing                0.00000   0.00000   0.00000   0.01270   0.02002   0.00000   0.11182   0.12500
hbv2_static                      0.00000   0.00000   0.00521   0.10417   0.04861   0.00000   0.07812   0.00000
hbv_long_static                  0.00000   0.00000   0.01492   0.08654   0.00000   0.00000   0.07281   0.98958
hbv_long_dyn2                    0.00032   0.00003   0.03209   0.17491   0.00006   0.00003   0.06134   1.00000
hbv_long_m4_xgrad                0.00093   0.00056   0.01176   0.05444   0.00000   0.00000   0.08222   1.00000
hbv11p_long_dyn_all              0.01143   0.02051   0.08140   0.13940   0.00010   0.02051   0.07080   1.00000
hbv2_long_dyn3                   0.00583   0.00787   0.09412   0.23456   0.00891   0.00717   0.08844   0.86719
hbv2_long_routing                0.00000   0.00024   0.08131   0.20988   0.00405   0.00000   0.09750   1.00000
hbv_long_dyn5_drop               0.00296   0.00858   0.04018   0.09145   0.00000   0.00858   0.06676   1.00000
hbv_long_variables               0.00117   0.00017   0.01092   0.05458   0.00000   0.00000   0.08117   0.97500
hbv11p_long_dyn2                 0.00049   0.00004   0.02197   0.08708   0.00252   0.00000   0.06217   1.00000
hbv2_long_static_cold            0.00356   0.02434   0.06801   0.18896   0.00000   0.02386   0.07450   0.98214
hbv_long_ties                    0.00825   0.00109   0.05100   0.05577   0.00000   0.00000   0.05664   1.00000
hbv_long_muwts                   0.00003   0.00000   0.00920   0.03774   0.00000   0.00000   0.06750   0.98958
hbv_long_muwts_dyn2              0.00000   0.00000   0.01324   0.07107   0.00000   0.00000   0.02105   1.00000
--- existing suite: test_gpu_parity.ORACLE_CASES (seed 7) and STREAM2_CASES (seed 21), records of 100 days and more ---
ORACLE Hbv T400 B37 M16 0dyn     0.00018   0.00007   0.01521   0.10092   0.00000   0.00000   0.05803   0.99831
ORACLE Hbv T300 B21 M16 2dyn     0.00028   0.00003   0.02119   0.09581   0.00013   0.00000   0.05701   0.99405
ORACLE Hbv T200 B130 M1 1dyn     0.00008   0.00004   0.01546   0.07319   0.00000   0.00000   0.08031   0.98462
ORACLE Hbv T150 B19 M5 2dyn      0.00239   0.00863   0.03684   0.06660   0.00000   0.00856   0.08014   0.84211
ORACLE Hbv T100 B5 M64 0dyn      0.00003   0.00003   0.00856   0.06944   0.00000   0.00000   0.10525   0.77500
ORACLE Hbv_1_1p T250 B23 M16 14dyn   0.01577   0.02639   0.10327   0.15862   0.00013   0.02637   0.05557   1.00000
ORACLE Hbv_2 T250 B40 M8 3dyn    0.00066   0.00005   0.05080   0.22020   0.00021   0.00000   0.08799   0.91875
ORACLE Hbv T129 B3 M16 3dyn      0.00000   0.00000   0.01227   0.09835   0.00000   0.00000   0.10627   1.00000
STREAM2 Hbv T140 B9 M16 0dyn     0.00010   0.00010   0.01195   0.06895   0.00000   0.00000   0.11498   0.92361
STREAM2 Hbv T133 B10 M16 2dyn    0.00000   0.00000   0.00672   0.05559   0.00324   0.00000   0.11212   0.92500
STREAM2 Hbv_2 T150 B11 M16 3dyn   0.00197   0.00330   0.04924   0.23034   0.00000   0.00322   0.09413   0.95455
STREAM2 Hbv T140 B9 M16 1dyn     0.00010   0.00010   0.01096   0.07406   0.00000   0.00000   0.11498   0.92361
STREAM2 Hbv_2 T150 B11 M16 2dyn   0.00193   0.00330   0.05072   0.22947   0.00015   0.00322   0.09413   0.95455
STREAM2 Hbv T140 B9 M16 5dyn     0.00427   0.00868   0.04916   0.09301   0.00045   0.00868   0.11424   0.91667
STREAM2 Hbv_2 T150 B11 M16 6dyn   0.00117   0.00008   0.05519   0.23780   0.00000   0.00000   0.09413   0.95455
--- new fixtures ---
hbv_wet_dyn3                     0.01458   0.00354   0.15750   0.28625   0.00125   0.00292   0.00688   1.00000
hbv11p_wet_list_drop             0.03750   0.03375   0.16687   0.22167   0.01354   0.03354   0.01833   1.00000
hbv2_wet_muwts_routing           0.04172   0.00344   0.23750   0.29688   0.00219   0.00266   0.05297   1.00000
--- new ABI-level problems and long records of Hbv (tests/daily_sets.py) ---
wet400                           0.02206   0.00235   0.15507   0.38930   0.00029   0.00125   0.06621   0.98529
wet400-d3                        0.01805   0.00235   0.15346   0.38930   0.00029   0.00125   0.06621   0.98529
wet400-static                    0.01637   0.00302   0.13561   0.30503   0.00000   0.00123   0.08950   0.99306
dry300-betaet                    0.00130   0.00250   0.08861   0.19861   0.02759   0.00000   0.06333   1.00000
wet1460                          0.01010   0.00146   0.12440   0.25670   0.00000   0.00036   0.08915   1.00000
wet129-muwts                     0.02574   0.00417   0.17141   0.29029   0.00006   0.00411   0.01284   0.64925
wet65-channels                   0.04462   0.00746   0.26355   0.41976   0.00036   0.00746   0.01349   0.68462
wet64-m64                        0.06738   0.00879   0.26685   0.44434   0.00000   0.00830   0.00000   0.42188
wet63-all-drop                   0.09051   0.06098   0.28239   0.26751   0.00018   0.06063   0.01290   0.66176
dry17-list                       0.00000   0.00000   0.00000   0.00433   0.06142   0.00000   0.03720   0.14706
wet16                            0.19916   0.03078   0.56763   0.59795   0.00000   0.02938   0.03685   0.46269
dry15                            0.00000   0.00000   0.00000   0.04167   0.04167   0.00000   0.01250   0.06250
wet2-all-drop                    0.75000   0.37115   0.98269   0.58750   0.00481   0.37019   0.05673   0.35769
wet1                             0.79412   0.45037   0.98529   0.63051   0.00000   0.45037   0.06618   0.26838
wet7300                          0.00195   0.00007   0.37293   0.10399   0.00000   0.00007   0.05151   1.00000
--- new ABI-level problems and long records of Hbv_1_1p (tests/daily_sets.py) ---
wet400                           0.02243   0.00404   0.16919   0.38507   0.00000   0.00243   0.06893   1.00000
wet400-all-drop                  0.04673   0.05243   0.21206   0.26092   0.00000   0.05195   0.05195   1.00000
wet400-list                      0.04526   0.06691   0.28669   0.18474   0.00684   0.06662   0.07467   1.00000
dry300                           0.00917   0.00259   0.04593   0.22176   0.03056   0.00000   0.07704   1.00000
wet129-muwts                     0.02673   0.00376   0.16991   0.38771   0.00006   0.00370   0.02193   0.63433
wet65-channels                   0.04994   0.00828   0.23858   0.44012   0.00012   0.00828   0.02213   0.66154
wet64-m64                        0.05347   0.00854   0.28003   0.66919   0.00195   0.00854   0.00000   0.42188
dry63                            0.00245   0.00058   0.03525   0.05917   0.05859   0.00000   0.10481   0.43382
wet17                            0.18218   0.02809   0.55180   0.60623   0.00088   0.02766   0.03863   0.52239
wet15-list                       0.31373   0.15196   0.71471   0.47549   0.00000   0.15196   0.03529   0.55882
wet2                             0.73077   0.24615   0.98846   0.58462   0.00000   0.24231   0.01923   0.33077
wet1                             0.78309   0.48897   0.96691   0.65809   0.00368   0.48897   0.05515   0.31250
wet1460                          0.01423   0.00255   0.12815   0.46729   0.00015   0.00045   0.09765   1.00000
--- new ABI-level problems and long records of Hbv_2 (tests/daily_sets.py) ---
wet400                           0.01312   0.00761   0.17235   0.46460   0.00000   0.00607   0.08213   0.94118
wet400-muwts                     0.01312   0.00761   0.17235   0.46460   0.00000   0.00607   0.08213   0.94118
wet400-list                      0.01893   0.01460   0.17357   0.50926   0.00000   0.01294   0.08213   0.94118
dry300                           0.04630   0.00991   0.20815   0.43639   0.03954   0.00574   0.08028   0.94444
wet129-static                    0.02673   0.00474   0.19721   0.43746   0.00046   0.00399   0.02997   0.67164
wet65-channels                   0.05290   0.00722   0.26012   0.42071   0.00036   0.00686   0.02083   0.73846
wet64-m64                        0.04810   0.00806   0.28345   0.55664   0.00000   0.00781   0.00000   0.42188
wet63-all-drop                   0.11485   0.07744   0.37442   0.32382   0.00018   0.07721   0.03285   0.61029
dry16                            0.00000   0.00000   0.00460   0.02574   0.02665   0.00000   0.04044   0.10294
wet15-muwts                      0.18657   0.03831   0.57960   0.61244   0.00000   0.03731   0.04527   0.49254
wet2-all-drop                    0.74231   0.36827   0.97500   0.59712   0.00385   0.36827   0.07692   0.34423
wet1                             0.80239   0.44301   0.98070   0.60938   0.00827   0.44301   0.13511   0.21783
wet1460                          0.02472   0.00242   0.18594   0.55771   0.00000   0.00049   0.10920   1.00000
(rain / snow, melt limited by the pack or by the potential, refreezing limited by the meltwater or by the potential,
tosoil > 0, wetness and ef free, evaporation limited by PET, the floor of SM, PERC = SUZ, and for the capillary models
capillary rise by the formula and the floor of SLZ are asserted too; for Hbv_2 both sides of elevation 2000 and of ac
2500, both clamps of (ac - parAC) / 1000 and its free range, the exp clamp and its free range, and SLZ + lf clamped at 0.)

What the table says of the suite as found: 19 of the 32 older fixtures never take Q0 > 0; one (hbv2_long_dyn3) takes
Q0, the soil excess, PERC = parPERC and soil-limited evaporation in 0.1 % of its lane-days each, no Hbv or Hbv_1_1p
fixture does; no synthetic problem of test_gpu_parity.py does, and the static-parameter ones stay under 0.1 % in Q0 and
under 0.02 % in the soil excess.  (The all-dynamic Hbv_1_1p problem and the cold Hbv problem of ORACLE_CASES do take the
soil excess in 0.9-2.6 % of their lane-days: dynamic parFC moves under the soil moisture.)

Unreachable branches, asserted never to occur (daily_sets.NEVER, and et_sm_limited for Hbv without parBETAET):
 * capillary rise limited by SLZ: cap = min(SLZ, parC * SLZ * (1 - min(SM / FC, 1))) with parC <= 1 and SLZ >= 0, so the
   second argument is at most SLZ.  The reference's min() is dead code there; the adjoint branch `wa` of
   minw(SLZ, capp) is unreachable (an SLZ carried in as 0 gives min(0, 0): not "SLZ < capp").
 * the floor of SM after capillary rise: SM >= nearzero already and cap >= 0.
 * soil-limited evaporation for Hbv without parBETAET: AET = min(SM, PET * min(SM / (LP * FC), 1)); with the factor
   below 1, SM < PET * SM / (LP * FC) needs LP * FC < PET, and LP * FC >= 0.2 * 50 = 10 mm while synth.forcing's PET is
   at most 6 mm/d; with the factor at 1, SM >= LP * FC >= 10 > PET.  With parBETAET < 1 in the table the factor of a dry
   soil is large enough (a soil of 0.0005 mm, BETAET 0.3: 0.03), and the branch is taken.

Protocol (tests/hourly_sets.py::compare_f64 through daily_sets.compare_f64): abi_util's committed tolerances.  g_params
(the two routing columns at ROUTE_ATOL_REL), g_muwts and the four routed rows are compared whole, with no exclusion.  An
element of flux, traj, state_out or g_x outside tolerance against float64 is admitted only if the oracle agrees there, at
the same tolerance, with the restatement run in float32; admitted elements are counted, printed and capped at 2e-3 of
the array.  The problem lists were chosen so that this holds here, on the CPU.  No element had to be named at ABI level
(nothing is named in tests/daily_sets.py); one element of the fixture hbv_wet_dyn3 is named in
tests/test_restate64.py with its float64 evidence (the floor of SM met exactly at its corner).

What the admitted elements are (oracle against float64; the float32 restatement shares every one of them):
 * forcing gradient -- d loss / d PET of days with PET exactly 0 (half of synth.forcing's midwinter days) on a soil that
   sits at FC to an ulp after shedding its excess: it stays there while nothing evaporates, and the masks SM / FC <= 1,
   (SM / FC) ** BETA <= 1 and excs >= 0 fall by the last bit.  From a wet start on day 0 this class alone was 11 of 3417
   elements of g_x on a 17-day problem (3.2e-3, above the cap), and on Hbv_2's wet400-muwts three elements agreed with no
   float32 evaluation (oracle -0.1304, float64 -0.3534 at g_x[0, 12, 2]: three evaluations, three resolutions of the
   tie).  The wet problems therefore start on day 120, where PET > 0 dries the soil below FC within the day; what is left
   are single midwinter days of the long records (Hbv_1_1p wet400 g_x[243, 7, 2]: oracle = float32 restatement 0.372533,
   float64 0.365882).
 * storages and flux rows -- the day a snowpack melts out (SNOWPACK keeps 0.1-2 mm of a pack of tens of mm, float32's
   accumulated rounding of the pack is its fourth digit; tests/test_restate64.py names the same thing on the Hbv_2
   fixtures) and the SWE / tosoil rows of that day: Hbv wet1460 SNOWPACK[417, lane 13] oracle = float32 restatement
   0.2550240, float64 0.2551091; tosoil[417, basin 3] 0.0690794 against 0.0691024.

Admitted elements, oracle against float64 (outside = admitted in every row; cap = 2e-3 of the array); g_params, g_muwts
and routed: none outside in any problem:

problem                 flux            traj            g_x
Hbv wet400              0               1 / 136340      1 / 20400
Hbv wet400-d3           0               0               1 / 20400
Hbv wet400-static       0               1 / 288720      0
Hbv wet1460             2 / 128480      6 / 233760      0
Hbv wet129-muwts        0               0               1 / 25929
Hbv wet7300             17 / 321200     11 / 292040     0
Hbv_1_1p wet400         1 / 81600       2 / 136340      0
Hbv_1_1p wet400-all-d.  2 / 81600       2 / 136340      3 / 20400
Hbv_1_1p wet400-list    5 / 81600       11 / 136340     1 / 20400
Hbv_1_1p wet129-muwts   0               1 / 87100       0
Hbv_1_1p dry63          0               3 / 87040       0
Hbv_1_1p wet1460        0               7 / 233760      0
Hbv_2 wet400            1 / 81600       0               4 / 20400
Hbv_2 wet400-muwts      1 / 81600       0               4 / 20400
Hbv_2 wet400-list       0               1 / 136340      0
Hbv_2 dry300            1 / 32400       2 / 54180       0
Hbv_2 wet63-all-drop    0               0               1 / 3213
Hbv_2 wet1460           0               1 / 233760      0
(the other 23 problems: nothing outside.)  The largest share is 2.0e-4 (Hbv_2 wet400, g_x).

float64 cost on 8 host threads: up to 0.6 s per problem up to 129 days, 0.9-2.7 s (300-400 days), 5-7 s (1460 days),
29 s (7300 days); the whole module 1 min on an otherwise idle host.
"""
import time

import numpy as np
import pytest
import torch

from . import abi_util as au
from . import daily_sets as ds
from . import golden_cases as gc
from . import restate_util as ru

_CACHE = {}
DAILY_CASES = [n for n, s in gc.CASES.items() if s["model"] in ds.MODELS]
WET_CASES = [n for n in DAILY_CASES if gc.CASES[n].get("wet_start")]
ALL = [(m, n) for m in ds.MODELS for n in ds.problems(m)]


def f64_run(model, name):
    """(problem, float64 result, coverage) of a problem of the sets, computed once per session."""
    key = (model, name)
    if key not in _CACHE:
        prob = ds.make(model, ds.problems(model)[name])
        ev = {}
        t = time.time()
        res = ru.abi_daily(prob, torch.float64, events=ev)
        cov = ds.coverage(ev)
        print(f"{model} {name}: float64 forward + backward {time.time() - t:.1f} s on {torch.get_num_threads()} threads")
        _CACHE[key] = (prob, res, cov)
    return _CACHE[key]


@pytest.mark.parametrize("model", ds.MODELS)
def test_new_problem_sets_take_the_branches(model):
    """Each model's set (long records included) takes every listed branch in at least 0.1 % of the lane-days (or lanes)
    of one of its problems; its wet400 problem and its long records take Q0 > 0, the soil excess and PERC = parPERC at
    that rate (the 7300-day record the soil excess at all); the branches argued unreachable in the module docstring
    never occur, and Hbv without parBETAET never limits evaporation by the soil moisture."""
    rows = {n: f64_run(model, n)[2] for n in ds.problems(model)}
    ds.assert_covered(model, rows, model)
    for n in ["wet400"] + list(ds.LONG_RECORDS[model]):
        c = rows[n]
        assert min(c["Q0"], c["perc_par"]) >= ds.COVER_MIN and c["meltout"] > 0, (model, n, c)
        assert c["excs"] >= (ds.COVER_MIN if n != "wet7300" else 5e-5), (model, n, c)
    for n in ds.problems(model):
        if ds.hbv_without_betaet(f64_run(model, n)[0]):
            assert rows[n]["et_sm_limited"] == 0.0, (model, n)


def _fixture_coverage(name):
    ev = {}
    ru.case_reverse(name, torch.float64, events=ev)
    return ds.coverage(ev)


WET_KEYS = ("Q0", "excs", "perc_par", "et_sm_limited")


def _all_four(c):
    return min(c[k] for k in WET_KEYS) >= ds.COVER_MIN


def test_wet_fixtures_take_the_branches_and_the_older_inputs_do_not():
    """Each of the three wet fixtures takes Q0 > 0, excs > 0, PERC = parPERC and evaporation limited by the soil
    moisture in at least 0.1 % of its lane-days, in the reference's own tape.  No other Hbv or Hbv_1_1p fixture does
    (of the Hbv_2 ones, hbv2_long_dyn3 does; the table shows 19 older fixtures that take Q0 > 0 in no lane-day at
    all).  No synthetic problem of test_gpu_parity.py (ORACLE_CASES, STREAM2_CASES; records of 100 days and
    more) takes all four at that rate, and every static-parameter one stays under 0.1 % in Q0 and under 0.02 % in the
    soil excess (the table of the module docstring)."""
    from .test_gpu_parity import ORACLE_CASES, STREAM2_CASES
    rows = {n: _fixture_coverage(n) for n in DAILY_CASES if not gc.CASES[n].get("two_call")}
    synth_rows = {}
    for tag, cases, seed in (("ORACLE", ORACLE_CASES, 7), ("STREAM2", STREAM2_CASES, 21)):
        for kw in cases:
            if kw["model"] in ds.MODELS and kw["T"] >= 100:
                prob = au.make_problem(seed=seed, **kw)
                ev = {}
                ru.abi_daily(prob, torch.float64, backward=False, events=ev)
                synth_rows[f"{tag} {kw['model']} T{kw['T']} B{kw['B']} M{kw['M']} {len(kw['dyn'])}dyn"] = ds.coverage(ev)
    print(ds.format_coverage({**rows, **synth_rows}))
    assert len(WET_CASES) == 3 and {gc.CASES[n]["model"] for n in WET_CASES} == set(ds.MODELS)
    assert all(_all_four(rows[n]) for n in WET_CASES), {n: rows[n] for n in WET_CASES}
    older = {n: c for n, c in rows.items() if n not in WET_CASES}
    assert not [n for n, c in older.items() if _all_four(c) and gc.CASES[n]["model"] != "Hbv_2"]
    assert not [n for n, c in synth_rows.items() if _all_four(c)]
    for n, c in synth_rows.items():
        if n.endswith(" 0dyn"):
            assert c["Q0"] < 1e-3 and c["excs"] < 2e-4, (n, c)


@pytest.mark.parametrize("model,name", ALL, ids=[f"{m}-{n}" for m, n in ALL])
def test_oracle_matches_float64(model, name, oracle_path):
    prob, want, _ = f64_run(model, name)
    got = au.run_problem(prob, oracle_path, device="cpu", x_grad=True)
    ds.compare_f64(prob, got, want, [lambda: ru.abi_daily(prob, torch.float32)], f"oracle-f64 {model} {name}")
