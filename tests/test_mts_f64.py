"""CPU tier: Hbv_2_mts through the C oracle against the float64 restatement of the multi-timescale orchestration
(tests/mts_sets.py: a daily `run("Hbv_2")`, the positional hand-off, `run_hourly`, windowed `gage_route`), on problems
whose wetness comes from the forcing (the daily model always starts from its default storages).

 (a) the restatement in float64 reproduces the reference's fixtures mts_train, mts_chunked and mts_wet_lists at
     helpers.compare's tolerances (the pin);
 (b) the problem set takes every listed branch of the hourly step, and hands over wet storages;
 (c) every problem of the set through Hbv_2_mts on the oracle against float64;
 (d) the resume path (load_from_cache, then use_from_cache) against float64 composed the same way and in one piece;
 (e) the temporal routing windows against gage routing over the whole record, where the two must agree.

Branch coverage of the hourly step, share of lane-hours in float64 (meltout: share of lanes), as
test_problem_set_takes_the_branches_and_hands_over_wet_storages prints it (seed 7):

problem                         IE    excess        Q0 et_sm_lim ef_clampe s_clamped  refreeze      rail   meltout
wet400                     0.01122   0.00002   0.24444   0.00000   0.86139   0.00115   0.11069   0.33897   0.35811
wet400-lists               0.01429   0.00002   0.23971   0.00000   0.88843   0.00277   0.11941   0.29733   0.37162
wet200-m16-sim             0.01069   0.00005   0.17041   0.00000   0.84182   0.00496   0.10891   0.33086   0.20455
wet130-m1-sim              0.01745   0.00000   0.28645   0.00000   0.87532   0.00620   0.01791   0.24179   0.11940
dry96                      0.00000   0.00000   0.00000   0.00186   0.00000   0.00000   0.28869   1.00000   0.00000
(the hourly soil excess is printed, not asserted: the daily model hands the soil over at or below FC, so that branch
belongs to the hourly model's own tests, which load storages.)

The hand-off, share of lanes and largest storages in mm:

problem          SUZ > parUZL   SM > FC / 2   pack > 1 mm   SM max   SUZ max   pack max
wet400           0.095          1.00          0.23          944      81.8      1355
wet400-lists     0.122          1.00          0.23          944      81.8      1355
wet200-m16-sim   0.068          0.98          0.19          943      91.0      970
wet130-m1-sim    0.179          1.00          0.24          920      125.2     1482
dry96            0              0             0.82          130      0         131

Admitted elements of the hourly state series, oracle against float64 (outside = admitted in every row; cap 2e-3 of
the array): wet400 33 / 296000, wet400-lists 56 / 296000, the two simulate problems and dry96 none; resume: first call
4 / 148000, second call 38 / 148000.  Everything else: nothing outside tolerance.

float64 cost on 8 host threads: 0.3-2.6 s per problem.

Protocol (mts_sets.compare_f64): abi_util's committed tolerances.  Qs, streamflow and the gradients of low_sta,
high_dyn, high_sta and p_distr are compared whole.  The hourly state series goes through hourly_sets.admit against the
restatement run in float32 (cap 2e-3 of the array).  Exact: grad/low_dyn == 0; grad/high_sta == 0 on the columns the
positional rule never reads (equal lists: the first 13 M; lists (parBETA, parK0, parBETAET) / (parF0, parALPHA, parFMIN,
parBETA): all but the member columns of hourly static positions 1 and 11).
"""
import time

import numpy as np
import pytest
import torch

from . import abi_util as au
from . import golden_mts as gm
from . import hourly_sets as hs
from . import mts_sets as ms
from .helpers import compare, load_golden

_CACHE = {}


def f64_run(name):
    """(spec, float64 result, hourly branch coverage) of a problem of the set, computed once per session."""
    if name not in _CACHE:
        spec = ms.PROBLEMS[name]
        ev = {}
        t = time.time()
        res = ms.mts_reverse(spec, torch.float64, events=ev)
        print(f"{name}: float64 forward + backward {time.time() - t:.1f} s on {torch.get_num_threads()} threads")
        _CACHE[name] = (spec, res, ms.coverage(spec, ev))
    return _CACHE[name]


@pytest.mark.parametrize("name", list(gm.CASES))
def test_restatement_matches_reference_fixture(name):
    """(a)"""
    ref = load_golden(name)
    res = ms.mts_reverse(gm.CASES[name], torch.float64)
    want = {k: ref[k] for k in ref.files if k.startswith(("out/", "grad/"))}
    assert sorted(k for k in res if k.startswith("out/")) == sorted(k for k in want if k.startswith("out/"))

    class R(dict):
        files = property(lambda self: list(self))
    compare(name, res, R(want))


def test_problem_set_takes_the_branches_and_hands_over_wet_storages():
    """(b)"""
    rows = {n: f64_run(n)[2] for n in ms.PROBLEMS}
    ms.assert_covered(rows)
    print("excess (not asserted): " + ", ".join(f"{n} {c['excess']:.5f}" for n, c in rows.items()))
    shares = {n: ms.handoff_shares(ms.PROBLEMS[n], f64_run(n)[1]) for n in ms.PROBLEMS}
    for n, s in shares.items():
        print(f"{n:16s} " + " ".join(f"{k} {v:.4g}" for k, v in s.items()))
    assert any(all(s[k] >= v for k, v in ms.HANDOFF_MIN.items()) for n, s in shares.items() if n.startswith("wet")), shares
    assert rows["dry96"]["et_sm_limited"] >= hs.COVER_MIN


@pytest.mark.parametrize("name", list(ms.PROBLEMS))
def test_oracle_matches_float64(name, oracle_backend):
    """(c).  Admitted elements of the state series seen here: wet400 33 / 296000, wet400-lists 56 / 296000 (cap 592),
    the other problems none."""
    spec, want, _ = f64_run(name)
    got = ms.run_model(spec, "cpu")
    ms.compare_f64(spec, got, want, [lambda: ms.mts_reverse(spec, torch.float32)], f"mts oracle-f64 {name}")


def resume_check(dev, label):
    """(d) -- shared with the GPU tier."""
    spec, split = ms.RESUME, 200
    inp = gm.build_inputs(spec)
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    params = lambda rows: ([t["low_dyn"], t["low_sta"]], [t["high_dyn"][rows].contiguous(), t["high_sta"], t["p_distr"]])  # noqa: E731
    xd = lambda rows: {"x_phy_low_freq": t["x_low"], "x_phy_high_freq": t["x_high"][rows].contiguous(),  # noqa: E731
                       "ac_all": t["ac_all"], "elev_all": t["elev_all"], "outlet_topo": t["outlet_topo"], "areas": t["areas"]}
    with torch.no_grad():
        one = ms.make_model(spec, dev)
        q_one = one(xd(slice(None)), params(slice(None)))["Qs"].cpu().numpy()
        m = ms.make_model(spec, dev)
        m.load_from_cache = True
        q1 = m(xd(slice(0, split)), params(slice(0, split)))["Qs"]
        s1 = ms.states_of(m)
        m.use_from_cache = True
        q2 = m(xd(slice(split, None)), params(slice(split, None)))["Qs"]
        s2 = ms.states_of(m)
    assert s1.shape[1] == split and s2.shape[1] == spec["T_high"] - split       # get_states(): the latest call's series
    q = torch.cat([q1, q2]).cpu().numpy()
    want = ms.mts_resume(spec, split, torch.float64)
    whole = ms.mts_reverse(spec, torch.float64, backward=False)
    # static parameters: the split changes nothing (float64 two-piece against one-piece, at the flux tolerance)
    au.assert_close(f"{label} float64 two-piece vs one-piece Qs", want["Qs"], whole["out/Qs"])
    au.assert_close(f"{label} float64 two-piece vs one-piece states", np.concatenate([want["states1"], want["states2"]], 1),
                    whole["hif_states"])
    au.assert_close(f"{label} Qs vs two-piece float64", q, want["Qs"])
    au.assert_close(f"{label} Qs vs one-piece float64", q, whole["out/Qs"])
    f32 = {}

    def alt(k):
        def f():
            if not f32:
                f32.update(ms.mts_resume(spec, split, torch.float32))
            return f32[k]
        return f
    for k, s in (("states1", s1), ("states2", s2)):
        hs.admit(f"{label} {k}", s, want[k], [alt(k)], hs._flux_tol)
    print(f"{label}: two-piece Qs equals one-piece Qs bit for bit: {np.array_equal(q, q_one)}")


def test_resume_matches_float64(oracle_backend):
    """(d)"""
    resume_check("cpu", "mts resume oracle")


def windows_check(dev, label):
    """(e) -- shared with the GPU tier.  `wet130-m1-sim` with train_warmup = 72 in windows of 40 rows: the windows
    read rows [0, 112) and [40, 130), the second keeps rows 112..129, each of which has its 72 taps (71 rows of history)
    inside the window; the first window starts where the record starts.  So the windowed streamflow equals gage routing
    over the whole record, in float64 to rounding and on the device within the flux tolerance."""
    base = ms.PROBLEMS["wet130-m1-sim"]
    spec = dict(base, chunks=dict(base["chunks"], train_warmup=72, simulate_temporal_chunk_size=40))
    assert ms.routing_windows(130, 72, 40) == [(0, 112, 0), (40, 130, 72)]
    want = ms.mts_reverse(spec, torch.float64, backward=False)
    inp = {k: torch.as_tensor(v).double() for k, v in gm.build_inputs(spec).items()}
    whole = ms.ru.restate().gage_route(torch.from_numpy(want["out/Qs"][:, :, 0]), inp["p_distr"], inp["outlet_topo"],
                                       inp["areas"]).unsqueeze(-1).numpy()
    assert np.abs(want["out/streamflow"] - whole).max() <= 1e-12 * np.abs(whole).max()
    got = ms.run_model(spec, dev)
    au.assert_close(f"{label} streamflow vs windowed float64", got["out/streamflow"], want["out/streamflow"])
    au.assert_close(f"{label} streamflow vs whole-record float64", got["out/streamflow"], whole)
    # with the problem's own warm-up of 24 rows the second window's one row sees a 25-tap hydrograph: windows matter
    short = f64_run("wet130-m1-sim")[1]["out/streamflow"]
    tol = au.FLUX_ATOL + au.FLUX_RTOL * np.abs(whole)
    assert (np.abs(short - whole) > tol)[-1].any() and not (np.abs(short - whole) > tol)[:-1].any()


def test_routing_windows(oracle_backend):
    """(e)"""
    windows_check("cpu", "mts oracle windows")
