"""GPU tier: the hourly model's HIP kernels (Step<MODEL_HOURLY>, csrc/hbv_step_hourly.h, in every kernel family that
instantiates it) and the gage-routing kernels against float64: oracle/hbv_restate64.py run in float64 on the host inside
the test.  tests/test_restate64.py pins that restatement to the reference's fixtures, tests/test_hourly_f64.py compares
the C oracle with it on the same problems and documents the inputs, the branch coverage and the protocol.

 (a) every hourly fixture through the drop-in module against the module-level restatement: Qs, streamflow, the state
     series, the gradients of p_dyn, p_sta, p_distr and (the wet fixtures) x_phy;
 (b) the ABI-level problems of tests/hourly_sets.py under the default dispatch, and the wet 400-hour problems under every
     adjoint family the hourly model can run, with what hbvx_last_dispatch reports asserted;
 (c) one water year (8760 hours) under the default dispatch: float32 drift over 8760 steps would show here;
 (d) gage routing against its float64 restatement directly, at the two GPU-only shapes of test_gage_route.py and over
     8760 hours.

Tolerances: abi_util's and helpers.compare's committed ones, nothing new.  g_params, g_muwts, p_dyn / p_sta / p_distr
gradients, Qs and streamflow are compared whole.  flux, traj, state_out and g_x (fixtures: states, grad/x_phy) go through
hourly_sets.admit: an element outside tolerance against float64 is admitted only if the kernel agrees there, at the same
tolerance, with a float32 evaluation of the same equations (the oracle, or the restatement run in float32); admitted
elements are counted, printed and capped at 2e-3 of the array; an element that agrees with neither fails the test.

Named elements (hourly_sets.PRECISION_ONLY: the last remainder of a box running empty; hourly_sets.TIES: the snow-free
min(0, 0) tie in d loss / d P) are held to their own bounds; their float64 evidence is beside them.

Host cost of the float64 runs, measured on the GPU machine's 16 host threads: 0.1-0.3 s per fixture, 0.1-0.5 s per
problem of up to 400 hours, 2.8 s for 2200 hours, 14 s for the water year; the whole module took 39 s of wall time
(float64 results are computed once per problem and shared by the adjoint families).
"""
import time

import numpy as np
import pytest
import torch

from . import abi_util as au
from . import golden_cases as gc
from . import hourly_sets as hs
from . import restate_util as ru
from .helpers import run_case
from .test_hourly_f64 import f64_run

pytestmark = pytest.mark.gpu

HOURLY_CASES = [n for n, s in gc.CASES.items() if s["model"] == "Hbv_2_hourly"]


@pytest.mark.parametrize("name", HOURLY_CASES)
def test_fixture_through_the_module_matches_float64(name, hip_backend):
    """(a)"""
    t = time.time()
    want = ru.hourly_case_reverse(name, torch.float64)
    print(f"{name}: float64 {time.time() - t:.1f} s")
    res = run_case(name, "cuda:0")
    hs.compare_case_f64(name, res, want, lambda: ru.hourly_case_reverse(name, torch.float32))


def _gpu_against_float64(name, kw, env_id, hip_backend, oracle_path):
    prob, want, _ = f64_run(name, kw)
    got = au.run_problem(prob, None, device="cuda:0", x_grad=True)
    fwd, bwd = hip_backend.last_dispatch(0), hip_backend.last_dispatch(1)
    print(f"{name} [{env_id}]: forward {fwd}, adjoint {bwd}")
    oracle = au.run_problem(prob, oracle_path, device="cpu", x_grad=True)
    hs.compare_f64(prob, got, want, [oracle, lambda: ru.abi_hourly(prob, torch.float32)], f"gpu-f64 {name} [{env_id}]", name)
    return fwd, bwd


@pytest.mark.parametrize("name", list(hs.ABI_PROBLEMS))
def test_abi_problem_matches_float64(name, hip_backend, oracle_path):
    """(b), default dispatch: every shape of the list.  Records of 129 hours and more run the time-parallel adjoint."""
    kw = hs.ABI_PROBLEMS[name]
    fwd, bwd = _gpu_against_float64(name, kw, "default", hip_backend, oracle_path)
    if kw["T"] >= 129:
        assert bwd == "chunked", (fwd, bwd)


# what each environment must have run on "wet400" / "wet400-f4" (three / four dynamic parameters, no ensemble weights)
FAMILIES = {
    "chunk16": ({"HBVX_CHUNK": "16"}, (None, "chunked")),
    "stream2-packed": ({"HBVX_STREAM_MIN": "1"}, ("stream2", "stream2")),
    "stream2-8wave": ({"HBVX_STREAM_MIN": "1", "HBVX_STREAM_MW_MIN": "1"}, ("stream2", "stream2")),
    "stream-rows-tiled": ({"HBVX_STREAM_MIN": "1", "HBVX_BWD": "tiled"}, ("stream2", "tiled")),
    "slotlist": ({"HBVX_STREAM_MIN": "1", "HBVX_STREAM_SLOTLIST": "1"}, ("stream2", "stream2")),
    # the one-wave kernels: HBVX_KERNEL=simple alone swaps the forward (a record of 400 hours keeps the time-parallel
    # adjoint); with the time-parallel adjoint switched off as well, the one-wave adjoint runs
    "simple-forward": ({"HBVX_KERNEL": "simple"}, ("simple", "chunked")),
    "simple": ({"HBVX_KERNEL": "simple", "HBVX_BWD": "tiled"}, ("simple", "simple")),
}


@pytest.mark.parametrize("env_id", list(FAMILIES))
@pytest.mark.parametrize("name", ["wet400", "wet400-f4"])
def test_wet_problem_under_every_adjoint_family(name, env_id, hip_backend, oracle_path, monkeypatch):
    """(b), the other families, each on a wet problem."""
    env, (want_fwd, want_bwd) = FAMILIES[env_id]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fwd, bwd = _gpu_against_float64(name, hs.ABI_PROBLEMS[name], env_id, hip_backend, oracle_path)
    assert (want_fwd is None or fwd == want_fwd) and bwd == want_bwd, f"{name} [{env_id}]: ran {(fwd, bwd)}"


def test_water_year_matches_float64(hip_backend, oracle_path):
    """(c)"""
    _, _, cov = f64_run("year8760", hs.LONG_RECORDS["year8760"])
    assert cov["meltout"] > 0 and cov["refreeze"] > 0
    fwd, bwd = _gpu_against_float64("year8760", hs.LONG_RECORDS["year8760"], "default", hip_backend, oracle_path)
    assert bwd == "chunked", (fwd, bwd)


@pytest.mark.parametrize("T,U,G,lag", [(700, 40, 9, True), (1000, 300, 1, False), (8760, 12, 4, True)])
def test_gage_routing_matches_float64(T, U, G, lag, hip_backend):
    """(d)"""
    from .test_gage_route import _problem, _restatement, _run
    pb = _problem(T, U, G, seed=200 + T)
    want = _restatement(pb, lag)
    got = _run(pb, lag, None, "cuda")
    au.assert_close(f"gage-f64 T{T} out", got[0], want[0])
    au.assert_grad_close(f"gage-f64 T{T} grad_qs", got[1], want[1])
    au.assert_grad_close(f"gage-f64 T{T} grad_dp", got[2], want[2], list(range(want[2].shape[-1])))
