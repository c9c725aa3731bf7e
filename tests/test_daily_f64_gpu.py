"""GPU tier: the daily models' HIP kernels (Step<MODEL_HBV10 / HBV11P / HBV20>, csrc/hbv_step.h, in every kernel family
that instantiates it) against float64: oracle/hbv_restate64.py run in float64 on the host inside the test.
tests/test_restate64.py pins that restatement to the reference's fixtures, tests/test_daily_f64.py compares the C oracle
with it on the same problems and documents the inputs, the branch coverage and the protocol.

 (a) every daily fixture through the drop-in module against the module-level restatement: every output, the storages,
     the parameter gradients and (where the case asks) the forcing gradient;
 (b) the ABI-level problems of tests/daily_sets.py under the default dispatch;
 (c) each model's "wet400" problem (the delta-MG pair dynamic for Hbv and Hbv_1_1p, the three-slot set for Hbv_2: the
     compiled sets; no ensemble weights) under every family the daily models can run, with the (forward, adjoint) pair
     hbvx_last_dispatch reports asserted and printed: the environments of test_gpu_parity.LONG_ENVS (time-parallel, streaming pair packed / eight-
     wave / rows + tiled, the checkpointed adjoints), the serial tiled adjoint, the tiled forward, the one-wave kernels,
     the slot-list streaming form; and both forms of the time-parallel adjoint (one trajectory pass / two passes, with
     hbvx_chunk_form asserted) on the static Hbv problem, the one shape the one-pass form runs;
 (d) the 7300-day record (the benchmark's record length) under the default dispatch and under the streaming pair: float32
     drift over 7300 steps would show here.

Tolerances: abi_util's and helpers.compare's committed ones, nothing new.  g_params (routing columns at ROUTE_ATOL_REL),
g_muwts, the routed rows, every module output and parameter gradient are compared whole.  flux, traj, state_out and
g_x (fixtures: states, grad/x_phy) go through hourly_sets.admit: an element outside tolerance against float64 is
admitted only if the kernel agrees there, at the same tolerance, with a float32 evaluation of the same equations (the
oracle, or the restatement run in float32); admitted elements are counted, printed and capped at 2e-3 of the array; an
element that agrees with neither fails the test.  The fixtures' elements that test_restate64.PRECISION_ONLY names are
reused as they are (a storage element at its bound there; a gradient block that a float32 tie decides is held to the
float32 restatement).

Float64 is computed once per problem (tests/test_daily_f64.py::f64_run) and shared by the families.
Host cost of the float64 runs, measured on the GPU machine's 16 host threads: 0.0-0.2 s per fixture, up to 0.2 s per
problem up to 129 days, 0.4-0.9 s for 300-400 days, 1.6-2.9 s for 1460 days, 9.7 s for the 7300-day record; the whole
module (125 tests) took 32 s of wall time.  The admitted counts of the kernels equal the oracle's in
tests/test_daily_f64.py's table within one element (Hbv wet7300 traj: 10 against 11).
"""
import ctypes as C
import time

import pytest
import torch

from . import abi_util as au
from . import daily_sets as ds
from . import golden_cases as gc
from . import restate_util as ru
from .helpers import run_case
from .test_daily_f64 import ALL, DAILY_CASES, f64_run
from .test_gpu_parity import LONG_ENVS
from .test_restate64 import PRECISION_ONLY

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", DAILY_CASES)
def test_fixture_through_the_module_matches_float64(name, hip_backend):
    """(a)"""
    t = time.time()
    want = ru.case_reverse(name, torch.float64)
    print(f"{name}: float64 {time.time() - t:.1f} s")
    res = run_case(name, "cuda:0")
    ds.compare_case_f64(name, res, want, lambda: ru.case_reverse(name, torch.float32), PRECISION_ONLY.get(name, ()))


def _gpu_against_float64(model, name, env_id, hip_backend, oracle_path, x_grad=True):
    prob, want, _ = f64_run(model, name)
    if not x_grad:
        want = {k: v for k, v in want.items() if k != "g_x"}
    got = au.run_problem(prob, None, device="cuda:0", x_grad=x_grad)
    fwd, bwd = hip_backend.last_dispatch(0), hip_backend.last_dispatch(1)
    print(f"{model} {name} [{env_id}]: forward {fwd}, adjoint {bwd}")
    oracle = au.run_problem(prob, oracle_path, device="cpu", x_grad=x_grad)
    ds.compare_f64(prob, got, want, [oracle, lambda: ru.abi_daily(prob, torch.float32)],
                   f"gpu-f64 {model} {name} [{env_id}]")
    return fwd, bwd


@pytest.mark.parametrize("model,name", [(m, n) for m, n in ALL if n != "wet7300"],
                         ids=[f"{m}-{n}" for m, n in ALL if n != "wet7300"])
def test_abi_problem_matches_float64(model, name, hip_backend, oracle_path):
    """(b), default dispatch: every shape of the lists.  Records of 129 days and more run the time-parallel adjoint."""
    fwd, bwd = _gpu_against_float64(model, name, "default", hip_backend, oracle_path)
    if ds.problems(model)[name]["T"] >= 129:
        assert bwd == "chunked", (fwd, bwd)


# What each environment must have run on a "wet400" problem -- at most three dynamic parameters from a compiled set, no
# ensemble weights, 17 basins x 4 members x 400 days, so every family holds it --: (environment, (forward, adjoint)) as
# hbvx_last_dispatch names them.  The first ten environments are test_gpu_parity.LONG_ENVS'.  On this small grid the
# pipelined forward runs unless the grid size is forced (HBVX_STREAM_MIN=1: the streaming forward, which also writes
# the checkpoints) or the tiled families are switched off; the checkpointed adjoint runs block-wise through the
# time-parallel kernels, serially with its segment in LDS, or as the streaming kernel with its segment on chip.
def _env(env_id):
    return LONG_ENVS[env_id][0]


FAMILIES = {
    "default": (_env("default"), ("pipe", "chunked")),
    "stream2-packed": (_env("stream2-packed"), ("stream2", "stream2")),
    "stream2-8wave": (_env("stream2-8wave"), ("stream2", "stream2")),
    "stream-rows-tiled": (_env("stream-rows-tiled"), ("stream2", "tiled")),
    "ckpt8-blocks": (_env("ckpt8-blocks"), ("pipe", "ckpt-block:chunked")),
    "ckpt4-lds": (_env("ckpt4-lds"), ("pipe", "ckpt-lds")),
    "ckpt16-stream": (_env("ckpt16-stream"), ("stream2", "ckpt-stream2")),
    "ckpt4-onchip": (_env("ckpt4-onchip"), ("pipe", "ckpt-stream2")),
    "ckpt8-onchip": (_env("ckpt8-onchip"), ("pipe", "ckpt-stream2")),
    "ckpt16-onchip": (_env("ckpt16-onchip"), ("pipe", "ckpt-stream2")),
    "bwd-tiled": ({"HBVX_BWD": "tiled"}, ("pipe", "tiled")),
    "fwd-tiled": ({"HBVX_FWD": "tiled"}, ("tiled", "chunked")),
    # the one-wave kernels: HBVX_KERNEL=simple alone swaps the forward (a record of 400 days keeps the time-parallel
    # adjoint); with the time-parallel adjoint switched off as well, the one-wave adjoint runs
    "simple-forward": ({"HBVX_KERNEL": "simple"}, ("simple", "chunked")),
    "simple": ({"HBVX_KERNEL": "simple", "HBVX_BWD": "tiled"}, ("simple", "simple")),
    # the compiled set handed over as a run-time slot list
    "slotlist": ({"HBVX_STREAM_MIN": "1", "HBVX_STREAM_SLOTLIST": "1"}, ("stream2", "stream2")),
}
assert set(LONG_ENVS) <= set(FAMILIES)


@pytest.mark.parametrize("env_id", list(FAMILIES))
@pytest.mark.parametrize("model", ds.MODELS)
def test_wet_problem_under_every_adjoint_family(model, env_id, hip_backend, oracle_path, monkeypatch):
    """(c)"""
    env, want = FAMILIES[env_id]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ran = _gpu_against_float64(model, "wet400", env_id, hip_backend, oracle_path)
    assert ran == want, f"{model} wet400 [{env_id}]: ran {ran}, meant {want}"


def _form(lib) -> int:
    f = lib.dll.hbvx_chunk_form
    f.restype = C.c_int
    return f()


@pytest.mark.parametrize("onepass", [True, False], ids=["one-pass", "two-pass"])
def test_both_forms_of_the_time_parallel_adjoint(onepass, hip_backend, oracle_path, monkeypatch):
    """(c): Hbv with static parameters, no ensemble weights and no forcing gradient runs the static adjoint in one
    trajectory pass; HBVX_CHUNK_ONEPASS=0 runs the two-pass form on the same problem."""
    if not onepass:
        monkeypatch.setenv("HBVX_CHUNK_ONEPASS", "0")
    fwd, bwd = _gpu_against_float64("Hbv", "wet400-static", "one-pass" if onepass else "two-pass", hip_backend,
                                    oracle_path, x_grad=False)
    form = _form(hip_backend)
    print(f"Hbv wet400-static: hbvx_chunk_form {form}")
    assert (fwd, bwd) == ("pipe", "chunked") and form == (1 if onepass else 2), (fwd, bwd, form)


@pytest.mark.parametrize("env_id", ["default", "stream2-packed"])
def test_benchmark_length_record_matches_float64(env_id, hip_backend, oracle_path, monkeypatch):
    """(d)"""
    env, want = FAMILIES[env_id]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ran = _gpu_against_float64("Hbv", "wet7300", env_id, hip_backend, oracle_path)
    assert ran == want, f"Hbv wet7300 [{env_id}]: ran {ran}, meant {want}"
