"""GPU tier: Hbv_2_mts on the HIP library against the float64 restatement of the multi-timescale orchestration
(tests/mts_sets.py, pinned to the reference's fixtures by tests/test_mts_f64.py, which also documents the problems, the
branch coverage and the protocol).

 (1) every problem of mts_sets.PROBLEMS under the default dispatch; records of 129 hours and more run the time-parallel
     adjoint -- the first time any adjoint family but the short-record one produces the gradient of `low_sta` through
     the three-tensor parameter sources that only Hbv_2_mts builds;
 (2) `wet400` and `wet400-lists` under every entry of test_hourly_f64_gpu.FAMILIES, with the dispatch asserted;
 (3) `wet200-m16-sim` with every input and parameter tensor on the host and the model on the GPU: outputs and the
     gradients (which arrive on the host leaves) against float64, the assembled Qs bit for bit against one block;
 (4) the temporal routing windows: `wet130-m1-sim` with train_warmup = 72 in windows of 40 rows against the windowed
     float64 restatement and against gage routing over the whole record (every kept row has its 72 taps inside its window);
 (5) the resume path: load_from_cache on hours [0, 200), use_from_cache on [200, 400).

Tolerances: abi_util's committed ones.  The hourly state series goes through hourly_sets.admit against the C oracle and
the restatement in float32.  Admitted elements seen on the MI355X, the same in every family: wet400 33 / 296000,
wet400-lists 56 / 296000 (cap 592); resume 4 and 37 / 148000 (cap 296); the other problems none.  The two-piece Qs of
the resume test equalled the one-piece Qs bit for bit (printed, not asserted).

Measured on the MI355X machine (16 host threads): float64 forward + backward 0.7 s (wet400), 0.5 s (wet400-lists), 0.9 s
(wet200-m16-sim), 0.3 s (wet130-m1-sim), 0.1 s (dry96), once per problem and shared.  Per test: (1) 1.1, 0.6, 1.4, 0.3,
0.1 s (float64 run and the oracle's float32 evaluation included); (2) 0.01 s for each of the 14; (3) 0.02 s; (4) 0.1 s;
(5) 0.3 s; the whole module 6 s.
"""
import time

import numpy as np
import pytest
import torch

from . import mts_sets as ms
from . import seam
from .test_hourly_f64_gpu import FAMILIES
from .test_mts_f64 import f64_run, resume_check, windows_check

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle_eval(name, spec, oracle_path):
    """The same problem through Hbv_2_mts on the C oracle, once per session (a float32 evaluation for `admit`)."""
    def f():
        if name not in _ORACLE:
            seam.use_library(oracle_path)
            try:
                _ORACLE[name] = ms.run_model(spec, "cpu")
            finally:
                seam.use_library(None)
        return _ORACLE[name]
    return f


def _gpu_against_float64(name, env_id, hip_backend, oracle_path, **run_kw):
    spec, want, _ = f64_run(name)
    t = time.time()
    got = ms.run_model(spec, "cuda:0", **run_kw)
    fwd, bwd = hip_backend.last_dispatch(0), hip_backend.last_dispatch(1)
    print(f"{name} [{env_id}]: forward {fwd}, adjoint {bwd}, {time.time() - t:.2f} s")
    ms.compare_f64(spec, got, want, [_oracle_eval(name, spec, oracle_path), lambda: ms.mts_reverse(spec, torch.float32)],
                   f"mts gpu-f64 {name} [{env_id}]")
    return got, fwd, bwd


@pytest.mark.parametrize("name", list(ms.PROBLEMS))
def test_problem_matches_float64(name, hip_backend, oracle_path):
    """(1)"""
    _, fwd, bwd = _gpu_against_float64(name, "default", hip_backend, oracle_path)
    if ms.PROBLEMS[name]["T_high"] >= 129:
        assert bwd == "chunked", (fwd, bwd)


@pytest.mark.parametrize("env_id", list(FAMILIES))
@pytest.mark.parametrize("name", ["wet400", "wet400-lists"])
def test_wet_problem_under_every_adjoint_family(name, env_id, hip_backend, oracle_path, monkeypatch):
    """(2)"""
    env, (want_fwd, want_bwd) = FAMILIES[env_id]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, fwd, bwd = _gpu_against_float64(name, env_id, hip_backend, oracle_path)
    assert (want_fwd is None or fwd == want_fwd) and bwd == want_bwd, f"{name} [{env_id}]: ran {(fwd, bwd)}"


def test_host_resident_inputs(hip_backend, oracle_path):
    """(3) -- the GPU twin of test_mts.py::test_spatial_chunking_does_not_change_runoff, with the tensors where a
    simulation keeps them."""
    name = "wet200-m16-sim"
    got, _, _ = _gpu_against_float64(name, "host inputs", hip_backend, oracle_path, input_dev="cpu")
    one = ms.run_model(ms.PROBLEMS[name], "cuda:0", input_dev="cpu", simulate_spatial_chunk_size=ms.PROBLEMS[name]["B"])
    assert np.array_equal(got["out/Qs"], one["out/Qs"])


def test_routing_windows(hip_backend):
    """(4)"""
    windows_check("cuda:0", "mts gpu windows")


def test_resume_matches_float64(hip_backend):
    """(5)"""
    resume_check("cuda:0", "mts resume gpu")
