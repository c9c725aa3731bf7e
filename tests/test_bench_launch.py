"""CPU tier: `python bench.py --gpus 2` starts its own ranks and prints one JSON line.

The ranks run on the host over gloo with the oracle standing in for the HIP library (installed in
every rank by tests/cpu_seam/sitecustomize.py): what is under test is the launcher, the sharding
(weak for cfg2, strong with an uneven split for cfg5), the max-over-ranks timing and the line's
contract -- not any arithmetic."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(oracle_path, *extra, gpus=2):
    env = dict(os.environ, HBVX_TEST_ABI_LIBRARY=oracle_path, HBVX_TEST_ROOT=ROOT, OMP_NUM_THREADS="1",
               PYTHONPATH=os.path.join(ROOT, "tests", "cpu_seam") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--device", "cpu", "--steps", "2",
           "--warmup", "1", "--no-cpu-baseline", "--no-secondary", *extra]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    assert len(lines[0]) < 4096, len(lines[0])     # a line a driver can read; the full record is on stderr
    return json.loads(lines[0])


def test_self_launch_weak_cfg2(oracle_path):
    r = _run(oracle_path, "--config", "cfg2", "--basins", "6", "--days", "40", "--nmul", "4")
    assert r["n_gpus"] == 2 and r["rccl_ranks"] == 2 and r["scaling"] == "weak"
    # the rank count comes from the collective itself (a ones-vector summed over the ranks), not from the launcher
    assert r["collective_check"] == {"backend": "gloo", "ranks_summed": 2, "nccl_version": None}
    assert r["config"]["basins_total"] == 12 and r["config"]["basins_per_gpu"] == 6
    assert len(r["rank_ms_per_step"]) == 2 and r["ms_per_step"] == pytest.approx(max(r["rank_ms_per_step"]), rel=1e-3)
    assert r["value"] == pytest.approx(12 * 4 * 40 / (r["ms_per_step"] * 1e-3), rel=1e-6)
    assert r["metric"].startswith("basin-ensemble-timesteps/sec") and r["dtype"] == "f32"


def test_self_launch_strong_cfg5_uneven(oracle_path):
    r = _run(oracle_path, "--config", "cfg5", "--basins", "9", "--days", "30", "--nmul", "2")
    assert r["n_gpus"] == 2 and r["scaling"] == "strong"
    assert r["config"]["basins_total"] == 9 and r["config"]["basins_per_gpu"] == 5   # rank 0 of ceil split 5 + 4
    assert r["value"] == pytest.approx(9 * 2 * 30 / (r["ms_per_step"] * 1e-3), rel=1e-6)


def test_self_launch_eight_ranks_weak_cfg2(oracle_path):
    """The shape of the driver's N = 8 run (it is the driver's to launch on the 8-GPU node): eight ranks over gloo,
    every rank its own 671-basin-shaped shard (small here), the collective itself reports eight summed ranks."""
    r = _run(oracle_path, "--config", "cfg2", "--basins", "5", "--days", "24", "--nmul", "2", gpus=8)
    assert r["n_gpus"] == 8 and r["rccl_ranks"] == 8 and r["scaling"] == "weak"
    assert r["collective_check"]["ranks_summed"] == 8
    assert r["config"]["basins_total"] == 40 and r["config"]["basins_per_rank"] == [5] * 8
    assert len(r["rank_ms_per_step"]) == 8 and r["ms_per_step"] == pytest.approx(max(r["rank_ms_per_step"]), rel=1e-3)
    assert r["value"] == pytest.approx(40 * 2 * 24 / (r["ms_per_step"] * 1e-3), rel=1e-6)


def test_self_launch_eight_ranks_strong_cfg5_uneven(oracle_path):
    """configs[4]'s split with a basin count that does not divide: 100 003 basins over eight ranks = seven blocks of
    12 501 and one of 12 496 (sharding.basin_range), one member and a few days so that the CPU stand-in finishes."""
    r = _run(oracle_path, "--config", "cfg5", "--basins", "100003", "--days", "6", "--nmul", "1", gpus=8)
    assert r["n_gpus"] == 8 and r["rccl_ranks"] == 8 and r["scaling"] == "strong"
    per = r["config"]["basins_per_rank"]
    assert per == [12501] * 7 + [12496] and sum(per) == 100003 == r["config"]["basins_total"]
    assert r["config"]["basins_per_gpu"] == 12501
    assert r["value"] == pytest.approx(100003 * 1 * 6 / (r["ms_per_step"] * 1e-3), rel=1e-6)


def test_plain_run_reports_the_headline_alone(oracle_path):
    """One rank without --full: set-up, warm-up, timed steps and the line -- no CPU baselines (which would run here, on the
    host, under --full) and no secondary configurations."""
    env = dict(os.environ, HBVX_TEST_ABI_LIBRARY=oracle_path, HBVX_TEST_ROOT=ROOT, OMP_NUM_THREADS="1",
               WORLD_SIZE="1", RANK="0",
               PYTHONPATH=os.path.join(ROOT, "tests", "cpu_seam") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--device", "cpu", "--steps", "2",
           "--warmup", "1", "--basins", "4", "--days", "20", "--nmul", "2"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    assert r["n_gpus"] == 1 and r["steps"] == 2 and r["warmup"] == 1
    assert r["value"] == pytest.approx(4 * 2 * 20 / (r["ms_per_step"] * 1e-3), rel=1e-6)
    assert "secondary" not in r and "cpu_baseline" not in r
    assert "cpu baselines" not in out.stderr and "secondary configs" not in out.stderr


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--device", "cpu"], env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "WORLD_SIZE" in (out.stderr + out.stdout)


def test_a_rank_that_dies_before_the_rendezvous_ends_the_job_quickly(oracle_path):
    """Rank 1 raises before init_process_group: the parent must stop rank 0 (which is waiting in the
    rendezvous) and exit non-zero within seconds, not after the collective's time-out."""
    import time
    env = dict(os.environ, HBVX_TEST_ABI_LIBRARY=oracle_path, HBVX_TEST_ROOT=ROOT, OMP_NUM_THREADS="1",
               HBVX_BENCH_FAIL_RANK="1",
               PYTHONPATH=os.path.join(ROOT, "tests", "cpu_seam") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--device", "cpu", "--steps", "1",
           "--warmup", "0", "--no-cpu-baseline", "--no-secondary", "--basins", "4", "--days", "20", "--nmul", "2"]
    t0 = time.time()
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    dt = time.time() - t0
    assert out.returncode != 0
    assert dt < 30.0, dt
    assert "[rank 1]" in out.stderr and "injected failure" in out.stderr
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
def test_bench_line_contract_on_gpu():
    """`python bench.py --full` on one GPU (child process): ONE JSON line with every field the driver reads, the
    roofline object priced on live HIP-event kernel times, the CPU baselines with their core count, and
    throughput consistent with the step time.  Small shape, the full code path."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "3", "--warmup", "1", "--no-secondary",
           "--basins", "64", "--days", "730", "--cpu-sample-days", "64"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    assert len(lines[0]) < 4096, len(lines[0])
    r = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in r, key
    assert r["n_gpus"] == 1 and r["steps"] == 3 and r["warmup"] == 1 and r["higher_is_better"] is True
    assert r["dtype"] == "f32" and r["data"] == "synthetic" and r["vs_baseline"] is None and "workload" in r["config"]
    assert r["value"] == pytest.approx(64 * 16 * 730 / (r["ms_per_step"] * 1e-3), rel=1e-6)
    rf = r["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in rf, key
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    # `achieved` and `frac` are rounded independently by bench.py (2 and 5 decimals): compare within those roundings,
    # never relative to a measured value (a value-dependent tolerance made this test a coin flip in round 2)
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) <= 1e-5 + 0.005 / rf["peak"]
    assert 0.0 < rf["avg_ms"] <= r["ms_per_step"] * 1.5
    cb = r["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in cb, key
    # `value` is the eager restatement of the reference's CPU path ("restatement"), the C port stands under "port";
    # only if no eager pass finished within its budget does the port take the value
    assert cb["kind"] in ("restatement", "port") and cb["cores"] >= 1 and cb["value"] > 0
    if cb["kind"] == "restatement":
        assert cb["port"]["kind"] == "port" and cb["port"]["value"] > 0
    smp = r["step_samples"]
    assert smp["n"] == 3 and smp["ms_min"] <= smp["ms_median"] <= smp["ms_max"]


@pytest.mark.gpu
def test_plain_bench_line_on_gpu():
    """`python bench.py` without --full on one GPU: the headline and its roofline, nothing that takes runs of its own."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--basins", "64",
           "--days", "730"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline", "step_samples"):
        assert key in r, key
    assert r["value"] == pytest.approx(64 * 16 * 730 / (r["ms_per_step"] * 1e-3), rel=1e-6)
    assert r["roofline"]["bound"] == "hbm" and 0.0 < r["roofline"]["avg_ms"] <= r["ms_per_step"] * 1.5
    assert "secondary" not in r and "cpu_baseline" not in r
