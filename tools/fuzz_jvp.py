#!/usr/bin/env python3
"""Randomised forward-mode sweep: the tangent kernels of Hbv, Hbv_1_1p and Hbv_2 (torch.autograd.forward_ad on the
HIP path) against forward AD of oracle/hbv_restate64.py in float64, over the draw space of tests/jvp_draws.py at the
tolerance of tests/test_jvp_f64_gpu.py.  Not part of the test tiers: a longer soak for the GPU box.

    python tools/fuzz_jvp.py [n_cases] [seed]
    python tools/fuzz_jvp.py --time-devices [n_cases] [seed]    # time the float64 restatement on the host and the GPU
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tests import jvp_draws as jd  # noqa: E402
from tests.test_jvp_f64_gpu import _compare_all  # noqa: E402


def time_devices(n_cases, seed):
    """Wall time of the float64 restatement per draw, host against GPU, on the same draws."""
    tot = {"cpu": 0.0, "cuda": 0.0}
    for i, spec in enumerate(jd.draws(n_cases, seed)):
        inp, dirs = jd.inputs(spec)
        row = []
        for dev in ("cpu", "cuda"):
            jd.run_restate(spec, inp, dirs, device=dev)          # warm (allocator, kernels)
            torch.cuda.synchronize()
            t = time.perf_counter()
            jd.run_restate(spec, inp, dirs, device=dev)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            tot[dev] += dt
            row.append(f"{dev} {dt:7.3f} s")
        print(f"[{i:3d}] {spec['model']:9s} T={spec['T']:3d} B={spec['B']:3d} M={spec['M']:2d}  " + "  ".join(row),
              flush=True)
    print(f"float64 restatement, {n_cases} draws: host {tot['cpu']:.1f} s ({torch.get_num_threads()} threads), "
          f"GPU {tot['cuda']:.1f} s", flush=True)
    return 0


def main(argv):
    timing = "--time-devices" in argv
    argv = [a for a in argv if a != "--time-devices"]
    n_cases = int(argv[0]) if argv else 60
    seed = int(argv[1]) if len(argv) > 1 else 0
    if timing:
        return time_devices(n_cases, seed)
    bad = 0
    t_start = time.time()
    for i, spec in enumerate(jd.draws(n_cases, seed)):
        try:
            inp, dirs = jd.inputs(spec)
            got = jd.run_hip(spec, inp, dirs)
            want, terms = jd.run_restate(spec, inp, dirs)
            _compare_all(f"draw {i}", got, want, terms)
            status = "ok"
        except AssertionError as e:
            bad += 1
            status = "MISMATCH " + str(e)[:300]
        except Exception as e:  # noqa: BLE001
            bad += 1
            status = "ERROR " + repr(e)[:300]
        print(f"[{i:3d}] {status:8.300s} {spec['model']} T={spec['T']} B={spec['B']} M={spec['M']} dyn={spec['dyn']} "
              f"drop={spec['dy_drop']} warm={spec['warm_up']}/{spec['warm_up_states']} muwts={spec['muwts']} "
              f"routing={spec['routing']} tangent={spec['tangent']} noncontig={spec['noncontig']} seed={spec['seed']}",
              flush=True)
    print(f"{n_cases - bad}/{n_cases} draws agree, {time.time() - t_start:.0f} s", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
