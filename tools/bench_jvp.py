#!/usr/bin/env python3
"""Time the plain forward call of Hbv against forward + JVP (torch.autograd.forward_ad, one tangent direction on the
raw parameters) -- the protocol of tools/bench_one.py: W warm-up + K timed calls, each between two HIP events, median.
One JSON line per shape:

    python tools/bench_jvp.py --steps 10 --warmup 3
    static   671 basins x 16 members x 7300 days, every parameter static
    dyn2     100 basins x 16 members x  730 days, parBETA and parBETAET dynamic
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

SHAPES = {"static": (671, 16, 7300, ()), "dyn2": (100, 16, 730, ("parBETA", "parBETAET"))}


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import hydrodl2_amd
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    for name in args.shapes:
        B, M, T, dyn = SHAPES[name]
        n = 12 + (1 if "parBETAET" in dyn else 0)
        ny = n * M + 2
        model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "dynamic_params": {"Hbv": list(dyn)}}, dev)
        x = torch.rand((T, B, 3), device=dev, generator=g) * torch.tensor([20.0, 30.0, 5.0], device=dev)
        x[..., 1] -= 10.0
        p = torch.randn((T, B, ny), device=dev, generator=g)
        d = torch.randn((T, B, ny), device=dev, generator=g)

        def plain():
            with torch.no_grad():
                model({"x_phy": x}, p)

        def dual():
            with fwAD.dual_level():
                out = model({"x_phy": x}, fwAD.make_dual(p, d))
                fwAD.unpack_dual(out["streamflow"]).tangent

        f_med, f_min, f_max = _median_ms(plain, args.steps, args.warmup)
        j_med, j_min, j_max = _median_ms(dual, args.steps, args.warmup)
        print(json.dumps({"shape": name, "B": B, "M": M, "T": T, "dynamic": list(dyn),
                          "forward_ms_median": round(f_med, 3), "forward_ms_range": [round(f_min, 3), round(f_max, 3)],
                          "forward_jvp_ms_median": round(j_med, 3),
                          "forward_jvp_ms_range": [round(j_min, 3), round(j_max, 3)],
                          "ratio": round(j_med / f_med, 3)}), flush=True)
        del p, d, x, model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
