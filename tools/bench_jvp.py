#!/usr/bin/env python3
"""Time the plain forward call of Hbv against forward + JVP (torch.autograd.forward_ad, one tangent direction on the
raw parameters) -- the protocol of tools/bench_one.py: W warm-up + K timed calls, each between two HIP events, median.
One JSON line per shape:

    python tools/bench_jvp.py --steps 10 --warmup 3
    static   671 basins x 16 members x 7300 days, every parameter static
    dyn2     100 basins x 16 members x  730 days, parBETA and parBETAET dynamic

With --directions D [D ...] also, per shape and D, one more line: hydrodl2_amd.jvp_batch of D compact directions on the
raw parameters with keys=('streamflow',) against D sequential one-direction forward_ad calls (the only way without the
batched kernels), the two alternating call by call; ms, ms per direction, the directions per lane (DL) and the grid the
library chose.  --jacobian times the whole static-parameter streamflow Jacobian (parameter_jacobian, 64 directions at a
time).
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


def _alternating_ms(fns, steps, warmup):
    """Medians of several callables timed in turn, call by call (so that drift hits all of them alike)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for fn, out in zip(fns, ms):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def _grid(B, M, D):
    """The launch of hbvx_forward_tangent_batch: one direction per lane (k_tan<.., TanBatchArgs> in csrc/hbv_tan.h), one wavefront
    per 64 / Mp basins (Mp: the next power of two >= M), the directions on the grid's second axis."""
    Mp = 1
    while Mp < M:
        Mp *= 2
    per_wave = 64 // Mp
    return 1, ((B + per_wave - 1) // per_wave, D)


def _directions(args, name, model, x, p, d, D):
    import hydrodl2_amd
    T, B, ny = p.shape
    dirs = torch.randn((D, B, ny), device=p.device)

    def batch():
        with torch.no_grad():
            hydrodl2_amd.jvp_batch(model, {"x_phy": x}, p, {"parameters": dirs}, keys=("streamflow",))

    def sequential():
        for _ in range(D):
            with fwAD.dual_level():
                out = model({"x_phy": x}, fwAD.make_dual(p, d))
                fwAD.unpack_dual(out["streamflow"]).tangent

    dl, grid = _grid(B, model.nmul, D)
    (b_med, b_min, b_max), (s_med, s_min, s_max) = _alternating_ms([batch, sequential], args.steps, args.warmup)
    print(json.dumps({"shape": name, "B": B, "T": T, "D": D, "dl": dl, "grid": list(grid),
                      "batch_ms_median": round(b_med, 3), "batch_ms_range": [round(b_min, 3), round(b_max, 3)],
                      "batch_ms_per_direction": round(b_med / D, 3),
                      "sequential_ms_median": round(s_med, 3), "sequential_ms_range": [round(s_min, 3), round(s_max, 3)],
                      "sequential_ms_per_direction": round(s_med / D, 3), "speedup": round(s_med / b_med, 2)}),
          flush=True)


def _jacobian(args, name, model, x, p):
    import hydrodl2_amd

    def jac():
        with torch.no_grad():
            return hydrodl2_amd.parameter_jacobian(model, {"x_phy": x}, p, max_directions=64)
    try:
        n_cols = len(hydrodl2_amd.sensitivity.jacobian_columns(model)[1])
    except ValueError:
        return
    med, lo, hi = _median_ms(jac, max(1, args.steps // 2), 1)
    print(json.dumps({"shape": name, "jacobian_columns": n_cols, "jacobian_ms_median": round(med, 3),
                      "jacobian_ms_range": [round(lo, 3), round(hi, 3)],
                      "ms_per_column": round(med / n_cols, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--directions", type=int, nargs="+", default=[])
    ap.add_argument("--jacobian", action="store_true")
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
        for D in args.directions:
            _directions(args, name, model, x, p, d, D)
        if args.jacobian:
            _jacobian(args, name, model, x, p)
        del p, d, x, model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
