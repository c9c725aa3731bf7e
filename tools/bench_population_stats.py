#!/usr/bin/env python3
"""Time `population_stats` (hydrodl2_amd/population.py, hbvx_population_stats in include/hbvx.h) against
`population_cost` on the same tree and against the route to a KGE per candidate there is without it:
`population_cost(return_series=True)` plus float64 KGE in torch over the [P,T_out,B] series.

    python tools/bench_population_stats.py [--steps 5] [--warmup 2] [--cands 16,64,256] [--models hbv,hbv_2]
                                           [--small-only | --big-only] [--cost-only] [--lib other.so]

Every parameter static, routing on: 12 * nmul + 2 candidate columns for Hbv (194 at nmul 16).  Two shapes, 671 x 16 x
7300 and 100 x 16 x 730, P in {16, 64, 256}.  One process; every variant is warmed at every shape it is timed at; a
timed repetition is one whole call between two HIP events, the variants alternating repetition by repetition; median
[min, max] over the repetitions.  Per (model, shape, P) one JSON line per variant with its peak memory (torch's
allocator, above what the inputs hold) and the kernel by itself (the library call timed by events of its own), and one
with the worst difference of the KGE of the two routes, |new - route| / (1 + |1 - route|).
--cost-only --lib <another build of the library> times `population_cost` alone on that library (when its cost-form
k_pop instances are the same instructions as this tree's by tools/compare_code.py, the figure on this tree is its own)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_population import peak_mb, timed  # noqa: E402


def kge_of_series(series, target):
    """Gupta 2009 per (candidate, basin) from the series, float64, unit weights: what a user does today."""
    s, o = series.double(), target.double()
    ms, mo = s.mean(1), o.mean(0)
    ds, do = s - ms.unsqueeze(1), o - mo
    sd_s, sd_o = ds.pow(2).mean(1).sqrt(), do.pow(2).mean(0).sqrt()
    r = (ds * do).mean(1) / (sd_s * sd_o)
    return 1 - ((r - 1) ** 2 + (sd_s / sd_o - 1) ** 2 + (ms / mo - 1) ** 2).sqrt()


def problem(name, dev, T, B, M):
    import hydrodl2_amd
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    gen = torch.Generator(device=dev).manual_seed(4)
    x_dict = {"x_phy": torch.from_numpy(synth.forcing(T, B, 92)).to(dev)}
    if name == "hbv_2":
        model = hydrodl2_amd.load_model("hbv_2", "Hbv_2")({"nmul": M, "dynamic_params": {"Hbv_2": []}}, dev)
        p = (torch.rand((T, B, model.learnable_param_count1), generator=gen, device=dev) * 0.96 + 0.02,
             torch.rand((B, model.learnable_param_count2), generator=gen, device=dev) * 0.96 + 0.02)
        x_dict["ac_all"] = torch.rand((B,), generator=gen, device=dev) * 2000 + 10
        x_dict["elev_all"] = torch.rand((B,), generator=gen, device=dev) * 3000
        row = p[1]
    else:
        model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "dynamic_params": {"Hbv": []}}, dev)
        p = torch.randn((T, B, model.learnable_param_count), generator=gen, device=dev)
        row = p[-1]
    _, cols = hydrodl2_amd.sensitivity.jacobian_columns(model, None)

    def draw(P):
        if name == "hbv_2":
            cand = (row[:, cols].unsqueeze(0) + 0.2 * (torch.rand((P, B, len(cols)), generator=gen, device=dev) - 0.5)).clamp(0.02, 0.98)
        else:
            cand = row[:, cols].unsqueeze(0) + 0.5 * torch.randn((P, B, len(cols)), generator=gen, device=dev)
        cand[0] = row[:, cols]
        return cand.contiguous()

    with torch.no_grad():
        flow = model(x_dict, p)["streamflow"][..., 0]
        target = (flow * torch.exp(0.2 * torch.randn(flow.shape, generator=gen, device=dev)) + 0.01).clone()
    return model, x_dict, p, target, draw, len(cols)


def bench_shape(args, dev, name, T, B, M, cands):
    import hydrodl2_amd
    from hydrodl2_amd import ops
    model, x_dict, p, target, draw, C = problem(name, dev, T, B, M)
    for P in cands:
        cand = draw(P)
        variants = {"population_cost": lambda: hydrodl2_amd.population_cost(model, x_dict, p, cand, target)["cost"]}
        if not args.cost_only:
            def new(transform):
                st = hydrodl2_amd.population_stats(model, x_dict, p, cand, target, transform=transform)
                return hydrodl2_amd.population_score(st, "kge")

            def route():
                got = hydrodl2_amd.population_cost(model, x_dict, p, cand, target, return_series=True)
                return kge_of_series(got["series"], target)

            for transform in ("none", "sqrt", "log"):
                variants[f"population_stats({transform}) + population_score(kge)"] = lambda t=transform: new(t)
            variants["population_cost(return_series) + float64 KGE in torch"] = route
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        last = {}
        for _ in range(args.steps):
            for k, fn in variants.items():
                t, last[k] = timed(fn)
                ms[k].append(t)
        base = {"model": name, "T": T, "B": B, "M": M, "C": C, "P": P}
        for k, fn in variants.items():
            mem = peak_mb(fn)
            ops.KERNEL_EVENTS = []
            fn()
            torch.cuda.synchronize()
            calls = {}
            for n, e0, e1 in ops.KERNEL_EVENTS:
                if n.startswith("hbvx_population"):
                    calls[n] = round(calls.get(n, 0.0) + e0.elapsed_time(e1), 3)
            ops.KERNEL_EVENTS = None
            print(json.dumps(dict(base, variant=k, ms_median=round(statistics.median(ms[k]), 3),
                                  ms_range=[round(min(ms[k]), 3), round(max(ms[k]), 3)], reps=len(ms[k]), peak_mb=mem,
                                  kernel_ms=calls)), flush=True)
        if not args.cost_only:
            a = last["population_stats(none) + population_score(kge)"]
            b = last["population_cost(return_series) + float64 KGE in torch"]
            ok = torch.isfinite(b)
            diff = float(((a - b).abs() / (1 + (1 - b).abs()))[ok].max())
            print(json.dumps(dict(base, variant="KGE of the two routes", worst_difference=diff,
                                  kge_range=[round(float(b[ok].min()), 3), round(float(b[ok].max()), 3)],
                                  without_a_score=[int((~torch.isfinite(a)).sum()), int((~ok).sum())])), flush=True)
        del cand, last
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cands", default="16,64,256")
    ap.add_argument("--models", default="hbv,hbv_2")
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--big-only", action="store_true")
    ap.add_argument("--cost-only", action="store_true", help="time population_cost alone (a library of the parent commit)")
    ap.add_argument("--lib", default=None, help="time another build of the library")
    args = ap.parse_args()
    if args.lib:
        from hydrodl2_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    cands = [int(v) for v in args.cands.split(",")]
    for name in args.models.split(","):
        if not args.big_only:
            bench_shape(args, dev, name, 730, 100, 16, cands)
        if not args.small_only:
            bench_shape(args, dev, name, 7300, 671, 16, cands)


if __name__ == "__main__":
    main()
