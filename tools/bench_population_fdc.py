#!/usr/bin/env python3
"""Time `population_fdc_stats` (hydrodl2_amd/population_fdc.py, hbvx_population_fdc in include/hbvx_pop_fdc.h) against
`population_stats` on the same tree -- what the flow scores alone cost -- and against the route to a flow-duration score
there is without it: `population_stats(return_series=True)` plus a chunked compare-and-sum in torch over the
[P,T_out,B] series.

    python tools/bench_population_fdc.py [--steps 5] [--warmup 2] [--cands 16,64,256] [--models hbv,hbv_2] [--thr 15]
                                         [--small-only | --big-only | --m1-only] [--stats-only] [--lib other.so]

Every parameter static, routing on.  Shapes: 671 x 16 x 7300 and 100 x 16 x 730, and one with a single member, 10736 x 1
x 730 (the lanes of the first, a tenth of its days), where a lane owns all K slots; P in {16, 64, 256}, K = 15 (the
default probabilities).  The protocol is tools/bench_population_stats.py's: one process; every variant is warmed at
every shape it is timed at; a timed repetition is one whole call between two HIP events, the variants alternating
repetition by repetition; median [min, max].  Per (model, shape, P) one JSON line per variant with its peak memory
(torch's allocator, above what the inputs hold) and the kernel by itself (the library call timed by events of its own),
and one with the agreement of the two routes' counts and volumes.  The series route is left out where its series would
not fit in --series-gib.
--stats-only --lib <another build of the library> times `population_stats` alone on that library (when its stats-form
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
from bench_population_stats import problem  # noqa: E402


def fdc_of_series(series, thr, chunk=4):
    """(count [P,K,B] int32, volume [P,K,B] float32) from the series, a few candidates at a time: what a user does today."""
    P, _, B = series.shape
    K = thr.shape[0]
    count = torch.empty((P, K, B), dtype=torch.int32, device=series.device)
    volume = torch.empty((P, K, B), dtype=torch.float32, device=series.device)
    for c0 in range(0, P, chunk):
        s = series[c0:c0 + chunk]
        for k in range(K):
            above = s > thr[k]
            count[c0:c0 + chunk, k] = above.sum(1)
            volume[c0:c0 + chunk, k] = torch.where(above, s, torch.zeros((), device=s.device)).sum(1)
    return count, volume


def bench_shape(args, dev, name, T, B, M, cands):
    import hydrodl2_amd
    from hydrodl2_amd import ops
    model, x_dict, p, target, draw, C = problem(name, dev, T, B, M)
    probs = [(i + 1) / (args.thr + 1) for i in range(args.thr)] if args.thr != 15 else None
    for P in cands:
        cand = draw(P)

        def stats():
            st = hydrodl2_amd.population_stats(model, x_dict, p, cand, target)
            return hydrodl2_amd.population_score(st, "kge")

        variants = {"population_stats(none) + population_score(kge)": stats}
        with_route = P * T * B * 4 / 2 ** 30 <= args.series_gib
        if not args.stats_only:
            def new():
                st = hydrodl2_amd.population_fdc_stats(model, x_dict, p, cand, target, probs=probs)
                return (hydrodl2_amd.population_score(st, "kge"), hydrodl2_amd.population_fdc_score(st, "fdc_freq"),
                        st["fdc"]["count"], st["fdc"]["volume"], st["fdc"]["thresholds"])

            def route():
                st = hydrodl2_amd.population_stats(model, x_dict, p, cand, target, return_series=True)
                return fdc_of_series(st["series"], thresholds)

            variants["population_fdc_stats + kge + fdc_freq"] = new
            thresholds = new()[4]
            if with_route:
                variants["population_stats(return_series) + compare-and-sum in torch"] = route
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
        base = {"model": name, "T": T, "B": B, "M": M, "C": C, "P": P, "K": args.thr}
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
        if not args.stats_only and with_route:
            _, _, count, volume, _ = last["population_fdc_stats + kge + fdc_freq"]
            count_r, volume_r = last["population_stats(return_series) + compare-and-sum in torch"]
            rel = ((volume.double() - volume_r.double()).abs() / volume_r.double().abs().clamp_min(1e-30))[volume_r > 0]
            print(json.dumps(dict(base, variant="counts and volumes of the two routes",
                                  counts_that_differ=int((count != count_r).sum()), slots=count.numel(),
                                  worst_relative_volume_difference=float(rel.max()) if rel.numel() else 0.0)), flush=True)
        del cand, last
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cands", default="16,64,256")
    ap.add_argument("--models", default="hbv,hbv_2")
    ap.add_argument("--thr", type=int, default=15, help="K: 15 is the default probabilities, any other K evenly spaced ones")
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--big-only", action="store_true")
    ap.add_argument("--m1-only", action="store_true")
    ap.add_argument("--series-gib", type=float, default=40.0, help="largest series the series route is timed with")
    ap.add_argument("--stats-only", action="store_true", help="time population_stats alone (a library of the parent commit)")
    ap.add_argument("--lib", default=None, help="time another build of the library")
    args = ap.parse_args()
    if args.lib:
        from hydrodl2_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    cands = [int(v) for v in args.cands.split(",")]
    only = args.small_only or args.big_only or args.m1_only
    for name in args.models.split(","):
        if args.small_only or not only:
            bench_shape(args, dev, name, 730, 100, 16, cands)
        if args.m1_only or not only:
            bench_shape(args, dev, name, 730, 10736, 1, cands)
        if args.big_only or not only:
            bench_shape(args, dev, name, 7300, 671, 16, cands)


if __name__ == "__main__":
    main()
