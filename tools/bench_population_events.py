#!/usr/bin/env python3
"""Time `population_event_stats` (hydrodl2_amd/population_events.py, hbvx_population_events in
include/hbvx_pop_events.h) against `population_stats` on the same tree -- what the flow scores alone cost -- and against
the route to the same event statistics there is without it: `population_stats(return_series=True)` plus
`ops.gage_events` on the [P,T_out,B] series (that kernel's lanes are just columns).

    python tools/bench_population_events.py [--steps 5] [--warmup 2] [--cands 16,64,256] [--models hbv,hbv_2]
                                            [--events 20] [--days 11] [--small-only | --big-only | --m1-only]
                                            [--stats-only] [--lib other.so]

Every parameter static, routing on.  Shapes: 671 x 16 x 7300 and 100 x 16 x 730, and one with a single member, 10736 x 1
x 730 (the lanes of the first, a tenth of its days), where 64 basins with 64 different cursors share a wave; P in {16,
64, 256}.  Windows: --events windows of --days days per basin, evenly spaced over the scored days and shifted by b % 7
days from basin to basin, so that the lanes of a wave open and close their windows on different days (`flood_events`
would give windows of the same count and length; its host loop over 10736 basins is not what is measured here).  The
protocol is tools/bench_population_fdc.py's: one process; every variant is warmed at every shape it is timed at; a timed
repetition is one whole call between two HIP events, the variants alternating repetition by repetition; median [min,
max].  Per (model, shape, P) one JSON line per variant with its peak memory (torch's allocator, above what the inputs
hold) and the kernels by themselves (the library calls timed by events of their own), and one with the agreement of the
two routes' events, which is exact.  The series route is left out where its series would not fit in --series-gib.
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


def spaced_windows(T_out, B, n_events, days):
    """(starts, ends) [E,B] int32 on the host: E windows of `days` days, one per stretch of T_out // E days, shifted by
    b % 7 days."""
    stride = T_out // n_events
    assert stride >= days + 7, f"{n_events} windows of {days} days (+ 6 of shift) do not fit in {T_out} days"
    e = torch.arange(n_events, dtype=torch.int32).unsqueeze(1) * stride
    starts = (e + (torch.arange(B, dtype=torch.int32) % 7).unsqueeze(0)).contiguous()
    return starts, (starts + (days - 1)).contiguous()


def bench_shape(args, dev, name, T, B, M, cands):
    import hydrodl2_amd
    from hydrodl2_amd import ops
    model, x_dict, p, target, draw, C = problem(name, dev, T, B, M)
    T_out = int(target.shape[0])
    events = spaced_windows(T_out, B, args.events, args.days)
    dev_events = tuple(t.to(dev) for t in events)
    for P in cands:
        cand = draw(P)

        def stats():
            st = hydrodl2_amd.population_stats(model, x_dict, p, cand, target)
            return hydrodl2_amd.population_score(st, "kge")

        variants = {"population_stats(none) + population_score(kge)": stats}
        with_route = P * T * B * 4 / 2 ** 30 <= args.series_gib
        if not args.stats_only:
            def new():
                st = hydrodl2_amd.population_event_stats(model, x_dict, p, cand, target, events)
                e = st["events"]
                return (hydrodl2_amd.population_score(st, "kge"), hydrodl2_amd.population_event_score(st, "peak_error"),
                        e["peak"], e["peak_day"], e["volume"])

            def route():
                st = hydrodl2_amd.population_stats(model, x_dict, p, cand, target, return_series=True)
                return (hydrodl2_amd.population_score(st, "kge"),) + tuple(ops.gage_events(st["series"], *dev_events))

            variants["population_event_stats + kge + peak_error"] = new
            if with_route:
                variants["population_stats(return_series) + ops.gage_events"] = route
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
        base = {"model": name, "T": T, "B": B, "M": M, "C": C, "P": P, "E": args.events, "days": args.days}
        for k, fn in variants.items():
            mem = peak_mb(fn)
            ops.KERNEL_EVENTS = []
            fn()
            torch.cuda.synchronize()
            calls = {}
            for n, e0, e1 in ops.KERNEL_EVENTS:
                if n.startswith("hbvx_population") or n.startswith("hbvx_gage_population"):
                    calls[n] = round(calls.get(n, 0.0) + e0.elapsed_time(e1), 3)
            ops.KERNEL_EVENTS = None
            print(json.dumps(dict(base, variant=k, ms_median=round(statistics.median(ms[k]), 3),
                                  ms_range=[round(min(ms[k]), 3), round(max(ms[k]), 3)], reps=len(ms[k]), peak_mb=mem,
                                  kernel_ms=calls)), flush=True)
        if not args.stats_only and with_route:
            got = last["population_event_stats + kge + peak_error"][2:]
            want = last["population_stats(return_series) + ops.gage_events"][1:]
            print(json.dumps(dict(base, variant="events of the two routes", slots=got[0].numel(),
                                  slots_that_differ=[int((a.view(torch.int32) != b.view(torch.int32)).sum())
                                                     for a, b in zip(got, want)])), flush=True)
        del cand, last
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cands", default="16,64,256")
    ap.add_argument("--models", default="hbv,hbv_2")
    ap.add_argument("--events", type=int, default=20, help="E: windows per basin")
    ap.add_argument("--days", type=int, default=11, help="days per window")
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
