#!/usr/bin/env python3
"""Time `population_period_stats` (hydrodl2_amd/population.py, hbvx_population_period in include/hbvx.h) against two
yardsticks:

  (a) `population_joint_stats` on daily observations, whose kernel is the parent commit's bit for bit
      (tools/compare_code.py): the price of the period machinery -- it scores days, not periods;
  (b) the route there was before to a score of period means: `population_joint_stats(return_series=True)`, period means
      of the two [P,T_out,B] series and float64 KGE of them in torch.

    python tools/bench_population_period.py [--steps 5] [--warmup 2] [--cands 16,64,256] [--models hbv,hbv_2]
                                            [--calendars monthly+8,daily+8] [--small-only | --big-only]

Every parameter static, routing on, aux key AET_hydro.  Two shapes, 671 x 16 x 7300 and 100 x 16 x 730, P in {16, 64,
256}.  Calendars: 'monthly+8' scores the flow by calendar months (365-day years) and the aux series by 8-day blocks,
'daily+8' the flow by days and the aux series by 8-day blocks.  Period targets are the period means of the row's own
series times exp(0.2 noise).  One process; every variant is warmed at every shape it is timed at; a timed repetition is
one whole call between two HIP events, the variants alternating repetition by repetition; median [min, max] over the
repetitions (bench.py's protocol, as tools/bench_population_joint.py).  Per (model, shape, calendar, P) one JSON line per
variant with its peak memory and the kernel by itself, and one with the worst difference of the two KGE from the chains
against float64 KGE over the kernel's own period series, |chains - series| / (1 + |1 - series|), at the smallest P."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_population import peak_mb, timed  # noqa: E402
from bench_population_joint import kge_of_series  # noqa: E402
from bench_population_stats import problem  # noqa: E402

MONTHS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)


def month_ends(T_out):
    ends, day = [], -1
    while True:
        for n in MONTHS:
            day += n
            if day >= T_out:
                return ends
            ends.append(day)


def period_means(series, cal):
    """float64 period means [..., K, B] of [..., T_out, B]: blocks by a reshape, a list of closing days one slice each."""
    if cal is None:
        return series.double()
    if isinstance(cal, int):
        K = series.shape[-2] // cal
        return series[..., :K * cal, :].double().unflatten(-2, (K, cal)).mean(-2)
    starts = [0] + [e + 1 for e in cal[:-1]]
    return torch.stack([series[..., s:e + 1, :].double().mean(-2) for s, e in zip(starts, cal)], dim=-2)


def bench_shape(args, dev, name, T, B, M, cands, calendars):
    import hydrodl2_amd
    from hydrodl2_amd import ops
    model, x_dict, p, target, draw, C = problem(name, dev, T, B, M)
    gen = torch.Generator(device=dev).manual_seed(5)
    aux_key = "AET_hydro"
    with torch.no_grad():
        primal = model(x_dict, p)
    flow, aux = primal["streamflow"][..., 0], primal[aux_key][..., 0]
    T_out = int(flow.shape[0])
    aux_daily = aux * torch.exp(0.2 * torch.randn(aux.shape, generator=gen, device=dev))
    seen = (torch.arange(T_out, device=dev) % 8 == 0).unsqueeze(1).expand_as(aux)
    aux_daily = torch.where(seen, aux_daily, torch.full_like(aux_daily, float("nan"))).contiguous()
    for cal_name in calendars:
        fcal = month_ends(T_out) if cal_name.startswith("monthly") else None
        acal = 8

        def noisy(series, cal):
            m = period_means(series, cal)
            return (m * torch.exp(0.2 * torch.randn(m.shape, generator=gen, device=dev, dtype=torch.float64))).float().contiguous()

        ftgt, atgt = target if fcal is None else noisy(flow, fcal), noisy(aux, acal)
        for P in cands:
            cand = draw(P)

            def new():
                st = hydrodl2_amd.population_period_stats(model, x_dict, p, cand, ftgt, fcal, atgt, aux_key, acal)
                return hydrodl2_amd.population_score(st["flow"], "kge"), hydrodl2_amd.population_score(st["aux"], "kge")

            def daily():
                st = hydrodl2_amd.population_joint_stats(model, x_dict, p, cand, target, aux_daily, aux_key)
                return hydrodl2_amd.population_score(st["flow"], "kge"), hydrodl2_amd.population_score(st["aux"], "kge")

            def series_route():
                st = hydrodl2_amd.population_joint_stats(model, x_dict, p, cand, target, aux_daily, aux_key, return_series=True)
                return (kge_of_series(period_means(st["flow"]["series"], fcal), ftgt),
                        kge_of_series(period_means(st["aux"]["series"], acal), atgt))

            variants = {"population_period_stats + 2 x population_score(kge)": new,
                        "(a) population_joint_stats on daily observations + 2 x population_score(kge)": daily,
                        "(b) population_joint_stats(return_series) + period means and float64 KGE in torch": series_route}
            for fn in variants.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in variants}
            for _ in range(args.steps):
                for k, fn in variants.items():
                    t, _ = timed(fn)
                    ms[k].append(t)
            base = {"model": name, "T": T, "B": B, "M": M, "C": C, "calendar": cal_name,
                    "periods": [len(fcal) if fcal else T_out, T_out // acal], "P": P}
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
            if P == min(cands):
                st = hydrodl2_amd.population_period_stats(model, x_dict, p, cand, ftgt, fcal, atgt, aux_key, acal,
                                                          return_series=True)
                line = dict(base, variant="KGE from the chains against float64 over the kernel's own period series")
                for term, tgt in (("flow", ftgt), ("aux", atgt)):
                    a = hydrodl2_amd.population_score(st[term], "kge")
                    b = kge_of_series(st[term]["series"], tgt)
                    ok = torch.isfinite(b) & torch.isfinite(a)
                    line[term] = {"worst_difference": float(((a - b).abs() / (1 + (1 - b).abs()))[ok].max()) if bool(ok.any()) else None,
                                  "kge_range": [round(float(b[ok].min()), 3), round(float(b[ok].max()), 3)] if bool(ok.any()) else None,
                                  "without_a_score": [int((~torch.isfinite(a)).sum()), int((~torch.isfinite(b)).sum())]}
                print(json.dumps(line), flush=True)
                del st
            del cand
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cands", default="16,64,256")
    ap.add_argument("--models", default="hbv,hbv_2")
    ap.add_argument("--calendars", default="monthly+8,daily+8")
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--big-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    cands = [int(v) for v in args.cands.split(",")]
    calendars = args.calendars.split(",")
    for name in args.models.split(","):
        if not args.big_only:
            bench_shape(args, dev, name, 730, 100, 16, cands, calendars)
        if not args.small_only:
            bench_shape(args, dev, name, 7300, 671, 16, cands, calendars)


if __name__ == "__main__":
    main()
