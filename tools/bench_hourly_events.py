#!/usr/bin/env python3
"""Time `hourly_population_event_stats` (hydrodl2_amd/hourly_events.py, include/hbvx_gage_events.h) against
  - `hourly_population_stats` alone: the call there was before, so the difference is the cost of the event term;
  - the route a user had to the same numbers: the same two stages with the hourly gage series kept
    (`ops.gage_population(want_gage=True)`), then max / argmax / sum over the windows in torch -- one gather of the
    windows' hours into [P,E,W,G], masked where a window is shorter than the longest.

    python tools/bench_hourly_events.py [--steps 5] [--warmup 2] [--cands 16,64,256] [--modes routing,both]
                                        [--events 10] [--hours 121] [--small-only | --big-only]

Two shapes: tools/bench_hourly_population.py's (2 160 hours, 4 000 units, 4 members, 100 gages; and 400 hours, 100
units, 10 gages), its topology and parameters.  The windows are `flood_events` on the noisy primal streamflow: up to
--events windows of --hours hours per gage (a 400-hour record has room for three of 121).  Modes: 'routing'
(distr_candidates only: stage 1 is not launched) and 'both'.  One process; every variant is warmed at every shape it is
timed at; a timed repetition is one whole call between two HIP events, the variants alternating repetition by repetition;
median [min, max] over the repetitions (bench.py's protocol).  Per (shape, mode, P) one JSON line per variant with its
peak memory and the time of each entry point by itself, one line that holds the two routes' numbers to each other, and
at the end the kernel's registers and occupancy from tools/kernel_resources.py."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_hourly_population import problem  # noqa: E402
from bench_population import peak_mb, timed  # noqa: E402


class TorchEvents:
    """The hook of hydrodl2_amd.hourly_population._evaluate that forms the event statistics of a chunk's series in torch."""
    exports = ()

    def __init__(self, starts, ends):
        self.starts, self.ends = starts, ends
        self.parts, self.bytes = [], 0

    def check(self, T, G, dev):
        s, f = self.starts.to(dev).long(), self.ends.to(dev).long()
        W = int((f - s).max()) + 1
        hours = s.unsqueeze(1) + torch.arange(W, device=dev).view(1, W, 1)              # [E,W,G]
        self.inside = (s.unsqueeze(1) >= 0) & (hours <= f.unsqueeze(1))
        self.hours = hours.clamp(0, T - 1)
        self.gages = torch.arange(G, device=dev).view(1, 1, G).expand_as(hours)
        self.s = s
        self.bytes = 4 * int(hours.numel())

    def chunk(self, series):
        w = series[:, self.hours, self.gages]                                            # [P,E,W,G]
        top, at = torch.where(self.inside, w, torch.full_like(w, float("-inf"))).max(2)
        volume = torch.where(self.inside, w, torch.zeros_like(w)).sum(2)
        self.parts.append((top, (at + self.s).int(), volume))

    def result(self):
        return tuple(torch.cat([p[i] for p in self.parts]) for i in range(3))


def bench_shape(args, dev, T, U, M, G, cands, modes):
    import hydrodl2_amd
    from hydrodl2_amd import ops
    from hydrodl2_amd.hourly_population import _evaluate
    model, xd, p = problem(dev, T, U, M, G)
    cols = torch.as_tensor(hydrodl2_amd.hourly_population_columns(model), device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    with torch.no_grad():
        flow = model(xd, p)["streamflow"][..., 0]
    tgt = (flow.double() * torch.exp(0.2 * torch.randn(flow.shape, generator=gen, device=dev, dtype=torch.float64))).float().contiguous()
    half = args.hours // 2
    events = hydrodl2_amd.flood_events(tgt, args.events, half, args.hours - 1 - half)
    events_dev = tuple(t.to(dev) for t in events)
    per_gage = (events[0] >= 0).sum(0)
    n_pair = int(p[2].shape[0])
    for mode in modes:
        for P in cands:
            cand = None if mode == "routing" else torch.rand((P, U, len(cols)), generator=gen, device=dev)
            dcand = torch.rand((P, n_pair, 3), generator=gen, device=dev)

            def new():
                st = hydrodl2_amd.hourly_population_event_stats(model, xd, p, tgt, events_dev, cand, dcand)
                return (hydrodl2_amd.population_score(st, "kge"), hydrodl2_amd.hourly_event_score(st, "peak_timing"),
                        st["events"]["peak"], st["events"]["peak_hour"], st["events"]["volume"])

            def parent():
                st = hydrodl2_amd.hourly_population_stats(model, xd, p, tgt, cand, dcand)
                return hydrodl2_amd.population_score(st, "kge")

            def by_torch():
                hook = TorchEvents(*events_dev)
                st = _evaluate(model, xd, p, tgt, cand, dcand, None, None, None, "none", None, False, None, hook)
                return (hydrodl2_amd.population_score(st, "kge"),) + hook.result()

            variants = {"hourly_population_event_stats + kge + peak_timing": new,
                        "hourly_population_stats + kge (no events: the call there was)": parent,
                        "gage_population(want_gage) + max / argmax / sum over the windows in torch": by_torch}
            for fn in variants.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in variants}
            for _ in range(args.steps):
                for k, fn in variants.items():
                    t, _ = timed(fn)
                    ms[k].append(t)
            base = {"T": T, "U": U, "M": M, "G": G, "pairs": n_pair, "mode": mode, "P": P, "event_rows": int(events[0].shape[0]),
                    "events_per_gage": [int(per_gage.min()), int(per_gage.max())], "hours": args.hours}
            for k, fn in variants.items():
                mem = peak_mb(fn)
                ops.KERNEL_EVENTS = []
                fn()
                torch.cuda.synchronize()
                calls = {}
                for n, e0, e1 in ops.KERNEL_EVENTS:
                    calls[n] = round(calls.get(n, 0.0) + e0.elapsed_time(e1), 3)
                ops.KERNEL_EVENTS = None
                print(json.dumps(dict(base, variant=k, ms_median=round(statistics.median(ms[k]), 3),
                                      ms_range=[round(min(ms[k]), 3), round(max(ms[k]), 3)], reps=len(ms[k]),
                                      peak_mb=mem, entry_ms=calls)), flush=True)
            a, b = new(), by_torch()
            present = (events_dev[0] >= 0).unsqueeze(0).expand_as(a[2])
            vol_scale = b[3][present].abs().clamp_min(1e-30)
            print(json.dumps(dict(base, variant="the two routes held to each other",
                                  kge_bits_equal=bool(torch.equal(a[0], b[0])),
                                  peaks_equal=bool(torch.equal(a[2][present], b[1][present])),
                                  hours_equal=bool(torch.equal(a[3][present], b[2][present])),
                                  worst_relative_volume_difference=float(((a[4] - b[3])[present].abs() / vol_scale).max()),
                                  peak_timing_range=[round(float(a[1][torch.isfinite(a[1])].min()), 3),
                                                     round(float(a[1][torch.isfinite(a[1])].max()), 3)])), flush=True)
            del cand, dcand
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cands", default="16,64,256")
    ap.add_argument("--modes", default="routing,both")
    ap.add_argument("--events", type=int, default=10)
    ap.add_argument("--hours", type=int, default=121)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--big-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    cands = [int(v) for v in args.cands.split(",")]
    if not args.big_only:
        bench_shape(args, dev, 400, 100, 4, 10, cands, args.modes.split(","))
    if not args.small_only:
        bench_shape(args, dev, 2160, 4000, 4, 100, cands, args.modes.split(","))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_table
    for row in kernel_table():
        if "k_gp_events" in row["name"] or "k_gp_score" in row["name"]:
            print(json.dumps({"kernel": row["name"], **{k: v for k, v in row.items() if k not in ("name", "symbol")}}), flush=True)


if __name__ == "__main__":
    main()
