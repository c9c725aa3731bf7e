#!/usr/bin/env python3
"""Time `hourly_population_fdc_stats` (hydrodl2_amd/hourly_fdc.py, include/hbvx_gage_fdc.h) against
  - `hourly_population_stats` alone: the call there was before, so the difference is the cost of the FDC term;
  - the route a user had to the same numbers: the same two stages with the hourly gage series kept
    (`ops.gage_population(want_gage=True)`), then in torch a compare-and-sum per level (chunked over the levels: nothing
    of size [P,K,T,G] is formed) and `torch.sort(dim=1, descending=True)` of the masked series with a gather at the ranks.

    python tools/bench_hourly_fdc.py [--steps 5] [--warmup 2] [--cands 16,64,256] [--modes routing,both]
                                     [--small-only | --big-only] [--series-only]

Two shapes: tools/bench_hourly_population.py's (2 160 hours, 4 000 units, 4 members, 100 gages; and 400 hours, 100
units, 10 gages), its topology and parameters; K = 15, the default probabilities.  Modes: 'routing' (distr_candidates
only: stage 1 is not launched) and 'both'.  One process; every variant is warmed at every shape it is timed at; a timed
repetition is one whole call between two HIP events, the variants alternating repetition by repetition; median [min,
max] over the repetitions (bench.py's protocol).  Per (shape, mode, P) one JSON line per variant with its peak memory
and the time of each entry point by itself (hbvx_gage_population_fdc is k_gp_fdc; hbvx_gage_population_quantiles is
k_gp_keys + k_gp_quant), one line with the host half of the call (the observed curve: `_FdcHook.check`) timed by
itself, one line that holds the two routes' numbers to each other; before all that, the two ops against torch's sort
and compare-and-sum on a random series alone (400 x 10, 2 160 x 100 and the cap, 16 384 x 100); and at the end the
kernels' registers, LDS and occupancy from tools/kernel_resources.py."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_hourly_population import problem  # noqa: E402
from bench_population import peak_mb, timed  # noqa: E402


class TorchFdc:
    """The hook of hydrodl2_amd.hourly_population._evaluate that forms the same statistics of a chunk's series in torch."""
    exports = ()

    def __init__(self, scored, thr, rank):
        self.scored, self.thr, self.rank = scored, thr, rank
        self.parts, self.bytes = [], 0

    def check(self, T, G, dev):
        K = int(self.thr.shape[0])
        self.bytes = 12 * K * G + 8 * T * G          # the outputs; the masked copy and the sorted copy of the series

    def chunk(self, series):
        sc = self.scored.unsqueeze(0)
        counts, volumes = [], []
        for k in range(int(self.thr.shape[0])):
            above = sc & (series > self.thr[k].view(1, 1, -1))
            counts.append(above.sum(1, dtype=torch.int32))
            volumes.append(torch.where(above, series, torch.zeros_like(series)).sum(1))
        ranked = torch.where(sc, series, torch.full_like(series, float("-inf"))).sort(1, descending=True).values
        idx = self.rank.long().clamp_min(0).unsqueeze(0).expand(series.shape[0], -1, -1)
        self.parts.append((torch.stack(counts, 1), torch.stack(volumes, 1), ranked.gather(1, idx)))

    def result(self):
        return tuple(torch.cat([p[i] for p in self.parts]) for i in range(3))


def bench_shape(args, dev, T, U, M, G, cands, modes):
    import hydrodl2_amd
    from hydrodl2_amd import ops
    from hydrodl2_amd.hourly_fdc import _FdcHook
    from hydrodl2_amd.hourly_population import _evaluate
    model, xd, p = problem(dev, T, U, M, G)
    cols = torch.as_tensor(hydrodl2_amd.hourly_population_columns(model), device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    with torch.no_grad():
        flow = model(xd, p)["streamflow"][..., 0]
    tgt = (flow.double() * torch.exp(0.2 * torch.randn(flow.shape, generator=gen, device=dev, dtype=torch.float64))).float().contiguous()
    n_pair = int(p[2].shape[0])
    # the host half by itself: the observed curve (the sort of the observations, thresholds, counts, volumes, ranks)
    host = []
    for _ in range(args.warmup + args.steps):
        hook = _FdcHook(xd, tgt, None, None, None, None, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hook.check(T, G, dev)
        torch.cuda.synchronize()
        host.append(1e3 * (time.perf_counter() - t0))
    host = host[args.warmup:]
    print(json.dumps({"T": T, "G": G, "variant": "the host half alone (_FdcHook.check: the observed curve)",
                      "ms_median": round(statistics.median(host), 3), "ms_range": [round(min(host), 3), round(max(host), 3)]}),
          flush=True)
    curve, scored = hook.curve, hook.scored.bool()
    for mode in modes:
        for P in cands:
            cand = None if mode == "routing" else torch.rand((P, U, len(cols)), generator=gen, device=dev)
            dcand = torch.rand((P, n_pair, 3), generator=gen, device=dev)

            def new():
                st = hydrodl2_amd.hourly_population_fdc_stats(model, xd, p, tgt, cand, dcand)
                return (hydrodl2_amd.population_score(st, "kge"), hydrodl2_amd.hourly_fdc_score(st, "fdc_quantile"),
                        st["fdc"]["count"], st["fdc"]["volume"], st["fdc"]["quantile"])

            def counts_only():
                st = hydrodl2_amd.hourly_population_fdc_stats(model, xd, p, tgt, cand, dcand,
                                                              thresholds=curve["thresholds"])
                return (hydrodl2_amd.population_score(st, "kge"), hydrodl2_amd.hourly_fdc_score(st, "fdc_freq"))

            def parent():
                st = hydrodl2_amd.hourly_population_stats(model, xd, p, tgt, cand, dcand)
                return hydrodl2_amd.population_score(st, "kge")

            def by_torch():
                hook = TorchFdc(scored, curve["thresholds"], curve["rank"])
                st = _evaluate(model, xd, p, tgt, cand, dcand, None, None, None, "none", None, False, None, hook)
                return (hydrodl2_amd.population_score(st, "kge"),) + hook.result()

            variants = {"hourly_population_fdc_stats(probs) + kge + fdc_quantile": new,
                        "hourly_population_fdc_stats(thresholds) + kge + fdc_freq (no sort)": counts_only,
                        "hourly_population_stats + kge (no FDC: the call there was)": parent,
                        "gage_population(want_gage) + compare-and-sum + torch.sort(dim=1) in torch": by_torch}
            for fn in variants.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in variants}
            for _ in range(args.steps):
                for k, fn in variants.items():
                    t, _ = timed(fn)
                    ms[k].append(t)
            base = {"T": T, "U": U, "M": M, "G": G, "pairs": n_pair, "mode": mode, "P": P, "K": int(curve["thresholds"].shape[0])}
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
            seen = (curve["n_hours"] > 0).view(1, 1, -1).expand_as(a[2])
            vol_scale = b[2][seen].abs().clamp_min(1e-30)
            print(json.dumps(dict(base, variant="the two routes held to each other",
                                  kge_bits_equal=bool(torch.equal(a[0], b[0])),
                                  counts_equal=bool(torch.equal(a[2][seen], b[1][seen])),
                                  quantiles_equal=bool(torch.equal(a[4][seen], b[3][seen])),
                                  worst_relative_volume_difference=float(((a[3] - b[2])[seen].abs() / vol_scale).max()))),
                  flush=True)
            del cand, dcand
            torch.cuda.empty_cache()


def sort_alone(args, dev, cands):
    """`ops.gage_quantiles` (k_gp_keys + k_gp_quant) and `ops.gage_fdc` (k_gp_fdc) against torch's sort + gather and
    compare-and-sum on a random [P,T,G] series by themselves: no model, no stage 1 or 2."""
    from hydrodl2_amd import ops
    from hydrodl2_amd.hourly_fdc import fdc_ranks
    from hydrodl2_amd.population_fdc import DEFAULT_PROBS
    gen = torch.Generator(device=dev).manual_seed(9)
    for T, G in ((400, 10), (2160, 100), (16384, 100)):
        for P in cands:
            series = torch.rand((P, T, G), generator=gen, device=dev).contiguous()
            scored = torch.rand((T, G), generator=gen, device=dev) < 0.9
            rank = fdc_ranks(scored.sum(0), DEFAULT_PROBS)
            thr = torch.rand((len(DEFAULT_PROBS), G), generator=gen, device=dev).contiguous()

            def by_torch_sort():
                ranked = torch.where(scored.unsqueeze(0), series, torch.full_like(series, float("-inf"))).sort(1, descending=True).values
                return ranked.gather(1, rank.long().clamp_min(0).unsqueeze(0).expand(P, -1, -1))

            def by_torch_counts():
                sc = scored.unsqueeze(0)
                return [(sc & (series > thr[k].view(1, 1, -1))).sum(1, dtype=torch.int32) for k in range(int(thr.shape[0]))]

            variants = {"ops.gage_quantiles": lambda: ops.gage_quantiles(series, scored, rank), "torch.sort(dim=1) + gather": by_torch_sort,
                        "ops.gage_fdc": lambda: ops.gage_fdc(series, scored, thr), "torch compare-and-sum per level (counts alone)": by_torch_counts}
            for fn in variants.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in variants}
            for _ in range(args.steps):
                for k, fn in variants.items():
                    t, _ = timed(fn)
                    ms[k].append(t)
            equal = bool(torch.equal(variants["ops.gage_quantiles"](), by_torch_sort()))
            print(json.dumps({"series_alone": True, "T": T, "G": G, "P": P, "K": len(DEFAULT_PROBS), "quantiles_equal": equal,
                              **{k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}}),
                  flush=True)
            del series
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cands", default="16,64,256")
    ap.add_argument("--modes", default="routing,both")
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--big-only", action="store_true")
    ap.add_argument("--series-only", action="store_true", help="only the kernels against torch on a random series")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    cands = [int(v) for v in args.cands.split(",")]
    sort_alone(args, dev, cands)
    if args.series_only:
        return
    if not args.big_only:
        bench_shape(args, dev, 400, 100, 4, 10, cands, args.modes.split(","))
    if not args.small_only:
        bench_shape(args, dev, 2160, 4000, 4, 100, cands, args.modes.split(","))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_table
    for row in kernel_table():
        if any(k in row["name"] for k in ("k_gp_fdc", "k_gp_keys", "k_gp_quant")):
            print(json.dumps({"kernel": row["name"], **{k: v for k, v in row.items() if k not in ("name", "symbol")}}), flush=True)


if __name__ == "__main__":
    main()
