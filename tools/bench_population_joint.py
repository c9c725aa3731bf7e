#!/usr/bin/env python3
"""Time `population_joint_stats` (hydrodl2_amd/population.py, hbvx_population_joint in include/hbvx.h) against the three
other routes to a streamflow score AND a score of a second series per candidate:

  (a) `population_stats` alone on the same build: what the aux term adds to the launch (it gives no aux score);
  (b) the route there was before: `population_cost(return_series=True)` plus a float64 KGE of the series for the flow,
      and P module forwards under no_grad with a float64 KGE of outputs[aux_key];
  (c) P module forwards with both scores in torch.

    python tools/bench_population_joint.py [--steps 5] [--warmup 2] [--cands 16,64,256] [--models hbv,hbv_2]
                                           [--aux-keys AET_hydro,SWE] [--small-only | --big-only]

Every parameter static, routing on.  Two shapes, 671 x 16 x 7300 and 100 x 16 x 730, P in {16, 64, 256}.  The flow
target is the streamflow at the row times exp(0.2 noise); the aux target is outputs[aux_key] at the row times
exp(0.2 noise), observed every 8th day (NaN elsewhere).  One process; every variant is warmed at every shape it is timed
at; a timed repetition is one whole call between two HIP events, the variants alternating repetition by repetition;
median [min, max] over the repetitions (bench.py's protocol, as tools/bench_population_stats.py).  Per (model, shape,
aux key, P) one JSON line per variant with its peak memory and the kernel by itself, and one with the worst difference
of the aux and flow KGE from the four chains against float64 KGE over the kernel's own series,
|chains - series| / (1 + |1 - series|), taken at the smallest P."""
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


def kge_of_series(series, target):
    """Gupta 2009 per (candidate, basin) from the series [P,T,B] and a target [T,B] with NaN where nothing is
    observed: float64, weight 1 on the observed days."""
    s, o = series.double(), target.double()
    w = (~torch.isnan(o)).double()
    o = torch.where(w > 0, o, torch.zeros_like(o))
    W = w.sum(0)
    ms, mo = (w * s).sum(1) / W, (w * o).sum(0) / W
    ds, do = s - ms.unsqueeze(1), o - mo
    sd_s, sd_o = ((w * ds * ds).sum(1) / W).sqrt(), ((w * do * do).sum(0) / W).sqrt()
    r = (w * ds * do).sum(1) / W / (sd_s * sd_o)
    return 1 - ((r - 1) ** 2 + (sd_s / sd_o - 1) ** 2 + (ms / mo - 1) ** 2).sqrt()


def bench_shape(args, dev, name, T, B, M, cands, aux_keys):
    import hydrodl2_amd
    from hydrodl2_amd import ops
    model, x_dict, p, target, draw, C = problem(name, dev, T, B, M)
    _, cols = hydrodl2_amd.sensitivity.jacobian_columns(model, None)
    two = isinstance(p, tuple)
    work = (p[1] if two else p).clone()             # the tensor whose static row the module route rewrites per candidate
    row = work if two else work[-1]
    pw = (p[0], work) if two else work
    gen = torch.Generator(device=dev).manual_seed(5)
    with torch.no_grad():
        primal = model(x_dict, p)
    for aux_key in aux_keys:
        aux = primal[aux_key][..., 0]
        aux_target = aux * torch.exp(0.2 * torch.randn(aux.shape, generator=gen, device=dev))
        seen = (torch.arange(aux.shape[0], device=dev) % 8 == 0).unsqueeze(1).expand_as(aux)
        aux_target = torch.where(seen, aux_target, torch.full_like(aux_target, float("nan"))).contiguous()
        for P in cands:
            cand = draw(P)

            def new():
                st = hydrodl2_amd.population_joint_stats(model, x_dict, p, cand, target, aux_target, aux_key)
                return hydrodl2_amd.population_score(st["flow"], "kge"), hydrodl2_amd.population_score(st["aux"], "kge")

            def flow_only():
                st = hydrodl2_amd.population_stats(model, x_dict, p, cand, target)
                return hydrodl2_amd.population_score(st, "kge"), None

            def forwards(keys):
                got = {k: [] for k in keys}
                with torch.no_grad():
                    for c in range(P):
                        row[:, cols] = cand[c]
                        out = model(x_dict, pw)
                        for k in keys:
                            tgt = target if k == "streamflow" else aux_target
                            got[k].append(kge_of_series(out[k][..., 0].unsqueeze(0), tgt)[0])
                return {k: torch.stack(v) for k, v in got.items()}

            def series_route():
                got = hydrodl2_amd.population_cost(model, x_dict, p, cand, target, return_series=True)
                return kge_of_series(got["series"], target), forwards((aux_key,))[aux_key]

            def module_route():
                got = forwards(("streamflow", aux_key))
                return got["streamflow"], got[aux_key]

            variants = {"population_joint_stats + 2 x population_score(kge)": new,
                        "(a) population_stats + population_score(kge), flow only": flow_only,
                        "(b) population_cost(return_series) + P forwards for the aux series, float64 KGE": series_route,
                        "(c) P forwards, both KGE in torch": module_route}
            for fn in variants.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in variants}
            for _ in range(args.steps):
                for k, fn in variants.items():
                    t, _ = timed(fn)
                    ms[k].append(t)
            base = {"model": name, "T": T, "B": B, "M": M, "C": C, "aux_key": aux_key, "P": P}
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
                st = hydrodl2_amd.population_joint_stats(model, x_dict, p, cand, target, aux_target, aux_key,
                                                         return_series=True)
                line = dict(base, variant="KGE from the chains against float64 over the kernel's own series")
                for term, tgt in (("flow", target), ("aux", aux_target)):
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
    ap.add_argument("--aux-keys", default="AET_hydro,SWE")
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--big-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    cands = [int(v) for v in args.cands.split(",")]
    aux_keys = args.aux_keys.split(",")
    for name in args.models.split(","):
        if not args.big_only:
            bench_shape(args, dev, name, 730, 100, 16, cands, aux_keys)
        if not args.small_only:
            bench_shape(args, dev, name, 7300, 671, 16, cands, aux_keys)


if __name__ == "__main__":
    main()
