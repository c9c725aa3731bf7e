#!/usr/bin/env python3
"""Time one filter window through `ensemble_step` (hydrodl2_amd/ensemble.py, hbvx_population_ensemble in
include/hbvx_pop_ens.h) against the route a user has without it: P module forwards over the window, each on a clone of
x_phy with its particle's precipitation noise and from its particle's cached storages (`load_states` / `get_states`,
cache_states=True), plus the float64 squared error of each forward's streamflow -- and a whole `particle_filter`.

    python tools/bench_population_ensemble.py [--steps 5] [--warmup 2] [--particles 64,256] [--windows 1,30]
                                              [--small-only | --big-only] [--filter-days 730] [--no-filter]

Hbv, every parameter static, routing on.  Shapes: 100 x 16 and 671 x 16 basins x members, P in {64, 256}, windows of 1
and 30 days in the middle of a 730-day record (day 365: the routing history is full), and `particle_filter` over 730 days
at 100 x 16 x 64 with one-day windows.  The loop of forwards routes each window from a zero history (the module has no
way to hand one over), so its series differ from the kernel's in the window's first 14 days: it is timed, not compared.
The protocol is tools/bench_population_events.py's: one process; every variant is warmed at every shape it is timed at;
a timed repetition is one whole call between two HIP events, the variants alternating repetition by repetition; median
[min, max].  Per (shape, P, window) one JSON line per variant with its peak memory (torch's allocator, above what the
inputs hold) and, for `ensemble_step`, the kernel by itself (the library call between events of its own)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_population import peak_mb, timed  # noqa: E402


def bench_shape(args, dev, T, B, M, particles, windows):
    import hydrodl2_amd
    from hydrodl2_amd import ops
    from hydrodl2_amd.ensemble import EnsembleState
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    cfg = {"nmul": M, "dynamic_params": {"Hbv": []}, "warm_up": 0}
    load = hydrodl2_amd.load_model("hbv", "Hbv")
    model, looped = load(dict(cfg), dev), load(dict(cfg, cache_states=True), dev)
    x = torch.from_numpy(synth.forcing(T, B, 92)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(4)
    p = torch.randn((1, B, model.learnable_param_count), generator=gen, device=dev).expand(T, -1, -1).contiguous()
    with torch.no_grad():
        target = (model({"x_phy": x}, p)["streamflow"][..., 0] * 1.1 + 0.05).clone()
    rec = hydrodl2_amd.ensemble_record(model, {"x_phy": x}, p)
    t0 = T // 2
    for P in particles:
        pm_all = torch.exp(0.4 * torch.randn((P, max(windows), B), generator=gen, device=dev) - 0.08)
        start = hydrodl2_amd.ensemble_step(rec, None, None, target, n_particles=P, t_begin=0, t_end=t0,
                                           prcp_mul=pm_all[:, 0].contiguous())["state"]
        for W in windows:
            pm = pm_all[:, :W].contiguous()
            xw, pw, tw = x[t0:t0 + W].contiguous(), p[t0:t0 + W].contiguous(), target[t0:t0 + W].double()

            def new():
                out = hydrodl2_amd.ensemble_step(rec, None, None, target, state=start, t_end=t0 + W, prcp_mul=pm)
                return out["sse"], out["state"]

            def loop():
                sse, states = [], []
                for c in range(P):
                    looped.load_states(tuple(start.states[c].unbind(0)))
                    xc = xw.clone()
                    xc[..., 0] = xc[..., 0] * pm[c]
                    with torch.no_grad():
                        y = looped({"x_phy": xc}, pw)["streamflow"][..., 0]
                    sse.append(((y.double() - tw) ** 2).sum(0))
                    states.append(torch.stack(looped.get_states()))
                return torch.stack(sse), EnsembleState(torch.stack(states), None, t0 + W)

            variants = {"ensemble_step": new, "P module forwards + float64 sse": loop}
            for fn in variants.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in variants}
            for _ in range(args.steps):
                for k, fn in variants.items():
                    t, _ = timed(fn)
                    ms[k].append(t)
            base = {"T": T, "B": B, "M": M, "P": P, "window": W}
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
        del pm_all, start
        torch.cuda.empty_cache()
    return model, x, p, target


def bench_filter(args, dev, model, x, p, target, P):
    import hydrodl2_amd
    T = min(args.filter_days, int(x.shape[0]))
    xd, pp, tg = {"x_phy": x[:T].contiguous()}, p[:T].contiguous(), target[:T].contiguous()
    sigma = 0.05 * tg.mean(0)

    def run():
        g = torch.Generator().manual_seed(7)
        return hydrodl2_amd.particle_filter(model, xd, pp, tg, P, 1, obs_sigma=sigma, prcp_sigma=0.4, state_sigma=0.5,
                                            generator=g)["mean"]

    run()
    torch.cuda.synchronize()
    ms = [timed(run)[0] for _ in range(max(args.steps // 2, 2))]
    print(json.dumps({"variant": "particle_filter, one-day windows", "T": T, "B": int(x.shape[1]), "P": P,
                      "ms_median": round(statistics.median(ms), 1), "ms_range": [round(min(ms), 1), round(max(ms), 1)],
                      "reps": len(ms), "ms_per_window": round(statistics.median(ms) / T, 3), "peak_mb": peak_mb(run)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--particles", default="64,256")
    ap.add_argument("--windows", default="1,30")
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--big-only", action="store_true")
    ap.add_argument("--filter-days", type=int, default=730)
    ap.add_argument("--no-filter", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    particles = [int(v) for v in args.particles.split(",")]
    windows = [int(v) for v in args.windows.split(",")]
    if not args.big_only:
        small = bench_shape(args, dev, 730, 100, 16, particles, windows)
        if not args.no_filter:
            bench_filter(args, dev, *small, 64)
    if not args.small_only:
        bench_shape(args, dev, 730, 671, 16, particles, windows)


if __name__ == "__main__":
    main()
