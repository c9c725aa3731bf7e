#!/usr/bin/env python3
"""Time the ensemble Kalman analysis step (hydrodl2_amd/enkf.py, hbvx_enkf_update in include/hbvx_enkf.h) against the route
a user has without it -- the same update written in float64 torch on the device, a dozen small kernels with [P,5,B,M]
float64 temporaries -- and a whole `enkf_filter` beside `particle_filter`.

    python tools/bench_enkf.py [--steps 5] [--warmup 2] [--particles 64,256] [--small-only | --big-only]
                               [--filter-days 730] [--no-filter]

Shapes: 100 x 16 and 671 x 16 basins x members, P in {64, 256}, both methods; the arrays are the storages [P,5,B,M], the
routing history [P,14,B] and one predicted row [P,1,B], as `enkf_filter` passes them with one-day windows.  Then
`enkf_filter` and `particle_filter` over 730 days at 100 x 16 x 64 with one-day windows, alternating.  The protocol is
tools/bench_population_ensemble.py's: one process; every variant is warmed at every shape it is timed at; a timed repetition
is one whole call between two HIP events, the variants alternating repetition by repetition; median [min, max].  One JSON
line per variant with its peak memory (torch's allocator, above what the inputs hold) and, for `enkf_update`, the library
call by itself (the memset and the launches between events of their own)."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_population import peak_mb, timed  # noqa: E402


def torch_update(states, history, row, y, obs, var, method, rho, eps, floor):
    """The update of include/hbvx_enkf.h in float64 torch (no skip rules: every basin is analysed)."""
    P = y.shape[0]
    y8, o8, R = y.double(), obs.double(), var.double()
    ybar = y8.mean(0)
    dy = y8 - ybar
    s = (dy * dy).sum(0) / (P - 1) + R
    alpha = 1.0 / (1.0 + torch.sqrt(R / s))
    outs = []
    for x, lo, shape in ((states, floor, (P, 1, -1, 1)), (history, 0.0, (P, 1, -1)), (row, -math.inf, (P, 1, -1))):
        x8 = x.double()
        d = dy.view(shape)
        K = (x8 * d).sum(0) / (P - 1) / s.view(shape[1:])
        if method == 0:
            xa = x8 + K * ((o8 + eps.double()) - y8).view(shape)
            m = x8.mean(0) + K * ((o8 + eps.double().mean(0)) - ybar).view(shape[1:])
        else:
            xbar = x8.mean(0)
            m = xbar + K * (o8 - ybar).view(shape[1:])
            xa = m + ((x8 - xbar) - (alpha.view(shape[1:]) * K) * d)
        if rho != 1.0:
            xa = m + rho * (xa - m)
        outs.append(xa.clamp_min(lo).float())
    return outs


def bench_update(args, dev, B, M, particles):
    from hydrodl2_amd import ops
    from hydrodl2_amd.enkf import _analyse
    gen = torch.Generator(device=dev).manual_seed(4)
    for P in particles:
        z = torch.randn((P, B), generator=gen, device=dev)
        y = (3.0 + z).contiguous()
        obs = 3.0 + 0.7 * torch.randn((B,), generator=gen, device=dev)
        var = torch.full((B,), 0.09, device=dev)
        eps = 0.3 * torch.randn((P, B), generator=gen, device=dev)
        states = (20.0 * torch.rand((1, 5, B, M), generator=gen, device=dev) *
                  torch.exp(0.3 * z.view(P, 1, B, 1) + 0.2 * torch.randn((P, 5, B, M), generator=gen, device=dev))).contiguous()
        history = (3.0 + 0.6 * z.view(P, 1, B) + 0.5 * torch.randn((P, 14, B), generator=gen, device=dev)).clamp_min(0).contiguous()
        row = y.view(P, 1, B).clone()
        for method, name in ((1, "sqrt"), (0, "perturbed")):
            e = eps if method == 0 else None

            def new():
                return _analyse(states, history, y, obs, var, name, 1.05, e, 1e-5, [row], -math.inf, None, False)[:3]

            def route():
                return torch_update(states, history, row, y, obs, var, method, 1.05, eps, 1e-5)

            a, b = new(), route()
            worst = max(float(((u - v).abs() / (v.abs() + 1e-3)).max()) for u, v in ((a[0], b[0]), (a[1], b[1]), (a[2][0], b[2])))
            assert worst < 1e-5, worst                  # the two routes compute the same update
            variants = {"enkf_update": new, "float64 torch": route}
            for fn in variants.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in variants}
            for _ in range(args.steps):
                for k, fn in variants.items():
                    t, _ = timed(fn)
                    ms[k].append(t)
            for k, fn in variants.items():
                mem = peak_mb(fn)
                ops.KERNEL_EVENTS = []
                fn()
                torch.cuda.synchronize()
                calls = {}
                for n, e0, e1 in ops.KERNEL_EVENTS:
                    calls[n] = round(calls.get(n, 0.0) + e0.elapsed_time(e1), 4)
                ops.KERNEL_EVENTS = None
                print(json.dumps({"B": B, "M": M, "P": P, "method": name, "variant": k,
                                  "ms_median": round(statistics.median(ms[k]), 4),
                                  "ms_range": [round(min(ms[k]), 4), round(max(ms[k]), 4)], "reps": len(ms[k]),
                                  "peak_mb": mem, "kernel_ms": calls, "max_rel_diff": worst}), flush=True)
        torch.cuda.empty_cache()


def bench_filters(args, dev, T, B, M, P):
    import hydrodl2_amd
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "dynamic_params": {"Hbv": []}, "warm_up": 0}, dev)
    x = torch.from_numpy(synth.forcing(T, B, 92)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(4)
    p = torch.randn((1, B, model.learnable_param_count), generator=gen, device=dev).expand(T, -1, -1).contiguous()
    with torch.no_grad():
        tg = (model({"x_phy": x}, p)["streamflow"][..., 0] * 1.1 + 0.05).clone()
    xd = {"x_phy": x}
    sigma = 0.05 * tg.mean(0)

    def pf():
        g = torch.Generator().manual_seed(7)
        return hydrodl2_amd.particle_filter(model, xd, p, tg, P, 1, obs_sigma=sigma, prcp_sigma=0.4, state_sigma=0.5,
                                            generator=g)["mean"]

    def kf(method):
        def run():
            g = torch.Generator().manual_seed(7)
            return hydrodl2_amd.enkf_filter(model, xd, p, tg, P, 1, obs_sigma=sigma, method=method, prcp_sigma=0.4,
                                            state_sigma=0.5, state_add_sigma=5.0, inflation=1.05, generator=g)["forecast_mean"]
        return run

    variants = {"particle_filter, one-day windows": pf, "enkf_filter sqrt, one-day windows": kf("sqrt"),
                "enkf_filter perturbed, one-day windows": kf("perturbed")}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(max(args.steps // 2, 2)):
        for k, fn in variants.items():
            ms[k].append(timed(fn)[0])
    for k, fn in variants.items():
        print(json.dumps({"variant": k, "T": T, "B": B, "M": M, "P": P, "ms_median": round(statistics.median(ms[k]), 1),
                          "ms_range": [round(min(ms[k]), 1), round(max(ms[k]), 1)], "reps": len(ms[k]),
                          "ms_per_window": round(statistics.median(ms[k]) / T, 3), "peak_mb": peak_mb(fn)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--particles", default="64,256")
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--big-only", action="store_true")
    ap.add_argument("--filter-days", type=int, default=730)
    ap.add_argument("--no-filter", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    particles = [int(v) for v in args.particles.split(",")]
    if not args.big_only:
        bench_update(args, dev, 100, 16, particles)
    if not args.small_only:
        bench_update(args, dev, 671, 16, particles)
    if not args.no_filter:
        bench_filters(args, dev, args.filter_days, 100, 16, 64)


if __name__ == "__main__":
    main()
