#!/usr/bin/env python3
"""Time `adj_population_period_stats` (hydrodl2_amd/adj_population.py, hbvx_adj_population_period in include/hbvx.h) --
monthly flow_sim plus an 8-day soil moisture, two KGE per candidate -- against the routes there were before:

  (a) `adj_population_stats` on daily observations: the price of the period machinery and of the aux term (it scores
      days of the flow alone);
  (b) `adj_population_stats(return_series=True)`, period means of the [P,T_out,B] series and float64 KGE in torch: the
      old route to the FLOW score;
  (c) P forwards of the module under ops.record_paths(want_traj=True), the ensemble mean of SM at the end of each day
      from each trajectory, its 8-day means and float64 KGE: the old route to the AUX score.

    python tools/bench_adj_population_period.py [--steps 5] [--warmup 2] [--loop-steps 2] [--cands 16,64,256]
                                                [--configs staged:0,staged:5,joint:0] [--joint-cands 64]
                                                [--small-only | --big-only] [--skip-loop]

The kernels of (a), (b) and (c) are the parent commit's instruction for instruction (tools/compare_code.py), so one
build times all four.  A config is solver:n, n the number of dynamic parameters (the first n of parBETA, parK0, parFC,
parUZL, parPERC; 5 takes the generic fetch); the joint solver is timed at --joint-cands only.  Two shapes, 671 x 16 x
7300 and 100 x 16 x 730.  One process; every variant is warmed at every shape it is timed at; a timed repetition is one
whole call (or one whole loop) between two HIP events, the variants alternating repetition by repetition; median [min,
max] over the repetitions.  Per (config, shape, P) one JSON line per variant with its peak memory (torch's allocator,
above what the inputs hold) and the kernel by itself, and at the smallest P one with the worst difference of the two
KGE from the chains against float64 KGE over the kernel's own period series, |chains - series| / (1 + |1 - series|)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_adj_population import DYN_ORDER  # noqa: E402
from bench_population import peak_mb, timed  # noqa: E402
from bench_population_joint import kge_of_series  # noqa: E402
from bench_population_period import month_ends, period_means  # noqa: E402

AUX_KEY, AUX_ROW, AUX_CAL = "SM", 2, 8


def bench_shape(args, dev, solver, n_dyn, T, B, M, cands):
    import hydrodl2_amd
    from hydrodl2_amd import ops
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    cfg = {"nmul": M, "dynamic_params": {"HbvAdj": list(DYN_ORDER[:n_dyn])}, "newton_solver": solver}
    model = hydrodl2_amd.load_model("hbv_adj", "HbvAdj")(cfg, dev)
    x_dict = {"x_phy": torch.from_numpy(synth.forcing(T, B, 92)).to(dev)}
    gen = torch.Generator(device=dev).manual_seed(4)
    p = torch.randn((T, B, model.learnable_param_count), generator=gen, device=dev)
    _, cols = hydrodl2_amd.sensitivity.jacobian_columns(model, None)
    C = len(cols)

    def forward(params):
        """(flow_sim [T,B], the ensemble mean of SM at the end of each day [T,B]) by the module's own route"""
        with torch.no_grad(), ops.record_paths(want_traj=True) as records:
            flow = model(x_dict, params)["flow_sim"][..., 0]
        rec = records[-1]
        return flow, rec.traj.view(5, rec.cfg.T + 1, B, M)[AUX_ROW, 1:].mean(-1)

    flow, aux = forward(p)
    T_out = int(flow.shape[0])
    fcal = month_ends(T_out)

    def noisy(series, cal):
        m = period_means(series, cal)
        return (m * torch.exp(0.2 * torch.randn(m.shape, generator=gen, device=dev, dtype=torch.float64))).float().contiguous()

    daily_tgt = (flow * 1.1 + 0.05).clone()
    ftgt, atgt = noisy(flow, fcal), noisy(aux, AUX_CAL)
    work = p.clone()
    for P in cands:
        cand = p[-1][:, cols].unsqueeze(0) + 0.5 * torch.randn((P, B, C), generator=gen, device=dev)
        cand[0] = p[-1][:, cols]

        def new():
            st = hydrodl2_amd.adj_population_period_stats(model, x_dict, p, cand, ftgt, fcal, atgt, AUX_KEY, AUX_CAL)
            return hydrodl2_amd.population_score(st["flow"], "kge"), hydrodl2_amd.population_score(st["aux"], "kge")

        def daily():
            return hydrodl2_amd.population_score(hydrodl2_amd.adj_population_stats(model, x_dict, p, cand, daily_tgt), "kge")

        def series_route():
            st = hydrodl2_amd.adj_population_stats(model, x_dict, p, cand, daily_tgt, return_series=True)
            return kge_of_series(period_means(st["series"], fcal), ftgt)

        def loop():
            out = []
            for c in range(P):
                work[-1][:, cols] = cand[c]
                out.append(period_means(forward(work)[1], AUX_CAL))
            return kge_of_series(torch.stack(out), atgt)

        variants = {"adj_population_period_stats (monthly flow + 8-day SM) + 2 x population_score(kge)": (new, args.steps),
                    "(a) adj_population_stats on daily observations + population_score(kge)": (daily, args.steps),
                    "(b) adj_population_stats(return_series) + monthly means and float64 KGE in torch": (series_route, args.steps)}
        if not args.skip_loop:
            variants["(c) P forwards with trajectories + 8-day SM means and float64 KGE in torch"] = \
                (loop, args.loop_steps if P < 256 else max(1, args.loop_steps - 1))
        for k, (fn, _) in variants.items():
            for _ in range(1 if k.startswith("(c)") else args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for rep in range(max(n for _, n in variants.values())):
            for k, (fn, n) in variants.items():
                if rep < n:
                    ms[k].append(timed(fn)[0])
        base = {"solver": solver, "n_dyn": n_dyn, "T": T, "B": B, "M": M, "C": C, "periods": [len(fcal), T_out // AUX_CAL],
                "P": P}
        for k, (fn, _) in variants.items():
            mem = peak_mb(fn)
            calls = {}
            if not k.startswith("(c)"):
                ops.KERNEL_EVENTS = []
                fn()
                torch.cuda.synchronize()
                for n, e0, e1 in ops.KERNEL_EVENTS:
                    if "population" in n:
                        calls[n] = round(calls.get(n, 0.0) + e0.elapsed_time(e1), 3)
                ops.KERNEL_EVENTS = None
            print(json.dumps(dict(base, variant=k, ms_median=round(statistics.median(ms[k]), 3),
                                  ms_range=[round(min(ms[k]), 3), round(max(ms[k]), 3)], reps=len(ms[k]), peak_mb=mem,
                                  kernel_ms=calls)), flush=True)
        if P == min(cands):
            st = hydrodl2_amd.adj_population_period_stats(model, x_dict, p, cand, ftgt, fcal, atgt, AUX_KEY, AUX_CAL,
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
    ap.add_argument("--loop-steps", type=int, default=2)
    ap.add_argument("--cands", default="16,64,256")
    ap.add_argument("--configs", default="staged:0,staged:5,joint:0", help="solver:number of dynamic parameters")
    ap.add_argument("--joint-cands", default="64", help="the populations the joint solver is timed at")
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--big-only", action="store_true")
    ap.add_argument("--skip-loop", action="store_true", help="leave route (c), the loop of P forwards, out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    for config in args.configs.split(","):
        solver, n_dyn = config.split(":")
        cands = [int(v) for v in (args.joint_cands if solver == "joint" else args.cands).split(",")]
        if not args.big_only:
            bench_shape(args, dev, solver, int(n_dyn), 730, 100, 16, cands)
        if not args.small_only:
            bench_shape(args, dev, solver, int(n_dyn), 7300, 671, 16, cands)


if __name__ == "__main__":
    main()
