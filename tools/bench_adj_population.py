#!/usr/bin/env python3
"""Time `adj_population_cost` (hydrodl2_amd/adj_population.py, hbvx_adj_population_cost in include/hbvx.h) against the
route it replaces: P forwards of the HbvAdj module under no_grad, each followed by the float64
`calibrate._series_cost`.

    python tools/bench_adj_population.py [--steps 5] [--warmup 2] [--loop-steps 2] [--cands 16,64,256]
                                         [--solvers staged,joint] [--dyn 0,1,5] [--small-only | --big-only]
                                         [--skip-loop | --loop-only] [--lib other.so]

Routing on; --dyn n makes the first n of parBETA, parK0, parFC, parUZL, parPERC dynamic (0 and 1: the slot-list fetch
of the kernel, 5: the generic one), every other parameter is a candidate column.  Two shapes, 671 x 16 x 7300 and 100 x
16 x 730, P in {16, 64, 256}.  One process; every variant is warmed at every shape it is timed at; a timed repetition is
one whole call (adj_population_cost) or one whole loop of P forwards between two HIP events, the two routes alternating
repetition by repetition; median [min, max] over the repetitions.  The loop writes each candidate into the static row
of ONE working copy of the parameter tensor in place.  Per (solver, dyn, shape, P): one JSON line per route with its
peak memory (torch's allocator, above what the inputs hold), and one with the library calls of an adj_population_cost
call timed by events of their own (the kernel by itself), the worst relative difference of the two routes' costs, and
whether the slowest adj_population_cost repetition beat the fastest loop.
--loop-only --lib <a library of the parent commit> times the loop alone on that library (the baseline);
--skip-loop --lib <variant> times the new call alone on a whole-library A/B variant."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_population import peak_mb, timed  # noqa: E402

DYN_ORDER = ("parBETA", "parK0", "parFC", "parUZL", "parPERC")


def bench_shape(args, dev, solver, n_dyn, T, B, M, cands):
    import hydrodl2_amd
    from hydrodl2_amd import ops
    from hydrodl2_amd.calibrate import _check_request, _series_cost
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    cfg = {"nmul": M, "dynamic_params": {"HbvAdj": list(DYN_ORDER[:n_dyn])}, "newton_solver": solver}
    model = hydrodl2_amd.load_model("hbv_adj", "HbvAdj")(cfg, dev)
    x_dict = {"x_phy": torch.from_numpy(synth.forcing(T, B, 92)).to(dev)}
    gen = torch.Generator(device=dev).manual_seed(4)
    p = torch.randn((T, B, model.learnable_param_count), generator=gen, device=dev)
    _, cols = hydrodl2_amd.sensitivity.jacobian_columns(model, None)
    C = len(cols)
    with torch.no_grad():
        target = (model(x_dict, p)["flow_sim"][..., 0] * 1.1 + 0.05).clone()
    req = _check_request(model, x_dict, p, target, None, None, None, 1)
    work = p.clone()
    new = not args.loop_only
    for P in cands:
        cand = p[-1][:, cols].unsqueeze(0) + 0.5 * torch.randn((P, B, C), generator=gen, device=dev)
        cand[0] = p[-1][:, cols]

        def pop():
            return hydrodl2_amd.adj_population_cost(model, x_dict, p, cand, target)["cost"]

        def loop():
            out = []
            with torch.no_grad():
                for c in range(P):
                    work[-1][:, cols] = cand[c]
                    out.append(_series_cost(req, model(x_dict, work), target, None))
            return torch.stack(out)

        n_loop = 0 if args.skip_loop else (args.loop_steps if P < 256 else max(1, args.loop_steps - 1))
        n_pop = args.steps if new else 0
        if new:
            for _ in range(args.warmup):
                pop()
        if n_loop:
            loop()                                  # P forwards warm the loop's shapes
        torch.cuda.synchronize()
        ms_pop, ms_loop = [], []
        a = b = None
        for k in range(max(n_pop, n_loop)):
            if k < n_pop:
                t, a = timed(pop)
                ms_pop.append(t)
            if k < n_loop:
                t, b = timed(loop)
                ms_loop.append(t)
        base = {"solver": solver, "n_dyn": n_dyn, "T": T, "B": B, "M": M, "C": C, "P": P}

        def line(variant, ms, **kw):
            print(json.dumps(dict(base, variant=variant, ms_median=round(statistics.median(ms), 3),
                                  ms_range=[round(min(ms), 3), round(max(ms), 3)], reps=len(ms), **kw)), flush=True)
        if new:
            line("adj_population_cost", ms_pop, peak_mb=peak_mb(pop))
        if n_loop:
            line("loop of P forwards + _series_cost", ms_loop, peak_mb=peak_mb(loop),
                 over_adj_population_cost=round(statistics.median(ms_loop) / statistics.median(ms_pop), 2) if new else None)
        if new:
            ops.KERNEL_EVENTS = []
            pop()
            torch.cuda.synchronize()
            calls = {}
            for n, e0, e1 in ops.KERNEL_EVENTS:
                calls[n] = round(calls.get(n, 0.0) + e0.elapsed_time(e1), 3)
            ops.KERNEL_EVENTS = None
            rdiff = float(((a.double() - b).abs() / b).max()) if n_loop else None
            print(json.dumps(dict(base, variant="adj_population_cost library calls (ms, summed per entry point)",
                                  calls_ms=calls, worst_relative_cost_difference_of_the_routes=rdiff,
                                  slowest_adj_population_cost_beats_fastest_loop=(max(ms_pop) < min(ms_loop)) if n_loop else None)),
                  flush=True)
        del cand, a, b
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-steps", type=int, default=2)
    ap.add_argument("--cands", default="16,64,256")
    ap.add_argument("--solvers", default="staged,joint")
    ap.add_argument("--dyn", default="0,1,5", help="numbers of dynamic parameters: 0..3 take the slot-list fetch, more the generic one")
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--big-only", action="store_true")
    ap.add_argument("--skip-loop", action="store_true", help="time adj_population_cost alone (A/B of library variants)")
    ap.add_argument("--loop-only", action="store_true", help="time the loop alone (the baseline, on a library of the parent commit)")
    ap.add_argument("--lib", default=None, help="time another build of the library")
    args = ap.parse_args()
    if args.lib:
        from hydrodl2_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    cands = [int(v) for v in args.cands.split(",")]
    for solver in args.solvers.split(","):
        for n_dyn in (int(v) for v in args.dyn.split(",")):
            if not args.big_only:
                bench_shape(args, dev, solver, n_dyn, 730, 100, 16, cands)
            if not args.small_only:
                bench_shape(args, dev, solver, n_dyn, 7300, 671, 16, cands)


if __name__ == "__main__":
    main()
