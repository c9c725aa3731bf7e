#!/usr/bin/env python3
"""Time `hourly_population_stats` (hydrodl2_amd/hourly_population.py, include/hbvx_gage_pop.h) against the route there
was before to the scores of P candidates of `Hbv_2_hourly`: P module forwards with `p_sta` and `parameters[2]`
substituted, period means and float64 KGE of `streamflow` in torch.

    python tools/bench_hourly_population.py [--steps 5] [--warmup 2] [--cands 16,64,256] [--modes both,routing]
                                            [--calendars hourly,24] [--small-only | --big-only]

Two shapes: bench.py's `hourly` workload (2 160 hours, 4 000 units, 4 members, 100 gages, parBETA / parK0 / parBETAET
dynamic, every gage draining ~2 % of the units) and a small one (400 hours, 100 units, 10 gages).  Modes: 'both' (unit
and routing candidates together) and 'routing' (distr_candidates only: stage 1 is not launched).  Calendars: every hour
scored, and 24-hour means.  One process; every variant is warmed at every shape it is timed at; a timed repetition is one
whole call between two HIP events, the variants alternating repetition by repetition; median [min, max] over the
repetitions (bench.py's protocol, as tools/bench_population_period.py).  Per (shape, mode, calendar, P) one JSON line per
variant with its peak memory and the time of each stage's entry point by itself, and at the smallest P one line with the
worst difference of the two routes' KGE, |new - old| / (1 + |1 - old|)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_population import peak_mb, timed  # noqa: E402

DYN = ["parBETA", "parK0", "parBETAET"]


def problem(dev, T, U, M, G):
    """bench.py's `hourly` workload at (T, U, M, G): (model, x_dict, parameters)."""
    import bench
    import hydrodl2_amd
    model = hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")({"nmul": M, "dynamic_params": {"Hbv_2_hourly": DYN}}, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    x = bench.synth_forcing(T, U, dev, g) * torch.tensor([1 / 8.0, 1.0, 1 / 24.0], device=dev)
    topo = (torch.rand((G, U), generator=g, device=dev) < 0.02).float()
    topo[torch.arange(U, device=dev) % G, torch.arange(U, device=dev)] = 1.0
    pd = torch.rand((T, U, len(DYN) * M), generator=g, device=dev)
    ps = torch.rand((U, (19 - len(DYN)) * M), generator=g, device=dev)
    pr = torch.rand((int(topo.sum()), 3), generator=g, device=dev)
    xd = {"x_phy": x.contiguous(), "ac_all": torch.rand(U, generator=g, device=dev) * 5000,
          "elev_all": torch.rand(U, generator=g, device=dev) * 3000, "outlet_topo": topo,
          "areas": torch.rand(U, generator=g, device=dev) * 90 + 5}
    return model, xd, (pd, ps, pr)


def period_means(series, cal):
    if cal is None:
        return series.double()
    K = series.shape[-2] // cal
    return series[..., :K * cal, :].double().unflatten(-2, (K, cal)).mean(-2)


def kge_of_series(sim, obs):
    """float64 KGE [P,G] of sim [P,K,G] against obs [K,G], unit weights."""
    s, o = sim.double(), obs.double()
    ms, mo = s.mean(1), o.mean(0)
    ss, so = s.std(1, unbiased=False), o.std(0, unbiased=False)
    r = ((s - ms.unsqueeze(1)) * (o - mo)).mean(1) / (ss * so)
    return 1 - ((r - 1) ** 2 + (ss / so - 1) ** 2 + (ms / mo - 1) ** 2).sqrt()


def bench_shape(args, dev, T, U, M, G, cands, modes, calendars):
    import hydrodl2_amd
    from hydrodl2_amd import ops
    model, xd, p = problem(dev, T, U, M, G)
    cols = torch.as_tensor(hydrodl2_amd.hourly_population_columns(model), device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    with torch.no_grad():
        flow = model(xd, p)["streamflow"][..., 0]
    n_pair = int(p[2].shape[0])
    for cal_name in calendars:
        cal = None if cal_name == "hourly" else int(cal_name)
        m = period_means(flow, cal)
        tgt = (m * torch.exp(0.2 * torch.randn(m.shape, generator=gen, device=dev, dtype=torch.float64))).float().contiguous()
        for mode in modes:
            for P in cands:
                cand = None if mode == "routing" else torch.rand((P, U, len(cols)), generator=gen, device=dev)
                dcand = torch.rand((P, n_pair, 3), generator=gen, device=dev)

                def new():
                    st = hydrodl2_amd.hourly_population_stats(model, xd, p, tgt, cand, dcand, periods=cal)
                    return hydrodl2_amd.population_score(st, "kge")

                def old():
                    out = []
                    with torch.no_grad():
                        for c in range(P):
                            ps = p[1]
                            if cand is not None:
                                ps = ps.clone()
                                ps[:, cols] = cand[c]
                            sim = model(xd, (p[0], ps, dcand[c]))["streamflow"][..., 0]
                            out.append(kge_of_series(period_means(sim, cal).unsqueeze(0), tgt)[0])
                    return torch.stack(out)

                variants = {"hourly_population_stats + population_score(kge)": new,
                            "P module forwards + period means and float64 KGE in torch": old}
                for fn in variants.values():
                    for _ in range(args.warmup):
                        fn()
                torch.cuda.synchronize()
                ms = {k: [] for k in variants}
                for _ in range(args.steps):
                    for k, fn in variants.items():
                        t, _ = timed(fn)
                        ms[k].append(t)
                base = {"T": T, "U": U, "M": M, "G": G, "pairs": n_pair, "mode": mode, "calendar": cal_name, "P": P}
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
                if P == min(cands):
                    a, b = new(), old()
                    ok = torch.isfinite(a) & torch.isfinite(b)
                    print(json.dumps(dict(base, variant="KGE of the two routes",
                                          worst_difference=float(((a - b).abs() / (1 + (1 - b).abs()))[ok].max()),
                                          kge_range=[round(float(b[ok].min()), 3), round(float(b[ok].max()), 3)],
                                          without_a_score=[int((~torch.isfinite(a)).sum()), int((~torch.isfinite(b)).sum())])),
                          flush=True)
                del cand, dcand
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cands", default="16,64,256")
    ap.add_argument("--modes", default="both,routing")
    ap.add_argument("--calendars", default="hourly,24")
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--big-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    cands = [int(v) for v in args.cands.split(",")]
    if not args.big_only:
        bench_shape(args, dev, 400, 100, 4, 10, cands, args.modes.split(","), args.calendars.split(","))
    if not args.small_only:
        bench_shape(args, dev, 2160, 4000, 4, 100, cands, args.modes.split(","), args.calendars.split(","))


if __name__ == "__main__":
    main()
