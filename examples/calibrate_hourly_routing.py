#!/usr/bin/env python3
"""A twin experiment for the routing search of the hourly model: does a flood-event term in the objective buy timing
that a KGE alone does not see?

The observations are the gage streamflow of `Hbv_2_hourly` at hidden distributed routing parameters (route_a, route_b,
route_tau per (gage, unit) pair) times a little noise.  The start is the hidden rows perturbed in the unit cube.  The
event windows come from `flood_events` on the observations.  Two searches from that start, both per gage and both
routing-only (stage 1 of the population evaluation never launches; every round is one call):

    hourly_routing_search(objective='kge')                       minimises 1 - KGE of the hourly flow
    hourly_routing_search(objective='kge', event_share=S, ...)   minimises (1 - S) (1 - KGE) + S peak_timing
and, with --fdc-share F > 0, a third one with a flow-duration term in the place of the event term:
    hourly_routing_search(objective='kge', fdc_share=F, ...)     minimises (1 - F) (1 - KGE) + F hourly_fdc_score

    python examples/calibrate_hourly_routing.py [--hours 480] [--units 40] [--gages 4] [--nmul 4] [--candidates 64]
                                                [--rounds 4] [--events 4] [--before 12] [--after 24] [--event-share 0.5]
                                                [--perturb 0.3] [--seed 0] [--fdc-share 0] [--fdc-metric fdc_freq]

Prints one JSON line: the basin-mean KGE and the basin-mean peak_timing IN HOURS (the mean |hour of the simulated peak -
hour of the observed peak| over a gage's events, mean over the gages) at the start, after the KGE-only search and after
the search with the event term, and the root-mean-square distance of the routing rows from the hidden ones in unit
space.  Every report also holds the basin-mean fdc_freq and fdc_quantile (`hourly_fdc_score` at the default fifteen
probabilities: the distance of the simulated flow-duration curve from the observed one along the probability axis and
along the flow axis).  Synthetic storm forcing (tests/synth.py), ONE seed (--seed, default 0): the line is what that seed gives, not a
mean over seeds, and nothing says the event term or the flow-duration term wins on another."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hydrodl2_amd  # noqa: E402
import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=int, default=480)
    ap.add_argument("--units", type=int, default=40)
    ap.add_argument("--gages", type=int, default=4)
    ap.add_argument("--nmul", type=int, default=4)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--events", type=int, default=4)
    ap.add_argument("--before", type=int, default=12)
    ap.add_argument("--after", type=int, default=24)
    ap.add_argument("--event-share", type=float, default=0.5)
    ap.add_argument("--perturb", type=float, default=0.3, help="half-width of the start's box around the hidden rows")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fdc-share", type=float, default=0.0, help="> 0: a third search with a flow-duration term of this share")
    ap.add_argument("--fdc-metric", default="fdc_freq", help="fdc_freq, fdc_vol, fdc_quantile or fdc_slope")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the example runs the HIP path; there is no CPU fallback"
    dev = torch.device("cuda:0")
    T, U, G, M, seed = args.hours, args.units, args.gages, args.nmul, args.seed
    model = hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")({"nmul": M, "dynamic_params": {"Hbv_2_hourly": []}}, dev)
    topo = (synth.uniform((G, U), seed, 13) < np.float32(0.3)).astype(np.float32)
    topo[np.arange(U) % G, np.arange(U)] = 1.0                      # every unit drains to a gage, gages share units
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    xd = {"x_phy": to(synth.forcing_hourly(T, U, seed, storm=5.0, day0=100.25)),
          "ac_all": to((synth.uniform((U,), seed, 7) * np.float32(5000.0)).astype(np.float32)),
          "elev_all": to((synth.uniform((U,), seed, 8) * np.float32(3000.0)).astype(np.float32)),
          "outlet_topo": to(topo),
          "areas": to((synth.uniform((U,), seed, 14) * np.float32(90.0) + np.float32(5.0)).astype(np.float32))}
    n_pair = int(topo.sum())
    p_dyn = to(synth.unit_parameters((T, U, 0), seed, 4))
    p_sta = to(synth.unit_parameters((U, 19 * M), seed, 6))
    hidden = to(synth.unit_parameters((n_pair, 3), seed, 15))
    noise = to(synth.normalish((T, G), seed, 195))
    with torch.no_grad():
        truth = model(xd, (p_dyn, p_sta, hidden))["streamflow"][..., 0]
    obs = (truth * torch.exp(0.05 * noise)).contiguous()
    gen = torch.Generator().manual_seed(seed)
    start = (hidden + (torch.rand((n_pair, 3), generator=gen).to(dev) - 0.5) * 2 * args.perturb).clamp(0.0, 1.0)
    events = hydrodl2_amd.flood_events(obs, args.events, args.before, args.after)
    params = (p_dyn, p_sta, start)

    def report(p_distr):
        st = hydrodl2_amd.hourly_population_event_stats(model, xd, (p_dyn, p_sta, p_distr), obs, events,
                                                        distr_candidates=p_distr.unsqueeze(0).contiguous())
        kge = hydrodl2_amd.population_score(st, "kge")[0]
        hours = hydrodl2_amd.hourly_event_score(st, "peak_timing", timing_scale=1.0)[0]
        fd = hydrodl2_amd.hourly_population_fdc_stats(model, xd, (p_dyn, p_sta, p_distr), obs,
                                                      distr_candidates=p_distr.unsqueeze(0).contiguous())
        return {"kge_mean": round(float(kge.nanmean()), 4), "peak_timing_hours_mean": round(float(hours.nanmean()), 3),
                "peak_error_mean": round(float(hydrodl2_amd.hourly_event_score(st, "peak_error")[0].nanmean()), 4),
                "fdc_freq_mean": round(float(hydrodl2_amd.hourly_fdc_score(fd, "fdc_freq")[0].nanmean()), 5),
                "fdc_quantile_mean": round(float(hydrodl2_amd.hourly_fdc_score(fd, "fdc_quantile")[0].nanmean()), 5),
                "rms_distance_to_hidden": round(float((p_distr - hidden).square().mean().sqrt()), 4)}

    common = dict(n_candidates=args.candidates, n_rounds=args.rounds, objective="kge")
    (_, _, by_kge), h_kge = hydrodl2_amd.hourly_routing_search(model, xd, params, obs, generator=torch.Generator().manual_seed(seed + 1),
                                                               **common)
    (_, _, by_both), h_both = hydrodl2_amd.hourly_routing_search(model, xd, params, obs, events=events, event_share=args.event_share,
                                                                 event_metric="peak_timing", timing_scale=24.0,
                                                                 generator=torch.Generator().manual_seed(seed + 1), **common)
    with_fdc = {}
    if args.fdc_share > 0:
        (_, _, by_fdc), h_fdc = hydrodl2_amd.hourly_routing_search(model, xd, params, obs, fdc_share=args.fdc_share,
                                                                   fdc_metric=args.fdc_metric,
                                                                   generator=torch.Generator().manual_seed(seed + 1), **common)
        with_fdc = {"fdc_share": args.fdc_share, "fdc_metric": args.fdc_metric, "search_with_fdc_term": report(by_fdc),
                    "cost_with_fdc_term": [round(float(v), 4) for v in h_fdc["cost"].mean(1)]}
    print(json.dumps({"seed": seed, "hours": T, "units": U, "gages": G, "pairs": n_pair, "candidates": args.candidates,
                      "rounds": args.rounds, "events_per_gage": (events[0] >= 0).sum(0).tolist(),
                      "window_hours": args.before + args.after + 1, "event_share": args.event_share,
                      "start": report(start), "kge_only_search": report(by_kge), "search_with_event_term": report(by_both),
                      "cost_kge_only": [round(float(v), 4) for v in h_kge["cost"].mean(1)],
                      "cost_with_event_term": [round(float(v), 4) for v in h_both["cost"].mean(1)], **with_fdc}))


if __name__ == "__main__":
    main()
