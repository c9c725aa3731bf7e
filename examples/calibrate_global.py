#!/usr/bin/env python3
"""A twin experiment for the population step: does a random search in front of Levenberg-Marquardt find a better
optimum than Levenberg-Marquardt alone from the same poor start?

The observations come from known static parameters.  The start is far from them (raw values drawn three times as
wide).  Two routes from that start, both per basin:

    calibrate                         LM alone: first order, accepts a step only when the cost falls
    population_search -> calibrate    a shrinking random search (hbvx_population_cost: every candidate of a round in
                                      one launch) picks the row LM starts from

    python examples/calibrate_global.py [--basins 32] [--days 730] [--nmul 4] [--candidates 256] [--rounds 3] [--lm-iters 8]
                                        [--objective sse|nse|kge|kge12] [--transform none|sqrt|log] [--model Hbv|HbvAdj]
                                        [--aux-key AET_hydro|SWE|srflow_no_rout|ssflow_no_rout|gwflow_no_rout |
                                                   SNOWPACK|MELTWATER|SM|SUZ|SLZ (HbvAdj)] [--aux-share 0.5]
                                        [--aux-period N] [--fdc-share S]
                                        [--event-share S] [--event-metric peak_error|peak_bias|peak_timing|volume_error]

--model HbvAdj runs the same experiment on the implicit scheme: adj_population_search (hbvx_adj_population_cost: every
candidate's days solved in registers) in front of calibrate, scored on 'flow_sim', from the module's own start (empty
storages); the routing parameters are then 'rout_a' and 'rout_b'.
--objective / --transform choose what the search minimises (hbvx_population_stats: NSE, KGE on the raw, square-root or
log flow); Levenberg-Marquardt after it is least squares on the raw flow either way.
--aux-key (Hbv, with --objective nse / kge / kge12) makes the twin problem also observe the hidden row's series of that
key every 8th day, and adds a third route: the search on (1 - share) * flow cost + share * (1 - NSE of the aux series)
(hbvx_population_joint: both scores of every candidate from one launch) in front of the same Levenberg-Marquardt.  The
line then carries, for the search with and without the aux term, the basin means of the flow and the aux scores at the
start and at the search's pick, and the distance of the picked row from the hidden one in unit space (the root mean
square over the searched columns of sigmoid(raw) differences, mean over the basins).
--aux-period N (with --aux-key) observes the aux series as what an N-day composite is: the MEANS of the hidden row's
series over blocks of N days, compared with the candidates' means over the same blocks (hbvx_population_period), instead
of one day's value in eight.  The flow stays daily.
--model HbvAdj takes --aux-key SNOWPACK, MELTWATER, SM, SUZ or SLZ: the second series is then the ensemble mean of that
storage at the end of each day (the hidden row's comes from the module's trajectory), and both forms of the aux
observation go through hbvx_adj_population_period.
--fdc-share S (Hbv, with --objective nse / kge / kge12, without --aux-key) adds a route: the search on (1 - S) * flow cost
+ S * fdc_freq, the mean distance between the simulated and the observed flow-duration curve at fifteen exceedance
probabilities (hbvx_population_fdc: the exceedance counts of every candidate from the launch that scores its flow), in
front of the same Levenberg-Marquardt.  The line then carries the basin-mean fdc_freq at the start and at the end of the
search with and without the term, beside the SSE / NSE / KGE of both.
--event-share S (Hbv, with --objective nse / kge / kge12, without --aux-key or --fdc-share) adds a route: the search on
(1 - S) * flow cost + S * the --event-metric score (default peak_error) over the ten highest separated floods of the
observations per basin, windows from three days before the observed peak to seven after (flood_events;
hbvx_population_events: every candidate's peak, day of the peak and volume in each window from the launch that scores
its flow), in front of the same Levenberg-Marquardt.  The line then carries the basin means of all four event scores at
the start and at the end of the search with and without the term, beside the SSE / NSE / KGE of both.  One seed: read a
difference between the two searches as one draw, not as a ranking.
Prints one JSON line: per route the summed cost and the number of basins in which it ended lower, with the cost of
the start and of the search's pick beside them, and -- whichever objective was searched -- the basin means of SSE, NSE
and KGE on the raw flow at the start and at the end of every route.  Synthetic forcings (tests/synth.py), a fixed seed.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import hydrodl2_amd  # noqa: E402
import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--basins", type=int, default=32)
    ap.add_argument("--days", type=int, default=730)
    ap.add_argument("--nmul", type=int, default=4)
    ap.add_argument("--candidates", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lm-iters", type=int, default=8)
    ap.add_argument("--objective", default="sse", choices=["sse", "nse", "kge", "kge12"],
                    help="what the population search minimises (1 - score for nse / kge / kge12)")
    ap.add_argument("--transform", default="none", choices=["none", "sqrt", "log"],
                    help="the flow the search scores: raw, square root or log(Q + eps)")
    ap.add_argument("--names", default=None,
                    help="default: parBETA,parFC,parK0,parK1,parK2,parLP,parPERC,parUZL and the two routing parameters")
    ap.add_argument("--model", default="Hbv", choices=["Hbv", "HbvAdj"])
    fluxes, storages = list(hydrodl2_amd.population.AUX_KEYS), list(hydrodl2_amd.adj_population.AUX_KEYS)
    ap.add_argument("--aux-key", default=None, choices=fluxes + storages,
                    help="also observe this series of the hidden row every 8th day and search on both scores "
                         "(a flux of Hbv, a storage of HbvAdj)")
    ap.add_argument("--aux-share", type=float, default=0.5, help="the aux term's share of the searched cost")
    ap.add_argument("--aux-period", type=int, default=None,
                    help="observe the aux series as N-day means of the hidden row instead of every 8th day")
    ap.add_argument("--fdc-share", type=float, default=0.0,
                    help="also search on (1 - S) * flow cost + S * fdc_freq, the distance between the flow-duration curves")
    ap.add_argument("--event-share", type=float, default=0.0,
                    help="also search on (1 - S) * flow cost + S * an event score over the observed floods")
    ap.add_argument("--event-metric", default="peak_error", choices=list(hydrodl2_amd.population_events.EVENT_METRICS))
    args = ap.parse_args()
    if args.event_share and (args.model != "Hbv" or args.objective == "sse" or args.aux_key or args.fdc_share
                             or not 0 < args.event_share <= 1):
        ap.error("--event-share S in (0, 1] goes with --model Hbv and --objective nse, kge or kge12, without --aux-key "
                 "or --fdc-share")
    if args.fdc_share and (args.model != "Hbv" or args.objective == "sse" or args.aux_key or not 0 < args.fdc_share <= 1):
        ap.error("--fdc-share S in (0, 1] goes with --model Hbv and --objective nse, kge or kge12, without --aux-key")
    if args.aux_period is not None and (not args.aux_key or args.aux_period < 1):
        ap.error("--aux-period N >= 1 goes with --aux-key")
    if args.aux_key and args.objective == "sse":
        ap.error("--aux-key goes with --objective nse, kge or kge12")
    if args.aux_key and args.aux_key not in (storages if args.model == "HbvAdj" else fluxes):
        ap.error(f"--aux-key of --model {args.model} is one of {storages if args.model == 'HbvAdj' else fluxes}")
    assert torch.cuda.is_available(), "the example runs on the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    T, B, M = args.days, args.basins, args.nmul
    adj = args.model == "HbvAdj"
    key = "flow_sim" if adj else "streamflow"
    names = (args.names or "parBETA,parFC,parK0,parK1,parK2,parLP,parPERC,parUZL,"
             + ("rout_a,rout_b" if adj else "route_a,route_b")).split(",")
    if adj:
        model = hydrodl2_amd.load_model("hbv_adj", "HbvAdj")({"nmul": M, "dynamic_params": {"HbvAdj": []}}, dev)
        search, stats = hydrodl2_amd.adj_population_search, hydrodl2_amd.adj_population_stats
    else:
        model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "dynamic_params": {"Hbv": []}}, dev)
        search, stats = hydrodl2_amd.population_search, hydrodl2_amd.population_stats
    x = {"x_phy": torch.from_numpy(synth.forcing(T, B, seed=71)).to(dev)}
    ny = model.learnable_param_count
    truth = torch.from_numpy(synth.raw_parameters(T, B, ny, seed=72)).to(dev)
    with torch.no_grad(), hydrodl2_amd.ops.record_paths(want_traj=True) as records:
        hidden = model(x, truth)
    obs = hidden[key][..., 0].clone()
    if adj and args.aux_key:
        # the storage at the end of each day, ensemble mean: rows 1..T of the trajectory [5, T + 1, B * M]
        k = storages.index(args.aux_key)
        hidden = dict(hidden)
        hidden[args.aux_key] = records[-1].traj.view(5, T + 1, B, M)[k, 1:].mean(-1, keepdim=True)
    # the poor start: the named columns of the static row drawn anew, three times as wide; everything else is the truth's
    _, cols = hydrodl2_amd.sensitivity.jacobian_columns(model, names)
    start = truth.clone()
    start[-1][:, cols] = torch.from_numpy(synth.raw_parameters(1, B, ny, seed=73, scale=3.0)).to(dev)[0][:, cols]

    lm_only, h_lm = hydrodl2_amd.calibrate(model, x, start, obs, names=names, n_iter=args.lm_iters)
    gen = torch.Generator().manual_seed(74)
    picked, h_ps = search(model, x, start, obs, names=names, n_candidates=args.candidates, n_rounds=args.rounds,
                          generator=gen, objective=args.objective, transform=args.transform)
    both, h_both = hydrodl2_amd.calibrate(model, x, picked, obs, names=names, n_iter=args.lm_iters)

    def worth(row):
        """Basin means of SSE, NSE and KGE of a parameter tensor on the raw flow, whichever objective was searched: one
        population_stats call with the row as its only candidate."""
        cand = row[-1][:, cols].unsqueeze(0).contiguous()
        st = stats(model, x, row, cand, obs, names=names)
        return {m: float(hydrodl2_amd.population_score(st, m).mean()) for m in ("sse", "nse", "kge")}

    joint = {}
    if args.aux_key:
        n = args.aux_period
        if n:
            K = obs.shape[0] // n                   # an incomplete last block is not observed
            aux_obs = hidden[args.aux_key][..., 0][:K * n].double().unflatten(0, (K, n)).mean(1).float().contiguous()
        else:
            aux_obs = torch.full_like(obs, float("nan"))
            aux_obs[::8] = hidden[args.aux_key][..., 0][::8]
        picked_aux, h_aux = search(model, x, start, obs, names=names, n_candidates=args.candidates, n_rounds=args.rounds,
                                   generator=torch.Generator().manual_seed(74), objective=args.objective,
                                   transform=args.transform, aux_target=aux_obs, aux_key=args.aux_key,
                                   aux_share=args.aux_share, aux_periods=n)
        both_aux, h_both_aux = hydrodl2_amd.calibrate(model, x, picked_aux, obs, names=names, n_iter=args.lm_iters)

        def both_scores(row):
            cand = row[-1][:, cols].unsqueeze(0).contiguous()
            if adj:
                st = hydrodl2_amd.adj_population_period_stats(model, x, row, cand, obs, None, aux_obs, args.aux_key, n,
                                                              names=names)
            elif n:
                st = hydrodl2_amd.population_period_stats(model, x, row, cand, obs, None, aux_obs, args.aux_key, n, names=names)
            else:
                st = hydrodl2_amd.population_joint_stats(model, x, row, cand, obs, aux_obs, args.aux_key, names=names)
            return {f"{term}_{m}": float(hydrodl2_amd.population_score(st[term], m).nanmean())
                    for term in ("flow", "aux") for m in ("nse", "kge")}

        def distance(row):
            d = torch.sigmoid(row[-1][:, cols]) - torch.sigmoid(truth[-1][:, cols])
            return float(d.pow(2).mean(1).sqrt().mean())

        joint = {
            "aux_key": args.aux_key, "aux_share": args.aux_share, **({"aux_period_days": n, "aux_periods_observed": int(aux_obs.shape[0])} if n else
               {"aux_days_observed": int((~torch.isnan(aux_obs[:, 0])).sum())}),
            "both_scores_start": both_scores(start),
            "both_scores_after_search_flow_only": both_scores(picked),
            "both_scores_after_search_with_aux": both_scores(picked_aux),
            "unit_distance_to_hidden_row": {"start": distance(start), "search_flow_only": distance(picked),
                                            "search_with_aux": distance(picked_aux),
                                            "search_flow_only_then_calibrate": distance(both),
                                            "search_with_aux_then_calibrate": distance(both_aux)},
            "mean_scores_search_with_aux_then_calibrate": worth(both_aux),
            "cost_search_with_aux_then_calibrate": float(h_both_aux["cost"][-1].sum()),
            "search_with_aux_history_mean": {k: [float(v) for v in h_aux[k].nanmean(1)] for k in ("cost", "score", "score_aux")},
        }

    if args.fdc_share:
        picked_fdc, h_fdc = search(model, x, start, obs, names=names, n_candidates=args.candidates, n_rounds=args.rounds,
                                   generator=torch.Generator().manual_seed(74), objective=args.objective,
                                   transform=args.transform, fdc_share=args.fdc_share)
        both_fdc, h_both_fdc = hydrodl2_amd.calibrate(model, x, picked_fdc, obs, names=names, n_iter=args.lm_iters)

        def fdc_freq(row):
            cand = row[-1][:, cols].unsqueeze(0).contiguous()
            st = hydrodl2_amd.population_fdc_stats(model, x, row, cand, obs, names=names)
            return float(hydrodl2_amd.population_fdc_score(st, "fdc_freq").nanmean())

        joint = {
            "fdc_share": args.fdc_share,
            "mean_fdc_freq": {"start": fdc_freq(start), "search_flow_only": fdc_freq(picked), "search_with_fdc": fdc_freq(picked_fdc),
                              "search_flow_only_then_calibrate": fdc_freq(both), "search_with_fdc_then_calibrate": fdc_freq(both_fdc)},
            "mean_scores_after_search_with_fdc": worth(picked_fdc),
            "mean_scores_search_with_fdc_then_calibrate": worth(both_fdc),
            "cost_search_with_fdc_then_calibrate": float(h_both_fdc["cost"][-1].sum()),
            "search_with_fdc_history_mean": {k: [float(v) for v in h_fdc[k].nanmean(1)] for k in ("cost", "score", "score_fdc")},
        }

    if args.event_share:
        events = hydrodl2_amd.flood_events(obs, 10, 3, 7)
        picked_ev, h_ev = search(model, x, start, obs, names=names, n_candidates=args.candidates, n_rounds=args.rounds,
                                 generator=torch.Generator().manual_seed(74), objective=args.objective,
                                 transform=args.transform, events=events, event_share=args.event_share,
                                 event_metric=args.event_metric)
        both_ev, h_both_ev = hydrodl2_amd.calibrate(model, x, picked_ev, obs, names=names, n_iter=args.lm_iters)

        def event_scores(row):
            cand = row[-1][:, cols].unsqueeze(0).contiguous()
            st = hydrodl2_amd.population_event_stats(model, x, row, cand, obs, events, names=names)
            return {m: float(hydrodl2_amd.population_event_score(st, m).nanmean())
                    for m in hydrodl2_amd.population_events.EVENT_METRICS}

        joint = {
            "event_share": args.event_share, "event_metric": args.event_metric,
            "events_per_basin_mean": float((events[0] >= 0).sum(0).double().mean()),
            "mean_event_scores": {"start": event_scores(start), "search_flow_only": event_scores(picked),
                                  "search_with_events": event_scores(picked_ev),
                                  "search_flow_only_then_calibrate": event_scores(both),
                                  "search_with_events_then_calibrate": event_scores(both_ev)},
            "mean_scores_after_search_with_events": worth(picked_ev),
            "mean_scores_search_with_events_then_calibrate": worth(both_ev),
            "cost_search_with_events_then_calibrate": float(h_both_ev["cost"][-1].sum()),
            "search_with_events_history_mean": {k: [float(v) for v in h_ev[k].nanmean(1)]
                                                for k in ("cost", "score", "score_event")},
        }

    c_start, c_lm = h_lm["cost"][0], h_lm["cost"][-1]
    c_pick, c_both = h_both["cost"][0], h_both["cost"][-1]
    print(json.dumps({
        **({"model": args.model} if adj else {}),
        "basins": B, "days": T, "nmul": M, "columns": len(cols), "candidates": args.candidates, "rounds": args.rounds,
        "lm_iters": args.lm_iters, "objective": args.objective, "transform": args.transform,
        "mean_scores_start": worth(start), "mean_scores_calibrate_alone": worth(lm_only),
        "mean_scores_after_population_search": worth(picked),
        "mean_scores_population_search_then_calibrate": worth(both),
        "cost_start": float(c_start.sum()),
        "cost_calibrate_alone": float(c_lm.sum()),
        "cost_after_population_search": float(c_pick.sum()),
        "cost_population_search_then_calibrate": float(c_both.sum()),
        "basins_where_search_then_calibrate_ends_lower": int((c_both < c_lm).sum()),
        "basins_where_calibrate_alone_ends_lower": int((c_lm < c_both).sum()),
        "population_search_history_summed": [float(v) for v in h_ps["cost"].sum(1)],
        **joint,
    }))


if __name__ == "__main__":
    main()
