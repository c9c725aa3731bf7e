#!/usr/bin/env python3
"""The twin experiment of examples/assimilate_pf.py for the ensemble Kalman filter: the same truth (wet carried-in
storages), the same observations (fixed-seed noise, 5 % of the basin's mean flow) and the same open loop (dry default
storages on 0.7 x the precipitation), and `enkf_filter` in place of `particle_filter`.

A particle filter can only choose among the storages its particles have, and 64 particles that start dry under a rain
deficit never contain the truth's wet storages.  The ensemble Kalman filter moves the storages by a gain, so what it needs
is a start with SPREAD: `--state-add-sigma` millimetres of additive noise on every storage, floored at the model's
nearzero (multiplicative noise on 0.001 mm stays at 0.001 mm).

    python examples/assimilate_enkf.py [--basins 8] [--days 150] [--nmul 4] [--particles 64] [--window 1] [--seed 5]
                                       [--method sqrt] [--prcp-sigma 0.4] [--state-add-sigma 50] [--inflation 1.05]
                                       [--horizon 30] [--check]

Prints one JSON line: the squared error against the TRUTH over days 30 .. end of the open loop, of the filter's
`forecast_mean` (each day before its observation is used) and of its `analysis_mean`, summed and per basin; the share of
(day, basin) pairs with a status that is not 0; and -- from a second run that stops `--horizon` days before the end,
followed by `ensemble_forecast` with the same precipitation noise -- the share of the truth's flows inside the
forecast's 5 % .. 95 % band.  --check exits 1 unless both summed errors are below the open loop's.  One seed: one draw.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import hydrodl2_amd  # noqa: E402
from assimilate_pf import SPIN, twin_setup  # noqa: E402


def twin_experiment(basins=8, days=150, nmul=4, particles=64, window=1, seed=5, method="sqrt", prcp_sigma=0.4,
                    state_add_sigma=50.0, inflation=1.05, horizon=30, device="cuda:0"):
    """The experiment above -> a dictionary of plain numbers and lists."""
    T, B = days, basins
    su = twin_setup(basins, days, nmul, device)
    model, x_open, params, truth, obs, sigma, open_loop = (su[k] for k in ("model", "x_open", "params", "truth", "obs",
                                                                           "sigma", "open_loop"))

    def run(T_run):
        gen = torch.Generator().manual_seed(seed)
        return hydrodl2_amd.enkf_filter(model, {"x_phy": x_open[:T_run].contiguous()}, params[:T_run].contiguous(),
                                        obs[:T_run], particles, window, obs_sigma=sigma, method=method,
                                        prcp_sigma=prcp_sigma, state_add_sigma=state_add_sigma, inflation=inflation,
                                        generator=gen), gen

    kf, _ = run(T)
    t8 = truth.double()
    err_open = ((open_loop - truth)[SPIN:].double() ** 2).sum(0)
    err_fc = ((kf["forecast_mean"] - t8)[SPIN:] ** 2).sum(0)
    err_an = ((kf["analysis_mean"] - t8)[SPIN:] ** 2).sum(0)
    status = kf["status"]
    out = {"basins": B, "days": T, "nmul": nmul, "particles": particles, "window": window, "seed": seed, "method": method,
           "prcp_sigma": prcp_sigma, "state_add_sigma": state_add_sigma, "inflation": inflation,
           "sse_open_loop": float(err_open.sum()), "sse_forecast": float(err_fc.sum()), "sse_analysis": float(err_an.sum()),
           "sse_open_loop_per_basin": [round(float(v), 4) for v in err_open],
           "sse_forecast_per_basin": [round(float(v), 4) for v in err_fc],
           "sse_analysis_per_basin": [round(float(v), 4) for v in err_an],
           "basins_improved": int((err_fc < err_open).sum()),
           "status_nonzero_share": float((status != 0).double().mean()),
           "status_2_or_3": int((status >= 2).sum()), "mean_spread": float(kf["spread"][SPIN:].mean())}
    if 0 < horizon < T - SPIN:
        head, gen = run(T - horizon)
        z = torch.randn((particles, horizon, B), generator=gen).to(device)
        pm = torch.exp(prcp_sigma * z - 0.5 * prcp_sigma ** 2).contiguous() if prcp_sigma > 0 else None
        fc = hydrodl2_amd.ensemble_forecast(model, {"x_phy": x_open[T - horizon:].contiguous()},
                                            params[T - horizon:].contiguous(), head["state"],
                                            quantiles=(0.05, 0.5, 0.95), prcp_mul=pm)
        lo, hi = fc["quantiles"][0], fc["quantiles"][2]
        future = truth[T - horizon:]
        out.update(horizon=horizon, band_coverage=float(((future >= lo) & (future <= hi)).double().mean()),
                   quantiles_ordered=bool(((fc["quantiles"][0] <= fc["quantiles"][1]) &
                                           (fc["quantiles"][1] <= fc["quantiles"][2])).all()),
                   sse_forecast_median=float(((fc["quantiles"][1] - future).double() ** 2).sum()),
                   sse_open_loop_horizon=float(((open_loop - truth)[T - horizon:].double() ** 2).sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--basins", type=int, default=8)
    ap.add_argument("--days", type=int, default=150)
    ap.add_argument("--nmul", type=int, default=4)
    ap.add_argument("--particles", type=int, default=64)
    ap.add_argument("--window", type=int, default=1)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--method", choices=("sqrt", "perturbed"), default="sqrt")
    ap.add_argument("--prcp-sigma", type=float, default=0.4)
    ap.add_argument("--state-add-sigma", type=float, default=50.0)
    ap.add_argument("--inflation", type=float, default=1.05)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--check", action="store_true",
                    help="exit 1 unless the forecast's and the analysis' squared errors are below the open loop's")
    a = ap.parse_args()
    out = twin_experiment(a.basins, a.days, a.nmul, a.particles, a.window, a.seed, a.method, a.prcp_sigma,
                          a.state_add_sigma, a.inflation, a.horizon)
    print(json.dumps(out))
    if a.check and not (out["sse_forecast"] < out["sse_open_loop"] and out["sse_analysis"] < out["sse_open_loop"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
