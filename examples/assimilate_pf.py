#!/usr/bin/env python3
"""A twin experiment for the particle filter: does assimilating streamflow pull a model with wrong storages and biased
rain towards the truth?

    truth       the model from WET carried-in storages on the record's precipitation; the observations are its routed
                streamflow plus fixed-seed Gaussian noise with a standard deviation of 5 % of the basin's mean flow
    open loop   the same parameters from the DRY default storages (0.001 mm) on 0.7 x the precipitation: what a user has
                who knows neither the storages nor the rain
    filter      `particle_filter` on the open loop's inputs: 64 particles, one-day windows (hbvx_population_ensemble: one
                launch per day for all particles), log-normal precipitation noise sigma 0.4, log-normal noise sigma 0.5 on
                the start storages, obs_sigma the observation noise's own, one seed

    python examples/assimilate_pf.py [--basins 8] [--days 150] [--nmul 4] [--particles 64] [--window 1] [--seed 5]
                                     [--prcp-sigma 0.4] [--state-sigma 0.5] [--horizon 30] [--check]

Prints one JSON line: the squared error against the TRUTH (not the observations) of the open loop and of the filtered mean
flow over days 30 .. end, summed and per basin, the mean effective sample size, the share of windows that resampled, and
-- from a second filter run that stops `--horizon` days before the end, followed by `ensemble_forecast` with the same
precipitation noise over those days -- the share of the truth's flows inside the forecast's 5 % .. 95 % band.
--check exits 1 unless the filter's summed squared error is below the open loop's.  One seed: this is one draw.
Synthetic forcings (tests/synth.py).
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

SPIN = 30       # days left out of the comparison: the filter starts as dry as the open loop


def twin_setup(basins=8, days=150, nmul=4, device="cuda:0"):
    """The truth, the observations and the open loop above (fixed seeds) -> a dictionary; examples/assimilate_enkf.py
    runs its filter on the same set-up."""
    T, B, M = days, basins, nmul
    cfg = {"nmul": M, "routing": True, "dynamic_params": {"Hbv": []}, "warm_up": 0}
    load = hydrodl2_amd.load_model("hbv", "Hbv")
    truth_model, model = load(dict(cfg, cache_states=True), device), load(dict(cfg), device)
    x = torch.from_numpy(synth.forcing(T, B, seed=201, day0=120.0)).to(device)
    # one row for every day: a shorter record (the forecast's head and horizon) then has the same static parameters
    params = torch.from_numpy(synth.raw_parameters(1, B, model.learnable_param_count, seed=202)).to(device)
    params = params.expand(T, -1, -1).contiguous()
    truth_model.load_states(tuple(torch.from_numpy(synth.wet_states(B, M, 203)).to(device).unbind(0)))
    with torch.no_grad():
        truth = truth_model({"x_phy": x}, params)["streamflow"][..., 0].clone()
    g = torch.Generator().manual_seed(204)
    sigma = 0.05 * truth.mean(0)                                                    # [B]
    obs = truth + sigma * torch.randn(truth.shape, generator=g).to(device)
    x_open = x.clone()
    x_open[..., 0] = x_open[..., 0] * 0.7
    with torch.no_grad():
        open_loop = model({"x_phy": x_open}, params)["streamflow"][..., 0].clone()
    return {"model": model, "x_open": x_open, "params": params, "truth": truth, "obs": obs, "sigma": sigma,
            "open_loop": open_loop}


def twin_experiment(basins=8, days=150, nmul=4, particles=64, window=1, seed=5, prcp_sigma=0.4, state_sigma=0.5,
                    horizon=30, device="cuda:0"):
    """The experiment above -> a dictionary of plain numbers and lists."""
    T, B, M = days, basins, nmul
    su = twin_setup(basins, days, nmul, device)
    model, x_open, params, truth, obs, sigma, open_loop = (su[k] for k in ("model", "x_open", "params", "truth", "obs",
                                                                           "sigma", "open_loop"))

    def run(T_run):
        gen = torch.Generator().manual_seed(seed)
        return hydrodl2_amd.particle_filter(model, {"x_phy": x_open[:T_run].contiguous()}, params[:T_run].contiguous(),
                                            obs[:T_run], particles, window, obs_sigma=sigma, prcp_sigma=prcp_sigma,
                                            state_sigma=state_sigma, generator=gen), gen

    pf, _ = run(T)
    err_open = ((open_loop - truth)[SPIN:].double() ** 2).sum(0)
    err_pf = ((pf["mean"] - truth.double())[SPIN:] ** 2).sum(0)
    out = {"basins": B, "days": T, "nmul": M, "particles": particles, "window": window, "seed": seed,
           "sse_open_loop": float(err_open.sum()), "sse_filter": float(err_pf.sum()),
           "sse_open_loop_per_basin": [round(float(v), 4) for v in err_open],
           "sse_filter_per_basin": [round(float(v), 4) for v in err_pf],
           "basins_improved": int((err_pf < err_open).sum()), "mean_ess": float(pf["ess"].mean()),
           "resampled_share": float(pf["resampled"].double().mean()), "degenerate_windows": int(pf["degenerate"].sum())}
    if 0 < horizon < T - SPIN:
        head, gen = run(T - horizon)
        P = particles
        z = torch.randn((P, horizon, B), generator=gen).to(device)
        pm = torch.exp(prcp_sigma * z - 0.5 * prcp_sigma ** 2).contiguous() if prcp_sigma > 0 else None
        fc = hydrodl2_amd.ensemble_forecast(model, {"x_phy": x_open[T - horizon:].contiguous()}, params[T - horizon:].contiguous(),
                                            head["state"], quantiles=(0.05, 0.5, 0.95), prcp_mul=pm)
        lo, hi = fc["quantiles"][0], fc["quantiles"][2]
        future = truth[T - horizon:]
        out.update(horizon=horizon, band_coverage=float(((future >= lo) & (future <= hi)).double().mean()),
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
    ap.add_argument("--prcp-sigma", type=float, default=0.4)
    ap.add_argument("--state-sigma", type=float, default=0.5)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--check", action="store_true", help="exit 1 unless the filter's squared error is below the open loop's")
    a = ap.parse_args()
    out = twin_experiment(a.basins, a.days, a.nmul, a.particles, a.window, a.seed, a.prcp_sigma, a.state_sigma, a.horizon)
    print(json.dumps(out))
    if a.check and not out["sse_filter"] < out["sse_open_loop"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
