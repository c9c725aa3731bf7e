#!/usr/bin/env python3
"""Twin experiment for the first-order uncertainty of a calibration (hydrodl2_amd.uncertainty).

    python examples/calibrate_uncertainty.py [--basins 32] [--days 730] [--later-days 365] [--nmul 1] [--iters 8]
                                             [--perturb 0.3] [--noise 0.2] [--names parBETA parFC parK1]

"Observations" of a first period come from the physics itself with a hidden static parameter row, plus Gaussian noise
of known standard deviation `--noise`.  Every basin runs its own Levenberg-Marquardt fit (`calibrate`); at the result
one `normal_equations` call gives the information matrix, `parameter_covariance` its inverse scaled by the estimated
residual variance, and `predictive_variance` carries that covariance to the simulated series of a LATER period (other
forcings, the fitted parameters): one primal run, the one-hot directions through the tangent kernels, one
hbvx_quadform call.  Printed: the estimated against the true noise variance, the standard deviation of every fitted
column, the largest correlations, and the share of the later period's noise-free truth that lies inside the simulated
series +- 2 sqrt(var).  Numbers only; nothing is asserted.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import hydrodl2_amd  # noqa: E402
from hydrodl2_amd.sensitivity import jacobian_columns  # noqa: E402


def forcings(T, B, dev, g):
    day = torch.arange(T, device=dev, dtype=torch.float32)[:, None]
    season = torch.sin(2 * torch.pi * day / 365.0)
    P = torch.clamp((torch.rand((T, B), generator=g, device=dev) - 0.7) * 60.0, min=0.0)
    Tm = 10 * season + 5 * torch.randn((T, B), generator=g, device=dev) + torch.rand((1, B), generator=g, device=dev) * 25 - 10
    PET = torch.clamp(3 + 2.5 * season, min=0).expand(T, B)
    return torch.stack([P, Tm, PET], -1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--basins", type=int, default=32)
    ap.add_argument("--days", type=int, default=730)
    ap.add_argument("--later-days", type=int, default=365)
    ap.add_argument("--nmul", type=int, default=1)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--perturb", type=float, default=0.3)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--names", nargs="+", default=["parBETA", "parFC", "parK1"])
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    dev = torch.device(args.device)
    key, B, T1, T2 = "streamflow", args.basins, args.days, args.later_days
    model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": args.nmul, "warm_up": 0, "dynamic_params": {"Hbv": []}}, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    x1, x2 = {"x_phy": forcings(T1, B, dev, g)}, {"x_phy": forcings(T2, B, dev, g)}
    row = torch.randn((B, model.learnable_param_count), generator=g, device=dev)       # the hidden static row
    with torch.no_grad():
        clean1 = model(x1, row.expand(T1, B, -1).contiguous())[key][..., 0].clone()
        clean2 = model(x2, row.expand(T2, B, -1).contiguous())[key][..., 0].clone()
    obs = clean1 + args.noise * torch.randn(clean1.shape, generator=g, device=dev)
    _, cols = jacobian_columns(model, args.names)
    start = row.expand(T1, B, -1).clone()
    start[..., cols] += args.perturb * torch.sign(torch.randn((B, len(cols)), generator=g, device=dev))

    fitted, hist = hydrodl2_amd.calibrate(model, x1, start, obs, names=args.names, n_iter=args.iters)
    print(f"Hbv: {B} basins x {args.nmul} members, fitted on {T1} days, {len(cols)} columns {args.names}")
    print(f"  summed cost {float(hist['cost'][0].sum()):.6g} -> {float(hist['cost'][-1].sum()):.6g}")

    neq = hydrodl2_amd.normal_equations(model, x1, fitted, obs, names=args.names)
    cov = hydrodl2_amd.parameter_covariance(neq)
    ok = ~cov["failed"]
    print(f"  basins without a covariance (not positive definite, or too few observations): {int((~ok).sum())}")
    print(f"  residual variance, median over basins: {float(cov['sigma2'][ok].median()):.4g} (true {args.noise ** 2:.4g})")
    err = (fitted[-1][:, cols] - row[:, cols]).abs().double()
    std = cov["std"]
    labels = [f"{n}[{m}]" for n in args.names for m in range(args.nmul)]
    for j, label in enumerate(labels):
        inside = float((err[ok, j] <= 2 * std[ok, j].to(err.device)).double().mean())
        print(f"  {label:12s} median std {float(std[ok, j].median()):.4g}   median |error| {float(err[ok, j].median()):.4g}"
              f"   |error| <= 2 std in {100 * inside:.0f} % of the basins")
    corr = cov["corr"][ok].abs().median(0).values
    pairs = sorted(((float(corr[i, j]), i, j) for i in range(len(cols)) for j in range(i)), reverse=True)[:3]
    for c, i, j in pairs:
        print(f"  median |corr| {labels[i]} ~ {labels[j]}: {c:.3f}")

    later = fitted[-1].expand(T2, B, -1).contiguous()
    pv = hydrodl2_amd.predictive_variance(model, x2, later, cov["factor"], names=args.names)
    sim, band = pv["outputs"][key][..., 0], 2 * torch.sqrt(pv["var"])
    okd = ok.to(sim.device)
    inside = ((sim - clean2).abs() <= band)[:, okd].double().mean()
    print(f"  later period, {T2} days: median band half-width {float(band[:, okd].median()):.4g}, "
          f"noise-free truth inside +- 2 sqrt(var) on {100 * float(inside):.1f} % of the basin-days")


if __name__ == "__main__":
    main()
