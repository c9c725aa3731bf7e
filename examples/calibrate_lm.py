#!/usr/bin/env python3
"""Twin experiment for the per-basin Levenberg-Marquardt calibration (hydrodl2_amd.calibrate).

    python examples/calibrate_lm.py [--basins 32] [--days 730] [--warm-up 0] [--nmul 1] [--iters 8] [--perturb 0.3]
                                    [--names parBETA parFC parK1] [--missing 0.1]

"Observations" come from the physics itself with a hidden static parameter field (as in examples/train_dpl.py), the
calibration starts from that field moved by `--perturb` in raw space, and every basin runs its own LM on the named
static parameters: one `normal_equations` call (one primal run, the one-hot directions through the tangent kernels,
hbvx_gram) and one trial forward per iteration.  A fraction `--missing` of the observations is NaN, as gauge records
are.  Prints the summed cost per iteration for Hbv and for HbvAdj.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import hydrodl2_amd  # noqa: E402
from hydrodl2_amd.sensitivity import jacobian_columns  # noqa: E402


def forcings(T, B, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    day = torch.arange(T, device=dev, dtype=torch.float32)[:, None]
    season = torch.sin(2 * torch.pi * day / 365.0)
    P = torch.clamp((torch.rand((T, B), generator=g, device=dev) - 0.7) * 60.0, min=0.0)
    Tm = 10 * season + 5 * torch.randn((T, B), generator=g, device=dev) + torch.rand((1, B), generator=g, device=dev) * 25 - 10
    PET = torch.clamp(3 + 2.5 * season, min=0).expand(T, B)
    return torch.stack([P, Tm, PET], -1).contiguous(), g


def twin(kind, args, dev):
    fam, key = (("hbv", "Hbv"), "streamflow") if kind == "Hbv" else (("hbv_adj", "HbvAdj"), "flow_sim")
    model = hydrodl2_amd.load_model(*fam)({"nmul": args.nmul, "warm_up": args.warm_up, "dynamic_params": {kind: []}}, dev)
    T, B = args.days + args.warm_up, args.basins
    x, g = forcings(T, B, dev, seed=0)
    xd = {"x_phy": x}
    truth = torch.randn((T, B, model.learnable_param_count), generator=g, device=dev)
    truth[:] = truth[-1]                                            # a static field: every row the same
    with torch.no_grad():
        obs = model(xd, truth)[key][..., 0].clone()
    if args.missing > 0:
        obs[torch.rand(obs.shape, generator=g, device=dev) < args.missing] = float("nan")
    _, cols = jacobian_columns(model, args.names)
    start = truth.clone()
    start[..., cols] += args.perturb * torch.sign(torch.randn((B, len(cols)), generator=g, device=dev))
    fitted, hist = hydrodl2_amd.calibrate(model, xd, start, obs, names=args.names, n_iter=args.iters)
    print(f"{kind}: {B} basins x {args.nmul} members x {args.days} days, {len(cols)} columns {args.names}")
    for i, c in enumerate(hist["cost"]):
        acc = "" if i == 0 else f"   accepted {int(hist['accepted'][i - 1].sum()):4d} / {B}"
        print(f"  iteration {i:2d}: summed cost {float(c.sum()):.6g}{acc}")
    err0 = (start[-1][:, cols] - truth[-1][:, cols]).abs().mean()
    err1 = (fitted[-1][:, cols] - truth[-1][:, cols]).abs().mean()
    print(f"  mean |raw parameter error| {float(err0):.3f} -> {float(err1):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--basins", type=int, default=32)
    ap.add_argument("--days", type=int, default=730)
    ap.add_argument("--warm-up", type=int, default=0)
    ap.add_argument("--nmul", type=int, default=1)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--perturb", type=float, default=0.3)
    ap.add_argument("--missing", type=float, default=0.1)
    ap.add_argument("--names", nargs="+", default=["parBETA", "parFC", "parK1"])
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    dev = torch.device(args.device)
    for kind in ("Hbv", "HbvAdj"):
        twin(kind, args, dev)


if __name__ == "__main__":
    main()
