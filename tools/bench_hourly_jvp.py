#!/usr/bin/env python3
"""Time Hbv_2_hourly.jvp_batch (forward-mode AD to 'Qs' and gage 'streamflow', D directions on one primal run) against
the module's plain forward and forward + backward at the same shape -- the protocol of tools/bench_jvp.py: W warm-up +
K timed calls, each between two HIP events, median, the variants alternating call by call.  One JSON line per variant:

    python tools/bench_hourly_jvp.py --steps 10 --warmup 3 [--directions 1 4 16] [--kernels]

The shape is the one DESIGN.md quotes for the gage routing: 4 000 units, 100 gages, 12 000 (gage, unit) pairs, 2 160
hours, nmul 4, every parameter static.  Directions: every input at once (p_sta, p_distr, x_phy).  --kernels adds the
time of each library call inside one jvp_batch of the largest D (HIP events around the calls, ops.KERNEL_EVENTS).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from bench_jvp import _alternating_ms  # noqa: E402

U, G, PER_GAGE, T, M = 4000, 100, 120, 2160, 4


def _inputs(dev):
    g = torch.Generator(device="cpu").manual_seed(7)
    topo = torch.zeros((G, U))
    for k in range(G):
        topo[k, torch.randperm(U, generator=g)[:PER_GAGE]] = 1.0
    x = torch.rand((T, U, 3), generator=g) * torch.tensor([1.5, 30.0, 0.25])
    x[..., 1] -= 10.0
    x_dict = {"x_phy": x, "ac_all": torch.rand(U, generator=g) * 5000.0, "elev_all": torch.rand(U, generator=g) * 3000.0,
              "outlet_topo": topo, "areas": torch.rand(U, generator=g) * 100.0 + 1.0}
    params = (torch.zeros((T, U, 0)), torch.rand((U, 19 * M), generator=g), torch.rand((G * PER_GAGE, 3), generator=g))
    return {k: v.to(dev) for k, v in x_dict.items()}, tuple(p.to(dev) for p in params)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--directions", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    import hydrodl2_amd
    from hydrodl2_amd import ops
    dev = torch.device("cuda:0")
    model = hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")({"nmul": M, "dynamic_params": {"Hbv_2_hourly": []}}, dev)
    x_dict, params = _inputs(dev)
    gen = torch.Generator(device=dev).manual_seed(8)

    def plain():
        with torch.no_grad():
            model(x_dict, params)

    leaves = tuple(p.clone().requires_grad_(True) for p in params)

    def fwd_bwd():
        out = model(x_dict, leaves)
        (out["streamflow"].sum() + out["Qs"].sum()).backward()
        for p in leaves:
            p.grad = None

    def jvp(tan):
        def f():
            with torch.no_grad():
                model.jvp_batch(x_dict, params, tan)
        return f

    tans = {D: {"p_sta": torch.randn((D,) + tuple(params[1].shape), device=dev, generator=gen) * 0.1,
                "p_distr": torch.randn((D,) + tuple(params[2].shape), device=dev, generator=gen) * 0.1,
                "x_phy": torch.randn((D,) + tuple(x_dict["x_phy"].shape), device=dev, generator=gen) * 0.05}
            for D in args.directions}
    fns = [plain, fwd_bwd] + [jvp(tans[D]) for D in args.directions]
    res = _alternating_ms(fns, args.steps, args.warmup)
    base = {"units": U, "gages": G, "pairs": G * PER_GAGE, "T": T, "M": M}
    (f_med, f_lo, f_hi), (b_med, b_lo, b_hi) = res[0], res[1]
    print(json.dumps(dict(base, variant="forward", ms_median=round(f_med, 3), ms_range=[round(f_lo, 3), round(f_hi, 3)])),
          flush=True)
    print(json.dumps(dict(base, variant="forward+backward", ms_median=round(b_med, 3),
                          ms_range=[round(b_lo, 3), round(b_hi, 3)])), flush=True)
    for D, (med, lo, hi) in zip(args.directions, res[2:]):
        print(json.dumps(dict(base, variant="jvp_batch", D=D, ms_median=round(med, 3), ms_range=[round(lo, 3), round(hi, 3)],
                              ms_per_direction=round((med - f_med) / D, 3), over_forward=round(med / f_med, 2),
                              over_forward_backward=round(med / b_med, 2))), flush=True)
    if args.kernels:
        D = max(args.directions)
        ops.KERNEL_EVENTS = []
        jvp(tans[D])()
        torch.cuda.synchronize()
        calls = [(name, round(e0.elapsed_time(e1), 3)) for name, e0, e1 in ops.KERNEL_EVENTS]
        ops.KERNEL_EVENTS = None
        print(json.dumps(dict(base, variant="jvp_batch calls", D=D, calls_ms=calls)), flush=True)


if __name__ == "__main__":
    main()
