#!/usr/bin/env python3
"""Time HbvAdj.jvp_batch (implicit-function forward-mode AD of 'flow_sim', D directions on one primal run) against the
same directions as one-direction calls and against the module's plain forward and forward + backward at the same
shape -- the protocol of tools/bench_jvp.py: W warm-up + K timed calls, each between two HIP events, median, the variants
alternating call by call.  One JSON line per variant:

    python tools/bench_adj_jvp.py --steps 10 --warmup 3 [--directions 1 4 16 64] [--kernels] [--lib libhbvx_<tag>.so]

The shape is BASELINE config 4: 671 basins x 16 members x 7300 days, parBETAET dynamic.  Directions: dense on the last
row of `parameters` (compact form, the per-basin Jacobian's: a full-form direction is 4.1 GB at this shape, 64 of them
do not fit the card) and dense on all of `x_phy`.  "D x 1": the D directions as D one-direction tangent calls on ONE
recorded primal run, so the comparison is between the tangent launches alone (a primal per call would only widen it);
every `jvp_batch` figure contains its one primal run, and "tangent only" is the same call without it.  --kernels adds the time of each library
call inside one jvp_batch of the largest D.  --lib: time a whole-library A/B variant (`python __graft_entry__.py variant
<tag> -DADJ_TAN_G=2 ...`) in place of the built library.
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

B, M, T = 671, 16, 7300


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--directions", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--days", type=int, default=T)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    import hydrodl2_amd
    from hydrodl2_amd import _lib, adj_jvp, ops
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    dev = torch.device("cuda:0")
    model = hydrodl2_amd.load_model("hbv_adj", "HbvAdj")({"nmul": M, "dynamic_params": {"HbvAdj": ["parBETAET"]}}, dev)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    days = args.days
    ny = 13 * M + 2
    x_dict = {"x_phy": torch.from_numpy(synth.forcing(days, B, 92)).to(dev)}
    gen = torch.Generator(device=dev).manual_seed(4)
    p = torch.randn((days, B, ny), generator=gen, device=dev)
    Dmax = max(args.directions)
    tan = {"parameters": torch.randn((Dmax, B, ny), generator=gen, device=dev) * 0.1,
           "x_phy": torch.randn((Dmax, days, B, 3), generator=gen, device=dev) * 0.05}     # D = 64: 3.8 GB

    def first(D):
        return {k: t[:D] for k, t in tan.items()}

    def plain():
        with torch.no_grad():
            model(x_dict, p)

    leaf = p.clone().requires_grad_(True)

    def fwd_bwd():
        model(x_dict, leaf)["flow_sim"].sum().backward()
        leaf.grad = None

    def jvp(D):
        def f():
            with torch.no_grad():
                model.jvp_batch(x_dict, p, first(D))
        return f

    with torch.no_grad(), ops.record_paths() as records:
        model(x_dict, p)

    def tangent_only(D, per_call):
        def f():
            with torch.no_grad():
                adj_jvp._directional(model, records, first(D), per_call)
        return f

    fns = [plain, fwd_bwd]
    for D in args.directions:
        fns += [jvp(D), tangent_only(D, D), tangent_only(D, 1)]
    res = _alternating_ms(fns, args.steps, args.warmup)
    base = {"basins": B, "M": M, "T": days, "lib": os.path.basename(_lib.LIB_PATH)}

    def line(variant, r, **kw):
        med, lo, hi = r
        print(json.dumps(dict(base, variant=variant, ms_median=round(med, 3), ms_range=[round(lo, 3), round(hi, 3)], **kw)),
              flush=True)

    line("forward", res[0])
    line("forward+backward", res[1])
    f_med = res[0][0]
    for k, D in enumerate(args.directions):
        whole, batched, singly = res[2 + 3 * k: 5 + 3 * k]
        line("jvp_batch", whole, D=D, ms_per_direction=round((whole[0] - f_med) / D, 3),
             over_forward_backward=round(whole[0] / res[1][0], 2))
        line("tangent only, one call", batched, D=D)
        line("tangent only, D x 1", singly, D=D, batched_over_singly=round(batched[0] / singly[0], 3))
    if args.kernels:
        ops.KERNEL_EVENTS = []
        jvp(Dmax)()
        torch.cuda.synchronize()
        calls = [(name, round(e0.elapsed_time(e1), 3)) for name, e0, e1 in ops.KERNEL_EVENTS]
        ops.KERNEL_EVENTS = None
        print(json.dumps(dict(base, variant="jvp_batch calls", D=Dmax, calls_ms=calls)), flush=True)


if __name__ == "__main__":
    main()
