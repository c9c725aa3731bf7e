#!/usr/bin/env python3
"""Time the predictive variance (hydrodl2_amd/uncertainty.py, hbvx_quadform in include/hbvx.h) against what a user can
do without it: the permuted Jacobian, a `bmm` against the factor, a square-sum.

    python tools/bench_quadform.py --steps 10 --warmup 3 [--shapes 671x7300,100x730] [--nmul 16] [--skip-models]

Two comparisons, each W warm-up + K timed calls between two HIP events, the variants alternating call by call, median
[min, max] (the protocol of tools/bench_jvp.py and tools/bench_normal_eq.py); one JSON line per variant.

1. The reduction alone, on random series [C,T,B] with C = 12 * nmul + 2 and a random lower-triangular factor [B,C,C]:
   `ops.quadform` on the direction-major series against
       Y = bmm(J.transpose(0, 1), factor.transpose(1, 2));  var = (Y * Y).sum(-1).T
   on the permuted copy J [T,B,C] -- once with the copy made outside the timed window (the torch side is given its
   preferred input for free), once with the permute inside.  Peak memory of each variant is what the caching allocator
   held at most ON TOP of the inputs it was given (the series and the factor; for the torch-on-J variant also J, which
   is counted separately as `input_gib`).  The kernel's multiply-adds: C (C + 1) / 2 + C per (day, basin).
2. The whole call: `predictive_variance` against `parameter_jacobian` + that route, for Hbv with every parameter
   static, with the peak memory of both.
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

GIB = float(1 << 30)


def line(base, variant, r, **kw):
    med, lo, hi = r
    print(json.dumps(dict(base, variant=variant, ms_median=round(med, 3), ms_range=[round(lo, 3), round(hi, 3)], **kw)),
          flush=True)


def peak_over_inputs(fn):
    """GiB the allocator held at most during one call of fn, over what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / GIB, 3)


def torch_route(J, factor):
    """J [T,B,C] -> var [T,B] as a user forms it today."""
    Y = torch.bmm(J.transpose(0, 1), factor.transpose(1, 2))        # [B,T,C]
    return (Y * Y).sum(-1).transpose(0, 1)


def bench_reduction(T, B, C, args, dev):
    from hydrodl2_amd import ops
    gen = torch.Generator(device=dev).manual_seed(7)
    s = torch.randn((C, T, B), generator=gen, device=dev)
    factor = torch.tril(torch.randn((B, C, C), generator=gen, device=dev)) / C ** 0.5
    base = {"part": "reduction", "T": T, "B": B, "C": C, "series_gib": round(s.numel() * 4 / GIB, 3)}

    def quadform():
        return ops.quadform(s, factor)

    def torch_with_permute():
        return torch_route(s.permute(1, 2, 0).contiguous(), factor)

    peaks = {"quadform": peak_over_inputs(quadform), "permute_inside": peak_over_inputs(torch_with_permute)}
    J = s.permute(1, 2, 0).contiguous()                              # what parameter_jacobian hands out

    def torch_on_J():
        return torch_route(J, factor)

    peaks["on_J"] = peak_over_inputs(torch_on_J)
    # same numbers (float32 sums in two different orders: compare against the size of the sum, not bit for bit)
    got, want = quadform(), torch_on_J()
    mag = torch.bmm(J.transpose(0, 1).abs(), factor.transpose(1, 2).abs()).square().sum(-1).transpose(0, 1)
    worst = float(((got - want).abs() / mag).max())
    del got, want, mag
    torch.cuda.empty_cache()
    res = _alternating_ms([quadform, torch_on_J, torch_with_permute], args.steps, args.warmup)
    macs = T * B * (C * (C + 1) // 2 + C)
    k = res[0][0] * 1e-3
    line(base, "hbvx_quadform", res[0], tflops=round(2 * macs / k / 1e12, 2), peak_gib_over_inputs=peaks["quadform"],
         worst_diff_over_sum_of_magnitudes=worst)
    line(base, "torch: bmm + square-sum on the permuted copy", res[1], over_hbvx_quadform=round(res[1][0] / res[0][0], 2),
         peak_gib_over_inputs=peaks["on_J"], input_gib=round(J.numel() * 4 / GIB, 3))
    line(base, "torch: the same with the permute inside", res[2], over_hbvx_quadform=round(res[2][0] / res[0][0], 2),
         peak_gib_over_inputs=peaks["permute_inside"])


def bench_model(T, B, M, args, dev):
    import hydrodl2_amd
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    x_dict = {"x_phy": torch.from_numpy(synth.forcing(T, B, 92)).to(dev)}
    gen = torch.Generator(device=dev).manual_seed(4)
    model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "dynamic_params": {"Hbv": []}}, dev)
    p = torch.randn((T, B, model.learnable_param_count), generator=gen, device=dev)
    C = len(hydrodl2_amd.sensitivity.jacobian_columns(model, None)[1])
    factor = torch.tril(torch.randn((B, C, C), generator=gen, device=dev)) / C ** 0.5

    def pv():
        with torch.no_grad():
            return hydrodl2_amd.predictive_variance(model, x_dict, p, factor)["var"]

    def jacobian_then_torch():
        with torch.no_grad():
            return torch_route(hydrodl2_amd.parameter_jacobian(model, x_dict, p, keys=("streamflow",))["streamflow"], factor)

    peaks = [peak_over_inputs(pv), peak_over_inputs(jacobian_then_torch)]
    res = _alternating_ms([pv, jacobian_then_torch], args.steps, args.warmup)
    base = {"part": "whole call", "model": "Hbv", "T": T, "B": B, "M": M, "C": C,
            "series_gib": round(C * T * B * 4 / GIB, 3)}
    line(base, "predictive_variance", res[0], peak_gib_over_inputs=peaks[0])
    line(base, "parameter_jacobian + bmm + square-sum", res[1], over_predictive_variance=round(res[1][0] / res[0][0], 2),
         peak_gib_over_inputs=peaks[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="671x7300,100x730", help="comma-separated BASINSxDAYS")
    ap.add_argument("--nmul", type=int, default=16)
    ap.add_argument("--skip-models", action="store_true")
    ap.add_argument("--skip-reduction", action="store_true")
    ap.add_argument("--lib", default=None, help="time a whole-library A/B variant (python __graft_entry__.py variant <tag> ...)")
    args = ap.parse_args()
    if args.lib:
        from hydrodl2_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(","):
        B, T = (int(n) for n in shape.split("x"))
        if not args.skip_reduction:
            bench_reduction(T, B, 12 * args.nmul + 2, args, dev)
            torch.cuda.empty_cache()
        if not args.skip_models:
            bench_model(T, B, args.nmul, args, dev)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
