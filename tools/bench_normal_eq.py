#!/usr/bin/env python3
"""Time the per-basin normal equations (hydrodl2_amd/calibrate.py, hbvx_gram in include/hbvx.h) against what a user can do
without them: `parameter_jacobian` followed by `torch.einsum('tbc,tbe->bce', J * w, J)` in float32.

    python tools/bench_normal_eq.py --steps 10 --warmup 3 [--days 7300] [--basins 671] [--nmul 16] [--skip-models]

Two comparisons, each W warm-up + K timed calls between two HIP events, the variants alternating call by call, median
[min, max] (the protocol of tools/bench_jvp.py); one JSON line per variant.

1. The reduction alone, on random series [C,T,B] with C = 12 * nmul + 2 (all static columns of Hbv / HbvAdj):
   `hbvx_gram` on the direction-major series against the einsum on the permuted copy J [T,B,C] (the copy is made once,
   outside the timed window: the torch side is given its preferred input for free; a second variant pays the permute).
   Achieved FLOP/s and bytes/s of the kernel count what the algorithm needs: C (C + 1) / 2 + C + 1 multiply-adds per
   (day, basin) -- one triangle, the right-hand side, the cost -- and one read of the series, weights and residuals
   plus one write of the outputs.
2. The whole call: `normal_equations` against `parameter_jacobian` + the two einsums + the cost, for Hbv with every
   parameter static and for HbvAdj at its benchmark configuration (parBETAET dynamic), both 671 x 16 x 7300.
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


def line(base, variant, r, **kw):
    med, lo, hi = r
    print(json.dumps(dict(base, variant=variant, ms_median=round(med, 3), ms_range=[round(lo, 3), round(hi, 3)], **kw)),
          flush=True)


def _lib_path():
    from hydrodl2_amd import _lib
    return _lib.LIB_PATH


def bench_reduction(args, dev):
    from hydrodl2_amd import ops
    T, B, C = args.days, args.basins, 12 * args.nmul + 2
    gen = torch.Generator(device=dev).manual_seed(7)
    s = torch.randn((C, T, B), generator=gen, device=dev)
    w = torch.rand((T, B), generator=gen, device=dev)
    r = torch.randn((T, B), generator=gen, device=dev)
    J = s.permute(1, 2, 0).contiguous()                      # what parameter_jacobian hands out

    def gram():
        ops.gram(s, w, r)

    def gram_only():
        ops.gram(s, w, None)

    def torch_on_J():
        Jw = J * w.unsqueeze(-1)
        torch.einsum('tbc,tbe->bce', Jw, J)
        torch.einsum('tbc,tb->bc', Jw, r)
        (w * r * r).sum(0)

    def torch_with_permute():
        Jp = s.permute(1, 2, 0).contiguous()
        Jw = Jp * w.unsqueeze(-1)
        torch.einsum('tbc,tbe->bce', Jw, Jp)
        torch.einsum('tbc,tb->bc', Jw, r)
        (w * r * r).sum(0)

    # same numbers (float32 sums in two different orders: compare against the size of the sum, not bit for bit)
    got = ops.gram(s, w, r)
    Jw = J * w.unsqueeze(-1)
    want = torch.einsum('tbc,tbe->bce', Jw, J)
    scale = torch.einsum('tbc,tbe->bce', Jw.abs(), J.abs())
    worst = float(((got[0] - want).abs() / scale).max())
    del Jw, want, scale, got
    res = _alternating_ms([gram, gram_only, torch_on_J, torch_with_permute], args.steps, args.warmup)
    base = {"part": "reduction", "T": T, "B": B, "C": C, "lib": os.path.basename(_lib_path())}
    macs = T * B * (C * (C + 1) // 2 + C + 1)
    nbytes = 4 * (C * T * B + 2 * T * B + B * C * C + B * C + B)
    k = res[0][0] * 1e-3
    line(base, "hbvx_gram (gram, rhs, cost)", res[0], tflops=round(2 * macs / k / 1e12, 2), tbytes_per_s=round(nbytes / k / 1e12, 3),
         worst_diff_over_sum_of_magnitudes=worst)
    line(base, "hbvx_gram (gram only)", res[1])
    line(base, "torch: J*w, einsum x2, cost, on the permuted copy", res[2], over_hbvx_gram=round(res[2][0] / res[0][0], 2))
    line(base, "torch: the same with the permute inside", res[3], over_hbvx_gram=round(res[3][0] / res[0][0], 2))


def bench_models(args, dev):
    import hydrodl2_amd
    from hydrodl2_amd import ops
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    T, B, M = args.days, args.basins, args.nmul
    x_dict = {"x_phy": torch.from_numpy(synth.forcing(T, B, 92)).to(dev)}
    gen = torch.Generator(device=dev).manual_seed(4)
    cases = [("Hbv", ("hbv", "Hbv"), {"nmul": M, "dynamic_params": {"Hbv": []}}, "streamflow"),
             ("HbvAdj", ("hbv_adj", "HbvAdj"), {"nmul": M, "dynamic_params": {"HbvAdj": ["parBETAET"]}}, "flow_sim")]
    for name, fam, cfg, key in cases:
        model = hydrodl2_amd.load_model(*fam)(cfg, dev)
        p = torch.randn((T, B, model.learnable_param_count), generator=gen, device=dev)
        with torch.no_grad():
            target = model(x_dict, p)[key][..., 0] * 1.1 + 0.05
        w = torch.rand((T, B), generator=gen, device=dev)

        def neq():
            with torch.no_grad():
                hydrodl2_amd.normal_equations(model, x_dict, p, target, weights=w)

        def jacobian_then_torch():
            with torch.no_grad():
                if name == "HbvAdj":
                    Jd = model.parameter_jacobian(x_dict, p)
                else:
                    Jd = hydrodl2_amd.parameter_jacobian(model, x_dict, p, keys=(key,))
                J = Jd[key]
                r = model(x_dict, p)[key][..., 0] - target       # parameter_jacobian does not hand out its primal
                Jw = J * w.unsqueeze(-1)
                torch.einsum('tbc,tbe->bce', Jw, J)
                torch.einsum('tbc,tb->bc', Jw, r)
                (w * r * r).sum(0)

        res = _alternating_ms([neq, jacobian_then_torch], args.steps, args.warmup)
        C = len(hydrodl2_amd.sensitivity.jacobian_columns(model, None)[1])
        base = {"part": "whole call", "model": name, "T": T, "B": B, "M": M, "C": C}
        line(base, "normal_equations", res[0])
        line(base, "parameter_jacobian + torch", res[1], over_normal_equations=round(res[1][0] / res[0][0], 2))
        ops.KERNEL_EVENTS = []
        neq()
        torch.cuda.synchronize()
        calls = {}
        for n, e0, e1 in ops.KERNEL_EVENTS:
            calls[n] = round(calls.get(n, 0.0) + e0.elapsed_time(e1), 3)
        ops.KERNEL_EVENTS = None
        print(json.dumps(dict(base, variant="normal_equations library calls (ms, summed per entry point)", calls_ms=calls)),
              flush=True)
        del model, p, target, w
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--days", type=int, default=7300)
    ap.add_argument("--basins", type=int, default=671)
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
    if not args.skip_reduction:
        bench_reduction(args, dev)
        torch.cuda.empty_cache()
    if not args.skip_models:
        bench_models(args, dev)


if __name__ == "__main__":
    main()
