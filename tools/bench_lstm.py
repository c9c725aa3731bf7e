#!/usr/bin/env python3
"""Sequence LSTM: hydrodl2_amd.lstm.SeqLSTM (include/hbvx_lstm.h) beside torch.nn.LSTM (MIOpen) on the
same weights and input, forward and forward+backward, at the delta-MG shape by default.

    python tools/bench_lstm.py [T B I H] [--state] [--jvp]

--state: also SeqLSTM with a carried initial state (h0, c0 requiring grad, the loss on out, h_n and c_n), next
to the zero-state call, on the same weights and input.
--jvp: forward + JVP (torch.autograd.forward_ad, one direction on x: hbvx_lstm_tangent behind the forward) against
the forward alone, at B and at 5 B, and the tangent kernel's own time.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from hydrodl2_amd import ops  # noqa: E402
from hydrodl2_amd.lstm import SeqLSTM  # noqa: E402


def timed(fn, steps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
    T, B, I, H = (nums + [730, 100, 256, 256])[:4] if len(nums) < 4 else nums[:4]
    steps = 20
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    fused = SeqLSTM(I, H).to(dev)
    ref = torch.nn.LSTM(I, H).to(dev)
    ref.load_state_dict(fused.state_dict())
    x = torch.randn(T, B, I, device=dev, requires_grad=True)
    gh = torch.randn(T, B, H, device=dev)

    def fwd(m):
        with torch.no_grad():
            return m(x)[0]

    def fwdbwd(m):
        for p in m.parameters():
            p.grad = None
        x.grad = None
        (m(x)[0] * gh).sum().backward()

    res = {"T": T, "B": B, "I": I, "H": H}
    for name, m in (("fused", fused), ("torch", ref)):
        res[f"{name}_fwd_ms"] = round(timed(lambda: fwd(m), steps), 3)
        res[f"{name}_fwdbwd_ms"] = round(timed(lambda: fwdbwd(m), steps), 3)
    if "--state" in sys.argv:
        h0 = (0.5 * torch.randn(1, B, H, device=dev)).requires_grad_(True)
        c0 = torch.randn(1, B, H, device=dev).requires_grad_(True)
        g2, g3 = torch.randn(1, B, H, device=dev), torch.randn(1, B, H, device=dev)

        def fwd_state():
            with torch.no_grad():
                return fused(x, (h0, c0))[0]

        def fwdbwd_state():
            for t in [x, h0, c0] + list(fused.parameters()):
                t.grad = None
            out, (hn, cn) = fused(x, (h0, c0))
            ((out * gh).sum() + (hn * g2).sum() + (cn * g3).sum()).backward()

        # alternated with the zero-state call, so that both see the same state of the box
        for _ in range(2):
            for key, fn in (("fused_fwd_ms", lambda: fwd(fused)), ("fused_state_fwd_ms", fwd_state),
                            ("fused_fwdbwd_ms", lambda: fwdbwd(fused)), ("fused_state_fwdbwd_ms", fwdbwd_state)):
                res.setdefault(key + "_runs", []).append(round(timed(fn, steps), 3))
        for key in ("fused_fwd_ms", "fused_state_fwd_ms", "fused_fwdbwd_ms", "fused_state_fwdbwd_ms"):
            res[key] = min(res[key + "_runs"])
        res["state_fwdbwd_over_zero_state"] = round(res["fused_state_fwdbwd_ms"] / res["fused_fwdbwd_ms"], 4)
    if "--jvp" in sys.argv:
        import torch.autograd.forward_ad as fwAD
        for Bj in (B, 5 * B):
            xj = torch.randn(T, Bj, I, device=dev)
            tj = torch.randn_like(xj)

            def fwd_only():
                with torch.no_grad():
                    return fused(xj)[0]

            def fwd_jvp():
                with torch.no_grad(), fwAD.dual_level():
                    return fwAD.unpack_dual(fused(fwAD.make_dual(xj, tj))[0]).tangent

            runs = {"fwd": [], "fwd_jvp": []}
            for _ in range(2):          # alternated, so that both see the same state of the box
                runs["fwd"].append(round(timed(fwd_only, steps), 3))
                runs["fwd_jvp"].append(round(timed(fwd_jvp, steps), 3))
            ops.KERNEL_EVENTS = []
            for _ in range(steps):
                fwd_jvp()
            torch.cuda.synchronize()
            ev, ops.KERNEL_EVENTS = ops.KERNEL_EVENTS, None
            r = {"B": Bj, "fwd_ms": min(runs["fwd"]), "fwd_jvp_ms": min(runs["fwd_jvp"]), "runs": runs}
            for n in ("hbvx_lstm_forward", "hbvx_lstm_tangent"):
                r[n + "_ms"] = round(sum(a.elapsed_time(b) for k, a, b in ev if k == n) / steps, 3)
            r["fwd_jvp_over_fwd"] = round(r["fwd_jvp_ms"] / r["fwd_ms"], 4)
            res.setdefault("jvp", []).append(r)
    ops.KERNEL_EVENTS = []
    for _ in range(steps):
        fwdbwd(fused)
    torch.cuda.synchronize()
    ev, ops.KERNEL_EVENTS = ops.KERNEL_EVENTS, None
    for n in ("hbvx_lstm_forward", "hbvx_lstm_backward"):
        ms = sum(a.elapsed_time(b) for k, a, b in ev if k == n) / steps
        res[n + "_ms"] = round(ms, 3)
        res[n + "_us_per_step"] = round(ms * 1e3 / T, 2)
    # what bounds the recurrence kernels: MFMA work and hand-off traffic per launch against the chip's peaks
    tiles = (B + 15) // 16
    flops = 2.0 * T * tiles * 16 * H * 4 * H                   # padded rows; forward = backward
    res["mfma"] = {d: {"tflops": round(flops / (res[f"hbvx_lstm_{d}_ms"] * 1e-3) / 1e12, 2),
                       "frac_of_fp32_mfma_peak": round(flops / (res[f"hbvx_lstm_{d}_ms"] * 1e-3) / 157.3e12, 4)}
                   for d in ("forward", "backward")}
    wgs = H // 16
    xch = {"forward": T * tiles * wgs * H * 16 * 4, "backward": T * tiles * wgs * H * 16 * 4 * 4}
    res["hand_off_load_TBps"] = {d: round(xch[d] / (res[f"hbvx_lstm_{d}_ms"] * 1e-3) / 1e12, 3) for d in xch}
    res["hbm_algorithmic_GB"] = {"forward": round(T * B * H * 4 * (4 + 4 + 1 + 1) / 1e9, 3),
                                 "backward": round(T * B * H * 4 * (4 + 4 + 2 + 1) / 1e9, 3)}
    err = (fwd(fused) - fwd(ref)).abs().max().item()
    res["max_abs_diff_vs_torch"] = err
    print(json.dumps(res))


if __name__ == "__main__":
    main()
