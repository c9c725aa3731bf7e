#!/usr/bin/env python3
"""Forward-mode AD of SeqLSTM along D directions: one batched call against D one-direction calls, the two
alternating call by call in one process (the protocol of tools/bench_jvp.py: warm-up per shape, every call between
two HIP events, median and range).  One JSON line per (shape, level, D):

    python tools/bench_lstm_jvp.py [dmg big] [--steps 7] [--warmup 2] [--directions 1 4 16 38] [--chain]

    dmg   T 730, B 100, H 256, I 256   (examples/train_dpl.py's defaults: 7 row tiles)
    big   T 730, B 671, H 256, I 256   (42 row tiles x 16 workgroups: one direction already fills the chip)

    level "abi"     the recurrence alone: hbvx_lstm_tangent_batch against D calls of hbvx_lstm_tangent on slices of
                    the same buffers (arming the slabs included on both sides)
    level "module"  SeqLSTM.jvp_batch (tangents on x) against D torch.autograd.forward_ad calls, one layer
    --chain         at dmg: Linear -> ReLU -> SeqLSTM -> Linear -> Hbv, 16 directions on the network's input
                    (examples/input_sensitivity.py) against 16 one-direction forward_ad chains

"spread" is (max - min) / median of an arm's samples; "faster_beyond_spread": the batch's slowest sample is below the
sequential arm's fastest.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

from hydrodl2_amd import _abi, lstm, ops  # noqa: E402
from hydrodl2_amd._lib import get_library  # noqa: E402

SHAPES = {"dmg": (730, 100, 256, 256), "big": (730, 671, 256, 256)}


def _alternating_ms(fns, steps, warmup):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for fn, out in zip(fns, ms):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
    return ms


def _report(tag, D, batch, seq):
    b, s = statistics.median(batch), statistics.median(seq)
    row = dict(tag)
    row.update({"D": D, "batch_ms_median": round(b, 3), "batch_ms_range": [round(min(batch), 3), round(max(batch), 3)],
                "batch_ms_per_direction": round(b / D, 3),
                "sequential_ms_median": round(s, 3), "sequential_ms_range": [round(min(seq), 3), round(max(seq), 3)],
                "sequential_ms_per_direction": round(s / D, 3),
                "batch_spread": round((max(batch) - min(batch)) / b, 3),
                "sequential_spread": round((max(seq) - min(seq)) / s, 3),
                "speedup": round(s / b, 2),
                "faster_beyond_spread": bool(max(batch) < min(seq)),
                "slower_beyond_spread": bool(min(batch) > max(seq))})
    print(json.dumps(row), flush=True)


def _abi_level(args, name, mod, x, D):
    lib = get_library()
    T, B, _ = x.shape
    H = mod.hidden_size
    with torch.no_grad():
        rec = lstm._primal(x, mod.weight_ih_l0, mod.weight_hh_l0, mod.bias_ih_l0, mod.bias_hh_l0, True, None, None)
    _, _, w_hh, gates, c_all, _, _, _, _ = rec
    gx_t = torch.randn(D, T, B, H, 4, device=x.device)
    h_t = torch.empty(D, T, B, H, device=x.device)
    c_t = torch.empty(D, B, H, device=x.device)
    r = _abi.LstmDesc(abi_version=_abi.LSTM_ABI_VERSION, T=T, B=B, H=H)
    nb, nb1 = lib.lstm_tangent_batch_workspace_bytes(r, D), lib.lstm_workspace_bytes(r)
    ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=x.device)
    ws1 = torch.empty((nb1 + 3) // 4, dtype=torch.float32, device=x.device)
    st = torch.cuda.current_stream().cuda_stream
    p = ops._ptr

    def batch():
        lib.lstm_tangent_batch(r, D, p(w_hh), p(gates), None, p(c_all), p(gx_t), None, None, p(h_t), p(c_t), p(ws), nb, st)

    def sequential():
        for d in range(D):
            lib.lstm_tangent(r, p(w_hh), p(gates), None, p(c_all), p(gx_t[d]), None, None, p(h_t[d]), p(c_t[d]),
                             p(ws1), nb1, st)

    ms = _alternating_ms([batch, sequential], args.steps, args.warmup)
    lib.lstm_check(r, p(ws), st)
    lib.lstm_check(r, p(ws1), st)
    tiles = (B + 15) // 16
    _report({"shape": name, "level": "abi", "T": T, "B": B, "H": H, "pairs": D * tiles}, D, *ms)


def _module_level(args, name, mod, x, D):
    T, B, I = x.shape
    x_t = torch.randn(D, T, B, I, device=x.device)

    def batch():
        mod.jvp_batch(x, tangents={"x": x_t}, max_directions=D)

    def sequential():
        for d in range(D):
            with torch.no_grad(), fwAD.dual_level():
                fwAD.unpack_dual(mod(fwAD.make_dual(x, x_t[d]))[0]).tangent

    ms = _alternating_ms([batch, sequential], args.steps, args.warmup)
    _report({"shape": name, "level": "module", "T": T, "B": B, "H": mod.hidden_size, "I": I}, D, *ms)


def _chain(args):
    import input_sensitivity as ins
    dev = torch.device("cuda:0")
    net, model, z, x = ins.setup(dev)
    D = 16
    z_t = torch.randn((D,) + tuple(z.shape), device=dev)

    def batch():
        ins.streamflow_tangents(net, model, z, x, z_t, max_directions=D)

    def sequential():
        for d in range(D):
            ins.streamflow_tangent_one(net, model, z, x, z_t[d])

    ms = _alternating_ms([batch, sequential], args.steps, args.warmup)
    _report({"shape": "dmg", "level": "chain", "T": z.shape[0], "B": z.shape[1], "H": net.lstm.hidden_size,
             "nmul": model.nmul}, D, *ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--directions", type=int, nargs="+", default=None)
    ap.add_argument("--levels", nargs="+", default=["abi", "module"], choices=["abi", "module"])
    ap.add_argument("--chain", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.shapes:
        T, B, I, H = SHAPES[name]
        torch.manual_seed(0)
        mod = lstm.SeqLSTM(I, H, check=False).to(dev)
        x = torch.randn(T, B, I, device=dev)
        for D in args.directions or ([1, 4, 16, 38] if name == "dmg" else [1, 4, 16]):
            if "abi" in args.levels:
                _abi_level(args, name, mod, x, D)
            torch.cuda.empty_cache()
            if "module" in args.levels:
                _module_level(args, name, mod, x, D)
            torch.cuda.empty_cache()
    if args.chain:
        _chain(args)


if __name__ == "__main__":
    main()
