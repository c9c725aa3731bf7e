#!/usr/bin/env python3
"""How does streamflow respond to each input channel of the parameter network?  Forward-mode AD through the whole
differentiable-parameter-learning chain of examples/train_dpl.py -- Linear -> ReLU -> SeqLSTM -> Linear -> Hbv -- with
one direction per input channel (forcings and static attributes; every basin and day perturbed at once), all
directions on ONE primal run:

    SeqLSTM.jvp_batch      the network's directions through hbvx_lstm_tangent_batch ((direction, row tile) pairs)
    hydrodl2_amd.jvp_batch  their image, a full-form [D,T,B,ny] parameter tangent, through the batched HBV kernels

    python examples/input_sensitivity.py [--basins 100] [--rho 365] [--warm-up 365] [--nmul 16] [--hidden 256] [--check]

Prints one JSON line per channel: the mean and the largest absolute streamflow response per unit of the (normalised)
channel, and the day of the largest basin-mean response.  --check compares two channels with the one-direction chain
under torch.autograd.forward_ad (one direction per pass through both models) and prints the largest difference
relative to the largest response.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import hydrodl2_amd  # noqa: E402
from train_dpl import ParamNet, synth  # noqa: E402

CHANNELS = ["prcp", "tmean", "pet"]


def streamflow_tangents(net, model, z, x, z_t, max_directions=16):
    """(streamflow [T',B,1], its tangents [D,T',B,1]) along the input directions z_t [D,T,B,n_in] of `net`
    (train_dpl.ParamNet on the fused LSTM) followed by `model`."""
    with torch.no_grad():
        pre = net.inp(z)
        (h, _), (h_t, _) = net.lstm.jvp_batch(torch.relu(pre), tangents={"x": (pre > 0) * (z_t @ net.inp.weight.T)},
                                              max_directions=max_directions)
        raw, raw_t = net.out(h), h_t @ net.out.weight.T                    # [T,B,ny], [D,T,B,ny]
        out, tan = hydrodl2_amd.jvp_batch(model, {"x_phy": x}, raw, {"parameters": raw_t}, keys=("streamflow",))
    return out["streamflow"], tan["streamflow"]


def streamflow_tangent_one(net, model, z, x, z_t):
    """The same along ONE direction z_t [T,B,n_in]: torch.autograd.forward_ad through both models."""
    with torch.no_grad(), fwAD.dual_level():
        q = model({"x_phy": x}, net(fwAD.make_dual(z, z_t)))["streamflow"]
        return fwAD.unpack_dual(q).tangent


def channel_directions(z):
    """[n_in, T, B, n_in]: direction c is one unit on input channel c, every basin and day."""
    n_in = z.shape[-1]
    z_t = torch.zeros((n_in,) + tuple(z.shape), device=z.device)
    for c in range(n_in):
        z_t[c, :, :, c] = 1.0
    return z_t


def setup(dev, basins=100, rho=365, warm_up=365, nmul=16, hidden=256, n_attr=8, seed=0):
    """(net, model, z, x): train_dpl.py's network (untrained, its seed), Hbv and synthetic data."""
    T = warm_up + rho
    cfg = {"nmul": nmul, "warm_up": warm_up, "dynamic_params": {"Hbv": ["parBETA", "parBETAET"]}}
    model = hydrodl2_amd.load_model("hbv", "Hbv")(cfg, dev)
    x, attrs = synth(T, basins, n_attr, dev, seed=seed)
    mean, std = x.mean((0, 1)), x.std((0, 1)) + 1e-6
    z = torch.cat([(x - mean) / std, attrs[None].expand(T, -1, -1)], -1).contiguous()
    torch.manual_seed(2)
    net = ParamNet(3 + n_attr, hidden, model.learnable_param_count, fused=True).to(dev)
    return net, model, z, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--basins", type=int, default=100)
    ap.add_argument("--rho", type=int, default=365)
    ap.add_argument("--warm-up", type=int, default=365)
    ap.add_argument("--nmul", type=int, default=16)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--max-directions", type=int, default=16)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    net, model, z, x = setup(dev, args.basins, args.rho, args.warm_up, args.nmul, args.hidden)
    z_t = channel_directions(z)
    q, q_t = streamflow_tangents(net, model, z, x, z_t, args.max_directions)
    names = CHANNELS + [f"attr{k}" for k in range(z.shape[-1] - len(CHANNELS))]
    for c, name in enumerate(names):
        s = q_t[c, :, :, 0]
        print(json.dumps({"channel": name, "mean_abs_dq": round(s.abs().mean().item(), 6),
                          "max_abs_dq": round(s.abs().max().item(), 6),
                          "day_of_largest_basin_mean": int(s.mean(1).abs().argmax().item()),
                          "mean_q": round(q.mean().item(), 6)}), flush=True)
    if args.check:
        for c in (0, z.shape[-1] - 1):
            one = streamflow_tangent_one(net, model, z, x, z_t[c])
            err = (one - q_t[c]).abs().max().item() / max(one.abs().max().item(), 1e-30)
            print(json.dumps({"check_channel": names[c], "max_diff_over_max_response": float(f"{err:.3g}")}), flush=True)


if __name__ == "__main__":
    main()
