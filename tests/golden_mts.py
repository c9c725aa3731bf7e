"""Multi-timescale golden cases (Hbv_2_mts): inputs, configs and the runner shared by
tests/golden/make_golden_mts.py (reference side), tests/test_mts.py (this package) and the
float64 problem set tests/mts_sets.py.  Every function takes a case name or a spec dict of the
same keys."""
from __future__ import annotations

import numpy as np
import torch

from . import synth

DYN = ["parBETA", "parK0", "parBETAET"]
DYN_HIGH_F4 = ["parF0", "parALPHA", "parFMIN", "parBETA"]
M = 4
N_LOW, N_HIGH = 16, 19
# the wet recipe: a spring start (day 60), daily precipitation x 4, then hourly storm forcing that continues the
# calendar; the daily model starts from its default storages, so the wetness of the hand-off comes from the forcing
WET = dict(day0=60.0, prcp_scale=4.0, storm=6.0)

CASES = {
    # all units fit one block, training mode: only the unit runoff 'Qs' is produced
    # (hbv_2_mts.py:193-195 switches the gage routing off).
    "mts_train": dict(T_low=40, T_high=96, B=7, G=3, seed=41, simulate=False,
                      chunks=dict(train_spatial_chunk_size=16, simulate_spatial_chunk_size=3,
                                  simulate_temporal_chunk_size=40, train_warmup=24)),
    # simulate mode: 3 spatial blocks of <= 3 units, routing in temporal chunks of 40 h with a
    # 24 h overlap.  On the reference this path needs the alias described in make_golden_mts.py.
    "mts_chunked": dict(T_low=30, T_high=120, B=7, G=3, seed=42, simulate=True,
                        chunks=dict(train_spatial_chunk_size=16, simulate_spatial_chunk_size=3,
                                    simulate_temporal_chunk_size=40, train_warmup=24)),
    # a wet record with DIFFERING dynamic lists on the daily and the hourly side: the positional hand-off
    # (hbv_2_mts.py:310-331) is no longer "daily block, then the tail of the hourly block"
    "mts_wet_lists": dict(T_low=150, T_high=130, B=7, G=3, seed=43, simulate=False, wet=WET,
                          low_dyn=DYN, high_dyn=DYN_HIGH_F4,
                          chunks=dict(train_spatial_chunk_size=16, simulate_spatial_chunk_size=3,
                                      simulate_temporal_chunk_size=40, train_warmup=24)),
}


def spec_of(case) -> dict:
    return CASES[case] if isinstance(case, str) else case


def dyn_lists(case):
    """(daily, hourly) dynamic-parameter lists of a case, in config order."""
    spec = spec_of(case)
    return list(spec.get("low_dyn", DYN)), list(spec.get("high_dyn", DYN))


def configs(case):
    spec = spec_of(case)
    m = spec.get("M", M)
    dl, dh = dyn_lists(spec)
    low = {"nmul": m, "dynamic_params": {"Hbv_2": dl}, "cache_states": True}
    high = {"nmul": m, "dynamic_params": {"Hbv_2_hourly": dh}}
    high.update(spec["chunks"])
    return low, high


def build_inputs(case) -> dict:
    spec = spec_of(case)
    Tl, Th, B, G, seed = spec["T_low"], spec["T_high"], spec["B"], spec["G"], spec["seed"]
    m = spec.get("M", M)
    dl, dh = dyn_lists(spec)
    out = {}
    wet = spec.get("wet")
    if wet:
        out["x_low"] = (synth.forcing(Tl, B, seed, day0=wet["day0"])
                        * np.array([wet["prcp_scale"], 1.0, 1.0], np.float32))
        out["x_high"] = synth.forcing_hourly(Th, B, seed + 1000, storm=wet["storm"], day0=wet["day0"] + Tl)
    else:
        out["x_low"] = synth.forcing(Tl, B, seed)
        out["x_high"] = (synth.forcing(Th, B, seed + 1000)
                         * np.array([1.0 / 8.0, 1.0, 1.0 / 24.0], np.float32))
    out["low_dyn"] = synth.unit_parameters((Tl, B, len(dl) * m), seed, 4)
    out["low_sta"] = synth.unit_parameters((B, (N_LOW - len(dl)) * m), seed, 6)
    out["high_dyn"] = synth.unit_parameters((Th, B, len(dh) * m), seed, 16)
    out["high_sta"] = synth.unit_parameters((B, (N_HIGH - len(dh)) * m), seed, 17)
    out["ac_all"] = (synth.uniform((B,), seed, 7) * np.float32(5000.0)).astype(np.float32)
    out["elev_all"] = (synth.uniform((B,), seed, 8) * np.float32(3000.0)).astype(np.float32)
    topo = (synth.uniform((G, B), seed, 13) < np.float32(0.45)).astype(np.float32)
    topo[np.arange(B) % G, np.arange(B)] = 1.0
    out["outlet_topo"] = topo
    out["areas"] = (synth.uniform((B,), seed, 14) * np.float32(90.0) + np.float32(5.0)).astype(np.float32)
    out["p_distr"] = synth.unit_parameters((int(topo.sum()), 3), seed, 15)
    return out


LEAVES = ["low_dyn", "low_sta", "high_dyn", "high_sta", "p_distr"]


def run(model, case, dev) -> dict:
    """Forward + backward of a case through `model` (reference or this package) with the inputs on `dev` (the
    model may compute elsewhere: the loss is formed where the outputs are)."""
    spec = spec_of(case)
    inp = build_inputs(spec)
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    for k in LEAVES:
        t[k].requires_grad_(True)
    model.set_mode(spec["simulate"])
    x_dict = {"x_phy_low_freq": t["x_low"], "x_phy_high_freq": t["x_high"], "ac_all": t["ac_all"],
              "elev_all": t["elev_all"], "outlet_topo": t["outlet_topo"], "areas": t["areas"]}
    params = ([t["low_dyn"], t["low_sta"]], [t["high_dyn"], t["high_sta"], t["p_distr"]])
    out = model(x_dict, params)
    res = {f"out/{k}": v.detach().cpu().numpy().copy() for k, v in out.items()}
    loss = 0.0
    for i, (k, v) in enumerate(sorted(out.items())):
        w = torch.from_numpy(synth.loss_weights(tuple(v.shape), spec["seed"], 50 + i)).to(v.device)
        loss = loss + (w * v).sum()
    loss.backward()
    for k in LEAVES:
        g = t[k].grad if t[k].grad is not None else torch.zeros_like(t[k])
        assert g.device == t[k].device, (k, g.device, t[k].device)
        res[f"grad/{k}"] = g.detach().cpu().numpy().copy()
    return res
