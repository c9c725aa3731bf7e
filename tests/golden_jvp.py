"""Forward-mode (JVP) cases shared by tests/golden/make_golden_jvp.py and tests/test_jvp_gpu.py.

A case is a golden case of golden_cases.CASES (same model, config and inputs) plus one tangent direction.  The
directions are synth.normalish arrays on stream ids that golden_cases.build_inputs does not use (it draws uniform
streams 1-15 and normalish streams 3 and 20-37), so a direction is bit-reproducible anywhere:

    JVP_STREAMS   parameters 70, p_dyn 71, p_sta 72, x_phy 73, muwts 74

Directions go on the parameters (both tuple members for Hbv_2), on x_phy for the *_xgrad cases and on muwts for
the *_muwts* cases.  The fixtures tests/golden/jvp_<case>.npz hold the reference's output tangents only.
"""
from __future__ import annotations

import numpy as np

from . import golden_cases as gc
from . import synth

JVP_STREAMS = {"parameters": 70, "p_dyn": 71, "p_sta": 72, "x_phy": 73, "muwts": 74}

JVP_CASES = [
    "cfg1_hbv_default", "hbv_static_m16", "hbv_warmup_states", "hbv_warmup_nostates", "hbv_dyn2", "hbv_dyn2_drop",
    "hbv_m3_xgrad", "hbv_muwts", "hbv_muwts_warmup", "hbv_comprout_m1", "hbv_ties", "hbv_variables",
    "hbv11p_dyn_all", "hbv11p_static", "hbv2_dyn3", "hbv2_dyn3_routing", "hbv2_static", "hbv_long_static",
    "hbv_long_dyn2", "hbv_long_ties", "hbv2_long_routing", "hbv2_long_static_cold",
]


def directions(name: str, inp: dict) -> dict:
    """Input name -> tangent array (float32, shaped like inp[name]) of JVP case `name`."""
    spec = gc.CASES[name]
    seed = spec["seed"]
    keys = ["p_dyn", "p_sta"] if spec["model"] == "Hbv_2" else ["parameters"]
    if spec.get("x_grad"):
        keys.append("x_phy")
    if spec.get("muwts"):
        keys.append("muwts")
    return {k: synth.normalish(inp[k].shape, seed, JVP_STREAMS[k]) for k in keys if inp[k].size}


def output_keys(name: str):
    """The output tangents a fixture holds: every flux key (BFI included)."""
    return gc.flux_keys(gc.CASES[name]["model"])
