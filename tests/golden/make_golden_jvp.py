#!/usr/bin/env python3
"""Generate the forward-mode fixtures tests/golden/jvp_<case>.npz by running the REFERENCE under
torch.autograd.forward_ad.

Runs only where a checkout of the reference is at hand (HYDRODL2_REFERENCE names its `src` directory, as for
make_golden.py).  Inputs are golden_cases.build_inputs(case); tangent directions are golden_jvp.directions(case):
synth.normalish on the streams golden_jvp.JVP_STREAMS lists (parameters 70, p_dyn 71, p_sta 72, x_phy 73,
muwts 74), none of which build_inputs uses.  Only the output tangents are stored ("tan/<flux key>").

    HYDRODL2_REFERENCE=<checkout>/src python tests/golden/make_golden_jvp.py            # all cases
    HYDRODL2_REFERENCE=<checkout>/src python tests/golden/make_golden_jvp.py hbv_ties   # one case
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import golden_cases as gc  # noqa: E402
from tests import golden_jvp as gj  # noqa: E402
from tests.golden.make_golden import _import_reference  # noqa: E402


def run_case(hydrodl2, name: str) -> dict:
    spec = gc.CASES[name]
    cls = hydrodl2.load_model(spec["model"].lower(), spec["model"])
    cfg = spec["config"]
    model = cls(None if cfg is None else dict(cfg), torch.device("cpu"))
    inp = gc.build_inputs(name)
    dirs = gj.directions(name, inp)
    rec = {"torch_version": np.array(torch.__version__)}
    if "torch_seed" in spec:
        torch.manual_seed(spec["torch_seed"])
    with fwAD.dual_level():
        def arg(k):
            t = torch.from_numpy(inp[k]).clone()
            return fwAD.make_dual(t, torch.from_numpy(dirs[k])) if k in dirs else t
        x_dict = {"x_phy": arg("x_phy")}
        if "muwts" in inp:
            x_dict["muwts"] = arg("muwts")
        if spec["model"] == "Hbv_2":
            x_dict["ac_all"] = torch.from_numpy(inp["ac_all"])
            x_dict["elev_all"] = torch.from_numpy(inp["elev_all"])
            params = (arg("p_dyn"), arg("p_sta"))
        else:
            params = arg("parameters")
        out = model(x_dict, params)
        for k in gj.output_keys(name):
            tan = fwAD.unpack_dual(out[k]).tangent
            rec[f"tan/{k}"] = (torch.zeros_like(out[k]) if tan is None else tan).detach().numpy().copy()
    return rec


def main(argv):
    hydrodl2 = _import_reference()
    names = argv or gj.JVP_CASES
    for name in names:
        rec = run_case(hydrodl2, name)
        path = os.path.join(HERE, f"jvp_{name}.npz")
        np.savez_compressed(path, **rec)
        print(f"{name}: {len(rec) - 1} tangents -> {os.path.basename(path)}")


if __name__ == "__main__":
    main(sys.argv[1:])
