"""CPU tier: what tests/test_daily_jvp_abi_gpu.py holds the daily tangent kernels to -- float64 forward AD of the
restatement (tests/daily_jvp_util.py::abi_forward_ad) on the problems of daily_jvp_util.TAN_PROBLEMS -- checked without
a GPU.

(1) The reference alone stays within the protocol.  Float32 forward AD of the restatement stands in for the kernel
    and goes through hourly_jvp_util.compare against float64, itself being the float32 evaluation: every element
    outside tolerance is admitted, so what is asserted is hourly_sets.ADMIT_CAP on flux, state_out and routed of
    every problem.  This is why three problems are taken at seed 9 (daily_jvp_util.SEED9).
(2) The list takes every branch of daily_sets.events_of(model) at COVER_MIN, in the float64 run.
(3) The float64 forward-AD tangent of wet64-m64 (one basin, 64 members) against the central difference of the float64
    restatement along the same direction, step 1e-6, at 1e-5 of each array's largest tangent, on the lane-days whose
    branch events are the same at both ends of the difference (a lane is left out from its first differing day on;
    a basin's flux rows and routed rows from the first such day of any of its lanes; at most 1 % of the lane-days).
    The direction's components on inputs that are exactly 0 are zeroed first: precipitation on the 70 % of dry days,
    the snowpack and meltwater carried in on the snow-free half of the lanes, the lower zone of the dry lanes.  There
    the model sits exactly on a corner (rain = P [T >= TT] with P = 0, tosoil = max(MELTWATER - CWH SNOWPACK, 0) with
    both 0), a central difference across a corner is the mean of two slopes, and forward AD gives one of them: with the
    whole direction the events differ in every lane from day 0 or 1 on (`rain` in 69 % of the lane-days, `tosoil` in
    55 %) and nothing is left to compare.  This pins the helper; it is no test of the kernels.

Elements of the float32 restatement outside tolerance against float64 (= admitted; cap 2e-3 of the array), measured
by (1); the 30 problems not listed have none in any array:

problem                       flux          state_out   routed
Hbv wet400                    2 / 74800     0           -
Hbv wet400-d3                 2 / 74800     0           -
Hbv wet129-muwts (seed 9)     2 / 95073     0           0
Hbv_1_1p wet400-all-drop      1 / 81600     0           -
Hbv_1_1p wet400-list          6 / 81600     0           1 / 27200
Hbv_2 wet400                  13 / 81600    0           -
Hbv_2 wet400-muwts            13 / 81600    0           -
The largest share is 1.6e-4 (Hbv_2 wet400, flux).  The largest float64 tangent of a problem is 4.3 (Hbv dry15) to 686
(Hbv wet1460): nothing is trivially zero.

(3) measured: no lane-day left out in any model; worst |finite difference - forward AD| / max|tangent| 1.1e-8 (Hbv
flux), 2.3e-9 (Hbv_1_1p flux; routed 8.1e-9), 1.1e-9 (Hbv_2 flux); state_out 2.0e-9 to 3.2e-9.

float64 forward AD on 8 host threads: 0.0 to 3.3 s per problem (wet1460); the module 76 s alone (its coverage runs,
float64 forward + backward, are shared with tests/test_daily_f64.py in a whole run).
"""
import time

import numpy as np
import pytest
import torch

from . import daily_jvp_util as du
from . import daily_sets as ds
from . import hourly_jvp_util as hu
from . import restate_util as ru
from .test_daily_f64 import f64_run

_F64 = {}


def f64_tangents(model, name):
    """Float64 forward AD of a problem of TAN_PROBLEMS, computed once per session."""
    if (model, name) not in _F64:
        prob, dirs = du.problem(model, name)
        t = time.time()
        _F64[model, name] = du.abi_forward_ad(prob, dirs)
        print(f"{model} {name}: float64 forward AD {time.time() - t:.1f} s on {torch.get_num_threads()} threads")
    return _F64[model, name]


@pytest.mark.parametrize("model,name", du.ALL, ids=du.IDS)
def test_reference_alone_stays_within_the_cap(model, name):
    prob, dirs = du.problem(model, name)
    want = f64_tangents(model, name)
    f32 = du.abi_forward_ad(prob, dirs, torch.float32)
    print(f"{model} {name}: largest float64 tangent {max(float(np.abs(want[k]).max()) for k in ('flux', 'state_out')):.3g}")
    for k in ("flux", "state_out", "routed"):
        if k in want:
            hu.compare(f"restate32-tan {model} {name} {k}", f32[k], want[k], f32[k], axis=0)
    assert float(np.abs(want["flux"]).max()) > 0 and float(np.abs(want["state_out"]).max()) > 0


@pytest.mark.parametrize("model", ds.MODELS)
def test_the_listed_problems_take_the_branches(model):
    rows = {}
    for name, (kw, seed) in du.TAN_PROBLEMS[model].items():
        if seed == 7:
            rows[name] = f64_run(model, name)[2]
        else:
            ev = {}
            ru.abi_daily(ds.make(model, kw, seed), torch.float64, events=ev)
            rows[f"{name} (seed {seed})"] = ds.coverage(ev)
    ds.assert_covered(model, rows, f"{model} tangent problems")


@pytest.mark.parametrize("model", ds.MODELS)
def test_float64_forward_ad_against_its_finite_difference(model):
    name, h = "wet64-m64", 1e-6
    prob, dirs = du.problem(model, name)
    # the direction's components on inputs that are exactly 0 are left out (module docstring): there the model sits on
    # a corner, and a central difference across a corner is the mean of two slopes, which no tangent is
    dirs = dict(dirs, x=dirs["x"] * (prob["x"] != 0), state_in=dirs["state_in"] * (prob["state_in"] != 0))
    tan = du.abi_forward_ad(prob, dirs)
    evp, evm = {}, {}
    up, dn = du.abi_values(prob, dirs, h, evp), du.abi_values(prob, dirs, -h, evm)
    differ = torch.zeros_like(evp["Q0"], dtype=torch.bool)                  # [T,B,M]
    for k in evp:
        if evp[k].dtype == torch.bool:
            differ |= evp[k] != evm[k]
    out = (differ.cumsum(0) > 0).numpy()                                    # a lane from its first differing day on
    share = float(out.mean())
    day_out = out.any(-1)                                                   # [T,B]
    keep = {"flux": ~day_out[None], "routed": ~day_out[None], "state_out": ~out[-1][None]}
    worst = {}
    for k in ("flux", "state_out", "routed"):
        if k in tan:
            fd = (up[k] - dn[k]) / (2 * h)
            err = np.abs(fd - tan[k]) * np.broadcast_to(keep[k], tan[k].shape)
            worst[k] = float(err.max() / np.abs(tan[k]).max())
    print(f"{model} {name}: {int(out.sum())} of {out.size} lane-days left out ({share:.2%}); "
          f"worst |finite difference - forward AD| / max|tangent|: " + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))
    assert share <= 0.01, share
    assert all(v <= 1e-5 for v in worst.values()), worst
