"""CPU tier: oracle/hbv_restate64.py, the float64 restatement of Hbv, Hbv_1_1p, Hbv_2 and Hbv_2_hourly, against the
fixtures the reference itself produced -- outputs, storages and reverse-mode gradients of every golden case of those models
(tests/golden/<case>.npz, at helpers.compare's committed tolerances) and the output tangents of the 22 forward-mode
fixtures (tests/golden/jvp_<case>.npz, at the tolerances of tests/test_jvp_gpu.py (a)).  Once pinned here, the
restatement is the float64 yardstick of tests/test_jvp_f64_gpu.py and, for the hourly model, of tests/test_hourly_f64.py
and tests/test_hourly_f64_gpu.py."""
import os

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from . import golden_cases as gc
from . import golden_jvp as gj
from . import restate_util as ru
from .helpers import GOLDEN_DIR, compare, load_golden
from .test_jvp_gpu import BFI_ATOL_REL, TAN_FLOOR, _assert_tangent_close

# every golden case of the three daily models (hbv_cache_states included: two calls, storages carried across; the
# three that start wet, with storages loaded into a cache_states module) and of
# the hourly model (the five dry ones and the three that start wet under storm forcing)
DAILY = [n for n, s in gc.CASES.items() if s["model"] in ("Hbv", "Hbv_1_1p", "Hbv_2")]
HOURLY = [n for n, s in gc.CASES.items() if s["model"] == "Hbv_2_hourly"]
CASES = DAILY + HOURLY


def test_scope():
    """The restatement's scope is every Hbv / Hbv_1_1p / Hbv_2 / Hbv_2_hourly fixture, and every forward-mode fixture."""
    assert len(DAILY) == 36 and len(HOURLY) == 8 and set(gj.JVP_CASES) <= set(DAILY)
    assert len(CASES) == len(gc.CASES)


# Elements where the float64 restatement and the reference's float32 run part for a reason of precision alone, each
# with its float64 evidence.  They are left out of the float64 comparison, bounded below, and these cases are also
# compared whole in float32, where the restatement reproduces the reference within the committed tolerances.
#  * hbv11p_long_dyn_all, member 4 of basin 4: on day 157 PERC = min(SUZ, parPERC) ties.  float64: SUZ 8.23424176,
#    parPERC 8.23424182 (SUZ below by 6e-8, so PERC = SUZ); the reference's float32 SUZ is 8.2342758, 3.4e-5 above its
#    parPERC after 157 days of rounding, so PERC = parPERC.  The gradient then follows the other one-sided slope through
#    SUZ: the 14 parameter columns of that member on days 53-157 differ (up to 14.3 against 5.9); nothing else does.
#  * Hbv_2's SNOWPACK series on the day a snowpack melts out: SP = SP + snow - melt leaves 0.17-0.78 of a 15-43 mm
#    pack, so the float32 rounding of the pack (5e-6 of it after 180 days of increments) becomes 2.5e-4 of the result.
#    float64 against the fixture: hbv2_long_routing (day 180) 0.171422 vs 0.171379 (pack 42.79), hbv2_long_dyn3
#    (day 187) 0.460176 vs 0.460056 (pack 21.69), hbv2_long_static_cold (day 184) 0.783688 vs 0.783583 (pack 15.51);
#    the next day both are 0.  Bound: 1e-5 x the member's largest SNOWPACK.
#  * the wet hourly fixtures, the same thing on a groundwater box in the last hour before it runs empty (the next
#    hour both sides are 0 to within 4e-9): the box held 32-113 mm, float32 carries 1e-5 .. 7e-5 mm of rounding, and
#    the last 0.04-0.3 mm are off by that.  float64 against the fixture: hourly_wet_routing SLZ hour 85 0.0352950 vs
#    0.0352803 (box 71.96) and hour 101 0.2545896 vs 0.2545463 (48.19); hourly_wet_muwts SUZ hours 159 / 188 / 199
#    0.0846214 vs 0.0846471 (45.58), 0.2950842 vs 0.2950192 (113.49), 0.0558768 vs 0.0558525 (32.23).  Same bound:
#    1e-5 x the member's largest value of that storage.  (hourly_wet_dyn3_drop has no such element.)
#  * hbv_wet_dyn3, d loss / d P of day 76 on basin 3 (P = 0): on day 75 evaporation takes all of member 1's soil moisture
#    (AET = SM < PET * ef) and SM is set to its floor, nearzero = 1e-5.  On day 76 no rain falls and PET * ef is 1.5e-16 mm (FC 61.8, LP 0.226, BETAET 2.68):
#    in float64 SM - AET is below the floor by that much, the floor acts again and stops the gradient; in float32
#    1e-5 - 1.5e-16 is 1e-5, the floor does not act and the gradient passes.  float64 -0.0926111, the reference and the
#    float32 restatement -0.1782486: the two one-sided values of a clamp met exactly at its corner.  Nothing else differs.
#    Bound ("jump", ...): the jump of the float64 value across the corner, |-0.0926111 - (-0.1782486)| = 0.0856375, the
#    other side taken from the float32 restatement run.
PRECISION_ONLY = {
    "hbv_wet_dyn3": [("grad/x_phy", (76, 3, 0), ("jump", 0.0856375))],
    "hbv11p_long_dyn_all": [("grad/parameters", (slice(None), 4, slice(4, 14 * 16, 16)), None)],
    "hbv2_long_routing": [("states", (0, 180, 5, 2), 1e-5)],
    "hbv2_long_dyn3": [("states", (0, 187, 5, 10), 1e-5)],
    "hbv2_long_static_cold": [("states", (0, 184, 3, 5), 1e-5)],
    "hourly_wet_routing": [("states", (4, 85, 2, 1), 1e-5), ("states", (4, 101, 7, 0), 1e-5)],
    "hourly_wet_muwts": [("states", (3, 159, 2, 0), 1e-5), ("states", (3, 188, 5, 0), 1e-5),
                         ("states", (3, 199, 0, 0), 1e-5)],
}


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference(name):
    res = ru.case_reverse(name)
    ref = load_golden(name)
    missing = [k for k in ref.files if k not in ("torch_version", "loss") and k not in res]
    assert not missing, missing
    if name in PRECISION_ONLY:
        res = dict(res)
        for key, idx, bound in PRECISION_ONLY[name]:
            got, want = res[key][idx], ref[key][idx]
            if isinstance(bound, tuple):       # a tie: within the jump of the float64 value across it
                assert abs(float(got) - float(want)) <= bound[1] * (1 + 1e-3), (name, got, want, bound)
            elif bound is not None:      # a storage element: within `bound` x the member's largest value of that storage
                scale = float(np.abs(ref[key][(idx[0], slice(None)) + tuple(idx[2:])]).max())
                assert abs(float(got) - float(want)) <= bound * scale, (name, got, want, scale)
            res[key] = res[key].copy()
            res[key][idx] = want       # the rest of the tensor is compared as usual
        compare(name, ru.case_reverse(name, torch.float32), ref)
    compare(name, res, ref)


@pytest.mark.parametrize("name", gj.JVP_CASES)
def test_restatement_tangents_match_reference(name):
    spec = gc.CASES[name]
    ref = np.load(os.path.join(GOLDEN_DIR, f"jvp_{name}.npz"))
    inp = gc.build_inputs(name)
    dirs = gj.directions(name, inp)
    masks = ru.masks_for(spec["model"], spec["config"], spec["B"], spec.get("torch_seed"))
    keys = gj.output_keys(name)
    with fwAD.dual_level():
        out, _, _ = ru.run_inputs(spec["model"], spec["config"], inp, masks, torch.float64, dirs=dirs)
        tan = ru.tangents(out, keys)
    top = max(float(np.abs(ref[f"tan/{k}"]).max()) for k in keys if k != "BFI")
    for k in keys:
        b = ref[f"tan/{k}"]
        if k == "BFI":
            _assert_tangent_close(f"restate-jvp:{name}:{k}", tan[k], b, atol_rel=BFI_ATOL_REL)
        else:
            m = float(np.abs(b).max())
            _assert_tangent_close(f"restate-jvp:{name}:{k}", tan[k], b, scale=m if m >= TAN_FLOOR * top else top)
