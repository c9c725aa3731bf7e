"""GPU tier: forward-mode AD of the drop-in modules on the three wet fixtures (hbv_wet_dyn3, hbv11p_wet_list_drop,
hbv2_wet_muwts_routing: cache_states, the storages of synth.wet_states loaded, tests/test_daily_f64.py counts their
branches) against forward AD of oracle/hbv_restate64.py in float64 (daily_jvp_util.module_forward_ad: duals on every
differentiable input and on the five loaded storages).

(e) hydrodl2_amd.sensitivity.jvp_batch along three directions over x_phy, the parameters, muwts and the loaded states
    (daily_jvp_util.module_directions, seeds 41-43): every output key under hourly_jvp_util.compare with the basins as
    the series and the case's largest tangent as the floor, BFI whole with the allowance of
    test_jvp_f64_gpu.BFI_TERM_REL x the basin's term size.  hbv_wet_dyn3, basin 3 from day 76 on and its BFI, is held
    to the restatement's FLOAT32 forward AD at the same tolerance (F32_HELD below).
(f) the same cases under torch.autograd.forward_ad with dual inputs and dual states (the one-direction kernels)
    against direction 0 of (e), by test_jvp_batch_gpu._compare_keys; whether the two are bit-identical goes to the
    parity report, as there.
(g) parameter_jacobian on hbv11p_wet_list_drop started from the loaded storages: the column of a static parameter
    against float64 forward AD along the matching one-hot direction, and -- parameter_jacobian refuses the name of a
    dynamic parameter -- the compact one-hot directions it would form for a column of parK0 and of parFC through
    jvp_batch: either column has kept basins (the direction moves day T-1 alone) and dropped ones (it moves every day).

Measured on the MI355X: no element of any key outside tolerance in (e) or (g), so nothing was admitted (in hbv_wet_dyn3
the kernels take the float32 restatement's side of the tie in basin 3); worst error / tolerance 0.36 (capillary of
hbv2_wet_muwts_routing, direction 2), BFI 0.006; (f) bit-identical on all three cases.  Float64 forward AD on the host:
0.3 to 2.0 s per case and direction; the module 6.1 s.
"""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from hydrodl2_amd.sensitivity import jvp_batch, one_hot_directions, parameter_jacobian

from . import daily_jvp_util as du
from . import golden_cases as gc
from . import golden_jvp as gj
from . import hourly_jvp_util as hu
from . import restate_util as ru
from .abi_util import REPORT
from .test_jvp_batch_gpu import _compare_keys
from .test_jvp_f64_gpu import BFI_TERM_REL
from .test_jvp_gpu import TAN_ATOL_REL, _assert_tangent_close, _inputs, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEEDS = (41, 42, 43)
# case -> (basin, first day) held to the float32 restatement instead of float64, the `bound None` rule of
# daily_sets.compare_case_f64.  hbv_wet_dyn3: the tie test_restate64.PRECISION_ONLY names for this fixture -- the floor
# of SM met exactly at its corner on day 75/76, basin 3, which float32 and float64 resolve differently.  In reverse
# mode it moves one element of grad/x_phy; in forward mode the other one-sided slope travels downstream: the float32
# restatement differs from float64 in basin 3 only, from day 77 on (seed 41: gwflow 60 of 1200 elements, AET_hydro 7,
# evapfactor 6, recharge 1, percolation 1, and BFI of basin 3; seeds 42 and 43: AET_hydro 5, evapfactor 5, recharge 1,
# percolation 1).  Every other basin and day goes against float64.
F32_HELD = {"hbv_wet_dyn3": (3, 76)}
_BATCH = {}
_WANT = {}


def _module(name):
    """A fresh module of the case as helpers.run_case prepares it: the storages loaded, the generator seeded."""
    model = _model(name, torch.device(DEV))
    model.load_states(tuple(torch.from_numpy(s.copy()).to(DEV) for s in gc.build_inputs(name)["states0"]))
    torch.manual_seed(gc.CASES[name].get("torch_seed", 0))
    return model


def _want(name, tag, dirs, dtype=torch.float64):
    if (name, tag, dtype) not in _WANT:
        _WANT[name, tag, dtype] = du.module_forward_ad(name, gc.build_inputs(name), dirs, dtype)
    return _WANT[name, tag, dtype]


def _batch(name):
    """jvp_batch of the case along the directions of SEEDS, run once per session: {key: [3, ...] float64 numpy}."""
    if name not in _BATCH:
        inp = gc.build_inputs(name)
        dirs = [du.module_directions(inp, s) for s in SEEDS]
        tangents = {("states" if k == "states0" else k): torch.from_numpy(np.stack([d[k] for d in dirs])).to(DEV)
                    for k in dirs[0]}
        _, x_dict, params = _inputs(name, DEV)
        _, tan = jvp_batch(_module(name), x_dict, params, tangents)
        _BATCH[name] = (dirs, {k: v.double().cpu().numpy() for k, v in tan.items()})
    return _BATCH[name]


def _compare_f64(label, name, got, tag, dirs):
    """{key: tangent} of the module against float64 forward AD along `dirs` under the protocol of (e)."""
    want = dict(_want(name, tag, dirs))
    terms = want.pop("bfi_terms")
    assert set(got) == set(want), (label, sorted(set(got) ^ set(want)))

    def f32():
        return _want(name, tag, dirs, torch.float32)
    if name in F32_HELD:
        b, t0 = F32_HELD[name]
        for k in want:
            want[k] = want[k].copy()
            if k == "BFI":
                want[k][b] = f32()[k][b]
            else:
                want[k][t0:, b] = f32()[k][t0:, b]
    top = max(float(np.abs(v).max()) for k, v in want.items() if k != "BFI")
    assert top > 0
    bad = []          # every key is compared before anything is raised
    for k, b in want.items():
        try:
            if k == "BFI":
                scale = max(float(np.abs(b).max()), 1e-30) + (BFI_TERM_REL / TAN_ATOL_REL) * terms
                _assert_tangent_close(f"{label}:{k}", got[k], b, scale=scale)
            else:
                hu.compare(f"{label}:{k}", got[k], b, lambda k=k: f32()[k], top=top, axis=1)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, " | ".join(bad)


@pytest.mark.parametrize("d", range(len(SEEDS)))
@pytest.mark.parametrize("name", du.WET_CASES)
def test_jvp_batch_against_float64(name, d, hip_backend):
    dirs, tan = _batch(name)
    assert set(tan) == set(gj.output_keys(name))
    _compare_f64(f"wet-jvpb:{name}:d{d}", name, {k: v[d] for k, v in tan.items()}, SEEDS[d], dirs[d])


@pytest.mark.parametrize("name", du.WET_CASES)
def test_forward_ad_against_jvp_batch(name, hip_backend):
    dirs, tan = _batch(name)
    model = _module(name)
    with fwAD.dual_level():
        _, x_dict, params = _inputs(name, DEV, {k: v for k, v in dirs[0].items() if k != "states0"})
        s_dir = torch.from_numpy(dirs[0]["states0"]).to(DEV)
        model.states = tuple(fwAD.make_dual(s, s_dir[k]) for k, s in enumerate(model.states))
        out = model(x_dict, params)
        one = {}
        for k in gj.output_keys(name):
            p, t = fwAD.unpack_dual(out[k])
            one[k] = (torch.zeros_like(p) if t is None else t).double().cpu().numpy()
    _compare_keys(f"wet-jvp-1dir:{name}", name, {k: v[0] for k, v in tan.items()}, one)
    n_diff = sum(int((tan[k][0] != one[k]).sum()) for k in one)
    worst = max(float(np.abs(tan[k][0] - one[k]).max()) for k in one)
    REPORT.append((f"wet-jvp-1dir-bit-identical:{name}:{'yes' if n_diff == 0 else 'no'}", worst, 0.0, n_diff,
                   sum(v.size for v in one.values())))


def test_parameter_jacobian_on_a_wet_start(hip_backend):
    name = "hbv11p_wet_list_drop"
    spec = gc.CASES[name]
    M, B = spec["config"]["nmul"], spec["B"]
    phys = list(gc.PHY_NAMES["Hbv_1_1p"])
    masks = ru.masks_for("Hbv_1_1p", spec["config"], B, spec["torch_seed"])
    for nm in ("parK0", "parFC"):
        m = np.asarray(masks[nm]) != 0
        assert m.any() and not m.all(), (nm, m)        # kept and dropped basins
    inp = gc.build_inputs(name)
    ny = inp["parameters"].shape[-1]
    cols = {"parBETA": phys.index("parBETA") * M, "parK0": phys.index("parK0") * M + 1, "parFC": phys.index("parFC") * M + 2}

    def one_hot(col):
        d = np.zeros_like(inp["parameters"])
        d[-1, :, col] = 1.0
        return {"parameters": d}
    _, x_dict, params = _inputs(name, DEV)
    model = _module(name)
    keys = list(model.flux_names)
    J = parameter_jacobian(model, x_dict, params, names=["parBETA"], keys=keys)
    assert J["columns"][0] == cols["parBETA"] and set(keys) == set(gj.output_keys(name))
    got = {k: (J[k][..., 0] if k == "BFI" else J[k][..., :1]).double().cpu().numpy() for k in keys}
    _compare_f64(f"wet-jacobian:{name}:parBETA", name, got, "parBETA", one_hot(cols["parBETA"]))
    dyn = ["parK0", "parFC"]
    with pytest.raises(ValueError, match="dynamic parameter"):
        parameter_jacobian(_module(name), x_dict, params, names=dyn)
    _, tan = jvp_batch(_module(name), x_dict, params,
                       {"parameters": one_hot_directions([cols[nm] for nm in dyn], B, ny, torch.device(DEV))})
    for c, nm in enumerate(dyn):
        got = {k: v[c].double().cpu().numpy() for k, v in tan.items()}
        _compare_f64(f"wet-jacobian:{name}:{nm}", name, got, nm, one_hot(cols[nm]))
