"""CPU tier: the C ABI of the hourly model's tangent calls (hbvx_hourly_tangent_batch, hbvx_gage_route_tangent_batch,
hbvx_gage_route_tangent_workspace_bytes; include/hbvx.h).  The cross-compiled library exports them under ABI 10, the
host refuses a bad call with a message before anything is launched (no GPU here: a launch would fail with a device
error instead), and a library without the exports is named as such after the primal ran."""
import numpy as np
import pytest
import torch

from hydrodl2_amd import _abi

from . import golden_cases as gc
from .test_tan_batch_abi import _batch, _desc

EXPORTS = ("hbvx_hourly_tangent_batch", "hbvx_gage_route_tangent_batch", "hbvx_gage_route_tangent_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    return _abi.Library(ge.build_hip())


def _hourly():
    return _desc(model=_abi.MODEL_HOURLY, n_param=19)


def _gage(T=8, U=3, G=2, NPAIR=4):
    r = _abi.GageDesc()
    r.abi_version, r.T, r.U, r.G, r.NPAIR, r.L, r.lag_uh = _abi.ABI_VERSION, T, U, G, NPAIR, min(T, 72), 1
    r.pair_unit = r.gage_ptr = r.pair_gage = r.unit_ptr = r.unit_pairs = r.areas = r.denom = r.dp = 64
    return r


def test_the_library_exports_the_calls_under_abi_10(lib):
    for name in EXPORTS:
        assert name in _abi.OPTIONAL_EXPORTS
        assert name not in lib.missing and hasattr(lib.dll, name), name
    assert lib.dll.hbvx_version() == 10


def test_recurrence_entry_refuses_before_any_launch(lib):
    d = _hourly()
    for daily in (_desc(), _desc(model=_abi.MODEL_HBV11P, n_param=14), _desc(model=_abi.MODEL_HBV20, n_param=16)):
        with pytest.raises(_abi.HbvxError, match=r"\(-3\).*hbvx_hourly_tangent_batch: the hourly model only"):
            lib.hourly_tangent_batch(daily, _batch(n_flux=12), 0)
    with pytest.raises(_abi.HbvxError, match="n_flux does not match model"):
        lib.hourly_tangent_batch(d, _batch(n_flux=11), 0)
    with pytest.raises(_abi.HbvxError, match="hbvx_hourly_tangent_batch: n_dir must be >= 1"):
        lib.hourly_tangent_batch(d, _batch(n_flux=12, n_dir=0), 0)
    with pytest.raises(_abi.HbvxError, match="hbvx_hourly_tangent_batch: too many directions"):
        lib.hourly_tangent_batch(d, _batch(n_flux=12, n_dir=70000), 0)
    with pytest.raises(_abi.HbvxError, match="flux_mask selects a series at or above n_flux"):
        lib.hourly_tangent_batch(d, _batch(n_flux=12, mask=1 << 12), 0)
    tb = _batch(n_flux=12)
    tb.tan_state_out = None
    with pytest.raises(_abi.HbvxError, match="tan_state_out is NULL"):
        lib.hourly_tangent_batch(d, tb, 0)
    tb = _batch(n_flux=12)
    tb.tan_flux = None
    with pytest.raises(_abi.HbvxError, match="tan_flux is NULL"):
        lib.hourly_tangent_batch(d, tb, 0)
    for t0 in (-1, 8):
        tb = _batch(n_flux=12)
        tb.dyn_t0 = t0
        with pytest.raises(_abi.HbvxError, match="dyn_t0"):
            lib.hourly_tangent_batch(d, tb, 0)
    # the daily entry points keep refusing the hourly model
    with pytest.raises(_abi.HbvxError, match="HBV 1.0 / 1.1p / 2.0 only"):
        lib.forward_tangent_batch(d, _batch(n_flux=12), 0)


def test_gage_entry_refuses_before_any_launch(lib):
    r = _gage()
    big = 1 << 40
    for n_dir in (0, -1, 70000):
        with pytest.raises(_abi.HbvxError, match="n_dir must be in 1..65535"):
            lib.gage_route_tangent_batch(r, n_dir, 64, 64, 64, 24, 64, 12, 64, 64, big, 0)
    with pytest.raises(_abi.HbvxError, match="gage routing buffer is NULL"):
        lib.gage_route_tangent_batch(r, 2, 64, 64, 64, 24, 64, 12, None, 64, big, 0)
    need = lib.gage_route_tangent_workspace_bytes(r, 2)
    # the transposed runoff once; per direction its transposed tangent, its tap tangents and its per-pair series
    assert need == 4 * (3 * 8 + 2 * (3 * 8 + 4 * 8 + 4 * 8))
    with pytest.raises(_abi.HbvxError, match="workspace missing or too small"):
        lib.gage_route_tangent_batch(r, 2, 64, 64, 64, 24, 64, 12, 64, 64, need - 1, 0)
    with pytest.raises(_abi.HbvxError, match="workspace missing or too small"):
        lib.gage_route_tangent_batch(r, 2, 64, 64, 64, 24, 64, 12, 64, None, need, 0)
    assert lib.gage_route_tangent_workspace_bytes(r, 0) == 0
    # the slabs bound the scratch: 100 000 directions of the DESIGN.md shape would be 10 TB unslabbed
    wide = _gage(T=2160, U=4000, G=100, NPAIR=12000)
    assert lib.gage_route_tangent_workspace_bytes(wide, 60000) <= (1 << 30) + 4 * 4000 * 2160
    assert lib.gage_route_tangent_workspace_bytes(wide, 2) < lib.gage_route_tangent_workspace_bytes(wide, 4)


def test_a_library_without_the_exports_names_the_missing_one(oracle_backend):
    """The CPU restatement under oracle/ has no hourly tangent calls: the primal runs on it (its states and its
    generator move), the first tangent call raises an error naming the export."""
    import hydrodl2_amd
    name = "hourly_dyn3"
    spec = gc.CASES[name]
    model = hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")(dict(spec["config"]), torch.device("cpu"))
    inp = gc.build_inputs(name)
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in inp.items()}
    x_dict = {k: t[k] for k in ("x_phy", "ac_all", "elev_all", "outlet_topo", "areas")}
    params = (t["p_dyn"], t["p_sta"], t["p_distr"])
    assert model.get_states() is None
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_hourly_tangent_batch"):
        model.jvp_batch(x_dict, params, {"p_sta": torch.ones((2,) + tuple(t["p_sta"].shape))})
    assert model.get_states() is not None           # the primal ran
    assert hydrodl2_amd.hourly_jvp_batch is not None
