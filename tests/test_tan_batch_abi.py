"""CPU tier: the C ABI of the batched tangent calls (hbvx_forward_tangent_batch, hbvx_route_tangent_batch,
hbvx_bfi_tangent_batch; include/hbvx.h).  The cross-compiled library exports them, hbvx_tan_batch has the layout of its
ctypes mirror, the host refuses a bad call with a message before anything is launched (no GPU here: a launch would
fail with a device error instead), and a library without the exports is named as such."""
import ctypes as C

import pytest
import torch

from hydrodl2_amd import _abi

BATCH_EXPORTS = ("hbvx_forward_tangent_batch", "hbvx_route_tangent_batch", "hbvx_bfi_tangent_batch")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    return _abi.Library(ge.build_hip())


def _desc(model=_abi.MODEL_HBV10, n_param=12, T=8, B=3, M=4):
    """A descriptor check_desc accepts; the pointers are never followed (every call below is refused on the host)."""
    d = _abi.Desc()
    d.abi_version = _abi.ABI_VERSION
    d.model, d.T, d.B, d.M, d.n_param = model, T, B, M, n_param
    d.raw_sigmoid = 1
    d.ch_prcp, d.ch_tmean, d.ch_pet = 0, 1, 2
    d.nearzero = 1e-5
    d.x, d.x_t_stride, d.x_b_stride = 64, B * 3, 3
    d.ac = d.elev = 64
    for i in range(n_param):
        d.p[i].sta, d.p[i].sta_b_stride = 64, n_param * M
        d.p[i].lo, d.p[i].hi = 0.5, 1.0
    return d


def _batch(n_flux=11, n_dir=2, mask=1):
    tb = _abi.TanBatch()
    tb.n_dir, tb.n_flux, tb.flux_mask = n_dir, n_flux, mask
    tb.tan_flux = tb.tan_state_out = 64
    return tb


def test_the_library_exports_the_batch_calls(lib):
    for name in BATCH_EXPORTS:
        assert name not in lib.missing and hasattr(lib.dll, name), name
    with pytest.raises(_abi.HbvxError, match="too many directions"):
        lib.forward_tangent_batch(_desc(), _batch(n_dir=70000), 0)


def test_struct_layout_matches_ctypes(lib):
    assert lib.dll.hbvx_sizeof(8) == C.sizeof(_abi.TanBatch)
    assert lib.dll.hbvx_version() == 10


def test_host_validation_refuses_before_any_launch(lib):
    d = _desc()
    with pytest.raises(_abi.HbvxError, match="n_dir must be >= 1"):
        lib.forward_tangent_batch(d, _batch(n_dir=0), 0)
    with pytest.raises(_abi.HbvxError, match="flux_mask selects a series at or above n_flux"):
        lib.forward_tangent_batch(d, _batch(mask=1 << 11), 0)
    tb = _batch()
    tb.tan_state_out = None
    with pytest.raises(_abi.HbvxError, match="tan_state_out is NULL"):
        lib.forward_tangent_batch(d, tb, 0)
    tb = _batch()
    tb.tan_flux = None
    with pytest.raises(_abi.HbvxError, match="tan_flux is NULL"):
        lib.forward_tangent_batch(d, tb, 0)
    with pytest.raises(_abi.HbvxError, match="n_flux does not match model"):
        lib.forward_tangent_batch(d, _batch(n_flux=12), 0)
    tb = _batch()
    tb.dyn_t0 = 8
    with pytest.raises(_abi.HbvxError, match="dyn_t0"):
        lib.forward_tangent_batch(d, tb, 0)
    hourly = _desc(model=_abi.MODEL_HOURLY, n_param=19)
    with pytest.raises(_abi.HbvxError, match="HBV 1.0 / 1.1p / 2.0 only"):
        lib.forward_tangent_batch(hourly, _batch(n_flux=12), 0)
    r = _abi.RouteDesc()
    r.abi_version, r.T, r.B, r.S, r.L = _abi.ABI_VERSION, 8, 3, 4, 8
    r.ra = r.rb = 64
    with pytest.raises(_abi.HbvxError, match="n_dir"):
        lib.route_tangent_batch(r, 0, 64, 64, None, 0, None, None, 0, 64, 0)
    with pytest.raises(_abi.HbvxError, match="n_dir"):
        lib.route_tangent_batch(r, 20000, 64, 64, None, 0, None, None, 0, 64, 0)
    with pytest.raises(_abi.HbvxError, match="NULL"):
        lib.route_tangent_batch(r, 2, 64, 64, None, 0, None, None, 0, None, 0)
    with pytest.raises(_abi.HbvxError, match="n_dir"):
        lib.bfi_tangent_batch(8, 3, 0, 64, 64, None, None, 0, 1e-5, 64, 0)
    with pytest.raises(_abi.HbvxError, match="bad arguments"):
        lib.bfi_tangent_batch(8, 3, 2, 64, 64, None, None, 0, 1e-5, None, 0)


def test_a_library_without_the_exports_names_the_missing_one(oracle_backend):
    """The CPU restatement under oracle/ has no batched tangent calls: the primal runs on it, the first tangent call
    raises an error naming the export."""
    import hydrodl2_amd
    from hydrodl2_amd.sensitivity import jvp_batch
    model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": 2, "dynamic_params": {"Hbv": []}}, torch.device("cpu"))
    T, B, ny = 6, 3, 12 * 2 + 2
    g = torch.Generator().manual_seed(0)
    x = torch.rand((T, B, 3), generator=g) * 10.0
    p = torch.randn((T, B, ny), generator=g)
    assert set(model({"x_phy": x}, p)) >= {"streamflow", "BFI"}
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_forward_tangent_batch"):
        jvp_batch(model, {"x_phy": x}, p, {"parameters": torch.ones(2, B, ny)}, keys=("streamflow",))
