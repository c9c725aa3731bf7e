"""CPU tier: the C ABI of the implicit scheme's tangent call (hbvx_adj_tangent_batch, include/hbvx.h) and the Python
entry points above it.  The cross-compiled library exports the call under ABI 10 and refuses a bad call with a message
before anything is launched (no GPU here: a launch would fail with a device error instead); the Python side refuses
what it cannot differentiate before the primal runs; a library without the export is named as such after it ran."""
import pytest
import torch

from hydrodl2_amd import _abi

from .test_hbv_adj import host_math_backend  # noqa: F401  (fixture)
from .test_step_math_host import steptest_lib  # noqa: F401  (fixture)
from .test_tan_batch_abi import _batch, _desc

TRAJ = 64      # never followed: every call below is refused on the host


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    return _abi.Library(ge.build_hip())


def _adj(n_param=13):
    d = _desc(model=_abi.MODEL_HBVADJ, n_param=n_param)
    d.adj_gtol, d.adj_max_iter = 1e-3, 3
    return d


def test_the_library_exports_the_call_under_abi_10(lib):
    assert "hbvx_adj_tangent_batch" in _abi.OPTIONAL_EXPORTS
    assert "hbvx_adj_tangent_batch" not in lib.missing and hasattr(lib.dll, "hbvx_adj_tangent_batch")
    assert lib.dll.hbvx_version() == 10


def test_entry_refuses_before_any_launch(lib):
    for d in (_adj(13), _adj(12)):
        with pytest.raises(_abi.HbvxError, match="hbvx_adj_tangent_batch: n_dir must be >= 1"):
            lib.adj_tangent_batch(d, _batch(n_flux=1, n_dir=0), TRAJ, 0)
        with pytest.raises(_abi.HbvxError, match="hbvx_adj_tangent_batch: too many directions"):
            lib.adj_tangent_batch(d, _batch(n_flux=1, n_dir=70000), TRAJ, 0)
        with pytest.raises(_abi.HbvxError, match="flux_mask selects a series at or above n_flux"):
            lib.adj_tangent_batch(d, _batch(n_flux=1, mask=2), TRAJ, 0)
        with pytest.raises(_abi.HbvxError, match="hbvx_adj_tangent_batch: traj is NULL"):
            lib.adj_tangent_batch(d, _batch(n_flux=1), None, 0)
        tb = _batch(n_flux=1)
        tb.tan_state_out = None
        with pytest.raises(_abi.HbvxError, match="tan_state_out is NULL"):
            lib.adj_tangent_batch(d, tb, TRAJ, 0)
        tb = _batch(n_flux=1)
        tb.muwts, tb.mu_d_stride = 64, 8
        with pytest.raises(_abi.HbvxError, match="hbvx_adj_tangent_batch: muwts must be NULL"):
            lib.adj_tangent_batch(d, tb, TRAJ, 0)
    d = _adj()
    with pytest.raises(_abi.HbvxError, match="hbvx_adj_tangent_batch: n_flux must be 1"):
        lib.adj_tangent_batch(d, _batch(n_flux=11), TRAJ, 0)
    tb = _batch(n_flux=1)
    tb.tan_flux = None
    with pytest.raises(_abi.HbvxError, match="tan_flux is NULL"):
        lib.adj_tangent_batch(d, tb, TRAJ, 0)
    for t0 in (-1, 8):
        tb = _batch(n_flux=1)
        tb.dyn_t0 = t0
        with pytest.raises(_abi.HbvxError, match="dyn_t0"):
            lib.adj_tangent_batch(d, tb, TRAJ, 0)
    tb = _batch(n_flux=1)
    tb.p[0].dyn = 64                    # parBETA is static in this descriptor
    with pytest.raises(_abi.HbvxError, match="dynamic tangent for a static parameter"):
        lib.adj_tangent_batch(d, tb, TRAJ, 0)


def test_entry_is_for_the_implicit_scheme_and_the_others_keep_refusing_it(lib):
    for other in (_desc(), _desc(model=_abi.MODEL_HBV11P, n_param=14), _desc(model=_abi.MODEL_HBV20, n_param=16),
                  _desc(model=_abi.MODEL_HOURLY, n_param=19)):
        with pytest.raises(_abi.HbvxError, match=r"\(-3\).*hbvx_adj_tangent_batch: the implicit scheme"):
            lib.adj_tangent_batch(other, _batch(n_flux=1), TRAJ, 0)
    with pytest.raises(_abi.HbvxError, match="HBV 1.0 / 1.1p / 2.0 only"):
        lib.forward_tangent_batch(_adj(), _batch(n_flux=1), 0)
    with pytest.raises(_abi.HbvxError, match="the hourly model only"):
        lib.hourly_tangent_batch(_adj(), _batch(n_flux=1), 0)


def _model(cfg=None, name=("hbv_adj", "HbvAdj")):
    import hydrodl2_amd
    cfg = cfg or {"nmul": 2, "dynamic_params": {"HbvAdj": ["parBETAET"]}}
    return hydrodl2_amd.load_model(*name)(cfg, torch.device("cpu"))


def test_python_entry_points_are_exported_and_refuse_before_the_primal():
    import hydrodl2_amd
    from hydrodl2_amd.adj_jvp import adj_jvp_batch, adj_parameter_jacobian
    assert hydrodl2_amd.adj_jvp_batch is adj_jvp_batch and hydrodl2_amd.adj_parameter_jacobian is adj_parameter_jacobian
    assert {"adj_jvp_batch", "adj_parameter_jacobian"} <= set(hydrodl2_amd.__all__)
    model = _model()
    T, B, ny = 6, 3, 13 * 2 + 2
    x = {"x_phy": torch.zeros(T, B, 3)}
    p = torch.zeros(T, B, ny)
    state = torch.get_rng_state()

    def refused(exc, match, tangents, m=model, **kw):
        with pytest.raises(exc, match=match):
            m.jvp_batch(x, p, tangents, **kw)

    refused(ValueError, "unknown tangent names", {"p_sta": torch.zeros(2, B, ny)})
    refused(ValueError, "unknown tangent names", {"muwts": torch.zeros(2, T, B, 2)})
    refused(ValueError, "at least one tangent", {})
    refused(ValueError, "leading direction axis", {"parameters": torch.zeros(2, B, ny), "x_phy": torch.zeros(3, T, B, 3)})
    refused(ValueError, "tangent of parameters must be", {"parameters": torch.zeros(2, T, B, ny - 1)})
    refused(ValueError, "tangent of parameters must be", {"parameters": torch.zeros(2, T - 1, B, ny)})
    refused(ValueError, "tangent of x_phy must be", {"x_phy": torch.zeros(2, T, B, 2)})
    refused(ValueError, "max_directions must be >= 1", {"parameters": torch.zeros(2, B, ny)}, max_directions=0)
    refused(ValueError, "graph=True", {"parameters": torch.zeros(2, B, ny)},
            m=_model({"nmul": 2, "graph": True, "dynamic_params": {"HbvAdj": ["parBETAET"]}}))
    with pytest.raises(ValueError, match="dynamic parameter"):
        model.parameter_jacobian(x, p, names=["parBETAET"])
    with pytest.raises(ValueError, match="no static parameter"):
        model.parameter_jacobian(x, p, names=["parC"])
    with pytest.raises(ValueError, match="max_directions must be >= 1"):
        model.parameter_jacobian(x, p, max_directions=0)
    # any other model
    hbv = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": 2, "dynamic_params": {"Hbv": []}}, torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="adj_jvp_batch is for HbvAdj, not Hbv"):
        adj_jvp_batch(hbv, x, p, {"parameters": torch.zeros(2, B, ny)})
    with pytest.raises(NotImplementedError, match="adj_jvp_batch is for HbvAdj"):
        adj_parameter_jacobian(hbv, x, p)
    assert torch.equal(torch.get_rng_state(), state)        # nothing ran: no dy_drop draw was made


def test_the_generic_paths_keep_refusing_the_model():
    import torch.autograd.forward_ad as fwAD
    import hydrodl2_amd
    model = _model()
    T, B, ny = 6, 3, 13 * 2 + 2
    x, p = torch.zeros(T, B, 3), torch.zeros(T, B, ny)
    with pytest.raises(NotImplementedError, match="forward-mode AD"):
        hydrodl2_amd.jvp_batch(model, {"x_phy": x}, p, {"parameters": torch.zeros(2, B, ny)})
    with pytest.raises(NotImplementedError, match="forward-mode AD"):
        hydrodl2_amd.parameter_jacobian(model, {"x_phy": x}, p)
    with fwAD.dual_level():
        with pytest.raises(NotImplementedError, match="forward-mode AD"):
            model({"x_phy": x}, fwAD.make_dual(p, torch.ones_like(p)))


def test_a_library_without_the_export_names_it_after_the_primal_ran(host_math_backend):  # noqa: F811
    """The host build of the math header (tests/hosttest/hbvx_host.cpp) has hbvx_adj_forward and no tangent call: the
    primal runs on it (the generator moves by one call's draws), the first tangent call raises the error naming the
    export."""
    model = _model({"nmul": 2, "dy_drop": 0.5, "dynamic_params": {"HbvAdj": ["parBETAET"]}})
    T, B, ny = 6, 3, 13 * 2 + 2
    g = torch.Generator().manual_seed(0)
    x = torch.rand((T, B, 3), generator=g) * 10.0
    p = torch.randn((T, B, ny), generator=g)
    torch.manual_seed(3)
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_adj_tangent_batch"):
        model.jvp_batch({"x_phy": x}, p, {"parameters": torch.ones(2, B, ny)})
    after = torch.get_rng_state()
    torch.manual_seed(3)
    model({"x_phy": x}, p)
    assert torch.equal(torch.get_rng_state(), after)
