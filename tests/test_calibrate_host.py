"""CPU tier: `lm_step` against numpy's float64 solver, and every refusal of `normal_equations` / `calibrate` that
happens before a library call (hydrodl2_amd/calibrate.py)."""
import numpy as np
import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi
from hydrodl2_amd.calibrate import calibrate, lm_step, normal_equations

from .test_hbv_adj import host_math_backend  # noqa: F401  (fixture)
from .test_step_math_host import steptest_lib  # noqa: F401  (fixture)


def _spd(B, C, seed):
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((B, 3 * C + 2, C)) * 10.0 ** rng.uniform(-1, 1, size=(B, 1, C))
    A = np.einsum("btc,bte->bce", J, J)
    g = rng.standard_normal((B, C)) * 5.0
    return A, g


@pytest.mark.parametrize("damping", [0.0, 1e-2, "per-basin"])
def test_lm_step_against_numpy_float64(damping):
    B, C, eps = 7, 9, 1e-12
    A, g = _spd(B, C, 1)
    lam = np.full(B, damping) if damping != "per-basin" else 10.0 ** np.linspace(-4, 1, B)
    neq = {"JtJ": torch.from_numpy(A).float(), "Jtr": torch.from_numpy(g).float()}
    arg = torch.from_numpy(lam) if damping == "per-basin" else float(damping)
    delta, info = lm_step(neq, arg, eps=eps)
    assert delta.dtype == torch.float32 and tuple(delta.shape) == (B, C)
    assert not info["failed"].any()
    A32, g32 = neq["JtJ"].double().numpy(), neq["Jtr"].double().numpy()        # what lm_step was given
    for b in range(B):
        M = A32[b] + lam[b] * np.diag(np.diag(A32[b])) + eps * np.eye(C)
        want = np.linalg.solve(M, -g32[b])
        # the solve is float64 on both sides; the result is rounded to float32 once
        np.testing.assert_allclose(delta[b].numpy(), want, rtol=1e-6, atol=0.0)


def test_damping_broadcast_and_refusals():
    A, g = _spd(4, 5, 2)
    neq = {"JtJ": torch.from_numpy(A).float(), "Jtr": torch.from_numpy(g).float()}
    d_scalar, _ = lm_step(neq, 0.5)
    d_vec, _ = lm_step(neq, torch.full((4,), 0.5))
    assert torch.equal(d_scalar, d_vec)
    d_mixed, _ = lm_step(neq, torch.tensor([0.5, 0.5, 7.0, 0.5]))
    assert torch.equal(d_mixed[[0, 1, 3]], d_scalar[[0, 1, 3]]) and not torch.equal(d_mixed[2], d_scalar[2])
    assert d_mixed[2].norm() < d_scalar[2].norm()             # more damping, shorter step
    with pytest.raises(ValueError, match="damping must be a number or"):
        lm_step(neq, torch.ones(3))
    with pytest.raises(ValueError, match="must not be negative"):
        lm_step(neq, -1.0)


def test_a_singular_basin_gets_a_zero_step_and_is_flagged():
    A, g = _spd(5, 4, 3)
    A[1] = 0.0                                                 # no sensitivity at all: singular with eps = 0
    A[3] = np.array([[1.0, 2, 0, 0], [2, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])   # indefinite
    neq = {"JtJ": torch.from_numpy(A).float(), "Jtr": torch.from_numpy(g).float()}
    delta, info = lm_step(neq, 0.0, eps=0.0)
    assert info["failed"].tolist() == [False, True, False, True, False]
    assert torch.equal(delta[1], torch.zeros(4)) and torch.equal(delta[3], torch.zeros(4))
    ok, _ = lm_step({"JtJ": neq["JtJ"][[0, 2, 4]], "Jtr": neq["Jtr"][[0, 2, 4]]}, 0.0, eps=0.0)
    assert torch.equal(delta[[0, 2, 4]], ok)                   # the failed basins do not disturb the others
    neq["JtJ"][0, 0, 0] = float("nan")
    delta, info = lm_step(neq, 1e-2)
    assert info["failed"].tolist() == [True, False, False, True, False] and torch.isfinite(delta).all()
    assert torch.equal(delta[0], torch.zeros(4))


def _model(name=("hbv", "Hbv"), **cfg):
    cls = name[1]
    cfg = {"nmul": 2, "dynamic_params": {cls: cfg.pop("dyn", [])}, **cfg}
    return hydrodl2_amd.load_model(*name)(cfg, torch.device("cpu"))


def test_the_calls_are_exported():
    assert hydrodl2_amd.normal_equations is normal_equations and hydrodl2_amd.calibrate is calibrate
    assert hydrodl2_amd.lm_step is lm_step
    assert {"normal_equations", "lm_step", "calibrate"} <= set(hydrodl2_amd.__all__)
    assert {"hbvx_gram", "hbvx_gram_workspace_bytes"} <= set(_abi.OPTIONAL_EXPORTS)


def test_refusals_happen_before_anything_runs():
    """No library is selected here and the tensors are host tensors: a call that got as far as the module's forward
    would fail with the package's own 'no CPU path' error instead of the refusal under test."""
    T, B = 8, 3
    x = {"x_phy": torch.zeros(T, B, 3)}
    state = torch.get_rng_state()
    hbv = _model(dyn=["parBETA"])
    ny = hbv.learnable_param_count
    p, tgt = torch.zeros(T, B, ny), torch.zeros(T, B)
    for fn in (normal_equations, calibrate):
        hourly = hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")({"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}},
                                                                        torch.device("cpu"))
        with pytest.raises(NotImplementedError, match="Hbv_2_hourly.*gages"):
            fn(hourly, x, p, tgt)
        hf = {"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}, "train_spatial_chunk_size": 4,
              "simulate_spatial_chunk_size": 4, "simulate_temporal_chunk_size": 4, "train_warmup": 1}
        mts = hydrodl2_amd.load_model("hbv_2_mts", "Hbv_2_mts")({"nmul": 2, "dynamic_params": {"Hbv_2": []}}, hf,
                                                                torch.device("cpu"))
        with pytest.raises(NotImplementedError, match="Hbv_2_mts.*gages"):
            fn(mts, x, p, tgt)
        with pytest.raises(ValueError, match="graph=True"):
            fn(_model(graph=True), x, p, tgt)
        with pytest.raises(ValueError, match="graph=True"):
            fn(_model(("hbv_adj", "HbvAdj"), graph=True), x, p, tgt)
        with pytest.raises(ValueError, match="'BFI'"):
            fn(hbv, x, p, tgt, key="BFI")
        with pytest.raises(KeyError, match="no flux key"):
            fn(hbv, x, p, tgt, key="flow_sim")
        with pytest.raises(KeyError, match="no flux key"):
            fn(_model(("hbv_adj", "HbvAdj")), x, torch.zeros(T, B, 12 * 2 + 2), tgt, key="streamflow")
        with pytest.raises(ValueError, match="no static parameter"):
            fn(hbv, x, p, tgt, names=["parNOPE"])
        with pytest.raises(ValueError, match="dynamic parameter"):
            fn(hbv, x, p, tgt, names=["parBETA"])
        for bad in (torch.zeros(T - 1, B), torch.zeros(T, B + 1), torch.zeros(T, B, 2), torch.zeros(B, T)):
            with pytest.raises(ValueError, match="target must be"):
                fn(hbv, x, p, bad)
        with pytest.raises(ValueError, match="target must be"):        # the days after the warm-up
            fn(_model(warm_up=3), x, p, tgt)
        with pytest.raises(ValueError, match="infinities"):
            fn(hbv, x, p, torch.full((T, B), float("inf")))
        w = torch.ones(T, B)
        w[2, 1] = -1e-3
        with pytest.raises(ValueError, match="must not be negative"):
            fn(hbv, x, p, tgt, weights=w)
        with pytest.raises(ValueError, match="weights must be"):
            fn(hbv, x, p, tgt, weights=torch.ones(T, B, 1))
        with pytest.raises(ValueError, match="max_directions must be >= 1"):
            fn(hbv, x, p, tgt, max_directions=0)
        init = _model()
        init.initialize = True
        with pytest.raises(ValueError, match="initialize"):
            fn(init, x, p, tgt)
    with pytest.raises(ValueError, match="dy_drop"):
        calibrate(_model(dyn=["parBETA"], dy_drop=0.3), x, p, tgt)
    with pytest.raises(ValueError, match="dy_drop"):
        calibrate(_model(("hbv_adj", "HbvAdj"), dyn=["parBETA"], dy_drop=0.3), x, torch.zeros(T, B, 12 * 2 + 2), tgt)
    with pytest.raises(ValueError, match="n_iter"):
        calibrate(hbv, x, p, tgt, n_iter=0)
    assert torch.equal(torch.get_rng_state(), state)            # nothing ran: no dy_drop draw was made


def test_a_non_finite_simulation_is_refused_and_missing_observations_are_masked():
    from hydrodl2_amd.calibrate import _Request, _residual
    req = _Request(False, "streamflow", "parameters", [0], 4, 2, 3)
    sim = torch.arange(8.0).reshape(4, 2)
    tgt = sim.clone() + 1.0
    tgt[1, 0] = tgt[3, 1] = float("nan")
    w, r = _residual(req, sim, tgt.unsqueeze(-1), None)
    assert w.tolist() == [[1, 1], [0, 1], [1, 1], [1, 0]] and r.tolist() == [[-1, -1], [0, -1], [-1, -1], [-1, 0]]
    w, r = _residual(req, sim, tgt, torch.full((4, 2), 0.5))
    assert w.tolist() == [[.5, .5], [0, .5], [.5, .5], [.5, 0]] and torch.isfinite(r).all()
    w, r = _residual(req, sim, sim + 1.0, None)
    assert w is None and r.tolist() == [[-1, -1]] * 4
    for bad in (float("nan"), float("inf")):
        broken = sim.clone()
        broken[2, 1] = bad
        with pytest.raises(ValueError, match="simulated streamflow holds non-finite"):
            _residual(req, broken, tgt, None)


def test_a_library_without_the_export_is_named_before_the_primal(host_math_backend):  # noqa: F811
    """The host build of the math header has the implicit scheme's forward and no hbvx_gram: both the operator and
    `normal_equations` raise the error naming the export, the latter before the module ran (no draw is consumed)."""
    from hydrodl2_amd import ops
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_gram"):
        ops.gram(torch.zeros(2, 4, 3))
    model = _model(("hbv_adj", "HbvAdj"), dyn=["parBETAET"], dy_drop=0.5)
    T, B, ny = 6, 3, 13 * 2 + 2
    xs, p = {"x_phy": torch.rand(T, B, 3)}, torch.randn(T, B, ny)
    state = torch.get_rng_state()
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_gram"):
        normal_equations(model, xs, p, torch.zeros(T, B))
    assert torch.equal(torch.get_rng_state(), state)
