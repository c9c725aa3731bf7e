"""GPU tier: hbvx_quadform through `ops.quadform`, and `predictive_variance` on Hbv, Hbv_2 and HbvAdj.

Bound of every comparison with float64 (tests/test_quadform_host.py has the derivation): y_e is a chain of at most C
fused multiply-adds, the square costs 2 gamma_C + gamma_C^2, the chain over e another gamma_C, so
    |q - q64| <= gamma_n * sum_e (sum_{c<=e} |m_ec s_c|)^2,  n = 3C + 4,  gamma_n = n u / (1 - n u),  u = 2^-24,
the sums of magnitudes in float64.  The float64 reference is an einsum over the SAME float32 series and the SAME
float32 factor (for `predictive_variance`: over the module's own parameter_jacobian output), so nothing but the
kernel's arithmetic is compared."""
import functools

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import ops
from hydrodl2_amd.calibrate import normal_equations
from hydrodl2_amd.uncertainty import parameter_covariance, predictive_variance

from . import synth

DEV = "cuda:0"
U = 2.0 ** -24
# (33, 130, 70): three basin groups, a partial tile of factor rows; (730, 130, 194): workgroups of four waves, the
# column count of the flagship Jacobian; the others run one wave per workgroup
SHAPES = [(1, 1, 1), (5, 3, 7), (257, 67, 17), (33, 130, 70), (730, 130, 194)]


def gamma(n):
    return n * U / (1.0 - n * U)


def bits(t):
    return t.contiguous().view(torch.int32)


def _reference(s, m):
    """float64 value and sum of magnitudes of |tril(m) s|^2 for series s [C,T,B] and factor m [B,C,C]."""
    m8 = torch.tril(torch.nan_to_num(m.double(), nan=0.0))
    s8 = s.double()
    y = torch.einsum("bec,ctb->etb", m8, s8)
    mag = torch.einsum("bec,ctb->etb", m8.abs(), s8.abs())
    return (y * y).sum(0), (mag * mag).sum(0)


@functools.lru_cache(maxsize=None)
def _problem(T, B, Cn):
    """Series with a stride above T*B between them (a slice of a longer record), a lower-triangular factor with NaN
    above the diagonal, and the float64 reference -- computed once, shared, never modified."""
    g = torch.Generator().manual_seed(1000 * T + 10 * B + Cn)
    full = torch.randn((Cn, T + 3, B), generator=g) * 10.0 ** (torch.rand((Cn, 1, 1), generator=g) * 4 - 2)
    m = torch.randn((B, Cn, Cn), generator=g) * 10.0 ** (torch.rand((B, 1, Cn), generator=g) * 2 - 1)
    m = torch.tril(m) + torch.triu(torch.full((Cn, Cn), float("nan")), 1)
    full, m = full.to(DEV), m.to(DEV)
    s = full[:, 2:2 + T]
    assert Cn == 1 or s.stride(0) > T * B
    return s, m, _reference(s, m)


def _check(name, got, want, mag, Cn):
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    assert bool((got >= 0).all()), f"{name}: a negative variance"
    err = (got.double() - want).abs()
    bound = gamma(3 * Cn + 4) * mag
    need = float((err / torch.where(bound > 0, bound, torch.ones_like(bound))).max())
    print(f"{name}: worst error / bound {need:.3f}")
    assert bool((err <= bound).all()), f"{name}: error {float(err.max()):.3e} exceeds the bound by {need:.2f}x"


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,Cn", SHAPES, ids=[f"{t}x{b}x{c}" for t, b, c in SHAPES])
def test_quadform_against_float64(hip_backend, T, B, Cn):
    assert ops._POISON, "the GPU tier runs with NaN-poisoned output and workspace buffers"
    s, m, (want, mag) = _problem(T, B, Cn)
    q = ops.quadform(s, m)                       # strided series, NaN above the diagonal
    assert tuple(q.shape) == (T, B) and q.dtype == torch.float32
    _check("quadform", q, want, mag, Cn)
    assert torch.equal(bits(ops.quadform(s, m)), bits(q)), "two calls differ"
    # the same series packed (series_stride == T*B), the factor with zeros above the diagonal: neither enters
    assert torch.equal(bits(ops.quadform(s.contiguous(), torch.tril(torch.nan_to_num(m)))), bits(q))


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,Cn", [(257, 67, 17), (33, 130, 70), (730, 130, 194)])
def test_bits_of_a_day_and_a_basin_depend_on_nothing_else(hip_backend, T, B, Cn):
    s, m, _ = _problem(T, B, Cn)
    q = ops.quadform(s, m)
    assert torch.equal(bits(ops.quadform(s[:, 3:20], m)), bits(q[3:20])), "a day slice differs"
    sel = sorted({b for b in (0, 2, 4, 63, 64, 66, B - 1) if b < B})
    got = ops.quadform(s[:, :, sel], m[sel])     # not unit-stride in B: ops.quadform packs it
    assert torch.equal(bits(got), bits(q[:, sel])), "a basin subset differs"


def test_quadform_refuses_tensors_it_cannot_take():
    """Host-side checks (no launch): runs without a GPU on the cross-compiled library."""
    import __graft_entry__ as ge
    from tests import seam
    ge.build_hip()
    seam.use_library(None)
    with pytest.raises(TypeError, match="series must be float32"):
        ops.quadform(torch.zeros(2, 4, 3, dtype=torch.float64), torch.zeros(3, 2, 2))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.quadform(torch.zeros(2, 4, 3), torch.zeros(3, 2, 2))


# -- predictive_variance -----------------------------------------------------------------------------------------
T_ALL, WARM, B, M = 40, 10, 5, 2


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(model, x_dict, parameters, key, target, weights, jacobian call) at warm_up 10, T 40, B 5, nmul 2, routing on:
    the cases of tests/test_normal_eq_gpu.py."""
    x = torch.from_numpy(synth.forcing(T_ALL, B, seed=11)).to(DEV)
    if kind == "Hbv":
        model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "warm_up": WARM, "routing": True,
                                                       "dynamic_params": {"Hbv": ["parBETA"]}}, DEV)
        p = torch.from_numpy(synth.raw_parameters(T_ALL, B, model.learnable_param_count, seed=12)).to(DEV)
        xd, key, T_out = {"x_phy": x}, "streamflow", T_ALL - WARM
        jac = lambda **kw: hydrodl2_amd.parameter_jacobian(model, xd, p, keys=(key,), max_directions=64, **kw)   # noqa: E731
    elif kind == "Hbv_2":
        model = hydrodl2_amd.load_model("hbv_2", "Hbv_2")({"nmul": M, "routing": True,
                                                           "dynamic_params": {"Hbv_2": ["parBETA", "parK0"]}}, DEV)
        p = (torch.from_numpy(synth.unit_parameters((T_ALL, B, model.learnable_param_count1), seed=13)).to(DEV),
             torch.from_numpy(synth.unit_parameters((B, model.learnable_param_count2), seed=14)).to(DEV))
        xd = {"x_phy": x, "ac_all": torch.from_numpy(synth.uniform((B,), 15) * 2000 + 10).to(DEV),
              "elev_all": torch.from_numpy(synth.uniform((B,), 16) * 3000).to(DEV)}
        key, T_out = "streamflow", T_ALL
        jac = lambda **kw: hydrodl2_amd.parameter_jacobian(model, xd, p, keys=(key,), max_directions=64, **kw)   # noqa: E731
    else:
        model = hydrodl2_amd.load_model("hbv_adj", "HbvAdj")({"nmul": M, "warm_up": WARM, "routing": True,
                                                              "dynamic_params": {"HbvAdj": []}}, DEV)
        p = torch.from_numpy(synth.raw_parameters(T_ALL, B, model.learnable_param_count, seed=17)).to(DEV)
        xd, key, T_out = {"x_phy": x}, "flow_sim", T_ALL - WARM
        jac = lambda **kw: hydrodl2_amd.adj_parameter_jacobian(model, xd, p, max_directions=64, **kw)            # noqa: E731
    target = torch.from_numpy(synth.uniform((T_out, B), 18) * 6.0).to(DEV)
    weights = torch.from_numpy(synth.uniform((T_out, B), 19) + 0.25).to(DEV)
    return model, xd, p, key, target, weights, jac


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["Hbv", "Hbv_2", "HbvAdj"])
def test_predictive_variance_against_the_models_own_jacobian(hip_backend, kind):
    model, xd, p, key, target, weights, jac = _case(kind)
    neq = normal_equations(model, xd, p, target, weights=weights)
    cov = parameter_covariance(neq, prior_precision=1.0)
    assert not cov["failed"].any() and cov["columns"] == neq["columns"]
    factor = cov["factor"]
    out = predictive_variance(model, xd, p, factor, max_directions=64)
    Jd = jac()
    J, cols = Jd[key], Jd["columns"]
    C = len(cols)
    assert out["columns"] == cols and tuple(out["var"].shape) == (J.shape[0], B)
    assert torch.equal(out["outputs"][key], neq["outputs"][key])
    want, mag = _reference(J.permute(2, 0, 1), factor)
    _check(f"{kind} var", out["var"], want, mag, C)
    assert float(out["var"].abs().max()) > 0
    # the same call three directions at a time: the series do not depend on their batch, nor does the form
    few = predictive_variance(model, xd, p, factor, max_directions=3)
    assert torch.equal(bits(few["var"]), bits(out["var"])), "var depends on max_directions"
    # a subset of names with the factor of the matching sub-covariance
    names = ["parFC", "parK2"]
    sub_neq = normal_equations(model, xd, p, target, names=names, weights=weights)
    sub_cov = parameter_covariance(sub_neq, prior_precision=1.0)
    sub = predictive_variance(model, xd, p, sub_cov["factor"], names=names)
    assert sub["columns"] == sub_neq["columns"] and len(sub["columns"]) == 2 * M
    idx = [cols.index(c) for c in sub["columns"]]
    want, mag = _reference(J[:, :, idx].permute(2, 0, 1), sub_cov["factor"])
    _check(f"{kind} var[{names}]", sub["var"], want, mag, len(idx))
    assert float(sub["var"].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["Hbv", "HbvAdj"])
def test_n_obs_counts_the_positive_weights(hip_backend, kind):
    model, xd, p, key, target, weights, _ = _case(kind)
    T_out = target.shape[0]
    plain = normal_equations(model, xd, p, target)
    assert plain["n_obs"].dtype == torch.int64 and plain["n_obs"].tolist() == [T_out] * B
    w0 = weights.clone()
    w0[::3] = 0.0                                # exact zeros do not count
    assert torch.equal(normal_equations(model, xd, p, target, weights=w0)["n_obs"], (w0 > 0).sum(0))
    miss = torch.from_numpy(synth.uniform(tuple(target.shape), 20) < 1.0 / 3.0).to(DEV)
    holes = torch.where(miss, torch.full_like(target, float("nan")), target)
    assert torch.equal(normal_equations(model, xd, p, holes)["n_obs"], (~miss).sum(0))
    assert torch.equal(normal_equations(model, xd, p, holes, weights=w0)["n_obs"], ((w0 > 0) & ~miss).sum(0))
