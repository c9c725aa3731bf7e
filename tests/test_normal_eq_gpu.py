"""GPU tier: hbvx_gram through `ops.gram`, `normal_equations` on Hbv, Hbv_2 and HbvAdj, and the LM loop `calibrate`.

Bound of every comparison with float64 (tests/test_gram_host.py has the derivation): an element is a sum of T
products, one rounding for the weight product, fused multiply-adds, at most T additions of slice sums -- for any
order of such a sum the error is at most gamma_n * sum_t |w s_c s_e|, n = T + 4, gamma_n = n u / (1 - n u), u = 2^-24,
the sum of magnitudes in float64.  The float64 reference is an einsum over the SAME float32 series (for
`normal_equations`: over the module's own parameter_jacobian output), so nothing but the summation is compared."""
import functools

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi, ops
from hydrodl2_amd.calibrate import calibrate, normal_equations

from . import synth

DEV = "cuda:0"
U = 2.0 ** -24
SHAPES = [(1, 1, 1), (5, 3, 7), (257, 67, 17), (1000, 5, 35), (730, 130, 194)]


def gamma(n):
    return n * U / (1.0 - n * U)


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _problem(T, B, Cn):
    """Series with a stride above T*B between them (a slice of a longer record), weights with exact zeros, residuals,
    and the float64 references with their sums of magnitudes -- computed once, shared, never modified."""
    g = torch.Generator().manual_seed(1000 * T + 10 * B + Cn)
    full = torch.randn((Cn, T + 3, B), generator=g) * 10.0 ** (torch.rand((Cn, 1, 1), generator=g) * 4 - 2)
    w = torch.rand((T, B), generator=g)
    w[torch.rand((T, B), generator=g) < 0.2] = 0.0
    r = torch.randn((T, B), generator=g)
    full, w, r = full.to(DEV), w.to(DEV), r.to(DEV)
    s = full[:, 2:2 + T]
    assert Cn == 1 or s.stride(0) > T * B
    s8, w8, r8 = s.double(), w.double(), r.double()
    ones = torch.ones_like(w8)
    ref = {}
    for form, ww in (("w", w8), ("plain", ones)):
        ref[form] = {"gram": (torch.einsum("ctb,etb,tb->bce", s8, s8, ww), torch.einsum("ctb,etb,tb->bce", s8.abs(), s8.abs(), ww)),
                     "rhs": (torch.einsum("ctb,tb->bc", s8, r8 * ww), torch.einsum("ctb,tb->bc", s8.abs(), r8.abs() * ww)),
                     "cost": ((r8 * r8 * ww).sum(0),) * 2}
    return s, w, r, ref


def _check(name, got, want, mag, T):
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = (got.double() - want).abs()
    bound = gamma(T + 4) * mag
    need = float((err / torch.where(bound > 0, bound, torch.ones_like(bound))).max())
    print(f"{name}: worst error / bound {need:.3f}")
    assert bool((err <= bound).all()), f"{name}: error {float(err.max()):.3e} exceeds the bound by {need:.2f}x"


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,Cn", SHAPES, ids=[f"{t}x{b}x{c}" for t, b, c in SHAPES])
def test_gram_against_float64(hip_backend, T, B, Cn):
    assert ops._POISON, "the GPU tier runs with NaN-poisoned output and workspace buffers"
    s, w, r, ref = _problem(T, B, Cn)
    for form in ("w+r", "w", "r", "plain") if Cn <= 35 else ("w+r", "plain"):
        ww = w if "w" in form else None
        rr = r if "r" in form else None
        gram, rhs, cost = ops.gram(s, ww, rr)
        rf = ref["w" if ww is not None else "plain"]
        _check(f"gram[{form}]", gram, *rf["gram"], T)
        assert torch.equal(bits(gram), bits(gram.transpose(1, 2))), "gram is not bit-symmetric"
        if rr is None:
            assert rhs is None and cost is None
        else:
            _check(f"rhs[{form}]", rhs, *rf["rhs"], T)
            _check(f"cost[{form}]", cost, *rf["cost"], T)
        again = ops.gram(s, ww, rr)
        for a, b in zip((gram, rhs, cost), again):
            assert (a is None and b is None) or torch.equal(bits(a), bits(b)), "two calls differ"
        # the same series packed (series_stride == T*B): the stride is not part of the arithmetic
        packed = ops.gram(s.contiguous(), ww, rr)
        assert torch.equal(bits(packed[0]), bits(gram))


@pytest.mark.gpu
def test_bits_of_a_column_pair_do_not_depend_on_the_other_columns(hip_backend):
    T, B, Cn = 257, 67, 17
    s, w, r, _ = _problem(T, B, Cn)
    gram, rhs, cost = ops.gram(s, w, r)
    cols = [0, 3, 8, 9, 16]
    g2, r2, c2 = ops.gram(s[cols], w, r)
    assert torch.equal(bits(g2), bits(gram[:, cols][:, :, cols]))
    assert torch.equal(bits(r2), bits(rhs[:, cols])) and torch.equal(bits(c2), bits(cost))


def test_gram_refuses_bad_arguments_and_a_library_without_the_export_names_it():
    """Host-side checks (no launch): runs without a GPU on the cross-compiled library."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    assert "hbvx_gram" not in lib.missing and "hbvx_gram_workspace_bytes" not in lib.missing
    g = _abi.GramDesc(abi_version=_abi.ABI_VERSION, T=4, B=3, C=2, series_stride=12)
    assert lib.gram_workspace_bytes(g) > 0
    with pytest.raises(_abi.HbvxError, match=r"\(-1\).*hbvx_gram: s is NULL"):
        lib.gram(g, None, None, None, 64, None, None, 64, 1 << 20, 0)
    with pytest.raises(_abi.HbvxError, match=r"\(-1\).*hbvx_gram: gram is NULL"):
        lib.gram(g, 64, None, None, None, None, None, 64, 1 << 20, 0)
    with pytest.raises(_abi.HbvxError, match=r"\(-1\).*rhs / cost is NULL"):
        lib.gram(g, 64, None, 64, 64, None, None, 64, 1 << 20, 0)
    with pytest.raises(_abi.HbvxError, match=r"\(-1\).*workspace"):
        lib.gram(g, 64, None, None, 64, None, None, 64, 8, 0)
    for field in ("T", "B", "C"):
        bad = _abi.GramDesc(abi_version=_abi.ABI_VERSION, T=4, B=3, C=2, series_stride=12)
        setattr(bad, field, 0)
        assert lib.gram_workspace_bytes(bad) == 0
        with pytest.raises(_abi.HbvxError, match=r"\(-2\).*T/B/C"):
            lib.gram(bad, 64, None, None, 64, None, None, 64, 1 << 20, 0)
    with pytest.raises(_abi.HbvxError, match=r"\(-2\).*series_stride"):
        lib.gram(_abi.GramDesc(abi_version=_abi.ABI_VERSION, T=4, B=3, C=2, series_stride=11), 64, None, None, 64, None, None,
                 64, 1 << 20, 0)
    with pytest.raises(_abi.HbvxError, match=r"\(-4\).*abi_version"):
        lib.gram(_abi.GramDesc(abi_version=9, T=4, B=3, C=2, series_stride=12), 64, None, None, 64, None, None, 64, 1 << 20, 0)
    lib.missing.append("hbvx_gram")             # a library built before the export existed
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_gram"):
        lib.gram(g, 64, None, None, 64, None, None, 64, 1 << 20, 0)


# -- normal_equations --------------------------------------------------------------------------------------------
T_ALL, WARM, B, M = 40, 10, 5, 2


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(model, x_dict, parameters, key, target, jacobian call) at warm_up 10, T 40, B 5, nmul 2, routing on."""
    x = torch.from_numpy(synth.forcing(T_ALL, B, seed=11)).to(DEV)
    if kind == "Hbv":
        model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "warm_up": WARM, "routing": True,
                                                       "dynamic_params": {"Hbv": ["parBETA"]}}, DEV)
        p = torch.from_numpy(synth.raw_parameters(T_ALL, B, model.learnable_param_count, seed=12)).to(DEV)
        xd, key, T_out = {"x_phy": x}, "streamflow", T_ALL - WARM
        jac = lambda: hydrodl2_amd.parameter_jacobian(model, xd, p, keys=(key,), max_directions=64)   # noqa: E731
    elif kind == "Hbv_2":
        model = hydrodl2_amd.load_model("hbv_2", "Hbv_2")({"nmul": M, "routing": True,
                                                           "dynamic_params": {"Hbv_2": ["parBETA", "parK0"]}}, DEV)
        p = (torch.from_numpy(synth.unit_parameters((T_ALL, B, model.learnable_param_count1), seed=13)).to(DEV),
             torch.from_numpy(synth.unit_parameters((B, model.learnable_param_count2), seed=14)).to(DEV))
        xd = {"x_phy": x, "ac_all": torch.from_numpy(synth.uniform((B,), 15) * 2000 + 10).to(DEV),
              "elev_all": torch.from_numpy(synth.uniform((B,), 16) * 3000).to(DEV)}
        key, T_out = "streamflow", T_ALL
        jac = lambda: hydrodl2_amd.parameter_jacobian(model, xd, p, keys=(key,), max_directions=64)   # noqa: E731
    else:
        model = hydrodl2_amd.load_model("hbv_adj", "HbvAdj")({"nmul": M, "warm_up": WARM, "routing": True,
                                                              "dynamic_params": {"HbvAdj": []}}, DEV)
        p = torch.from_numpy(synth.raw_parameters(T_ALL, B, model.learnable_param_count, seed=17)).to(DEV)
        xd, key, T_out = {"x_phy": x}, "flow_sim", T_ALL - WARM
        jac = lambda: hydrodl2_amd.adj_parameter_jacobian(model, xd, p, max_directions=64)            # noqa: E731
    target = torch.from_numpy(synth.uniform((T_out, B), 18) * 6.0).to(DEV)
    weights = torch.from_numpy(synth.uniform((T_out, B), 19) + 0.25).to(DEV)
    return model, xd, p, key, target, weights, jac


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["Hbv", "Hbv_2", "HbvAdj"])
def test_normal_equations_against_the_models_own_jacobian(hip_backend, kind):
    model, xd, p, key, target, weights, jac = _case(kind)
    neq = normal_equations(model, xd, p, target, weights=weights, max_directions=64)
    Jd = jac()
    J, cols = Jd[key], Jd["columns"]
    assert neq["columns"] == cols and tuple(neq["JtJ"].shape) == (B, len(cols), len(cols))
    T_out = J.shape[0]
    sim = neq["outputs"][key][..., 0]
    r8 = (sim - target).double()                       # the float32 residual the call formed
    J8, w8 = J.double(), weights.double()
    _check(f"{kind} JtJ", neq["JtJ"], torch.einsum("tbc,tbe,tb->bce", J8, J8, w8),
           torch.einsum("tbc,tbe,tb->bce", J8.abs(), J8.abs(), w8), T_out)
    _check(f"{kind} Jtr", neq["Jtr"], torch.einsum("tbc,tb->bc", J8, r8 * w8),
           torch.einsum("tbc,tb->bc", J8.abs(), r8.abs() * w8), T_out)
    _check(f"{kind} cost", neq["cost"], (r8 * r8 * w8).sum(0), (r8 * r8 * w8).sum(0), T_out)
    assert float(neq["JtJ"].abs().max()) > 0 and float(neq["Jtr"].abs().max()) > 0
    # the same call three directions at a time: the series do not depend on their batch, nor do the sums
    few = normal_equations(model, xd, p, target, weights=weights, max_directions=3)
    assert few["columns"] == cols
    for k in ("JtJ", "Jtr", "cost"):
        assert torch.equal(bits(few[k]), bits(neq[k])), f"{k} depends on max_directions"
    # a subset of names gives the matching block
    names = ["parFC", "parK2"]
    sub = normal_equations(model, xd, p, target, names=names, weights=weights)
    idx = [cols.index(c) for c in sub["columns"]]
    assert len(idx) == 2 * M and torch.equal(bits(sub["JtJ"]), bits(neq["JtJ"][:, idx][:, :, idx]))
    assert torch.equal(bits(sub["Jtr"]), bits(neq["Jtr"][:, idx]))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["Hbv", "HbvAdj"])
def test_missing_observations_are_zero_weights(hip_backend, kind):
    model, xd, p, key, target, weights, _ = _case(kind)
    miss = torch.from_numpy(synth.uniform(tuple(target.shape), 20) < 1.0 / 3.0).to(DEV)
    assert 0 < int(miss.sum()) < miss.numel()
    holes = torch.where(miss, torch.full_like(target, float("nan")), target)
    for wts in (None, weights):
        got = normal_equations(model, xd, p, holes, weights=wts)
        base = torch.ones_like(target) if wts is None else wts
        want = normal_equations(model, xd, p, torch.where(miss, torch.full_like(target, 123.0), target),
                                weights=torch.where(miss, torch.zeros_like(base), base))
        for k in ("JtJ", "Jtr", "cost"):
            assert torch.isfinite(got[k]).all() and torch.equal(bits(got[k]), bits(want[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["Hbv", "Hbv_2", "HbvAdj"])
def test_fixed_point_has_zero_gradient_and_cost(hip_backend, kind):
    model, xd, p, key, target, weights, _ = _case(kind)
    with torch.no_grad():
        own = model(xd, p)[key].clone()
    neq = normal_equations(model, xd, p, own, weights=weights)
    assert not neq["Jtr"].any() and not neq["cost"].any()
    assert float(neq["JtJ"].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["Hbv", "HbvAdj"])
def test_calibrate_on_the_twin_problem(hip_backend, kind):
    """Observations from a hidden static parameter field; the start is the truth moved by 0.3 in raw space in the three
    named parameters.  The accept rule makes every basin's recorded cost non-increasing; the test checks the rule."""
    T, Bn, names = 120, 6, ["parBETA", "parFC", "parK1"]
    fam = ("hbv", "Hbv") if kind == "Hbv" else ("hbv_adj", "HbvAdj")
    model = hydrodl2_amd.load_model(*fam)({"nmul": 1, "dynamic_params": {kind: []}}, DEV)
    x = {"x_phy": torch.from_numpy(synth.forcing(T, Bn, seed=31)).to(DEV)}
    truth = torch.from_numpy(synth.raw_parameters(T, Bn, model.learnable_param_count, seed=32)).to(DEV)
    with torch.no_grad():
        key = "streamflow" if kind == "Hbv" else "flow_sim"
        obs = model(x, truth)[key][..., 0].clone()
    _, cols = hydrodl2_amd.sensitivity.jacobian_columns(model, names)
    start = truth.clone()
    sign = torch.tensor([[1.0, -1.0, 1.0], [-1.0, 1.0, 1.0]], device=DEV).repeat(Bn // 2, 1)
    start[-1][:, cols] += 0.3 * sign
    keep_start, keep_obs, keep_x = start.clone(), obs.clone(), x["x_phy"].clone()
    fitted, hist = calibrate(model, x, start, obs, names=names, n_iter=6)
    assert torch.equal(start, keep_start) and torch.equal(obs, keep_obs) and torch.equal(x["x_phy"], keep_x)
    cost = hist["cost"]
    assert tuple(cost.shape) == (7, Bn) and tuple(hist["accepted"].shape) == (6, Bn) and hist["columns"] == cols
    assert bool(torch.isfinite(cost).all()) and bool((cost[1:] <= cost[:-1]).all()), "a basin's recorded cost rose"
    # the rule itself: the cost moved exactly where a step was accepted, the damping went down there and up elsewhere
    assert torch.equal(cost[1:] < cost[:-1], hist["accepted"])
    lam = hist["damping"]
    assert torch.allclose(lam[1:], torch.where(hist["accepted"][:-1], lam[:-1] * 0.1, lam[:-1] * 10.0), rtol=1e-12)
    first, last = float(cost[0].sum()), float(cost[-1].sum())
    print(f"calibrate {kind}: summed cost {first:.6g} -> {last:.6g} (ratio {last / first:.3e}), "
          f"accepted {int(hist['accepted'].sum())} of {hist['accepted'].numel()} steps")
    assert first > 0 and last < first
    # only the named columns of the static row moved
    moved = (fitted != start)
    assert not moved[:-1].any() and not moved[-1][:, [c for c in range(start.shape[-1]) if c not in cols]].any()
    with torch.no_grad():
        again = ((model(x, fitted)[key][..., 0].double() - obs.double()) ** 2).sum(0).cpu()
    assert torch.allclose(again, cost[-1], rtol=1e-9)
