"""GPU tier: the tangent kernels (k_tan<.., TanArgs>, and k_route_tan_batch, k_bfi_tan_batch at one direction, behind
Hbv, Hbv_1_1p and Hbv_2 under torch.autograd.forward_ad) against forward AD of oracle/hbv_restate64.py in float64 on
the same float32 inputs, at _assert_tangent_close's default tolerance (rtol 1e-3, atol 2e-6 x max|float64 tangent| of
the key) -- BFI included.

(a') the 22 forward-mode fixture cases of test_jvp_gpu.py (a) against float64 (there BFI is held to 1e-2 only,
     the reference's own float32 BFI tangent being off by up to 8e-3);
(g)  a fixed-seed slice of tools/fuzz_jvp.py: 32 draws over model, M in {1,3,5,8,16,32,64}, B in {1,17,67,130}
     (k_bfi_tan_batch's 16-basin and k_route_tan_batch's 64-basin blocks with a partial last block), T in {2,9,33,129,400}
     (a short unit hydrograph, idle BFI slices, several route chunks), warm-up with and without states, dy_drop,
     muwts of every accepted shape, permuted `variables`, Hbv_2 routing on and off across the ac / elevation
     switches, tangents on each input alone and on all at once, non-contiguous inputs; its coverage is printed
     and asserted;
(h)  per basin, <w_b, (Jv)_b> == <(J^T w)_b, v_b> against the module's backward for the largest draw of each model
     (basins are independent in these models; same drop masks in both calls);
(i)  at 130 basins x 16 x 400 days: JVP(a u + b v) == a JVP(u) + b JVP(v), and two identical calls bit-identical;
(j)  Hbv_2 with routing and a tangent on only one member of (p_dyn, p_sta);
(k)  x_phy as a [T,B,3] view of a [B,T,3] buffer gives the outputs of a contiguous x_phy.

The float64 runs are on the host: on the MI355X machine the 32 fuzz draws took 4.7 s there (16 threads) against 7.3 s
on the GPU in float64 (tools/fuzz_jvp.py --time-devices) -- a restated day is ~100 small operators.
"""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from . import golden_cases as gc
from . import golden_jvp as gj
from . import jvp_draws as jd
from . import restate_util as ru
from .abi_util import REPORT
from .test_jvp_gpu import TAN_ATOL_REL, TAN_FLOOR, _assert_tangent_close, _run_jvp

pytestmark = pytest.mark.gpu

N_DRAWS, SEED = 32, 20261030
# Two additions to the default tolerance, each for a value float64 has and float32 cannot hold:
#  * a series whose float64 tangent is below TAN_FLOOR of the case's largest is priced at the largest, as in
#    test_jvp_gpu.py (a).  Float64 evidence (hbv_m3_xgrad, hbv_muwts, hbv_variables, hbv11p_static, hbv2_dyn3_routing):
#    ssflow's value is exactly 0 there (SUZ <= parPERC every day, so SUZ - min(SUZ, parPERC) = 0 and Q1 = K1 * 0),
#    float64 forward AD leaves 8e-18 .. 5e-17 of rounding in its tangent, the kernels 0;
#  * BFI's tangent is the difference of two terms, 100 dS2 / S0' and 100 S2 dS0' / S0'^2 (restate_util.bfi_term_scale);
#    where they cancel, float32 rounds each term, not the difference.  Float64 evidence (hbv2_static, basin 2): the
#    terms are 596.048696 and 596.048597, the tangent 9.9e-5; the kernel gives 1.52e-4, 5.3e-5 off = 4.4e-8 of the
#    terms.  BFI gets BFI_TERM_REL x that basin's term size on top of the default.
BFI_TERM_REL = 1e-6
# A draw that misses float64 but matches the restatement run in float32 at the same tolerance is a threshold flip: at
# a near-tie of a min / clamp / comparison the float32 state lands on the other side, and the tangent follows the
# other one-sided slope from there on.  Such draws are counted, printed and bounded (test_gpu_fuzz.py does the same for
# gradients).  Measured on the MI355X (seed 20261030): draw 11 (Hbv_2, 130 x 5 x 400, cold start) in basin 2 only --
# evapfactor's tangent on day 261 is 0.526951 in the kernel and in float32, -0.0684728 in float64, 139 streamflow
# elements of 52000 differ by up to 3.4 % of their value; draw 5 (Hbv_2, 130 x 8 x 129) in 5 streamflow elements of
# 16770, 2.8 x the tolerance.
MAX_FLIP_DRAWS = 2


def _compare_all(label, got, want, bfi_terms):
    assert set(got) == set(want), (label, sorted(set(got) ^ set(want)))
    top = max([float(np.abs(v).max()) for k, v in want.items() if k != "BFI"] + [1e-30])
    for k, b in want.items():
        m = max(float(np.abs(b).max()), 1e-30)
        if k == "BFI":
            scale = m + (BFI_TERM_REL / TAN_ATOL_REL) * bfi_terms
        else:
            scale = m if m >= TAN_FLOOR * top else top
        _assert_tangent_close(f"{label}:{k}", got[k], b, scale=scale)


# (a') ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gj.JVP_CASES)
def test_jvp_fixture_cases_against_float64(name):
    spec = gc.CASES[name]
    inp = gc.build_inputs(name)
    dirs = gj.directions(name, inp)
    _, got = _run_jvp(name, dirs)
    masks = ru.masks_for(spec["model"], spec["config"], spec["B"], spec.get("torch_seed"))
    aux = {}
    with fwAD.dual_level():
        out, _, _ = ru.run_inputs(spec["model"], spec["config"], inp, masks, torch.float64, dirs=dirs, aux=aux)
        want = ru.tangents(out, gj.output_keys(name))
        terms = ru.bfi_term_scale(aux)
    _compare_all(f"jvp-f64:{name}", got, want, terms)


# (g) -----------------------------------------------------------------------------------------------------------------
def test_fuzz_slice_against_float64(capsys):
    specs = jd.draws(N_DRAWS, SEED)
    cov = jd.coverage(specs)
    with capsys.disabled():
        print(f"\njvp-f64 fuzz coverage ({N_DRAWS} draws, seed {SEED}): {cov}")
    assert cov["model"] == sorted(jd.MODELS)
    assert cov["M"] == jd.MS and cov["B"] == jd.BS and cov["T"] == jd.TS
    assert cov["warm_up"] == ["none", "nostates", "states"] and cov["dy_drop"] == [0.0, 0.3]
    assert cov["muwts"] == ["1bcast", "T", "bcast", "none"] and len(cov["variables"]) >= 2
    assert cov["hbv2_routing_straddled"] == [False, True]
    assert len(cov["tangent"]) == sum(len(v) for v in jd.TANS.values())
    assert cov["noncontig_tangent"] == ["muwts", "params", "x_phy"]
    bad, flips = [], []         # every draw is compared before anything is raised
    for i, spec in enumerate(specs):
        inp, dirs = jd.inputs(spec)
        got = jd.run_hip(spec, inp, dirs)
        want, terms = jd.run_restate(spec, inp, dirs)
        label = f"jvp-fuzz:{i}:{spec['model']}:T{spec['T']}B{spec['B']}M{spec['M']}"
        try:
            _compare_all(label, got, want, terms)
        except AssertionError as e:
            # a threshold flip: the same equations in float32 take the kernel's branch (so they agree with it at the
            # same tolerance) where float64 takes the other one
            want32, terms32 = jd.run_restate(spec, inp, dirs, dtype=torch.float32)
            try:
                _compare_all(label + ":f32", got, want32, terms32)
                flips.append(f"draw {i}: {e}")
            except AssertionError as e32:
                bad.append(f"draw {i} {spec}: {e} | against float32 too: {e32}")
    with capsys.disabled():
        print("\n".join([f"jvp-f64 fuzz: {len(flips)} threshold-flip draws (bound {MAX_FLIP_DRAWS})"] + flips + bad))
    assert not bad, f"{len(bad)} of {N_DRAWS} draws disagree with float64 and float32"
    assert len(flips) <= MAX_FLIP_DRAWS, flips


# (h) -----------------------------------------------------------------------------------------------------------------
def _basin_axis(name, arr):
    """Axis of the basins in input `name` (muwts [B,M] has them first)."""
    return 0 if name == "p_sta" or (name == "muwts" and arr.ndim == 2) else 1


@pytest.mark.parametrize("model", jd.MODELS)
def test_per_basin_dot_product_against_backward(model):
    specs = [s for s in jd.draws(N_DRAWS, SEED) if s["model"] == model and s["B"] > 1]
    spec = dict(max(specs, key=lambda s: s["T"] * s["B"] * s["M"]))
    spec["tangent"] = "all"
    import hydrodl2_amd
    inp, dirs = jd.inputs(spec)
    tan = jd.run_hip(spec, inp, dirs)
    B = spec["B"]
    w = {k: jd.synth.loss_weights(v.shape, spec["seed"], 20 + i) for i, (k, v) in enumerate(sorted(tan.items()))}
    dev = torch.device("cuda")
    mod = hydrodl2_amd.load_model(model.lower(), model)(jd.config(spec), dev)
    torch.manual_seed(spec["torch_seed"])
    x_dict, params, leaves = jd.module_args(spec, inp, dirs, dev, requires_grad=True)
    out = mod(x_dict, params)
    loss = sum((torch.from_numpy(w[k]).to(dev) * out[k]).sum() for k in w)
    loss.backward()
    lhs = np.zeros(B)
    nw, njv = np.zeros(B), np.zeros(B)
    for k, t in tan.items():
        wk = w[k].astype(np.float64)
        ax = 0 if t.ndim == 1 else 1
        lhs += np.moveaxis(wk * t, ax, 0).reshape(B, -1).sum(1)
        nw += np.moveaxis(wk ** 2, ax, 0).reshape(B, -1).sum(1)
        njv += np.moveaxis(t ** 2, ax, 0).reshape(B, -1).sum(1)
    rhs = np.zeros(B)
    for k, v in dirs.items():
        g = leaves[k].grad.double().cpu().numpy()
        ax = _basin_axis(k, g)
        rhs += np.moveaxis(g * np.asarray(v, np.float64), ax, 0).reshape(B, -1).sum(1)
    # 1e-4 x |w_b| |Jv_b| per basin (test_jvp_gpu.py (d)'s bound, per basin), floored at 1e-7 of the largest basin's
    # product: a basin whose tangent is all but zero is held to the rounding of the others
    prod = np.sqrt(nw * njv)
    tol = 1e-4 * prod + 1e-7 * prod.max()
    err = np.abs(lhs - rhs)
    REPORT.append((f"jvp-dot-basin:{model}", float(err.max()), float((err / tol).max()), int((err > tol).sum()), B))
    bad = np.nonzero(err > tol)[0]
    assert not bad.size, f"{model} {spec}: basins {bad.tolist()[:10]}: lhs {lhs[bad][:4]} rhs {rhs[bad][:4]}"


# (i) -----------------------------------------------------------------------------------------------------------------
def test_linearity_and_determinism_large():
    spec = dict(model="Hbv", M=16, B=130, T=400, dyn=["parBETA", "parK0"], seed=777, torch_seed=5, dy_drop=0.3,
                variables=["prcp", "tmean", "pet"], cold=False, raw_scale=1.0, routing=True, warm_up=20,
                warm_up_states=True, muwts="T", tangent="all", noncontig=[])
    inp, u = jd.inputs(spec)
    v = {k: jd.synth.normalish(a.shape, spec["seed"], 90 + i) for i, (k, a) in enumerate(sorted(u.items()))}
    a, b = 0.75, -1.5
    uv = {k: (a * u[k].astype(np.float64) + b * v[k].astype(np.float64)).astype(np.float32) for k in u}
    ju, jv, juv = (jd.run_hip(spec, inp, d) for d in (u, v, uv))
    for k in ju:
        want = a * ju[k] + b * jv[k]
        _assert_tangent_close(f"jvp-linear:{k}", juv[k], want, scale=max(np.abs(a * ju[k]).max(), np.abs(b * jv[k]).max(), 1e-30))
    again = jd.run_hip(spec, inp, uv)
    for k in juv:
        np.testing.assert_array_equal(again[k], juv[k], err_msg=f"second identical JVP call differs: {k}")


# (j) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("member", ["p_dyn", "p_sta"])
def test_hbv2_routing_tangent_on_one_tuple_member(member):
    """Hbv_2 with routing: a tangent on one member of (p_dyn, p_sta) only -- with p_dyn alone the routing parameters'
    tangent comes from a member that has none (ops._hbv_tangent passes a null pointer to k_route_tan_batch)."""
    spec = dict(model="Hbv_2", M=4, B=67, T=129, dyn=["parK0", "parBETA"], seed=4242, torch_seed=3, dy_drop=0.0,
                variables=["prcp", "tmean", "pet"], cold=False, raw_scale=1.0, routing=True, warm_up=0,
                warm_up_states=True, muwts=None, tangent=member, noncontig=[])
    inp, dirs = jd.inputs(spec)
    want, terms = jd.run_restate(spec, inp, dirs)
    _compare_all(f"jvp-tuple:{member}", jd.run_hip(spec, inp, dirs), want, terms)


# (k) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", jd.MODELS)
def test_forcing_view_with_basins_outer(model):
    """x_phy a [T,B,3] view of a [B,T,3] buffer: the pipelined forward cannot address it (launch_pipe.hip: day_outer)
    and must leave it to the tiled forward -- it used to read zeros for every basin past the first tile row."""
    import hydrodl2_amd
    spec = dict(model=model, M=8, B=67, T=129, dyn=[], seed=99, torch_seed=1, dy_drop=0.0,
                variables=["prcp", "tmean", "pet"], cold=False, raw_scale=1.0, routing=True, warm_up=0,
                warm_up_states=True, muwts=None, tangent="x_phy", noncontig=[])
    inp, _ = jd.inputs(spec)
    mod = hydrodl2_amd.load_model(model.lower(), model)(jd.config(spec), torch.device("cuda"))
    outs = []
    for nc in ([], ["x_phy"]):
        with torch.no_grad():
            x_dict, params, _ = jd.module_args(dict(spec, noncontig=nc), inp, {}, "cuda")
            assert x_dict["x_phy"].is_contiguous() == (not nc)
            outs.append({k: v.cpu().numpy() for k, v in mod(x_dict, params).items()})
    for k in outs[0]:
        np.testing.assert_allclose(outs[1][k], outs[0][k], rtol=1e-6, atol=1e-6, err_msg=f"{model}:{k}")
