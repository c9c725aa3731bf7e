"""GPU tier: forward-mode AD of HbvAdj (hydrodl2_amd.adj_jvp_batch / HbvAdj.jvp_batch, adj_parameter_jacobian) on the
HIP kernel k_adj_tan_batch, on the shapes of tests/test_hbv_adj.py::CASES -- one ragged wave, one exact wave, a
non-power-of-two member count with cold forcing and dy_drop, two waves behind a flux-less 40-day warm-up, and five
dynamic parameters (the generic parameter fetch; up to three take the slot-list instances).

The reference is the float64 oracle's own JVP (torch.autograd.functional.jvp of oracle/hbv_adj_oracle.py), computed
once per case and shared by the tests that need it.  Finite differences are not a reference here: the value is an
inexact Newton iterate, the derivative the exact implicit-function one at it."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from .test_hbv_adj import CASES, SOLVERS, _close, _inputs, adj_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDS = [f"M{c['M']}-T{c['T']}" for c in CASES]
_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hydrodl2_amd", "csrc",
                    "hbv_adj_kernels.h")
GROUP = int(re.search(r"#define ADJ_TAN_G (\d+)", open(_HDR).read()).group(1))     # directions per wave


def _case_inputs(case):
    betaet = "parBETAET" in case["cfg"]["dynamic_params"]["HbvAdj"]
    return _inputs(case["T"], case["B"], case["M"], case["seed"], betaet, case.get("cold", False), case.get("scale", 1.0))


def _directions(case):
    """Three directions: dense on `parameters` (full form), compact on `parameters`, dense on all of `x_phy`."""
    x, p, _ = _case_inputs(case)
    g = torch.Generator().manual_seed(1000 + case["seed"])
    full = torch.randn(p.shape, generator=g) * 0.3
    compact = torch.randn(p.shape[1:], generator=g) * 0.3
    vx = torch.randn(x.shape, generator=g)
    return full, compact, vx


def _model(cfg, **extra):
    import hydrodl2_amd
    return hydrodl2_amd.load_model("hbv_adj", "HbvAdj")(dict(cfg, **extra), torch.device(DEV))


def _policy(tight):
    return dict(newton_gtol=1e-6, newton_max_iter=12) if tight else {}


@functools.lru_cache(maxsize=None)
def _reference(idx, tight, routing=True):
    """[3,T_out,B,1] float64: the oracle's JVP along the three directions of _directions (same seed handling as
    test_hbv_adj._run_case: the dy_drop masks are drawn from the seeded default generator)."""
    case = CASES[idx]
    cfg = dict(case["cfg"], **_policy(tight))
    x, p, _ = _case_inputs(case)
    full, compact, vx = _directions(case)
    last = torch.zeros_like(p)
    last[-1] = compact

    def f(xx, pp):
        return adj_oracle.hbv_adj_forward(xx, pp, nmul=cfg["nmul"], warm_up=cfg.get("warm_up", 0),
                                          dynamic_params=cfg["dynamic_params"]["HbvAdj"], dy_drop=cfg.get("dy_drop", 0.0),
                                          gtol=cfg.get("newton_gtol", 1e-3), max_iter=cfg.get("newton_max_iter", 3),
                                          routing=routing)[0]

    out = []
    zx, zp = torch.zeros_like(x).double(), torch.zeros_like(p).double()
    for tx, tp in ((zx, full.double()), (zx, last.double()), (vx.double(), zp)):
        torch.manual_seed(5)
        out.append(torch.autograd.functional.jvp(f, (x.double(), p.double()), (tx, tp))[1].numpy())
    return np.stack(out)


def _three(case):
    """The three directions as one D = 3 request, each input zero where it is not the direction's."""
    x, p, _ = _case_inputs(case)
    full, compact, vx = _directions(case)
    last = torch.zeros_like(p)
    last[-1] = compact
    pt = torch.stack([full, last, torch.zeros_like(p)])
    xt = torch.stack([torch.zeros_like(x), torch.zeros_like(x), vx])
    return {"parameters": pt.to(DEV), "x_phy": xt.to(DEV)}


def _jvp(case, tangents, seed=5, **cfg_extra):
    x, p, _ = _case_inputs(case)
    m = _model(case["cfg"], **cfg_extra)
    torch.manual_seed(seed)
    with torch.no_grad():
        out, tan = m.jvp_batch({"x_phy": x.to(DEV)}, p.to(DEV), tangents)
    return out["flow_sim"], tan["flow_sim"]


# -- 1. against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_tangents_match_the_float64_jvp_converged(idx, solver, hip_backend):
    case = CASES[idx]
    want = _reference(idx, True)
    _, got = _jvp(case, _three(case), newton_solver=solver, **_policy(True))
    got = got.cpu().numpy()
    assert got.shape == want.shape
    for d, name in enumerate(("parameters (full)", "parameters (last row)", "x_phy")):
        _close(name, got[d], want[d], 2e-3, 2e-4)
    # the compact form IS the full tensor that is zero except in its last row
    _, compact, _ = _directions(case)
    _, got_c = _jvp(case, {"parameters": compact.unsqueeze(0).to(DEV)}, newton_solver=solver, **_policy(True))
    assert torch.equal(got_c[0].cpu(), torch.from_numpy(got[1]))


def test_tangents_match_the_float64_jvp_reference_policy(hip_backend):
    case = CASES[1]
    want = _reference(1, False)
    got = _jvp(case, _three(case))[1].cpu().numpy()
    for d, name in enumerate(("parameters (full)", "parameters (last row)", "x_phy")):
        _close(name, got[d], want[d], 5e-2, 5e-3)


# -- 2. duality with the module's own backward ---------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_dot_product_against_backward(idx, hip_backend):
    """|<w, Jv> - <J^T w, v>| <= 1e-4 ||w|| ||Jv|| (the bound of tests/test_jvp_gpu.py), default solver and policy."""
    case = CASES[idx]
    x, p, w = _case_inputs(case)
    v = _directions(case)[0]
    jv = _jvp(case, {"parameters": v.unsqueeze(0).to(DEV)})[1][0].double().cpu()
    m = _model(case["cfg"])
    pp = p.to(DEV).clone().requires_grad_(True)
    torch.manual_seed(5)
    out = m({"x_phy": x.to(DEV)}, pp)["flow_sim"]
    ww = w[-out.shape[0]:]
    (out * ww.to(DEV)).sum().backward()
    lhs = float((ww.double() * jv).sum())
    rhs = float((pp.grad.double().cpu() * v.double()).sum())
    bound = 1e-4 * float(ww.double().norm()) * float(jv.norm())
    print(f"<w,Jv> {lhs:.9g}  <JTw,v> {rhs:.9g}  diff {abs(lhs - rhs):.3e}  bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


# -- 3. batch invariance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [0, 3, 4], ids=[IDS[0], IDS[3], IDS[4]])
def test_a_direction_does_not_depend_on_its_batch(idx, hip_backend):
    case = CASES[idx]
    x, p, _ = _case_inputs(case)
    D = GROUP + 1
    g = torch.Generator().manual_seed(7)
    tan = {"parameters": (torch.randn((D,) + tuple(p.shape), generator=g) * 0.3).to(DEV),
           "x_phy": torch.randn((D,) + tuple(x.shape), generator=g).to(DEV)}
    m = _model(case["cfg"])
    xd, pd = {"x_phy": x.to(DEV)}, p.to(DEV)

    def run(t, **kw):
        torch.manual_seed(5)
        with torch.no_grad():
            return m.jvp_batch(xd, pd, t, **kw)[1]["flow_sim"]

    whole = run(tan)
    assert whole.shape[0] == D and torch.isfinite(whole).all()
    for d in range(D):
        one = run({k: t[d:d + 1] for k, t in tan.items()})       # D = 1 works
        assert one.shape[0] == 1 and torch.equal(one[0], whole[d]), d
    assert torch.equal(run(tan, max_directions=2), whole)


# -- 4. the primal is untouched ------------------------------------------------------------------------------------
def test_primal_and_generator_move_as_in_one_plain_call(hip_backend):
    case = CASES[2]                                  # dy_drop 0.5, three dynamic parameters
    x, p, _ = _case_inputs(case)
    m = _model(case["cfg"])
    xd, pd = {"x_phy": x.to(DEV)}, p.to(DEV)
    torch.manual_seed(5)
    with torch.no_grad():
        plain = m(xd, pd)["flow_sim"]
    after_plain = torch.get_rng_state()
    out, _ = _jvp(case, _three(case))
    torch.manual_seed(5)
    with torch.no_grad():
        out2, _ = m.jvp_batch(xd, pd, _three(case))
    assert torch.equal(torch.get_rng_state(), after_plain)     # exactly one call's draws
    assert torch.equal(out, plain) and torch.equal(out2["flow_sim"], plain)
    torch.manual_seed(5)
    with torch.no_grad():
        again = m(xd, pd)["flow_sim"]
    assert torch.equal(again, plain)


# -- 5. edges ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _short_reference(T, routing):
    """The oracle's JVP of the first T days of CASES[0] (static parameters only, no warm-up), tight Newton."""
    x, p, full, vx = _short(T)

    def f(xx, pp):
        return adj_oracle.hbv_adj_forward(xx, pp, nmul=CASES[0]["M"], gtol=1e-6, max_iter=12, routing=routing)[0]

    return torch.autograd.functional.jvp(f, (x.double(), p.double()), (vx.double(), full.double()))[1].numpy()


def _short(T):
    case = CASES[0]
    x, p, _ = _case_inputs(case)
    full, _, vx = _directions(case)
    return x[:T].contiguous(), p[:T].contiguous(), full[:T].contiguous(), vx[:T].contiguous()


@pytest.mark.parametrize("T,routing", [(1, True), (2, True), (CASES[0]["T"], False)], ids=["T1", "T2", "no-routing"])
def test_short_records_and_no_routing(T, routing, hip_backend):
    """T = 1 and T = 2: the prologue and the epilogue of the one-day-ahead prefetch; routing=False: the raw series."""
    x, p, full, vx = _short(T)
    m = _model(CASES[0]["cfg"], routing=routing, **_policy(True))
    with torch.no_grad():
        out, tan = m.jvp_batch({"x_phy": x.to(DEV)}, p.to(DEV), {"parameters": full.unsqueeze(0).to(DEV),
                                                                  "x_phy": vx.unsqueeze(0).to(DEV)})
    got = tan["flow_sim"].cpu().numpy()
    assert got.shape == (1, T, CASES[0]["B"], 1) and out["flow_sim"].shape == (T, CASES[0]["B"], 1)
    _close("flow_sim tangent", got[0], _short_reference(T, routing), 2e-3, 2e-4)


def test_zero_and_unread_directions_move_nothing(hip_backend):
    case = CASES[0]                                  # static parameters only: the model reads row T-1 alone
    x, p, _ = _case_inputs(case)
    zero = _jvp(case, {"parameters": torch.zeros((2,) + tuple(p.shape), device=DEV),
                       "x_phy": torch.zeros((2,) + tuple(x.shape), device=DEV)})[1]
    assert zero.shape[0] == 2 and (zero == 0).all()
    unread = _directions(case)[0].clone()
    unread[-1] = 0.0                                 # confined to rows below T-1
    moved = _jvp(case, {"parameters": unread.unsqueeze(0).to(DEV)})[1]
    assert (moved == 0).all()


# -- 6. Jacobian ---------------------------------------------------------------------------------------------------
def test_jacobian_columns_are_one_hot_directions(hip_backend):
    from hydrodl2_amd.sensitivity import one_hot_directions
    case = CASES[0]
    x, p, _ = _case_inputs(case)
    m = _model(case["cfg"])
    xd, pd = {"x_phy": x.to(DEV)}, p.to(DEV)
    with torch.no_grad():
        J = m.parameter_jacobian(xd, pd)
        cols = J["columns"]
        assert cols == list(range(12 * case["M"] + 2))          # every static parameter and both routing columns
        assert J["flow_sim"].shape == (case["T"], case["B"], len(cols))
        hot = one_hot_directions(cols, case["B"], p.shape[2], DEV)
        tan = m.jvp_batch(xd, pd, {"parameters": hot})[1]["flow_sim"]
        assert torch.equal(J["flow_sim"], tan[..., 0].permute(1, 2, 0))
        some = m.parameter_jacobian(xd, pd, names=["parFC", "rout_b"], max_directions=3)
        assert some["columns"] == list(range(case["M"], 2 * case["M"])) + [12 * case["M"] + 1]
        assert torch.equal(some["flow_sim"], J["flow_sim"][..., some["columns"]])
        # J @ v for a random static v against the compact-direction JVP, within the bound of the duality test
        v = _directions(case)[1].to(DEV)
        jv = m.jvp_batch(xd, pd, {"parameters": v.unsqueeze(0)})[1]["flow_sim"][0, ..., 0].double()
        Jv = (J["flow_sim"].double() * v[:, cols].double().unsqueeze(0)).sum(-1)
    assert float((Jv - jv).norm()) <= 1e-4 * float(jv.norm())


# -- 7. refusals ---------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(hip_backend):
    import torch.autograd.forward_ad as fwAD
    case = CASES[0]
    x, p, _ = _case_inputs(case)
    xd, pd = {"x_phy": x.to(DEV)}, p.to(DEV)
    m = _model(case["cfg"])
    ok = torch.zeros((2,) + tuple(p.shape[1:]), device=DEV)
    with pytest.raises(ValueError, match="graph=True"):
        _model(case["cfg"], graph=True).jvp_batch(xd, pd, {"parameters": ok})
    with pytest.raises(ValueError, match="unknown tangent names"):
        m.jvp_batch(xd, pd, {"states": torch.zeros(2, 5, case["B"], case["M"], device=DEV)})
    with pytest.raises(ValueError, match="tangent of parameters must be"):
        m.jvp_batch(xd, pd, {"parameters": ok[..., :-1]})
    with pytest.raises(ValueError, match="tangent of x_phy must be"):
        m.jvp_batch(xd, pd, {"x_phy": torch.zeros((2,) + tuple(x.shape[:2]) + (4,), device=DEV)})
    with pytest.raises(ValueError, match="dynamic parameter"):
        _model(CASES[1]["cfg"]).parameter_jacobian(xd, pd, names=["parBETA"])
    with fwAD.dual_level():
        with pytest.raises(NotImplementedError, match="forward-mode AD"):
            m(xd, fwAD.make_dual(pd, torch.ones_like(pd)))
