"""CPU tier: the implicit model (HbvAdj: csrc/hbv_adj_step.h compiled for the host, driven through the module) against
float64 on problems whose wet branches are taken.  tests/test_hbv_adj.py's CASES start from empty storages and run 36-90
days: the soil never fills, the upper zone never passes parUZL.  The problems of tests/adj_sets.py start from
synth.wet_states (handed to HbvAdj._forward_eager as `state`, to the oracle as `y0`) or multiply the precipitation by 4.

Branch coverage at the float64 root (share of lane-days; the largest over the problems, printed in full by
test_every_branch_is_taken): SM > FC 0.61 (wet1; 0.026 on wet120, 0 on both zero-start problems: a carried-in state is
needed), q0 active 0.83, perc = PERC 1.0, ef clamped 0.83, et = SM 0.014 and SM below the 1e-8 floor 0.082 (storm120, the
zero start: from y2t = 0 with PET > 0 the root of the soil equation is -et(1e-8) < 0, and the next day starts below
zero -- AdjStaged::soil handles that start, `live` false; only the comment claiming storages >= 0 is loose),
all four (perc side x q0 side) combinations of AdjStaged::gw >= 0.013.  No listed branch is unreachable.

Protocol: hourly_sets.admit with the float32 oracle as the alternative evaluation, tolerances test_hbv_adj._close's
converged ones.  Measured on the host build, worst error / tolerance over the problems and both solvers: values
0.0019, parameter gradient 0.0010, start gradient 0.0069, the host tangent chain 0.0009; no element needed admission.
"""
import numpy as np
import pytest
import torch

from . import adj_sets as A
from .test_adj_tanstep_host import NAMES13, tanlib  # noqa: F401  (fixture)
from .test_hbv_adj import adj_oracle, host_math_backend  # noqa: F401  (fixture)
from .test_step_math_host import steptest_lib  # noqa: F401  (fixture)


def test_oracle_gradient_on_a_wet_start_is_the_implicit_function_derivative():
    """Central finite differences of the oracle's converged forward from filled storages, with respect to the
    parameters AND the start y0.  An element is used only if both displaced runs take the branches of the centre run on
    every lane-day (away from kinks); at least 8 parameter elements and 8 start elements must qualify."""
    T, B, M = 12, 3, 2
    dyn = ["parBETA", "parBETAET"]
    x = torch.from_numpy(A.synth.forcing(T, B, 80, day0=60.0))
    p = torch.from_numpy(A.synth.raw_parameters(T, B, 13 * M + 2, 80, 2.0)).double()
    w = torch.from_numpy(A.synth.loss_weights((T, B, 1), 80, 70)).double()
    y0 = A.to_lanes(torch.from_numpy(A.synth.wet_states(B, M, 80))).double()

    def run(pv, yv, grad=False):
        ev = {}
        pv, yv = pv.clone().requires_grad_(grad), yv.clone().requires_grad_(grad)
        with torch.set_grad_enabled(grad):
            out, _ = adj_oracle.hbv_adj_forward(x, pv, nmul=M, dynamic_params=dyn, gtol=1e-11, max_iter=40, y0=yv,
                                                events=ev)
            loss = (out * w).sum()
        if grad:
            loss.backward()
        return float(loss.detach()), ev, pv.grad, yv.grad

    _, ev0, gp, gy = run(p, y0, True)
    assert float(torch.stack([ev0[k].double().mean() for k in ("sm_above_fc", "q0_active", "perc_par")]).min()) > 0.01
    rng = np.random.default_rng(0)
    worst, used = [0.0, 0.0], [0, 0]
    for which, (base, g, h) in enumerate(((p, gp, 1e-5), (y0, gy, 1e-4))):
        for _ in range(600):
            idx = tuple(int(rng.integers(n)) for n in base.shape)
            if abs(float(g[idx])) < 1e-8 or used[which] >= 12:
                continue
            e = torch.zeros_like(base)
            e[idx] = h
            a = run(p + e, y0) if which == 0 else run(p, y0 + e)
            b = run(p - e, y0) if which == 0 else run(p, y0 - e)
            if any(not (torch.equal(a[1][k], ev0[k]) and torch.equal(b[1][k], ev0[k])) for k in ev0):
                continue                      # a kink between the displaced runs
            fd = (a[0] - b[0]) / (2 * h)
            worst[which] = max(worst[which], abs(fd - float(g[idx])) / max(abs(float(g[idx])), 1e-6))
            used[which] += 1
    print(f"finite differences: parameters {used[0]} elements, worst {worst[0]:.2e}; start {used[1]}, worst {worst[1]:.2e}")
    assert min(used) >= 8, used
    assert max(worst) < 2e-3, worst


def test_the_oracle_without_a_start_is_the_oracle_from_zeros():
    """y0=None returns what y0 = zeros returns, and the branch record does not touch the result."""
    prob = A.inputs("wet9")
    kw = A.oracle_kw(prob)
    a, ia = adj_oracle.hbv_adj_forward(prob["x"], prob["p"], **kw)
    ev = {}
    b, ib = adj_oracle.hbv_adj_forward(prob["x"], prob["p"], y0=torch.zeros(prob["B"] * prob["M"], 5), events=ev, **kw)
    assert torch.equal(a, b) and torch.equal(ia, ib)
    assert set(ev) == set(A.EVENTS) and all(v.shape == (prob["T"], prob["B"] * prob["M"]) and v.dtype == torch.bool
                                            for v in ev.values())


def test_every_branch_is_taken():
    """Each branch of adj_sets.EVENTS in at least COVER_MIN of the lane-days of at least one problem, counted at the
    float64 root.  None is argued unreachable."""
    rows = {name: A.coverage(name) for name in A.PROBLEMS}
    A.assert_covered(rows)
    # what the module docstring says of the starts
    assert rows["storm120"]["sm_above_fc"] == 0.0 and rows["storm120"]["sm_floor"] > 0.05
    assert rows["wet120"]["et_sm_limited"] == 0.0 and rows["wet120"]["sm_above_fc"] > 0.02


@pytest.mark.parametrize("solver", A.SOLVERS)
@pytest.mark.parametrize("name", list(A.PROBLEMS))
def test_host_math_matches_float64(name, solver, host_math_backend):  # noqa: F811
    """Converged: flow_sim, the parameter gradient and the gradient to the start, both solvers."""
    got = A.product_run("cpu", name, solver)
    A.compare_f64(f"host {name} [{solver}]", name, got)


def test_a_start_of_zeros_is_the_default_start(host_math_backend):  # noqa: F811
    """state = zeros and state = None: the same numbers, through the warm-up pass too."""
    a = A.product_run("cpu", "storm90-warmup", tight=False)
    b = A.product_run("cpu", "storm90-warmup", tight=False, zero_state=True)
    assert np.array_equal(a["flow"], b["flow"]) and np.array_equal(a["g_params"], b["g_params"])
    assert np.isfinite(b["g_state"]).all() and np.abs(b["g_state"]).max() > 0


def product_trajectory(device, name):
    """The solved trajectory [5,T+1,N] of the default module (staged solve, reference policy) on problem `name`."""
    from hydrodl2_amd import ops
    prob = A.inputs(name)
    m = A.model(device, prob, tight=False)
    st = None if prob["state"] is None else prob["state"].to(device)
    with ops.record_paths() as records, torch.no_grad():
        m._forward_eager({"x_phy": prob["x"].to(device)}, prob["p"].to(device), state=st)
    assert len(records) == 1 and records[0].traj is not None
    return records[0].traj


@pytest.mark.parametrize("name", ["wet120", "storm90-warmup-wet"])
def test_host_tangent_chain_matches_the_float64_jvp(name, tanlib, host_math_backend):  # noqa: F811
    """adj_tanstep of csrc/hbv_adj_step.h (compiled for the host, one lane-day per row) chained over the product's own
    solved trajectory of a wet record -- through the warm-up pass where there is one -- along the three directions of
    adj_sets.tan_inputs (parameters, x_phy, start), against the float64 oracle's JVP.  Without routing: the chain is
    the kernel's day loop, not the unit hydrograph's.  k_adj_tan_batch runs the same header on the GPU
    (tests/test_adj_f64_gpu.py)."""
    from hydrodl2_amd import ops
    prob, vp, vx, vs = A.tan_inputs(name)
    T, B, M, wu = prob["T"], prob["B"], prob["M"], prob["cfg"]["warm_up"]
    N = B * M
    m = A.model("cpu", prob, routing=False)
    with ops.record_paths() as records, torch.no_grad():
        m._forward_eager({"x_phy": prob["x"]}, prob["p"], state=prob["state"])
    traj = torch.cat([A.to_lanes(r.traj.view(5, r.cfg.T + 1, B, M).permute(1, 0, 2, 3))[1:] for r in records])   # [T,N,5]
    kw = {k: v for k, v in A.oracle_kw(prob).items() if k not in A.ROOT_POLICY}
    betaet = "parBETAET" in kw["dynamic_params"]
    n = 13 if betaet else 12
    lo = torch.tensor([adj_oracle.BOUNDS[k][0] for k in NAMES13[:n]], dtype=torch.float64)
    span = torch.tensor([adj_oracle.BOUNDS[k][1] - adj_oracle.BOUNDS[k][0] for k in NAMES13[:n]], dtype=torch.float64)

    def theta_of(pp):              # unit parameters of every day of both passes, [T,N,n]
        _, pw, pr, _, _ = adj_oracle.lane_inputs(prob["x"], pp, routing=False, **kw)
        return pr if pw is None else torch.cat([pw, pr])

    def rows(a):                   # -> float32 [T,N,13]
        out = np.zeros((T, N, 13), np.float32)
        out[..., :n] = a.numpy()
        return out

    clim = prob["x"].unsqueeze(1).repeat(1, M, 1, 1).view(T, N, 3).numpy()
    want = A.tangent_reference(name, routing=False)
    zero_p, zero_c = np.zeros((T, N, 13), np.float32), np.zeros((T, N, 3), np.float32)
    bad = []
    theta, theta_dot = torch.autograd.functional.jvp(theta_of, prob["p"].double(), vp.double())
    p_rows = rows(lo + theta * span)
    for d, what in enumerate(("parameters", "x_phy", "start")):
        p_dot = rows(theta_dot * span) if d == 0 else zero_p
        c_dot = vx.unsqueeze(1).repeat(1, M, 1, 1).view(T, N, 3).numpy() if d == 1 else zero_c
        x_dot = np.ascontiguousarray(A.to_lanes(vs).numpy()) if d == 2 else np.zeros((N, 5), np.float32)
        q = np.zeros((T, N), np.float32)
        for t in range(T):
            nxt = np.full((N, 5), np.nan, np.float32)
            tanlib.adj_tan_rows(int(betaet), N, *(np.ascontiguousarray(a[t]).ctypes.data for a in (p_rows, clim)),
                                np.ascontiguousarray(traj[t].numpy()).ctypes.data, x_dot.ctypes.data,
                                np.ascontiguousarray(p_dot[t]).ctypes.data, np.ascontiguousarray(c_dot[t]).ctypes.data,
                                nxt.ctypes.data, q[t].ctypes.data)
            x_dot = nxt
        got = q[wu:].reshape(T - wu, M, B).astype(np.float64).mean(1)[..., None]
        try:
            A.close_f64(f"adj-f64 host tangent chain {name} {what}", got, want[d],
                        lambda d=d: A.tangent_reference(name, "float32", routing=False)[d], A.GRAD_TOL)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, " | ".join(bad)


def assert_accepted(name, traj):
    ks, gs = A.accepted_state_residuals(name, traj, gtol=1e-3)
    print(f"{name}: largest |G_k| {np.array2string(gs, precision=3)}; (|G_k| - gtol [k=2]) / (2^-23 scale) "
          f"{np.array2string(ks, precision=3)}; committed K_ROUND {A.K_ROUND}")
    A.au.REPORT.append((f"adj-accepted {name}", float(gs.max()), float(ks.max() / A.K_ROUND), int((ks > A.K_ROUND).sum()), 5))
    assert (ks <= A.K_ROUND).all(), (name, ks, gs)


@pytest.mark.parametrize("name", ["wet120", "storm120"])
def test_accepted_state_under_the_reference_policy(name, host_math_backend):  # noqa: F811
    """The acceptance test the staged solve promises (csrc/hbv_adj_step.h: G0 = G1 = G3 = G4 = 0 up to rounding and
    |G2| <= gtol), on whole wet records: the product's solved trajectory put into the oracle's float64 residual.
    Allowance: adj_sets.K_ROUND * 2^-23 * the largest of the equation's fluxes and of the storages it reads on that
    lane-day; measured on this build 2.88 at the most (G1 on wet120), committed 11.5; |G2| itself stays below gtol
    (9.995e-4 at the most)."""
    assert_accepted(name, product_trajectory("cpu", name))
