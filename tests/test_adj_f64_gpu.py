"""GPU tier: the implicit model's HIP kernels (csrc/hbv_adj_step.h in hbv_adj_kernels.h, the adj paths of hbv_pipe.h
and hbv_tiled.h, k_adj_tan_batch) against float64 on the wet problems of tests/adj_sets.py.  tests/test_adj_f64.py runs
the same problems through the host build and documents the inputs, the branch coverage and the protocol.

 (a) every problem, both solvers, default dispatch: flow_sim, the parameter gradient and the gradient to the start;
 (b) the other kernel forms on wet120 (HBVX_FWD=tiled bit-identical to the pipeline, HBVX_CHUNK=8, HBVX_KERNEL=simple)
     and on wet65-three / wet64-list (HBVX_CHUNK=8 with a ragged last chunk, HBVX_FWD=tiled bit-identical);
 (c) k_adj_tan_batch on wet120, wet64-list, storm90-warmup and wet9 along a dense parameter direction, a dense x_phy
     direction and a STATE tangent handed to ops.hbv_tangent_batch as s_t on the record of the run from the start
     (storm90-warmup: a start of zeros carried as a tensor; storm90-warmup-wet: filled storages entering the warm-up
     pass): against the float64 oracle's JVP, D = 1, 2, 3 bit-identical column by column, per-basin duality with the
     module's backward;
 (d) the acceptance test of the staged solve on the GPU trajectory of wet120 (adj_sets.K_ROUND as committed);
 (e) what hourly_sets.admit admitted.

The float64 runs are computed once per problem (adj_sets.oracle_run, adj_sets.tangent_reference) and shared.

Measured on an MI355X (the kernels use pow_fast_ and div_approx_; the host build does not), worst error / tolerance over
the module: values 0.0019, parameter gradient 0.0014, start gradient 0.0069, tangents 0.0014 -- the head-room of the host
build; nothing admitted; per-basin duality at most 1.6e-3 of its bound; accepted states 2.88 x 2^-23 x scale at the most
(G1; host 2.88), |G2| <= 9.995e-4.  51 tests, 15 s of wall time, float64 runs included.
"""
import time

import numpy as np
import pytest
import torch

from . import adj_sets as A
from . import hourly_sets as hs
from .test_adj_f64 import assert_accepted, product_trajectory

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T0 = time.time()
TAN_PROBLEMS = A.TAN_PROBLEMS


# ---- (a) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", A.SOLVERS)
@pytest.mark.parametrize("name", list(A.PROBLEMS))
def test_problem_matches_float64(name, solver, hip_backend):
    got = A.product_run(DEV, name, solver)
    if name == "wet120" and solver == "staged":
        assert hip_backend.last_dispatch(0) == "pipe"
    A.compare_f64(f"gpu {name} [{solver}]", name, got)


# ---- (b) -------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("tight", [False, True], ids=["reference-policy", "converged"])
@pytest.mark.parametrize("name", ["wet120", "wet65-three", "wet64-list"])
def test_tiled_forward_equals_the_pipeline(name, tight, hip_backend, monkeypatch):
    """HBVX_FWD=tiled pins the single stepper wave: same block code, same ensemble add order -- the same bits in
    values, parameter gradient and start gradient.  (wet64-list has five dynamic parameters, more than the pipeline
    stages: both runs are the tiled kernel, the comparison is then one of repeatability.)"""
    a = A.product_run(DEV, name, tight=tight)
    monkeypatch.setenv("HBVX_FWD", "tiled")
    b = A.product_run(DEV, name, tight=tight)
    assert set(a) == {"flow", "g_params", "g_state"} and _same_bits(a, b)


@pytest.mark.parametrize("name", ["wet120", "wet65-three", "wet64-list"])
def test_time_parallel_adjoint_matches_float64(name, hip_backend, monkeypatch):
    """Chunks of 8 days: the time-parallel adjoint on these short records (65 and 64 days: a ragged and a full last
    chunk; slot-list instances up to three dynamic parameters, the generic ones for wet64-list's five)."""
    monkeypatch.setenv("HBVX_CHUNK", "8")
    A.compare_f64(f"gpu {name} [chunk8]", name, A.product_run(DEV, name))


def test_one_wave_kernels_match_float64(hip_backend, monkeypatch):
    monkeypatch.setenv("HBVX_KERNEL", "simple")
    A.compare_f64("gpu wet120 [simple]", "wet120", A.product_run(DEV, "wet120"))


# ---- (c) -------------------------------------------------------------------------------------------------------------
def _three(name):
    """The three directions as one D = 3 request, each input zero where it is not the direction's."""
    _, vp, vx, vs = A.tan_inputs(name)
    z = torch.zeros_like
    return torch.stack([vp, z(vp), z(vp)]), torch.stack([z(vx), vx, z(vx)]), torch.stack([z(vs), z(vs), vs])


def _tangents(name, p_t, x_t, s_t, tight=True, max_directions=None):
    """[D,T',B,1] from k_adj_tan_batch on the records of one run of the module from the start: adj_jvp._directional
    with a state tangent entering the first record."""
    from hydrodl2_amd import ops
    prob = A.inputs(name, True)
    m = A.model(DEV, prob, tight=tight)
    torch.manual_seed(5)
    with ops.record_paths() as records, torch.no_grad():
        m._forward_eager({"x_phy": prob["x"].to(DEV)}, prob["p"].to(DEV), state=prob["state"].to(DEV))
    assert len(records) == (2 if prob["cfg"]["warm_up"] else 1)
    D = p_t.shape[0]
    out = []
    for c0 in range(0, D, max_directions or D):
        c1 = min(D, c0 + (max_directions or D))
        st = s_t[c0:c1].to(DEV).contiguous()
        for rec in records:
            last = rec is records[-1]
            res = ops.hbv_tangent_batch(rec, c1 - c0, x_t[c0:c1].to(DEV).contiguous(), None, st,
                                        [p_t[c0:c1].to(DEV).contiguous()], flux_mask=1 if last else 0,
                                        n_routed=1 if (last and rec.cfg.route is not None) else 0)
            st = res.state_out
        out.append((res.routed if res.routed is not None else res.flux)[:, 0].unsqueeze(-1))
    return torch.cat(out, dim=0).cpu()


@pytest.mark.parametrize("name", TAN_PROBLEMS)
def test_tangents_match_the_float64_jvp(name, hip_backend):
    """The start direction of storm90-warmup is not held to float64: from zeros every storage sits on its clamp and the
    derivative to the start is decided by the side rounding puts the first days on -- the float32 oracle itself is
    outside the tolerance on 95 of its 250 elements.  storm90-warmup-wet is the same run from filled storages."""
    want = A.tangent_reference(name)
    got = _tangents(name, *_three(name)).numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    bad = []
    for d, what in enumerate(("parameters", "x_phy", "start")):
        if name == "storm90-warmup" and what == "start":
            continue
        try:
            A.close_f64(f"adj-f64 gpu tangent {name} {what}", got[d], want[d],
                        lambda d=d: A.tangent_reference(name, "float32")[d], A.GRAD_TOL)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, " | ".join(bad)


@pytest.mark.parametrize("name", TAN_PROBLEMS)
def test_a_direction_does_not_depend_on_its_batch(name, hip_backend):
    """D = 1, 2, 3: the direction group of k_adj_tan_batch is 2, so D = 1 and D = 3 leave a half-filled group."""
    p_t, x_t, s_t = _three(name)
    # mixed: parameters + forcing + start, parameters + forcing, start alone
    p_t, x_t, s_t = p_t + p_t.roll(1, 0), x_t + x_t.roll(2, 0), s_t + s_t.roll(1, 0)
    whole = _tangents(name, p_t, x_t, s_t, tight=False)
    assert whole.shape[0] == 3 and torch.isfinite(whole).all() and all(float(whole[d].abs().max()) > 0 for d in range(3))
    for d in range(3):
        assert torch.equal(_tangents(name, p_t[d:d + 1], x_t[d:d + 1], s_t[d:d + 1], tight=False)[0], whole[d]), d
    assert torch.equal(_tangents(name, p_t[:2], x_t[:2], s_t[:2], tight=False), whole[:2])
    assert torch.equal(_tangents(name, p_t[1:], x_t[1:], s_t[1:], tight=False), whole[1:])
    assert torch.equal(_tangents(name, p_t, x_t, s_t, tight=False, max_directions=2), whole)


@pytest.mark.parametrize("name", TAN_PROBLEMS)
def test_per_basin_duality_with_the_backward(name, hip_backend):
    """Per basin b: |<w_b, (Jv)_b> - <(J^T w)_b, v_b>| <= 1e-4 ||w_b|| ||(Jv)_b|| (tests/test_adj_jvp_gpu.py's bound), v a
    parameter AND a start direction, default solver and policy, the backward that of the same wet run."""
    prob, vp, _, vs = A.tan_inputs(name)
    jv = _tangents(name, vp[None], torch.zeros((1,) + tuple(prob["x"].shape)), vs[None], tight=False)[0].double()
    got = A.product_run(DEV, name, tight=False, zero_state=True)
    w = prob["w"].double()
    lhs = (w * jv).sum((0, 2))
    rhs = (torch.from_numpy(got["g_params"]).double() * vp.double()).sum((0, 2)) \
        + (torch.from_numpy(got["g_state"]).double() * vs.double()).sum((0, 2))
    bound = 1e-4 * w.norm(dim=(0, 2)) * jv.norm(dim=(0, 2))
    err = (lhs - rhs).abs()
    print(f"{name}: per-basin |<w,Jv> - <JTw,v>| / bound {np.array2string((err / bound).numpy(), precision=4)}")
    A.au.REPORT.append((f"adj-tan-dot-basin:{name}", float(err.max()), float((err / bound).max()),
                        int((err > bound).sum()), prob["B"]))
    assert (lhs.abs() > 0).all() and (err <= bound).all(), (err, bound)


# ---- (d) -------------------------------------------------------------------------------------------------------------
def test_accepted_state_under_the_reference_policy(hip_backend):
    assert_accepted("wet120", product_trajectory(DEV, "wet120"))


# ---- (e) -------------------------------------------------------------------------------------------------------------
def test_admission_report(hip_backend):
    """Last: what the module admitted (the expectation from the host build: nothing), each within the cap."""
    mine = [(n, k, size) for n, k, size in hs.ADMITTED if n.startswith("adj-f64 gpu")]
    for n, k, size in mine:
        print(f"admitted {k} of {size}: {n}")
    print(f"{len(mine)} admitting comparisons, {sum(k for _, k, _ in mine)} elements; module wall time "
          f"{time.time() - T0:.0f} s since import")
    assert all(k <= hs.ADMIT_CAP * size for _, k, size in mine)
