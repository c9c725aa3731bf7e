"""GPU tier: the daily models' tangent kernels at the level of the C ABI -- hbvx_forward_tangent_batch (k_tan<..,
TanBatchArgs> around Step<HBV10 / HBV11P / HBV20>::tan), hbvx_route_tangent_batch, hbvx_bfi_tangent_batch and the
one-direction hbvx_forward_tangent (k_tan<.., TanArgs>) -- on the problems of tests/daily_jvp_util.py::TAN_PROBLEMS,
whose wet branches are taken (tests/test_daily_jvp_f64.py asserts the coverage and that the reference alone stays
within the protocol).

(a) Against forward AD of oracle/hbv_restate64.py in float64 along one direction over x, params, muwts and state_in:
    the 11 / 12 flux rows, tan_state_out and the four routed rows at TAN_RTOL + TAN_ATOL_REL x max|float64 tangent of
    the series| under hourly_sets.admit (an element outside tolerance is admitted only where it agrees with the
    restatement's float32 forward AD; at most ADMIT_CAP of an array), BFI's tangent whole with the allowance of
    test_jvp_f64_gpu.BFI_TERM_REL x the basin's term size.
(b) Per basin, <gflux_b, (Jv)_b> + <grouted_b, (Jv)routed_b> == <g_params_b, v> + <g_x_b, v> + <g_muwts_b, v> against
    hbvx_backward on the same primal, with a zero state_in direction, within 1e-4 |w||Jv| + 1e-7 max: both sides take
    the kernel's own branches.
(c) On wet400, wet2(-all-drop) and wet65-channels of each model: directions 0, 3 and 4 of a D = 5 call are
    bit-identical to D = 1 calls, a mask of rows {0, 5, 10} to those rows of the full mask, and the one-direction
    entry point (k_tan<.., TanArgs>; ops._hbv_tangent on the recorded call) to D = 1 at the full mask.

Measured on the MI355X.  (a) elements outside tolerance against float64, every one admitted -- the same counts, problem
by problem, as the float32 restatement's in tests/test_daily_jvp_f64.py: flux 2 / 74800 (Hbv wet400, wet400-d3), 2 / 95073
(Hbv wet129-muwts), 1 / 81600 (Hbv_1_1p wet400-all-drop), 6 / 81600 and routed 1 / 27200 (Hbv_1_1p wet400-list), flux
13 / 81600 (Hbv_2 wet400, wet400-muwts); nothing outside in state_out or in the other 30 problems, no lane had to be
named.  Worst error / tolerance where nothing is outside: flux 0.56 (Hbv_2 dry300), state_out 0.11 (Hbv wet400), routed
0.11 (Hbv_2 wet400-list), BFI 0.08 (Hbv_1_1p wet400-list).  (b) worst per-basin error / bound 1.4e-3 (Hbv wet1).  Float64
forward AD on the host: up to 2.4 s per problem (Hbv wet400, with the first primal), 0.8 s for wet1460; the module
12.4 s.
"""
import types

import numpy as np
import pytest
import torch

from hydrodl2_amd import ops

from . import abi_util as au
from . import daily_jvp_util as du
from . import hourly_jvp_util as hu
from .test_jvp_f64_gpu import BFI_TERM_REL
from .test_jvp_gpu import TAN_ATOL_REL, _assert_tangent_close

pytestmark = pytest.mark.gpu

BIT_PROBLEMS = [(m, n) for m in du.TAN_PROBLEMS for n in ("wet400", "wet2" if m == "Hbv_1_1p" else "wet2-all-drop",
                                                          "wet65-channels")]
_RUNS = {}
_WANT = {}


def _primal(model, name):
    """(problem, direction, run_problem result with gradients, PathRecord), run once per session."""
    if (model, name) not in _RUNS:
        prob, dirs = du.problem(model, name)
        with ops.record_paths() as recs:
            res = au.run_problem(prob, None, device="cuda", x_grad=True)
        _RUNS[model, name] = (prob, dirs, res, recs[-1])
    return _RUNS[model, name]


def _stack(rec, dirs_list, key):
    if key not in dirs_list[0]:
        return None
    return torch.from_numpy(np.stack([d[key] for d in dirs_list])).to(rec.x.device)


def _tangent(prob, rec, dirs_list, mask=None, state=True):
    """hbvx_forward_tangent_batch (and, on a routing problem at the full mask, the routing and BFI tangents) on the
    recorded call along the directions of `dirs_list`: dict of numpy arrays with a leading direction axis."""
    full = (1 << rec.cfg.n_flux) - 1
    mask = full if mask is None else mask
    routing = prob["routing"] and mask == full
    res = ops.hbv_tangent_batch(rec, len(dirs_list), _stack(rec, dirs_list, "x"), _stack(rec, dirs_list, "muwts"),
                                _stack(rec, dirs_list, "state_in") if state else None, [_stack(rec, dirs_list, "params")],
                                flux_mask=mask, n_routed=4 if routing else 0, want_bfi=routing)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res._asdict().items() if v is not None}


def _one_direction(rec, dirs):
    """The one-direction entry point on the recorded call, as HbvPath.jvp calls it."""
    ctx = types.SimpleNamespace(cfg=rec.cfg, has_bfi=rec.routed is not None, state_tangent=True,
                                saved_tensors=(rec.x, rec.state_in, rec.muwts, rec.ac, rec.elev, rec.flux, rec.uh,
                                               rec.routed) + tuple(rec.ptensors))
    dev = rec.x.device
    t = {k: torch.from_numpy(v).to(dev) for k, v in dirs.items()}
    out = ops._hbv_tangent(ctx, t["x"], t["state_in"], t.get("muwts"), None, None, [t["params"]])
    torch.cuda.synchronize()
    nr = 4 if rec.routed is not None else 0
    res = {"state_out": out[0].cpu().numpy(), "flux": torch.stack([r[..., 0] for r in out[4 + nr:]]).cpu().numpy()}
    if nr:
        res.update(bfi=out[3].cpu().numpy(), routed=torch.stack([r[..., 0] for r in out[4:4 + nr]]).cpu().numpy())
    return res


def _want(model, name):
    if (model, name) not in _WANT:
        prob, dirs = du.problem(model, name)
        _WANT[model, name] = du.abi_forward_ad(prob, dirs)
    return _WANT[model, name]


@pytest.mark.parametrize("model,name", du.ALL, ids=du.IDS)
def test_tangents_against_float64(model, name, hip_backend):
    prob, dirs, _, rec = _primal(model, name)
    got = _tangent(prob, rec, [dirs])
    want = _want(model, name)
    f32 = {}

    def alt(k):
        def f():
            if not f32:
                f32.update(du.abi_forward_ad(prob, dirs, torch.float32))
            return f32[k]
        return f
    bad = []          # every array is compared before anything is raised
    for k in ("flux", "state_out", "routed"):
        if k in want:
            err = np.abs(got[k][0] - want[k])
            tol = hu.tan_tol(max(float(np.abs(want[k]).max()), 1e-300))(want[k])
            au.REPORT.append((f"daily-tan:{model}:{name}:{k}", float(err.max()), float((err / tol).max()),
                              int((err > tol).sum()), err.size))
            try:
                hu.compare(f"daily-tan:{model}:{name}:{k}", got[k][0], want[k], alt(k))
            except AssertionError as e:
                bad.append(str(e))
    if "bfi" in want:
        scale = max(float(np.abs(want["bfi"]).max()), 1e-30) + (BFI_TERM_REL / TAN_ATOL_REL) * want["bfi_terms"]
        try:
            _assert_tangent_close(f"daily-tan:{model}:{name}:bfi", got["bfi"][0], want["bfi"], scale=scale)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, " | ".join(bad)


@pytest.mark.parametrize("model,name", du.ALL, ids=du.IDS)
def test_per_basin_transpose_identity_against_backward(model, name, hip_backend):
    prob, dirs, res, rec = _primal(model, name)
    B = prob["B"]
    tan = _tangent(prob, rec, [dirs], state=False)
    pairs = [(prob["gflux"], tan["flux"][0])] + ([(prob["grouted"], tan["routed"][0])] if prob["routing"] else [])
    lhs, nw, njv = np.zeros(B), np.zeros(B), np.zeros(B)
    for w, jv in pairs:
        w, jv = w.astype(np.float64), jv.astype(np.float64)
        lhs += (w * jv).sum((0, 1))
        nw += (w ** 2).sum((0, 1))
        njv += (jv ** 2).sum((0, 1))
    rhs = (res["g_params"].astype(np.float64) * dirs["params"]).sum((0, 2))
    rhs += (res["g_x"].astype(np.float64) * dirs["x"]).sum((0, 2))
    if "muwts" in prob:
        rhs += (res["g_muwts"].astype(np.float64) * dirs["muwts"]).sum((0, 2))
    prod = np.sqrt(nw * njv)
    tol = 1e-4 * prod + 1e-7 * prod.max()
    err = np.abs(lhs - rhs)
    au.REPORT.append((f"daily-tan-dot-basin:{model}:{name}", float(err.max()), float((err / tol).max()),
                      int((err > tol).sum()), B))
    print(f"{model} {name}: worst per-basin |<w,Jv> - <J^T w,v>| / tolerance {float((err / tol).max()):.3g}")
    bad = np.nonzero(err > tol)[0]
    assert bad.size == 0, (model, name, bad[:5], lhs[bad[:5]], rhs[bad[:5]], tol[bad[:5]])


@pytest.mark.parametrize("model,name", BIT_PROBLEMS, ids=[f"{m}-{n}" for m, n in BIT_PROBLEMS])
def test_directions_masks_and_the_one_direction_kernel_are_bit_identical(model, name, hip_backend):
    prob, _, _, rec = _primal(model, name)
    five = [hu.abi_directions(prob, seed=31 + d) for d in range(5)]
    all5 = _tangent(prob, rec, five)
    for d in (0, 3, 4):
        one = _tangent(prob, rec, [five[d]])
        assert set(one) == set(all5)
        for k in one:
            assert np.array_equal(all5[k][d], one[k][0]), (model, name, d, k)
    rows = (0, 5, 10)
    sel = _tangent(prob, rec, five, mask=sum(1 << k for k in rows))
    assert sel["flux"].shape[1] == 3
    for i, k in enumerate(rows):
        assert np.array_equal(sel["flux"][:, i], all5["flux"][:, k]), (model, name, k)
    assert np.array_equal(sel["state_out"], all5["state_out"])
    single = _one_direction(rec, five[0])
    assert set(single) == set(all5)
    for k in single:
        assert np.array_equal(single[k], all5[k][0]), (model, name, "one-direction entry point", k)
