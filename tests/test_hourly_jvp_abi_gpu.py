"""GPU tier: hbvx_hourly_tangent_batch (k_tan<MODEL_HOURLY, true, TanBatchArgs> around Step<MODEL_HOURLY>::tan) at the
level of the C ABI against forward AD of oracle/hbv_restate64.py's pbm_hourly in float64, on problems of
tests/hourly_sets.py whose wet branches are taken: all twelve series and tan_state_out at TAN_RTOL + TAN_ATOL_REL x
max|float64 tangent of the series| under hourly_sets.admit (an element outside tolerance is admitted only where it
agrees with the restatement run in float32; at most ADMIT_CAP of an array).  On the same problems: the per-basin
transpose identity against hbvx_backward's gradients, direction d of a D = 5 call bit-identical to D = 1, and a mask of
rows {0, 5, 10} bit-identical to those rows of the full mask."""
import numpy as np
import pytest
import torch

from hydrodl2_amd import ops

from . import abi_util as au
from . import hourly_jvp_util as hu
from . import hourly_sets as hs

pytestmark = pytest.mark.gpu

PROBLEMS = ("dry25", "wet24", "wet1", "wet2-all-drop", "wet65-channels", "wet64-m64", "wet129-muwts")
FULL = (1 << 12) - 1
_RUNS = {}


def _primal(name):
    """(problem, run_problem result with gradients, PathRecord) of the problem, run once per session."""
    if name not in _RUNS:
        prob = hu.with_explicit_start(hs.make(hs.ABI_PROBLEMS[name]))
        with ops.record_paths() as recs:
            res = au.run_problem(prob, None, device="cuda", x_grad=True)
        _RUNS[name] = (prob, res, recs[-1])
    return _RUNS[name]


def _tangent(rec, dirs_list, mask=FULL, state=True):
    """hbvx_hourly_tangent_batch on the recorded call along the directions of `dirs_list`: (flux [D,n_sel,T,B],
    state_out [D,5,B,M]) as numpy."""
    dev = rec.x.device

    def stack(key):
        if key not in dirs_list[0]:
            return None
        return torch.from_numpy(np.stack([d[key] for d in dirs_list])).to(dev)
    res = ops.hbv_tangent_batch(rec, len(dirs_list), stack("x"), stack("muwts"), stack("state_in") if state else None,
                                [stack("params")], flux_mask=mask)
    torch.cuda.synchronize()
    return res.flux.cpu().numpy(), res.state_out.cpu().numpy()


@pytest.mark.parametrize("name", PROBLEMS)
def test_series_and_state_tangents_against_float64(name, hip_backend):
    prob, _, rec = _primal(name)
    dirs = hu.abi_directions(prob)
    flux, state = _tangent(rec, [dirs])
    want = hu.abi_forward_ad(prob, dirs)
    f32 = {}

    def alt(k):
        def f():
            if not f32:
                f32.update(hu.abi_forward_ad(prob, dirs, torch.float32))
            return f32[k]
        return f
    hu.compare(f"hourly-tan:{name}:flux", flux[0], want["flux"], alt("flux"))
    hu.compare(f"hourly-tan:{name}:state_out", state[0], want["state_out"], alt("state_out"))


@pytest.mark.parametrize("name", PROBLEMS)
def test_per_basin_transpose_identity_against_backward(name, hip_backend):
    """<gflux_b, (J v)_b> == <(J^T gflux)_b, v_b> with a zero state_in tangent (run_problem's backward has no gradient
    for the storages carried in)."""
    prob, res, rec = _primal(name)
    B = prob["B"]
    dirs = hu.abi_directions(prob)
    flux, _ = _tangent(rec, [dirs], state=False)
    jv = flux[0].astype(np.float64)                       # [12,T,B]
    w = prob["gflux"].astype(np.float64)
    lhs = (w * jv).sum((0, 1))
    rhs = (res["g_params"].astype(np.float64) * dirs["params"]).sum((0, 2))
    rhs += (res["g_x"].astype(np.float64) * dirs["x"]).sum((0, 2))
    if "muwts" in prob:
        rhs += (res["g_muwts"].astype(np.float64) * dirs["muwts"]).sum((0, 2))
    prod = np.sqrt((w ** 2).sum((0, 1)) * (jv ** 2).sum((0, 1)))
    tol = 1e-4 * prod + 1e-7 * prod.max()
    err = np.abs(lhs - rhs)
    au.REPORT.append((f"hourly-tan-dot-basin:{name}", float(err.max()), float((err / tol).max()), int((err > tol).sum()), B))
    print(f"{name}: worst per-basin |<w,Jv> - <J^T w,v>| / tolerance {float((err / tol).max()):.3g}")
    bad = np.nonzero(err > tol)[0]
    assert bad.size == 0, (name, bad[:5], lhs[bad[:5]], rhs[bad[:5]], tol[bad[:5]])


@pytest.mark.parametrize("name", PROBLEMS)
def test_directions_and_masks_are_bit_identical(name, hip_backend):
    prob, _, rec = _primal(name)
    five = [hu.abi_directions(prob, seed=31 + d) for d in range(5)]
    flux5, state5 = _tangent(rec, five)
    for d in (0, 3, 4):
        flux1, state1 = _tangent(rec, [five[d]])
        assert np.array_equal(flux5[d], flux1[0]) and np.array_equal(state5[d], state1[0]), (name, d)
    rows = (0, 5, 10)
    sel, state_sel = _tangent(rec, five, mask=sum(1 << k for k in rows))
    assert sel.shape[1] == 3
    for i, k in enumerate(rows):
        assert np.array_equal(sel[:, i], flux5[:, k]), (name, k)
    assert np.array_equal(state_sel, state5)
