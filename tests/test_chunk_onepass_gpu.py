"""GPU tier: the one-pass static adjoint (hbv_chunked.h, k_bwd_chunk_onepass + k_bwd_chunk_fold + k_bwd_chunk_reduce)
against the two-pass form (k_bwd_chunk_phi / k_bwd_chunk_sweep / k_bwd_chunk_reduce) that HBVX_CHUNK_ONEPASS=0 forces,
in the same process on the same inputs.  Both forms run the same a-propagation, so the forward, the trajectory and the
adjoint entering the record are identical; the static-parameter gradients are the same sums in another association
and must agree within tests/abi_util.py's gradient tolerances.  Each case asserts which form ran (hbvx_chunk_form)."""
import ctypes as C

import numpy as np
import pytest
import torch

from hydrodl2_amd import _abi
from hydrodl2_amd.ops import ParamSource, RouteSource, StepConfig, hbv_path
from tests import seam

from .abi_util import BOUNDS, MODEL_ID, assert_grad_close, column_groups, make_problem

pytestmark = pytest.mark.gpu


def _form(lib) -> int:
    f = lib.dll.hbvx_chunk_form
    f.restype = C.c_int
    return f()


def _run(prob, rows):
    """Forward + backward of `prob` on cuda:0 with the loss on the flux rows `rows` (and the routed series);
    returns (parameter gradient, state gradient at the start)."""
    seam.use_library(None)
    dev = torch.device("cuda:0")
    T, B, M, n, ny = prob["T"], prob["B"], prob["M"], prob["n"], prob["ny"]
    x = torch.from_numpy(prob["x"]).to(dev)
    p = torch.from_numpy(prob["params"]).to(dev).requires_grad_(True)
    srcs = []
    for i, name in enumerate(prob["names"]):
        lo, hi = BOUNDS[name]
        srcs.append(ParamSource(slot=_abi.PARAM_SLOTS.index(name), lo=float(lo), hi=float(hi), tensor_idx=0,
                                sta_off=(T - 1) * B * ny + i * M, sta_bs=ny))
    cfg = StepConfig(model=MODEL_ID[prob["model"]], n_param=n, n_flux=11, T=T, t0=0, B=B, ckpt_days=0, M=M,
                     raw_sigmoid=True, channels=(0, 1, 2), nearzero=1e-5, params=srcs)
    off = (T - 1) * B * ny + n * M
    cfg.route = RouteSource(0, off, off + 1, ny, [0, 2.9], [0, 6.5])
    po = hbv_path(cfg, x, None, None, None, None, p)
    gf = torch.from_numpy(prob["gflux"]).to(dev)
    loss = sum((po.flux[k][..., 0] * gf[k]).sum() for k in rows)
    loss = loss + (torch.stack([r[..., 0] for r in po.routed]) * torch.from_numpy(prob["grouted"]).to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return p.grad.cpu().numpy()


CASES = [(T, B, M, chunk, betaet, rows) for T, B, M, chunk in [(1000, 37, 4, "16"), (730, 53, 16, None)]
         for betaet in (False, True) for rows in ("streamflow", "all")]
# the headline shape (bench.py cfg2: 671 basins x 16 members x 7300 days), once per loss form
CASES += [(7300, 671, 16, None, False, "streamflow"), (7300, 671, 16, None, True, "all")]


@pytest.mark.parametrize("T,B,M,chunk,betaet,rows", CASES)
def test_onepass_matches_two_pass(T, B, M, chunk, betaet, rows, hip_backend, monkeypatch):
    if chunk:
        monkeypatch.setenv("HBVX_CHUNK", chunk)       # (1000 days in 16-day chunks: the last one is ragged)
    prob = make_problem(model="Hbv", T=T, B=B, M=M, betaet=betaet, seed=45)
    rws = (0,) if rows == "streamflow" else tuple(range(11))
    monkeypatch.setenv("HBVX_CHUNK_ONEPASS", "0")
    b = _run(prob, rws)
    assert hip_backend.last_dispatch(1) == "chunked" and _form(hip_backend) == 2
    monkeypatch.delenv("HBVX_CHUNK_ONEPASS")
    a = _run(prob, rws)
    assert hip_backend.last_dispatch(1) == "chunked" and _form(hip_backend) == 1
    assert np.isfinite(a).all()
    assert_grad_close("g_params", a, b, column_groups(prob["ny"], M))
