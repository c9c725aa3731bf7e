"""GPU tier: the library neither reads nor writes `aux` (include/hbvx.h, hbvx_fwd_out.aux / hbvx_bwd_io.aux).

Until ABI 8 the forward saved the two pre-clamp powers of every lane-day there and the adjoint read them back; since
ABI 9 the adjoint recomputes them and the pointer is documented as ignored.  This pins that promise for every kernel
family: each case runs once as the package calls the library (aux NULL) and once with `forward` / `backward` /
`backward_live` interposed so that out.aux / io.aux point at one device buffer [2, T, B*M] filled with a NaN bit
pattern.  A kernel that read the buffer would carry the NaN into an output; one that wrote it would break the pattern.
Every returned array must be equal bit for bit between the two runs and the buffer untouched.  With K-day checkpoints
(HBVX_TRAJ_CKPT) the interposer leaves aux NULL: that forward refuses anything else ("checkpoints: aux must be NULL").

The methods are replaced on the Library class, not on one handle: run_problem reloads the handle (tests/seam.py).

Shapes: T = 131 (two 64-day chunks and a ragged third for the time-parallel adjoint, at least four tiles of the
pipelined forward, the last one short), B = 9, M = 16 (four basins per wave: the third wave holds one)."""
import numpy as np
import pytest
import torch

from hydrodl2_amd import _abi

from .abi_util import make_problem, run_problem
from .test_chunk_onepass_gpu import _form

pytestmark = pytest.mark.gpu

T, B, M = 131, 9, 16
SENTINEL = 0x7FC0BEEF      # a quiet NaN with a payload no arithmetic produces
KEYS = ("flux", "routed", "state_out", "traj", "g_params", "g_x")

# id: (make_problem arguments, environment, x_grad, (forward, adjoint) of hbvx_last_dispatch, chunk form or None)
CASES = {
    # the one-pass static adjoint takes no call with a forcing gradient (launch_chunked.hip): the case as the package's
    # training step makes it, and once with the forcing gradient so that g_x is compared on the static model too
    "static-onepass": (dict(model="Hbv"), {}, False, ("pipe", "chunked"), 1),
    "static-xgrad": (dict(model="Hbv"), {}, True, ("pipe", "chunked"), None),
    "static-twopass": (dict(model="Hbv"), {"HBVX_CHUNK_ONEPASS": "0"}, True, ("pipe", "chunked"), 2),
    "tiled": (dict(model="Hbv_1_1p", dyn=("parBETA",)), {"HBVX_FWD": "tiled", "HBVX_BWD": "tiled"}, True,
              ("tiled", "tiled"), None),
    "stream2-packed": (dict(model="Hbv", dyn=("parBETA", "parBETAET")), {"HBVX_STREAM_MIN": "1"}, True,
                       ("stream2", "stream2"), None),
    "stream2-rows": (dict(model="Hbv", dyn=("parBETA", "parBETAET")), {"HBVX_STREAM_MIN": "1", "HBVX_BWD": "tiled"}, True,
                     ("stream2", "tiled"), None),
    # HBVX_KERNEL=simple pins the one-wave forward; a record of 128 days or more still takes the time-parallel adjoint,
    # so the one-wave adjoint needs that one switched off as well
    "simple": (dict(model="Hbv_2", dyn=("parFC",)), {"HBVX_KERNEL": "simple"}, True, ("simple", "chunked"), None),
    "simple-adjoint": (dict(model="Hbv_2", dyn=("parFC",)), {"HBVX_KERNEL": "simple", "HBVX_BWD": "tiled"}, True,
                       ("simple", "simple"), None),
    # block-wise re-materialisation: 64-day blocks (8 K), each below the time-parallel adjoint's 128 days
    "ckpt-block": (dict(model="Hbv", dyn=("parBETA",)), {"HBVX_CKPT_DAYS": "8", "HBVX_CKPT_BLOCK": "16"}, True,
                   ("pipe", "ckpt-block:tiled"), None),
}


def _interpose(monkeypatch, buf, calls):
    """Library.forward / backward / backward_live hand the real call a non-NULL aux (not with checkpoints)."""
    real = {k: getattr(_abi.Library, k) for k in ("forward", "backward", "backward_live")}

    def point(name, st):
        calls.append(name)
        if (st.traj_layout & 0xFF) != _abi.TRAJ_CKPT:
            st.aux = buf.data_ptr()

    def forward(self, desc, out, stream):
        point("forward", out)
        return real["forward"](self, desc, out, stream)

    def backward(self, desc, io, stream):
        point("backward", io)
        return real["backward"](self, desc, io, stream)

    def backward_live(self, desc, io, n_live4, stream):
        point("backward_live", io)
        return real["backward_live"](self, desc, io, n_live4, stream)

    monkeypatch.setattr(_abi.Library, "forward", forward)
    monkeypatch.setattr(_abi.Library, "backward", backward)
    monkeypatch.setattr(_abi.Library, "backward_live", backward_live)


@pytest.mark.parametrize("case", list(CASES))
def test_a_non_null_aux_is_neither_read_nor_written(case, hip_backend, monkeypatch):
    kw, env, x_grad, want_dispatch, want_form = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = make_problem(T=T, B=B, M=M, seed=29, **kw)

    def run():
        res = run_problem(prob, None, device="cuda:0", x_grad=x_grad)
        assert (hip_backend.last_dispatch(0), hip_backend.last_dispatch(1)) == want_dispatch
        if want_form is not None:
            assert _form(hip_backend) == want_form
        return res

    plain = run()
    buf = torch.full((2, T, B * M), SENTINEL, dtype=torch.int32, device="cuda:0")
    calls = []
    with monkeypatch.context() as m:
        _interpose(m, buf, calls)
        poked = run()
    assert "forward" in calls and ("backward" in calls or "backward_live" in calls), calls

    ckpt = "HBVX_CKPT_DAYS" in env      # (run_problem does not return the checkpoints)
    want_keys = {k for k in KEYS if not (k == "traj" and ckpt) and not (k == "g_x" and not x_grad)}
    assert set(plain) == want_keys and set(poked) == want_keys
    for k in sorted(want_keys):
        a, b = np.ascontiguousarray(plain[k]), np.ascontiguousarray(poked[k])
        assert a.dtype == np.float32 and a.shape == b.shape, k
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{k}: a non-NULL aux moved bits"
    assert np.isfinite(plain["g_params"]).all() and np.abs(plain["g_params"]).max() > 0.0
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()), "the library wrote to aux"
