"""GPU tier: accuracy of the one-pass static adjoint against float64.  The one-pass form (hbv_chunked.h,
k_bwd_chunk_onepass + k_bwd_chunk_fold + k_bwd_chunk_reduce) sums a static gradient in another association than the
two-pass form: per chunk G_c a_c + g0_c, where G_c and g0_c accumulate the whole chunk before the incoming adjoint
multiplies them, instead of day by day from the true adjoint.  Both forms run the drop-in Hbv module on the same float32
inputs in one process (HBVX_CHUNK_ONEPASS=0 forces the two-pass form), and oracle/hbv_restate64.py evaluates the same
loss in float64 on the host.  For every parameter group (the members of one parameter, each routing column) the
one-pass form's rms error against float64 must not exceed twice the two-pass form's.

The largest single error of a group is printed but not bounded.  On that measure, with the streamflow loss, parPERC
reaches 2.2 x (4.3e-7 against 2.0e-7, on a group maximum of 0.93) and parUZL 1.9 x.  These are the groundwater
parameters, whose per-day terms (aPERC = SLZ share - SUZ share) cancel.  The one-pass form sums them per unit vector
over the whole chunk in float32, before the incoming adjoint weights them.  Both errors are 5e-7 of the group's
largest, a quarter of the suite's gradient tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import golden_cases as gc
from . import restate_util as ru
from . import synth
from .abi_util import column_groups

pytestmark = pytest.mark.gpu

T, B, M, SEED = 730, 32, 16, 47


def _form(lib) -> int:
    f = lib.dll.hbvx_chunk_form
    f.restype = C.c_int
    return f()


def _inputs(loss):
    names = gc.PHY_NAMES["Hbv"]
    ny = len(names) * M + 2
    x = synth.forcing(T, B, SEED)
    p = synth.raw_parameters(T, B, ny, SEED)
    keys = ["streamflow"] if loss == "streamflow" else gc.flux_keys("Hbv")
    return x, p, keys, ny


def _weights(keys, out):
    return {k: synth.loss_weights(tuple(out[k].shape), SEED, 20 + i) for i, k in enumerate(keys)}


def _gpu_grad(x, p, keys):
    import hydrodl2_amd
    dev = torch.device("cuda:0")
    cls = hydrodl2_amd.load_model("hbv", "Hbv")
    model = cls(gc._cfg("Hbv", M), dev)
    pt = torch.from_numpy(p).to(dev).requires_grad_(True)
    out = model({"x_phy": torch.from_numpy(x).to(dev)}, pt)
    w = _weights(keys, out)
    loss = sum((torch.from_numpy(w[k]).to(dev) * out[k]).sum() for k in keys)
    loss.backward()
    torch.cuda.synchronize()
    return pt.grad.double().cpu().numpy()


def _f64_grad(x, p, keys):
    x64 = torch.from_numpy(x).double()
    p64 = torch.from_numpy(p).double().requires_grad_(True)
    out, _ = ru.restate().run("Hbv", x64, p64, **ru.config_kwargs("Hbv", gc._cfg("Hbv", M)))
    w = _weights(keys, out)
    loss = sum((torch.from_numpy(w[k]).double() * out[k]).sum() for k in keys)
    loss.backward()
    return p64.grad.numpy()


@pytest.mark.parametrize("loss", ["streamflow", "all"])
def test_onepass_loses_no_accuracy_against_float64(loss, hip_backend, monkeypatch):
    x, p, keys, ny = _inputs(loss)
    monkeypatch.setenv("HBVX_CHUNK_ONEPASS", "0")
    g_two = _gpu_grad(x, p, keys)
    assert hip_backend.last_dispatch(1) == "chunked" and _form(hip_backend) == 2
    monkeypatch.delenv("HBVX_CHUNK_ONEPASS")
    g_one = _gpu_grad(x, p, keys)
    assert hip_backend.last_dispatch(1) == "chunked" and _form(hip_backend) == 1
    g64 = _f64_grad(x, p, keys)
    # every parameter is static: its gradient sits in row T-1 (the rows above are zero in all three)
    assert not g_one[:-1].any() and not g_two[:-1].any()
    groups = column_groups(ny, M)
    lines, bad = [], []
    for gid in np.unique(groups):
        cols = groups == gid
        ref = g64[-1, :, cols]
        d1, d2 = g_one[-1, :, cols] - ref, g_two[-1, :, cols] - ref
        r1, r2 = float(np.sqrt((d1 ** 2).mean())), float(np.sqrt((d2 ** 2).mean()))
        m1, m2 = float(np.abs(d1).max()), float(np.abs(d2).max())
        top = float(np.abs(ref).max())
        lines.append(f"group {gid:3d}: max|g64| {top:.3e}  rms error one-pass {r1:.3e} two-pass {r2:.3e}  "
                     f"max error one-pass {m1:.3e} two-pass {m2:.3e}")
        # the bound on the group's rms error (a floor of 1e-9 of the group's largest only for a group the two-pass
        # form gets exactly right); the largest single error is printed, not bounded: see the module docstring
        if not r1 <= 2.0 * r2 + 1e-9 * top:
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, bad
