"""GPU tier: the grouped one-pass static adjoint (hbv_chunked.h: k_bwd_chunk_onepass as a workgroup of G waves whose
chunks' maps are composed on chip, one map per group for the scan and the fold) against the two-pass form that
HBVX_CHUNK_ONEPASS=0 forces, in the same process on the same inputs, with the harness and tolerances of
tests/test_chunk_onepass_gpu.py.  HBVX_ONEPASS_GROUP sets the group size; every case asserts the form and the group
size that ran (hbvx_chunk_form, hbvx_onepass_group).  The shapes are the smallest at which the grouping can go wrong:

  a  130 x 5 x 16, 64-day chunks: 3 chunks (64, 64, 2 days) -- one group smaller than the group size, a two-day chunk,
     a second wave of lanes with one basin of four
  b  256 x 37 x 4, 16-day chunks: 16 chunks, 4 full groups; 16 basins per wave, the last wave partly empty
  c  1000 x 37 x 4, 16-day chunks: 63 chunks, the last of 8 days -- 15 groups and one of 3
  d  300 x 1 x 16, 16-day chunks: a single basin

each with parBETAET off and on, with the streamflow loss and the all-series loss, at group sizes 1, 2 and 4.  The
two-pass gradient of a (shape, parBETAET, loss) is computed once and shared.

Accuracy against float64 at 1460 x 16 x 16 (23 chunks, 6 groups of 4): for every parameter group the rms error of the
grouped form (group size 4) must be at most 2 x the two-pass form's, as in tests/test_chunk_onepass_f64_gpu.py; where
the ungrouped form (group size 1) already exceeds that bound at this shape, the grouped form is held to 1.25 x the
ungrouped form's rms error instead -- the composition adds one float32 rounding per stored row to the 64-day float32
sums that dominate.  The per-group figures of all three forms are printed (profiles/r15_onepass_group.md has them)."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import golden_cases as gc
from . import restate_util as ru
from . import synth
from .abi_util import assert_grad_close, column_groups, make_problem
from .test_chunk_onepass_gpu import _form, _run

pytestmark = pytest.mark.gpu


def _group(lib) -> int:
    f = lib.dll.hbvx_onepass_group
    f.restype = C.c_int
    return f()


SHAPES = {"a": (130, 5, 16, None), "b": (256, 37, 4, "16"), "c": (1000, 37, 4, "16"), "d": (300, 1, 16, "16")}
_two_pass = {}


def _problem_and_reference(case, betaet, rows, hip_backend, monkeypatch):
    T, B, M, chunk = SHAPES[case]
    if chunk:
        monkeypatch.setenv("HBVX_CHUNK", chunk)
    prob = make_problem(model="Hbv", T=T, B=B, M=M, betaet=betaet, seed=45)
    rws = (0,) if rows == "streamflow" else tuple(range(11))
    key = (case, betaet, rows)
    if key not in _two_pass:
        monkeypatch.setenv("HBVX_CHUNK_ONEPASS", "0")
        ref = _run(prob, rws)
        assert hip_backend.last_dispatch(1) == "chunked" and _form(hip_backend) == 2
        monkeypatch.delenv("HBVX_CHUNK_ONEPASS")
        ref.setflags(write=False)
        _two_pass[key] = ref
    return prob, rws, _two_pass[key]


@pytest.mark.parametrize("group", [1, 2, 4])
@pytest.mark.parametrize("rows", ["streamflow", "all"])
@pytest.mark.parametrize("betaet", [False, True])
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_grouped_onepass_matches_two_pass(case, betaet, rows, group, hip_backend, monkeypatch):
    prob, rws, ref = _problem_and_reference(case, betaet, rows, hip_backend, monkeypatch)
    monkeypatch.setenv("HBVX_ONEPASS_GROUP", str(group))
    got = _run(prob, rws)
    assert hip_backend.last_dispatch(1) == "chunked" and _form(hip_backend) == 1
    assert _group(hip_backend) == group
    assert np.isfinite(got).all()
    assert_grad_close("g_params", got, ref, column_groups(prob["ny"], prob["M"]))


# ---- accuracy against float64 ------------------------------------------------------------------------------------
T64, B64, M64, SEED = 1460, 16, 16, 47


def _gpu_grad(x, p, keys):
    import hydrodl2_amd
    dev = torch.device("cuda:0")
    model = hydrodl2_amd.load_model("hbv", "Hbv")(gc._cfg("Hbv", M64), dev)
    pt = torch.from_numpy(p).to(dev).requires_grad_(True)
    out = model({"x_phy": torch.from_numpy(x).to(dev)}, pt)
    loss = sum((torch.from_numpy(synth.loss_weights(tuple(out[k].shape), SEED, 20 + i)).to(dev) * out[k]).sum()
               for i, k in enumerate(keys))
    loss.backward()
    torch.cuda.synchronize()
    return pt.grad.double().cpu().numpy()


def _f64_grad(x, p, keys):
    p64 = torch.from_numpy(p).double().requires_grad_(True)
    out, _ = ru.restate().run("Hbv", torch.from_numpy(x).double(), p64, **ru.config_kwargs("Hbv", gc._cfg("Hbv", M64)))
    loss = sum((torch.from_numpy(synth.loss_weights(tuple(out[k].shape), SEED, 20 + i)).double() * out[k]).sum()
               for i, k in enumerate(keys))
    loss.backward()
    return p64.grad.numpy()


@pytest.mark.parametrize("loss", ["streamflow", "all"])
def test_grouping_loses_no_accuracy_against_float64(loss, hip_backend, monkeypatch):
    ny = len(gc.PHY_NAMES["Hbv"]) * M64 + 2
    x, p = synth.forcing(T64, B64, SEED), synth.raw_parameters(T64, B64, ny, SEED)
    keys = ["streamflow"] if loss == "streamflow" else gc.flux_keys("Hbv")
    monkeypatch.setenv("HBVX_CHUNK_ONEPASS", "0")
    g_two = _gpu_grad(x, p, keys)
    assert hip_backend.last_dispatch(1) == "chunked" and _form(hip_backend) == 2
    monkeypatch.delenv("HBVX_CHUNK_ONEPASS")
    g_by = {}
    for group in (1, 4):
        monkeypatch.setenv("HBVX_ONEPASS_GROUP", str(group))
        g_by[group] = _gpu_grad(x, p, keys)
        assert hip_backend.last_dispatch(1) == "chunked" and _form(hip_backend) == 1 and _group(hip_backend) == group
    g64 = _f64_grad(x, p, keys)
    groups = column_groups(ny, M64)
    lines, bad = [], []
    for gid in np.unique(groups):
        cols = groups == gid
        ref = g64[-1, :, cols]
        r2, r1, r4 = (float(np.sqrt(((g[-1, :, cols] - ref) ** 2).mean())) for g in (g_two, g_by[1], g_by[4]))
        top = float(np.abs(ref).max())
        # 2 x the two-pass form's rms error; where the ungrouped form is already past that, 1.25 x the ungrouped form's.
        # (A floor of 1e-9 of the group's largest only for a group the two-pass form gets exactly right.)
        ungrouped_within = r1 <= 2.0 * r2
        bound = (2.0 * r2 if ungrouped_within else 1.25 * r1) + (1e-9 * top if r2 == 0.0 else 0.0)
        lines.append(f"{loss} group {gid:3d}: max|g64| {top:.3e}  rms error two-pass {r2:.3e} ungrouped {r1:.3e} "
                     f"({r1 / max(r2, 1e-300):.2f} x) grouped {r4:.3e} ({r4 / max(r2, 1e-300):.2f} x two-pass, "
                     f"{r4 / max(r1, 1e-300):.2f} x ungrouped)  bound {'2 x two-pass' if ungrouped_within else '1.25 x ungrouped'}")
        if not r4 <= bound:
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, bad
