"""GPU tier: the pipelined forward (hbv_pipe.h) on eleven-day static tiles, with the soil stage's output tile at five
rows per day (six with the capillary flux) instead of seven (eight): the two saved-power rows are gone, no build
keeps them.  The arithmetic is Step::fwd_* in day order, so the kernel must equal the tiled family, which
HBVX_FWD=tiled forces, bit for bit: all fluxes, the final storages and every trajectory row.

Shapes: T = 44 (four whole tiles, the shortest record the pipeline takes), 45 (a one-day tail), 54 (a ten-day tail),
131 (a long record, ten-day tail); B = 5, so the second workgroup of a 16-member run holds one basin of four and its
other lanes are inactive; M = 16 (trajectory through LDS and the drainer waves) and 4 (the stepper waves store it).
Once for Hbv_1_1p -- the two-stage pipeline, six rows -- and once for Hbv with {parBETA, parBETAET} dynamic: those
keep their eight-day tiles, but their soil tile has the new row count too."""
import numpy as np
import pytest

from .abi_util import make_problem, run_problem

pytestmark = pytest.mark.gpu

KEYS = ("flux", "routed", "state_out", "traj")


def _both(prob, hip_backend, monkeypatch):
    a = run_problem(prob, None, device="cuda:0", backward=True)
    assert hip_backend.last_dispatch(0) == "pipe"
    monkeypatch.setenv("HBVX_FWD", "tiled")
    b = run_problem(prob, None, device="cuda:0", backward=True)
    assert hip_backend.last_dispatch(0) == "tiled"
    return a, b


def _assert_same_bits(prob, a, b):
    assert a["flux"].shape[0] == (11 if prob["model"] == "Hbv" else 12)
    assert a["traj"].shape == (5, prob["T"] + 1, prob["B"] * prob["M"])
    for k in KEYS:
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), \
            (k, int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum()))


@pytest.mark.parametrize("M", [16, 4])
@pytest.mark.parametrize("T", [44, 45, 54, 131])
def test_static_eleven_day_tiles_equal_the_tiled_forward(T, M, hip_backend, monkeypatch):
    prob = make_problem(model="Hbv", T=T, B=5, M=M, seed=61)
    a, b = _both(prob, hip_backend, monkeypatch)
    _assert_same_bits(prob, a, b)


def test_below_four_tiles_the_tiled_forward_runs(hip_backend):
    prob = make_problem(model="Hbv", T=43, B=5, M=16, seed=61)
    run_problem(prob, None, device="cuda:0", backward=False)
    assert hip_backend.last_dispatch(0) == "tiled"


def test_two_stage_pipeline_with_six_rows(hip_backend, monkeypatch):
    prob = make_problem(model="Hbv_1_1p", T=54, B=5, M=16, seed=62)
    a, b = _both(prob, hip_backend, monkeypatch)
    _assert_same_bits(prob, a, b)


def test_dynamic_pair_on_eight_day_tiles_with_five_rows(hip_backend, monkeypatch):
    prob = make_problem(model="Hbv", T=45, B=5, M=16, dyn=("parBETA", "parBETAET"), seed=63)
    a, b = _both(prob, hip_backend, monkeypatch)
    _assert_same_bits(prob, a, b)
