"""GPU tier: k_bwd_chunk_fold (hbv_chunked.h) keeps the bits of the static-parameter gradient.  The fold sums, per
parameter and group of four chunk maps, G_c a_c + g0_c over the group's chunks in ascending c, each term from g0 with
`v += G[k] * a[k]` in ascending k, in float64; its loads may be regrouped (two chunks' rows in registers before the
first multiply), its sums may not.

At 1460 days x 16 basins x 16 members (23 chunks, 6 groups: the shape tests/test_chunk_onepass_group_gpu.py holds to
float64), with the streamflow loss and the all-series loss, the static row of the parameter gradient must have the
bits recorded in tests/golden/chunk_fold_static_grad.npz -- the gradients of the build before the loads were regrouped,
which that test's tolerances pin.  No tolerance: every kernel on this path sums in a fixed order."""
import numpy as np
import pytest

from . import golden_cases as gc
from . import synth
from .helpers import load_golden
from .test_chunk_onepass_gpu import _form
from .test_chunk_onepass_group_gpu import B64, M64, SEED, T64, _gpu_grad, _group

pytestmark = pytest.mark.gpu


def static_grad(loss):
    ny = len(gc.PHY_NAMES["Hbv"]) * M64 + 2
    x, p = synth.forcing(T64, B64, SEED), synth.raw_parameters(T64, B64, ny, SEED)
    keys = ["streamflow"] if loss == "streamflow" else gc.flux_keys("Hbv")
    return _gpu_grad(x, p, keys)[-1].astype(np.float32)        # (float32 -> float64 -> float32: exact)


@pytest.mark.parametrize("loss", ["streamflow", "all"])
def test_fold_keeps_the_recorded_bits(loss, hip_backend):
    got = static_grad(loss)
    assert hip_backend.last_dispatch(1) == "chunked" and _form(hip_backend) == 1 and _group(hip_backend) == 4
    want = load_golden("chunk_fold_static_grad")[loss]
    assert got.shape == want.shape and want.dtype == np.float32
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), (f"{int(diff.sum())} of {diff.size} elements differ in bits; largest difference "
                            f"{np.abs(got.astype(np.float64) - want).max():.3e} on a largest element of {np.abs(want).max():.3e}")
