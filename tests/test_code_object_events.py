"""CPU tier: the event form of k_pop (hydrodl2_amd/csrc/hbv_pop.h) in the BUILT library's gfx950 code objects, resources
only (tools/kernel_resources.py; no GPU needed): an instance per model and transform, three waves per SIMD by registers
for HBV 1.0 / 1.1p as in the stats form (HBV 2.0 has two there and keeps two), no scratch and no spill anywhere, and no
LDS -- the cursor and the slot are six registers, and a row is addressed with a 32-bit offset from a scalar base precisely
so that no per-lane 64-bit address is carried through the day loop."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "hydrodl2_amd", "csrc", "libhbvx.so")

# k_pop<MODEL, BETAET, TR, PopEventArgs>: HBV 1.0 with and without parBETAET, 1.1p, 2.0
MODELS = {"hbv10": "0, false", "hbv10-betaet": "0, true", "hbv11p": "1, true", "hbv20": "2, true"}


@pytest.fixture(scope="module")
def instances():
    if not os.path.exists(LIB):
        pytest.skip("libhbvx.so not built")
    import kernel_resources
    return {r["name"].split("(")[0]: r for r in kernel_resources.kernel_table(LIB) if "PopEventArgs" in r["name"]}


def test_the_instances_exist_and_keep_their_occupancy(instances):
    assert len(instances) == 12, sorted(instances)
    for model, head in MODELS.items():
        for tr in (0, 1, 2):
            r = instances.get(f"void k_pop<{head}, {tr}, PopEventArgs>")
            assert r is not None, (model, tr)
            # (scalar registers that overflow go to VGPR lanes, not to memory -- tests/test_code_object.py -- as in the
            # stats form; scratch == 0 says that nothing of either kind reaches memory)
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (model, tr, r)
            assert r["agpr"] == 0 and r["max_threads"] == 64, (model, tr, r)
            assert r["lds"] == 0, (model, tr, r)
            assert r["waves_per_simd"] >= (2 if model == "hbv20" else 3), (model, tr, r["vgpr"])
