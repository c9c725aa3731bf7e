"""CPU tier: the kernels of include/hbvx_gage_fdc.h (hydrodl2_amd/csrc/hbv_gage_pop.h) in the BUILT library's gfx950 code
objects, resources only (tools/kernel_resources.py; no GPU needed).  k_gp_fdc keeps threshold, count and volume of its
block of eight levels in registers: no scratch, no spill, no LDS, and eight waves per SIMD by registers.  k_gp_quant's
column is DYNAMIC LDS sized by the call's T, so its static LDS is zero too -- at the cap the column alone is the 64 KB a
launch may ask for -- and the transpose k_gp_keys has its one 32 x 33 tile."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "hydrodl2_amd", "csrc", "libhbvx.so")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        pytest.skip("libhbvx.so not built")
    import kernel_resources
    return {r["name"].split("(")[0]: r for r in kernel_resources.kernel_table(LIB) if "gagepop::k_gp_" in r["name"]}


def test_the_kernels_exist_without_scratch_or_spill(kernels):
    for name in ("gagepop::k_gp_fdc", "gagepop::k_gp_quant", "gagepop::k_gp_keys"):
        r = kernels.get(name)
        assert r is not None, (name, sorted(kernels))
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        assert r["agpr"] == 0 and r["waves_per_simd"] == 8, r


def test_their_lds_and_workgroups(kernels):
    fdc, quant, keys = (kernels["gagepop::k_gp_" + k] for k in ("fdc", "quant", "keys"))
    assert fdc["lds"] == 0 and fdc["max_threads"] == 64 and fdc["vgpr"] <= 64, fdc
    assert quant["lds"] == 0 and quant["max_threads"] == 256, quant         # the column is dynamic LDS
    assert keys["lds"] == 32 * 33 * 4 and keys["max_threads"] == 256, keys
    # the neighbours this file's kernels stand between are there as before
    assert "gagepop::k_gp_events" in kernels and "gagepop::k_gp_route" in kernels
