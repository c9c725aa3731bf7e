"""CPU tier: the built gfx950 code of the batched tangent-linear kernel (hbvx.hip, k_fwd_tan_batch<MODEL, BETAET, DL>).
Only DL = 1 is built (one direction per lane is what the measurements left, profiles/r07_jvp_batch.md): an instance
fits the register file of one wave (512 VGPRs), nothing spills (no scratch traffic in the day loop), and, since the
directions are resident waves beside each other, it keeps the one-direction kernel's occupancy.  The
one-direction kernel beside it keeps the figures of DESIGN.md §0 F1."""
import os
import re
import sys

import pytest

from .test_code_object import LIB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB):
        pytest.skip("libhbvx.so not built")
    import kernel_resources
    return {r["name"].split("(")[0]: r for r in kernel_resources.kernel_table(LIB)}


def test_batch_instances_do_not_spill_and_fit_one_wave(table):
    names = [n for n in table if "k_fwd_tan_batch<" in n]
    dls = sorted({int(re.search(r", (\d+)>$", n).group(1)) for n in names})
    assert dls == [1], names                            # the instances that lost the measurement are not shipped
    assert len(names) == 4, names                       # HBV 1.0 with and without parBETAET, 1.1p, 2.0
    for n in names:
        r = table[n]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (n, r)       # nothing goes to memory
        assert r["vgpr"] + r["agpr"] <= 512, (n, r["vgpr"], r["agpr"])
        assert r["waves_per_simd"] >= 1, (n, r)
        one = table[n.replace("k_fwd_tan_batch<", "k_fwd_tan<")[:-len(", 1>")] + ">"]
        assert r["waves_per_simd"] == one["waves_per_simd"], (n, r["vgpr"], one["vgpr"])
        assert r["lds"] == 0, (n, r["lds"])             # the ensemble sum is a butterfly over lanes


def test_route_and_bfi_batch_kernels_match_their_one_direction_siblings(table):
    for one, many in (("k_route_tan", "k_route_tan_batch"), ("k_bfi_tan", "k_bfi_tan_batch")):
        a, b = table[one], table[many]
        assert b["vgpr_spill"] == 0 and b["scratch"] == 0, (many, b)
        assert b["vgpr"] == a["vgpr"] and b["lds"] == a["lds"], (one, a, many, b)


def test_one_direction_kernels_keep_their_registers(table):
    names = [n for n in table if "k_fwd_tan<" in n]
    assert len(names) == 4, names
    for n in names:
        r = table[n]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert 144 <= r["vgpr"] <= 195, (n, r["vgpr"])
