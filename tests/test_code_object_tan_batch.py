"""CPU tier: the built gfx950 code of the tangent-linear kernels (hbv_tan.h, hbvx.hip).  k_tan<MODEL, BETAET,
TanBatchArgs> carries one direction per lane (what the measurements left, profiles/r07_jvp_batch.md): an instance fits
the register file of one wave (512 VGPRs), nothing spills (no scratch traffic in the day loop), and, since the
directions are resident waves beside each other, it keeps the one-direction instance's occupancy.  The one-direction
instance k_tan<MODEL, BETAET, TanArgs> beside it (an instantiation of its own for its speed, profiles/r09_tan_unify.md)
keeps the figures of DESIGN.md §0 F1.  No instance has more registers than the kernel it replaced when the three texts
became one (profiles/r14_tan_one_source.md).  k_route_tan_batch and k_bfi_tan_batch serve the one-direction entry
points too and keep the figures of the kernels they replaced there."""
import os
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


# waves per SIMD of k_tan<MODEL, BETAET, TanArgs>, which a several-direction instance must keep (profiles/r07_jvp_batch.md)
WAVES_PER_SIMD = {"<0, false>": 3, "<0, true>": 3, "<1, true>": 2, "<2, true>": 2}
# VGPRs of k_fwd_tan<MODEL, BETAET> and k_fwd_tan_batch<MODEL, BETAET>, the separate texts these instances replaced
VGPR_ONE = {"<0, false>": 144, "<0, true>": 152, "<1, true>": 170, "<2, true>": 195}
VGPR_BATCH = {"<0, false>": 145, "<0, true>": 153, "<1, true>": 171, "<2, true>": 195}


def daily(table, args):
    """<MODEL, BETAET> -> kernel name, of the daily k_tan instances that take `args`"""
    out = {}
    for n in table:
        if "k_tan<" in n and n.endswith(args + ">") and not n[n.index("<"):].startswith("<4,"):    # 4: MODEL_HOURLY
            model, betaet = n[n.index("<") + 1:].split(", ")[:2]
            out[f"<{model}, {betaet}>"] = n
    return out


def test_batch_instances_do_not_spill_and_fit_one_wave(table):
    names, ones = daily(table, "TanBatchArgs"), daily(table, "TanArgs")
    # HBV 1.0 with and without parBETAET, 1.1p, 2.0; no directions-per-lane argument (those instances lost, ibid.)
    assert sorted(names) == sorted(WAVES_PER_SIMD), names
    for key, n in names.items():
        r = table[n]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (n, r)       # nothing goes to memory
        assert r["vgpr"] + r["agpr"] <= 512, (n, r["vgpr"], r["agpr"])
        one = table[ones[key]]
        assert r["waves_per_simd"] == one["waves_per_simd"] == WAVES_PER_SIMD[key], (n, r["vgpr"], one["vgpr"])
        assert r["lds"] == 0, (n, r["lds"])             # the ensemble sum is a butterfly over lanes


def test_route_and_bfi_kernels_keep_the_one_direction_figures(table):
    """k_route_tan had 102 VGPRs and no LDS, k_bfi_tan 20 VGPRs and 16 KB of LDS; neither is built any more."""
    for name, vgpr, lds in (("k_route_tan_batch", 102, 0), ("k_bfi_tan_batch", 20, 16384)):
        r = table[name]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] == vgpr and r["lds"] == lds, (name, r)
    assert "k_route_tan" not in table and "k_bfi_tan" not in table


def test_one_direction_kernels_keep_their_registers(table):
    names, ones = daily(table, "TanBatchArgs"), daily(table, "TanArgs")
    assert len(names) + len(ones) == 8 and sorted(ones) == sorted(VGPR_ONE), (names, ones)
    for found, most in ((ones, VGPR_ONE), (names, VGPR_BATCH)):
        for key, n in found.items():
            r = table[n]
            assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
            assert 144 <= r["vgpr"] <= most[key], (n, r["vgpr"])
