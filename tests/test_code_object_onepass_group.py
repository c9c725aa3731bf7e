"""CPU tier: the built gfx950 code of the grouped one-pass static adjoint (hbv_chunked.h, k_bwd_chunk_onepass as a
workgroup of G waves that fold their chunks' maps into one through an LDS hand-over slot).  The slot must not cost the
kernel the residency its registers allow: with w waves per SIMD a CU holds w * 4 / G workgroups, and their LDS must
fit the CU's 160 KB.  The slot is dynamic LDS (a call with group size 1 allocates none), so a workgroup's LDS is the
kernel's fixed size from the code object plus the slot size the launcher passes, which the library reports
(hbvx_onepass_slot_bytes).  The hand-over synchronises with workgroup barriers, and the fold and the scan that follow
must not spill."""
import ctypes as C
import os
import sys

import pytest

from .test_code_object import LIB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CU_LDS = 160 * 1024
GROUPS = (2, 4)


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB):
        pytest.skip("libhbvx.so not built")
    import kernel_resources
    return {r["name"].split("(")[0]: r for r in kernel_resources.kernel_table(LIB)}


def test_the_slot_leaves_room_for_the_residency_the_registers_allow(table):
    dll = C.CDLL(LIB)
    dll.hbvx_onepass_slot_bytes.restype = C.c_int
    names = [n for n in table if "k_bwd_chunk_onepass<" in n]
    assert len(names) == 4, names
    for n in names:
        r = table[n]
        n_param = 13 if "<true," in n else 12
        slot = dll.hbvx_onepass_slot_bytes(n_param)
        # the rows of one map for 64 lanes in float32: 30 of Phi and phi, 51 / 55 of G and g0
        assert slot == (30 + (55 if n_param == 13 else 51)) * 64 * 4, (n, slot)
        lds = r["lds"] + slot
        for g in GROUPS:
            resident = r["waves_per_simd"] * 4 // g
            print(f"{n}: {r['vgpr']} VGPRs, {r['waves_per_simd']} waves per SIMD; group {g}: {resident} workgroups x "
                  f"{lds} B = {resident * lds} B of LDS")
            assert lds * resident <= CU_LDS, (n, g, lds, resident)


def test_the_hand_over_uses_workgroup_barriers():
    if not os.path.exists(LIB):
        pytest.skip("libhbvx.so not built")
    import kernel_resources
    dis = kernel_resources.disassemble(LIB, ["k_bwd_chunk_onepassILb"])
    assert len(dis) == 4, sorted(dis)
    for sym, ins in dis.items():
        assert any(x.startswith("s_barrier") for x in ins), sym


def test_fold_and_scan_do_not_spill(table):
    names = [n for n in table if "k_bwd_chunk_fold<" in n or n.startswith("k_bwd_chunk_scan")]
    assert len(names) == 3, names
    for n in names:
        assert table[n]["vgpr_spill"] == 0 and table[n]["scratch"] == 0, (n, table[n])
