"""CPU tier: the built gfx950 code of the kernels that the eleven-day forward tiles and the live-row adjoint changed.

One-pass adjoint (hbv_chunked.h): the six k_bwd_chunk_onepass_live instances (parBETAET off / on x 1, 2, 3 live rows)
and the two runoff-only k_bwd_chunk_onepass instances must keep three waves per SIMD -- at most 168 VGPRs -- with no
scratch and no spill; and, as for the four-row kernel (tests/test_code_object_onepass_group.py), the hand-over slot of a grouped
call must leave room for the workgroups that residency allows.

Pipelined forward (hbv_pipe.h): the static HBV 1.0 instances run 1024 threads per workgroup -- four waves per SIMD,
at most 128 VGPRs -- with eleven days of forcings in the filler wave's registers instead of ten: no scratch, no
vector register spilled, no fixed LDS (the tile is dynamic LDS, sized and checked on the host; the descriptor's
scalars that the compiler parks in vector-register lanes were there before and cost no memory)."""
import ctypes as C
import os
import sys

import pytest

from .test_code_object import LIB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CU_LDS = 160 * 1024


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB):
        pytest.skip("libhbvx.so not built")
    import kernel_resources
    return {r["name"].split("(")[0]: r for r in kernel_resources.kernel_table(LIB)}


def _clean(r):
    return r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0


def test_live_row_instances_keep_three_waves_without_scratch(table):
    live = {n: r for n, r in table.items() if "k_bwd_chunk_onepass_live<" in n}
    assert len(live) == 6, sorted(live)
    four = {be: table[f"void k_bwd_chunk_onepass<{be}, false>"] for be in ("false", "true")}
    for n, r in list(live.items()) + [(f"k_bwd_chunk_onepass<{be}, false>", r) for be, r in four.items()]:
        print(f"{n}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS, {r['waves_per_simd']} waves per SIMD")
        assert r["waves_per_simd"] == 3 and r["vgpr"] <= 168, (n, r)
        assert _clean(r) and r["lds"] == 0, (n, r)


def test_the_slot_leaves_room_for_the_live_row_instances(table):
    dll = C.CDLL(LIB)
    dll.hbvx_onepass_slot_bytes.restype = C.c_int
    for n, r in table.items():
        if "k_bwd_chunk_onepass_live<" not in n:
            continue
        lds = r["lds"] + dll.hbvx_onepass_slot_bytes(13 if "<true," in n else 12)
        for g in (2, 4):
            assert lds * (r["waves_per_simd"] * 4 // g) <= CU_LDS, (n, g, lds)


def test_static_pipelined_forward_has_no_scratch_on_eleven_day_tiles(table):
    names = [n for n in table if n.startswith("void k_fwd_pipe<0, ") and n.endswith(", false, false, 0>")]
    assert len(names) == 6, names
    for n in names:
        r = table[n]
        print(f"{n}: {r['vgpr']} VGPRs, {r['waves_per_simd']} waves per SIMD")
        assert r["max_threads"] == 1024 and r["vgpr"] <= 128 and r["waves_per_simd"] >= 4, (n, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, (n, r)
