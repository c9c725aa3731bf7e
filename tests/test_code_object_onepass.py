"""CPU tier: the built gfx950 code of the one-pass static adjoint (hbv_chunked.h, k_bwd_chunk_onepass).  It holds the
five unit adjoints, the offset and their parameter-gradient sums in registers: no VGPR spills; three waves per SIMD
for the runoff-only loss (156 / 161 VGPRs, the headline's form), two with the full adjoint step of the all-series loss
(179 / 187) -- forced to four waves the compiler spills 19-33 values in the first two instances, 84-98 in the others;
and its next day's loads are not waited for where they are
issued (the check of test_code_object.py::test_the_adjoints_prefetch_is_not_waited_for_where_it_is_issued)."""
import os
import sys

import pytest

from .test_code_object import LIB, _load_bursts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ONEPASS = ["void hbvx::k_bwd_chunk_onepass<%s, %s>" % (b, g) for b in ("false", "true") for g in ("false", "true")]


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB):
        pytest.skip("libhbvx.so not built")
    import kernel_resources
    return {r["name"].split("(")[0]: r for r in kernel_resources.kernel_table(LIB)}


def test_onepass_kernels_do_not_spill_and_keep_three_waves(table):
    names = [n for n in table if "k_bwd_chunk_onepass<" in n]
    assert len(names) == 4, names
    for n in names:
        r = table[n]
        assert r["vgpr_spill"] == 0, (n, r["vgpr_spill"])
        assert r["waves_per_simd"] >= (2 if n.endswith(", true>") else 3), (n, r["vgpr"])
    red = [n for n in table if "k_bwd_chunk_fold<" in n]
    assert red and all(table[n]["vgpr_spill"] == 0 for n in red)


def _waits_behind(ins, a, b):
    return [ins[i] for i in range(a, min(b + 6, len(ins))) if ins[i].startswith("s_waitcnt") and "vmcnt" in ins[i]]


def test_onepass_prefetch_is_not_waited_for_where_it_is_issued():
    """All four instances: no vmcnt wait inside or right behind a burst of loads in the day loop (the loop that issues
    the next day's loads).  The runoff-only instances (the headline's) also have none anywhere in the kernel.  The
    all-series instances wait once inside the first day's burst before the loop (register reuse among the eleven
    series loads of the prologue; the two-pass k_bwd_chunk_phi<0, false, 0, true> instance waits six times there): a
    round trip per chunk of 64 days, not per day."""
    if not os.path.exists(LIB):
        pytest.skip("libhbvx.so not built")
    import kernel_resources
    kernels = ["k_bwd_chunk_onepassILb%dELb%dEE" % (b, g) for b in (0, 1) for g in (0, 1)]
    dis = kernel_resources.disassemble_addr(LIB, kernels)
    assert len(dis) == len(kernels), sorted(dis)
    for sym, ains in dis.items():
        ins = [x for _, x in ains]
        bursts = _load_bursts(ins)
        h, e = max(kernel_resources.loops_of(ains), key=lambda hb: hb[1] - hb[0])      # the day loop
        in_loop = [(a, b) for a, b in bursts if h <= a and b <= e + 6]
        assert in_loop, f"{sym}: no load burst in the day loop (pattern changed?)"
        runoff_only = sym.split("onepass")[1].startswith(("ILb0ELb0E", "ILb1ELb0E"))     # GFULL == false
        for a, b in (bursts if runoff_only else in_loop):
            waits = _waits_behind(ins, a, b)
            assert not waits, f"{sym}: {waits} between / right behind the loads at instructions {a}..{b}"
