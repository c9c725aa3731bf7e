"""CPU tier: the built gfx950 code of the hourly model's tangent kernels (hbv_tan.h, hbv_gage.h).  The recurrence is
k_tan<MODEL_HOURLY, true, TanBatchArgs>, the several-direction kernel's text around Step<MODEL_HOURLY>: one direction per
wave, it fits the register file of one wave, nothing spills, it has no more registers than k_hourly_tan_batch had as a
text of its own (profiles/r14_tan_one_source.md), and the ensemble sum is a butterfly over lanes (no LDS).  The gage
tangent kernels exist under their names without spills.  The kernel counts the other code-object tests assert are
unchanged: exactly one instance of k_tan has MODEL_HOURLY, and it takes TanBatchArgs."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

GAGE_TAN = ("k_gage_uh_tan", "k_gage_lag_tan", "k_gage_sum_tan")


@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as ge
    import kernel_resources
    return {r["name"].split("(")[0]: r for r in kernel_resources.kernel_table(ge.build_hip())}


MODEL_HOURLY = "<4,"         # hbv_step.h: MODEL_HOURLY = 4


def test_hourly_recurrence_kernel(table):
    names = [n for n in table if "k_tan<" in n and n[n.index("<"):].startswith(MODEL_HOURLY)]
    assert len(names) == 1, names
    assert names[0].endswith("TanBatchArgs>"), names       # no one-direction instance: one direction is n_dir = 1
    r = table[names[0]]
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 512, (r["vgpr"], r["agpr"])
    assert r["vgpr"] <= 229, r["vgpr"]          # k_hourly_tan_batch's
    assert r["lds"] == 0, r["lds"]
    assert r["waves_per_simd"] >= 2, r          # directions are resident waves beside each other


def test_gage_tangent_kernels(table):
    for name in GAGE_TAN:
        r = table[name]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 512, (name, r)
    # the FIR stays LDS-staged: one column and one set of weights at a time, like k_gage_lag_fwd
    assert table["k_gage_lag_tan"]["lds"] == table["k_gage_lag_fwd"]["lds"] > 0


def test_other_kernel_counts_are_unchanged(table):
    daily = [n for n in table if "k_tan<" in n and not n[n.index("<"):].startswith(MODEL_HOURLY)]
    assert len([n for n in daily if n.endswith("TanArgs>")]) == 4
    assert len([n for n in daily if n.endswith("TanBatchArgs>")]) == 4
    assert not [n for n in table if "k_fwd_tan" in n or "k_hourly_tan_batch" in n]      # the three texts k_tan replaced
    assert len(table) > 250
