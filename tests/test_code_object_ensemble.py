"""CPU tier: the ensemble form of k_pop (hydrodl2_amd/csrc/hbv_pop.h) in the BUILT library's gfx950 code objects,
resources only (tools/kernel_resources.py; no GPU needed): an instance per model and transform, no scratch and no spill
anywhere, no LDS, and the occupancy of the stats form it extends -- three waves per SIMD by registers for HBV 1.0 / 1.1p,
two for HBV 2.0 -- although it carries two more per-lane pointers, two more prefetched values and the window's bounds
through the day loop (the registers of both forms are printed here and recorded in DESIGN.md's table)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "hydrodl2_amd", "csrc", "libhbvx.so")

# k_pop<MODEL, BETAET, TR, Args>: HBV 1.0 with and without parBETAET, 1.1p, 2.0
MODELS = {"hbv10": "0, false", "hbv10-betaet": "0, true", "hbv11p": "1, true", "hbv20": "2, true"}


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB):
        pytest.skip("libhbvx.so not built")
    import kernel_resources
    return {r["name"].split("(")[0]: r for r in kernel_resources.kernel_table(LIB) if "k_pop<" in r["name"]}


def test_the_instances_exist_without_scratch_and_keep_the_stats_forms_occupancy(table):
    ens = {k: r for k, r in table.items() if "PopEnsArgs" in k}
    assert len(ens) == 12, sorted(ens)
    for model, head in MODELS.items():
        for tr in (0, 1, 2):
            r = ens.get(f"void k_pop<{head}, {tr}, PopEnsArgs>")
            s = table.get(f"void k_pop<{head}, {tr}, PopStatsArgs>")
            assert r is not None and s is not None, (model, tr)
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (model, tr, r)
            assert r["agpr"] == 0 and r["max_threads"] == 64 and r["lds"] == 0, (model, tr, r)
            print(f"{model} transform {tr}: stats {s['vgpr']} VGPR / {s['waves_per_simd']} waves, "
                  f"ensemble {r['vgpr']} VGPR / {r['waves_per_simd']} waves")
            assert r["waves_per_simd"] >= s["waves_per_simd"] == (2 if model == "hbv20" else 3), (model, tr, r["vgpr"])
