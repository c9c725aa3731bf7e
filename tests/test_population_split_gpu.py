"""GPU tier: the launch split of `ops.population` above POP_MAX_CAND candidates.  With the cap set to 2, the three
candidates of a record go in two launches (2 + 1) whose pointers are offset by c0 candidates -- the compact candidate
tensor by c0*B*Cn (+ the column), the [P,B] sums by c0*B, the flow series by c0*rows_f*B, the aux series by c0*rows_a*B --
and every returned [P,B] tensor and series must have the bits of the same call in one launch.  All seven exports.

The records are the smallest of the two GPU suites at which each offset can be told from the others:
  - explicit models: 'hbv-m3-b5-t40-cutoff-subset' of test_population_gpu.py -- P = 3, t_first = 10, a column subset with a
    routing column among the candidates (column != 0, Cn != ny); the flow in periods of 8 days and the aux series in periods
    of 5 on its 40 scored days, so rows_f = 5 and rows_a = 8, neither T_out;
  - the implicit scheme: 'wet9' of test_adj_population_gpu.py -- P = 3, 9 scored days; the same two calendars scaled to
    that length are periods of 2 and of 3 days (8 / 40 and 5 / 40 of 9 days would be 2 and 1, and periods of one day give
    rows_a = T_out), so rows_f = 4 and rows_a = 3.
No tolerance is involved."""
import pytest
import torch

from hydrodl2_amd import ops
from hydrodl2_amd.adj_population import adj_population_cost, adj_population_period_stats, adj_population_stats
from hydrodl2_amd.population import (population_cost, population_joint_stats, population_period_stats,
                                     population_stats)

from . import synth
from . import test_adj_population_gpu as adj_suite
from . import test_population_gpu as suite
from .test_population_gpu import bits

EXPLICIT, IMPLICIT = "hbv-m3-b5-t40-cutoff-subset", "wet9"
SUMS = ("sse", "s1", "s2", "s3")

# export -> (the record's suite, the record, the call, what it takes beside the daily target: the flow and the aux calendar
# (None: daily) and the aux key (None: no aux term), the transform)
CALLS = {
    "hbvx_population_cost": (suite, EXPLICIT, population_cost, None),
    "hbvx_population_stats": (suite, EXPLICIT, population_stats, dict(transform="log")),
    "hbvx_population_joint": (suite, EXPLICIT, population_joint_stats, dict(transform="sqrt", aux_key="SWE")),
    "hbvx_population_period": (suite, EXPLICIT, population_period_stats,
                               dict(transform="log", aux_key="AET_hydro", periods=8, aux_periods=5)),
    "hbvx_adj_population_cost": (adj_suite, IMPLICIT, adj_population_cost, None),
    "hbvx_adj_population_stats": (adj_suite, IMPLICIT, adj_population_stats, dict(transform="sqrt")),
    "hbvx_adj_population_period": (adj_suite, IMPLICIT, adj_population_period_stats,
                                   dict(transform="log", aux_key="SM", periods=2, aux_periods=3)),
}


def _tensors(out):
    """{name: tensor} of every [P,B] tensor and series a population call returned."""
    if "cost" in out:
        return {k: out[k] for k in ("cost", "series")}
    if "flow" not in out:
        return {k: out[k] for k in SUMS + ("series",)}
    return {f"{term}.{k}": out[term][k] for term in ("flow", "aux") for k in SUMS + ("series",)}


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(CALLS))
def test_a_split_call_has_the_bits_of_one_launch(hip_backend, monkeypatch, entry):
    mod, name, call, kw = CALLS[entry]
    cs = mod.case(name)
    assert cs.P == 3 and cs.weights is None
    T_out, B = cs.T_out, cs.B
    args, rows = [cs.target], {"flow": T_out, "aux": T_out}
    kw = dict(kw or {})
    if "periods" in kw:
        rows = {"flow": T_out // kw["periods"], "aux": T_out // kw["aux_periods"]}
        assert len({T_out, rows["flow"], rows["aux"]}) == 3
        args = [torch.from_numpy(synth.uniform((rows["flow"], B), 293) * 6.0).to(suite.DEV), kw.pop("periods")]
    if "aux_key" in kw:
        aux_target = torch.from_numpy(synth.uniform((rows["aux"], B), 294) * 3.0).to(suite.DEV)
        args += [aux_target, kw.pop("aux_key")] + ([kw.pop("aux_periods")] if "aux_periods" in kw else [])
    launches = []
    launch = ops._call
    monkeypatch.setattr(ops, "_call", lambda lib, what, *a: launches.append(what) or launch(lib, what, *a))

    def run():
        cs.prepare()
        launches.clear()
        out = call(cs.model, cs.xd, cs.p, cs.cand, *args, names=cs.names, return_series=True, **kw)
        return _tensors(out), launches.count(entry)

    whole, n = run()
    assert n == 1
    monkeypatch.setattr(ops, "POP_MAX_CAND", 2)
    split, n = run()
    assert n == 2, "three candidates under a cap of two are two launches"
    assert list(split) == list(whole)
    for key, want in whole.items():
        term = "aux" if key.startswith("aux.") else "flow"
        assert tuple(want.shape) == ((cs.P, rows[term], B) if key.endswith("series") else (cs.P, B)), key
        assert bool(torch.isfinite(want).all()), f"{key}: a poisoned element was left"
        assert torch.equal(bits(split[key]), bits(want)), f"{key}: the split call has other bits"
    # the candidates differ, and so do their numbers: a launch that read another launch's candidates would show
    first = whole["cost" if "cost" in whole else "sse" if "sse" in whole else "flow.sse"]
    assert len({float(v) for v in first[:, 0]}) == cs.P
