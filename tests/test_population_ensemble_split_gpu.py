"""GPU tier: the launch split of `ops.population_ensemble` above POP_MAX_CAND particles, after the pattern of
tests/test_population_split_gpu.py.  With the cap set to 2, the three particles of 'hbv-m3-b5-t40-cutoff-subset' go in two
launches (2 + 1) whose pointers are offset by c0 particles -- the candidates by c0*B*Cn, the [P,B] sums by c0*B, the
series by c0*rows*B, state_out by c0*5*B*M, hist_out by c0*14*B, ancestor by c0*B, p_mul by c0*W*B (per day) and t_add
by c0*B (per particle) -- while state_in / hist_in stay whole (an ancestor indexes all sources, and without one the
launch passes src_first = c0).  Every output must have the bits of the same call in one launch, with and without an
ancestor index.  The window is the record's second half, so the sources are three different states.  No tolerance."""
import pytest
import torch

from hydrodl2_amd import ops

from .test_population_ensemble_gpu import BASE, KEYS, case, noise, record, same, step
from .test_population_gpu import DEV


@pytest.mark.gpu
@pytest.mark.parametrize("with_ancestor", [False, True], ids=["identity", "ancestor"])
def test_a_split_call_has_the_bits_of_one_launch(hip_backend, monkeypatch, with_ancestor):
    cs = case(BASE)
    rec = record(BASE)
    T, B, P = rec.main.cfg.T, cs.B, 3
    pm, ta = noise(BASE, P)
    src = step(BASE, P, t_begin=0, t_end=20, prcp_mul=pm[:, :20].contiguous(), temp_add=ta)["state"]
    anc = None
    if with_ancestor:
        anc = torch.tensor([[(c + 2 * b + 1) % P for b in range(B)] for c in range(P)], dtype=torch.int32, device=DEV)
    launches = []
    launch = ops._call
    monkeypatch.setattr(ops, "_call", lambda lib, what, *a: launches.append(what) or launch(lib, what, *a))

    def run():
        launches.clear()
        out = step(BASE, P, state=src, ancestor=anc, t_begin=20, t_end=T, prcp_mul=pm[:, 20:].contiguous(), temp_add=ta,
                   transform="log", return_series=True)
        return out, launches.count("hbvx_population_ensemble")

    whole, n = run()
    assert n == 1
    monkeypatch.setattr(ops, "POP_MAX_CAND", 2)
    split, n = run()
    assert n == 2, "three particles under a cap of two are two launches"
    for key in KEYS + ("series",):
        assert bool(torch.isfinite(whole[key]).all()), f"{key}: a poisoned element was left"
        same(split[key], whole[key], f"split {key}")
    same(split["state"].states, whole["state"].states, "split storages")
    same(split["state"].history, whole["state"].history, "split history")
    assert bool(torch.isfinite(whole["state"].states).all()) and bool(torch.isfinite(whole["state"].history).all())
    # the particles differ, and so do their numbers: a launch that read another launch's particles would show
    assert len({float(v) for v in whole["sse"][:, 0]}) == P
    assert len({float(v) for v in whole["state"].states[:, 2, 0, 0]}) == P
