"""GPU tier: `population_fdc_stats` / `population_fdc_score` / `population_search(fdc_share=...)`
(hydrodl2_amd/population_fdc.py) on hbvx_population_fdc, the FDC form of k_pop.

The cases are those of tests/test_population_gpu.py (its `Case` / `case`, with the reasons for every shape) under the twin
targets of tests/test_population_stats_gpu.py.  Their lane mappings are the ones that can go wrong here: M = 1, B = 67
(a lane owns every threshold, R = K, and a partly filled second wave), M = 2 and M = 3 (padded member lanes that own
slots), M = 16, B = 5 (one slot per lane, and lanes of basins beyond B in the wave).

  stats bits    the four chains, n_obs and the series are `population_stats`' bit for bit, under every transform.
  own series    count[p,k,b] is exactly the number of scored days on which the call's own series lies above thr[k,b], and
                volume[p,k,b] has the bits of the host restatement (tests/hosttest/popfdc_host.cpp) over that series --
                with the thresholds the observations give, and with thresholds at ranks n//4, n//2, 3n//4 of candidate
                0's own scored flows, where candidate 0's count must be the rank itself.
  written       no poison value (-1 / NaN) is left in count / volume at K = 1, 15 and 32.
  independence  a slot's bits do not depend on K, the order of the thresholds, the lane that owned it, the other
                candidates, return_series or the call.
  module route  against one module forward per candidate (`Case.yardstick`, the parent's code): two float32 forwards may
                put a day on either side of a threshold, so |count - count_yardstick| is held to the number of scored days
                whose yardstick flow lies within a relative band of the threshold.  The band is four times the worst
                per-day relative difference between `population_cost(return_series=True)` and the yardstick series -- the
                parent's two routes, measured in the same run and printed.  On the MI355X of
                profiles/r24_population_fdc.md that difference was MEASURED_SERIES_RDIFF below: zero on all six records
                (at these shapes the module's forward is the one-wave kernel whose day step and routing `k_pop` restates,
                and the series are equal bit for bit, as tests/test_population_gpu.py notes), so the band is zero, no
                yardstick day lies inside it and every count must BE the module route's.  A card on which the two routes
                differ fails the recorded band first, not the counts.
  search        fdc_share = 0 is the search without the arguments bit for bit; with fdc_share = 0.5 no basin's mixed cost
                rises and history['score_fdc'] is finite where the flow score is."""
import functools

import numpy as np
import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import ops
from hydrodl2_amd.population import population_cost, population_score, population_search, population_stats
from hydrodl2_amd.population_fdc import DEFAULT_PROBS, population_fdc_score, population_fdc_stats

from . import synth
from .test_popfdc_host import load_fdclib
from .test_popfdc_host import run as run_host
from .test_population_gpu import CASES, DEV, bits, case
from .test_population_stats_gpu import TRANSFORMS, twin

KEYS = ("sse", "s1", "s2", "s3")
# worst per-day relative difference between population_cost's series and the module route's over the cases (MI355X:
# 0.0 on each of the six, the series are bit-equal); the band of the module-route test is four times this
MEASURED_SERIES_RDIFF = 0.0
BAND = 4 * MEASURED_SERIES_RDIFF
NEAR_CAP = 0.02


def fdc(name, transform="none", cand=None, **kw):
    cs = case(name)
    tgt = twin(name)            # (runs the module when it is first asked for: before prepare(), not after)
    cs.prepare()
    return population_fdc_stats(cs.model, cs.xd, cs.p, cs.cand if cand is None else cand, tgt, cs.names, cs.weights,
                                transform=transform, **kw)


def scored_days(name):
    """[T_out,B] bool: the days that enter the curve -- a finite target and a weight > 0."""
    cs = case(name)
    tgt = twin(name)
    return torch.isfinite(tgt) if cs.weights is None else torch.isfinite(tgt) & (cs.weights > 0)


@functools.lru_cache(maxsize=None)
def own_series(name):
    """[P,T_out,B]: every candidate's series from a first `population_stats(return_series=True)` call.  Computed once."""
    cs = case(name)
    tgt = twin(name)
    cs.prepare()
    return population_stats(cs.model, cs.xd, cs.p, cs.cand, tgt, cs.names, cs.weights, return_series=True)["series"].clone()


@functools.lru_cache(maxsize=None)
def rank_levels(name):
    """Thresholds from candidate 0's own series: per basin the scored flows sorted descending, the values at ranks n//4,
    n//2, 3n//4 -> (thr [3,B] float32, ranks [3,B] int64, free [3,B] bool: no tie at the rank, so exactly `rank` flows lie
    above it; half [3,B] float32: each level moved half-way to the next distinct smaller flow).  Computed once."""
    series, scored = own_series(name)[0], scored_days(name)
    T, B = series.shape
    thr, half = torch.zeros(3, B), torch.zeros(3, B)
    ranks, free = torch.zeros(3, B, dtype=torch.int64), torch.zeros(3, B, dtype=torch.bool)
    for b in range(B):
        v = series[scored[:, b], b].cpu().sort(descending=True).values
        n = int(v.numel())
        for i, r in enumerate((n // 4, n // 2, 3 * n // 4)):
            if n == 0:
                continue
            ranks[i, b], thr[i, b] = r, v[r]
            free[i, b] = bool(torch.isfinite(v[r])) and (r == 0 or bool(v[r - 1] > v[r]))
            below = v[v < v[r]]
            nxt = float(below[0]) if below.numel() else 0.5 * float(v[r])
            half[i, b] = 0.5 * (float(v[r]) + nxt)
    return thr.to(DEV), ranks, free, half.to(DEV)


def counted_by_torch(series, thr, scored):
    """[P,K,B] int64: ((series[p,:,b] > thr[k,b]) & scored).sum() -- the exceedance count of a series by its definition."""
    return ((series.unsqueeze(1) > thr.unsqueeze(0).unsqueeze(2)) & scored.unsqueeze(0).unsqueeze(0)).sum(2)


@pytest.fixture(scope="module")
def fdclib():
    return load_fdclib()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_the_stats_are_population_stats_bit_for_bit(hip_backend, name):
    assert ops._POISON, "the GPU tier runs with poisoned output buffers"
    cs = case(name)
    tgt = twin(name)
    for transform in TRANSFORMS:
        cs.prepare()
        want = population_stats(cs.model, cs.xd, cs.p, cs.cand, tgt, cs.names, cs.weights, transform=transform,
                                return_series=True)
        got = fdc(name, transform, return_series=True)
        assert set(got) == set(want) | {"fdc"}
        for key in KEYS + ("series", "shift"):
            assert got[key].dtype == torch.float32 and torch.equal(bits(got[key]), bits(want[key])), (transform, key)
        assert torch.equal(got["n_obs"], want["n_obs"]) and got["columns"] == want["columns"]
        assert got["transform"] == transform and (got["eps"] is None) == (transform != "log")
        if got["eps"] is not None:
            assert torch.equal(bits(got["eps"]), bits(want["eps"]))
        for k in ("W", "e1", "e2"):
            assert torch.equal(got["obs"][k], want["obs"][k])
        for metric in ("nse", "kge"):
            assert torch.equal(population_score(got, metric), population_score(want, metric))
        plain = fdc(name, transform)
        assert "series" not in plain and all(torch.equal(bits(plain[k]), bits(want[k])) for k in KEYS)
        f = got["fdc"]
        K = len(DEFAULT_PROBS)
        assert tuple(f["count"].shape) == tuple(f["volume"].shape) == (cs.P, K, cs.B)
        assert f["count"].dtype == torch.int32 and f["volume"].dtype == torch.float32
        assert tuple(f["thresholds"].shape) == (K, cs.B) and f["probs"].tolist() == list(DEFAULT_PROBS)
        assert torch.equal(f["n_days"], scored_days(name).sum(0)) and torch.equal(f["n_days"], want["n_obs"])
        # the counts do not move with the transform: the comparison is on the flow itself
        if transform == "none":
            first = f
        assert torch.equal(f["count"], first["count"]) and torch.equal(bits(f["volume"]), bits(first["volume"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_counts_and_volumes_against_the_calls_own_series(hip_backend, fdclib, name):
    cs = case(name)
    scored = scored_days(name)
    thr_rank, ranks, free, _ = rank_levels(name)
    assert bool(free.any()), "no tie-free rank in this case: the rank check would be empty"
    for label, kw in (("probs", {}), ("ranks", {"thresholds": thr_rank})):
        got = fdc(name, "sqrt", return_series=True, **kw)
        f, series = got["fdc"], got["series"]
        thr = f["thresholds"]
        assert torch.equal(bits(series), bits(own_series(name)))
        want = counted_by_torch(series, thr, scored)
        assert torch.equal(f["count"].long(), want), f"{label}: a count is not the count of the call's own series"
        assert int(want.min()) < int(want.max()), f"{label}: every slot counts the same: the thresholds cut nothing"
        en = scored.cpu().numpy()
        for p in range(cs.P):
            n_host, v_host = run_host(fdclib, series[p].cpu().numpy(), en, thr.cpu().numpy())
            assert np.array_equal(f["count"][p].cpu().numpy(), n_host), (label, p)
            assert np.array_equal(f["volume"][p].cpu().numpy().view(np.uint32), v_host.view(np.uint32)), \
                f"{label}: candidate {p}'s volumes are not the host restatement's bits"
        # the observed side of the same thresholds, by the same comparison
        tgt32 = torch.where(scored, twin(name), torch.zeros_like(twin(name)))
        assert torch.equal(f["obs_count"], counted_by_torch(tgt32.unsqueeze(0), thr, scored)[0])
        if label == "ranks":
            # candidate 0 against its own ranks: exactly `rank` scored flows lie above a tie-free level
            c0 = f["count"][0].long().cpu()
            assert torch.equal(c0[free], ranks[free]), "candidate 0's count at a tie-free rank is not the rank"
            assert f["probs"] is None and torch.equal(bits(thr), bits(thr_rank))
            print(f"{name}: {int(free.sum())} of {free.numel()} rank slots tie-free, ranks {int(ranks.min())} .. {int(ranks.max())}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_every_element_is_written(hip_backend, name):
    assert ops._POISON, "the GPU tier runs with poisoned output buffers"
    cs = case(name)
    n_days = scored_days(name).sum(0)
    for K in (1, 15, 32):
        probs = [(i + 1) / (K + 1) for i in range(K)]
        f = fdc(name, probs=probs)["fdc"]
        assert tuple(f["count"].shape) == tuple(f["volume"].shape) == (cs.P, K, cs.B)
        assert bool((f["count"] >= 0).all()), f"K = {K}: a poisoned count (-1) was left"
        assert bool(torch.isfinite(f["volume"]).all()), f"K = {K}: a poisoned or non-finite volume was left"
        assert bool((f["count"] <= n_days.view(1, 1, -1)).all())
        assert bool((f["count"][:, :, cs.B - 1] >= 0).all())        # the last basin: in a partly filled wave where B % (64 / Mp) != 0
        assert bool(((f["count"] == 0) == (f["volume"] == 0)).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_a_slot_depends_on_its_candidate_and_threshold_alone(hip_backend, name):
    cs = case(name)
    base = fdc(name, return_series=True)["fdc"]
    thr = base["thresholds"]
    assert bool(torch.isfinite(thr).all())
    K = thr.shape[0]

    def same(f, ks, what, cands=slice(None)):
        assert torch.equal(f["count"], base["count"][cands][:, ks]), f"{what}: other counts"
        assert torch.equal(bits(f["volume"]), bits(base["volume"][cands][:, ks])), f"{what}: other volume bits"

    same(fdc(name, return_series=True)["fdc"], slice(None), "a second call")
    same(fdc(name)["fdc"], slice(None), "without return_series")
    same(fdc(name, thresholds=thr.clone())["fdc"], slice(None), "the same levels given as thresholds")
    for k in (0, 7, K - 1):
        same(fdc(name, thresholds=thr[k:k + 1].contiguous())["fdc"], [k], f"threshold {k} alone (K = 1)")
    rev = list(range(K - 1, -1, -1))
    same(fdc(name, thresholds=thr[rev].contiguous())["fdc"], rev, "the thresholds reversed")
    # K = 32: every slot twice and two a third time -- with one member a lane owns all 32 (R = 32)
    wide = list(range(K)) + list(range(K)) + [3, 11]
    same(fdc(name, thresholds=thr[wide].contiguous())["fdc"], wide, "K = 32")
    if cs.P > 1:
        perm = list(range(cs.P - 1, -1, -1))
        same(fdc(name, cand=cs.cand[perm].contiguous())["fdc"], slice(None), "the candidates permuted", perm)
        c = cs.P - 1
        same(fdc(name, cand=cs.cand[c:c + 1].contiguous())["fdc"], slice(None), f"candidate {c} alone", [c])
        # the candidates differ, and so do their curves: the candidate index reaches the parameters
        assert not torch.equal(base["count"][0], base["count"][1]) or not torch.equal(base["volume"][0], base["volume"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_counts_against_the_module_route(hip_backend, name):
    cs = case(name)
    tgt, scored = twin(name), scored_days(name)
    want_series = cs.yardstick[0]                                               # [P,T_out,B], one module forward per candidate
    # the parent's two routes, in this run: population_cost's series against the module's
    cs.prepare()
    cost_series = population_cost(cs.model, cs.xd, cs.p, cs.cand, tgt, cs.names, cs.weights, return_series=True)["series"]
    a, b = cost_series.double(), want_series.double()
    assert bool(((a == b) | (b != 0)).all())
    rdiff = float(torch.where(b != 0, (a - b).abs() / b.abs().clamp_min(1e-300), torch.zeros_like(b)).max())
    print(f"{name}: population_cost's series against the module route: worst per-day relative difference {rdiff:.3e} "
          f"(recorded {MEASURED_SERIES_RDIFF:.3e}, band {BAND:.3e})")
    assert rdiff <= BAND, "the two routes of the parent differ by more than the recorded band"
    _, _, _, half = rank_levels(name)
    thr = half.unsqueeze(0).unsqueeze(2).double()                               # [1,3,1,B]
    ys = b.unsqueeze(1)                                                         # [P,1,T_out,B]
    sc = scored.unsqueeze(0).unsqueeze(0)
    near = (((ys - thr).abs() <= BAND * thr.abs()) & sc).sum(2)                 # [P,3,B]
    pairs = cs.P * 3 * int(scored.sum())
    share = int(near.sum()) / max(pairs, 1)
    print(f"{name}: {int(near.sum())} of {pairs} (slot, day) pairs of the yardstick inside the band ({share:.4%}, cap {NEAR_CAP:.0%})")
    assert share <= NEAR_CAP
    count_y = counted_by_torch(want_series, half, scored)
    assert int(count_y.min()) < int(count_y.max())
    f = fdc(name, thresholds=half)["fdc"]
    diff = (f["count"].long() - count_y).abs()
    print(f"{name}: worst |count - yardstick| {int(diff.max())}, slots that differ {int((diff > 0).sum())} of {diff.numel()}")
    assert bool((diff <= near).all()), "a count is further from the module route's than the days inside the band allow"


@pytest.mark.gpu
def test_population_search_with_an_fdc_term(hip_backend):
    """The twin problem of tests/test_population_stats_gpu.py::test_population_search_on_kge with a flow-duration term."""
    T, B, M = 40, 5, 2
    model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "dynamic_params": {"Hbv": []}}, DEV)
    x = {"x_phy": torch.from_numpy(synth.forcing(T, B, seed=61)).to(DEV)}
    truth = torch.from_numpy(synth.raw_parameters(T, B, model.learnable_param_count, seed=62)).to(DEV)
    with torch.no_grad():
        obs = model(x, truth)["streamflow"][..., 0].clone()
    start = torch.from_numpy(synth.raw_parameters(T, B, model.learnable_param_count, seed=63, scale=1.5)).to(DEV)
    keep = [t.clone() for t in (start, obs, x["x_phy"])]

    def search(seed, **kw):
        g = torch.Generator().manual_seed(seed)
        return population_search(model, x, start, obs, n_candidates=32, n_rounds=3, generator=g, **kw)

    # fdc_share = 0 is the search without the arguments: bits and history keys
    for kw in ({}, {"objective": "kge"}):
        old, hist_old = search(5, **kw)
        new, hist_new = search(5, fdc_share=0.0, fdc_probs=(0.1, 0.5, 0.9), fdc_metric="fdc_vol", **kw)
        assert torch.equal(bits(old), bits(new)) and set(hist_old) == set(hist_new) and "score_fdc" not in hist_new
        for key in set(hist_old) - {"columns"}:
            assert torch.equal(hist_old[key], hist_new[key]), key

    for metric in ("fdc_freq", "fdc_vol"):
        best, hist = search(5, objective="kge", fdc_share=0.5, fdc_metric=metric)
        assert all(torch.equal(a, b) for a, b in zip((start, obs, x["x_phy"]), keep)), "an input was modified"
        cost, score, score_fdc = hist["cost"], hist["score"], hist["score_fdc"]
        assert tuple(cost.shape) == tuple(score.shape) == tuple(score_fdc.shape) == (4, B)
        assert cost.dtype == score_fdc.dtype == torch.float64
        assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(score_fdc[torch.isfinite(score)]).all())
        assert bool((score_fdc >= 0).all())
        assert bool(torch.isfinite(cost).all()) and bool((cost[1:] <= cost[:-1]).all()), "a basin's mixed cost rose"
        assert torch.allclose(cost, 0.5 * (1.0 - score) + 0.5 * score_fdc, rtol=1e-14, atol=0)
        assert bool((cost[-1] < cost[0]).any()), "32 candidates x 3 rounds improved no basin"
        assert torch.equal(hist["best_index"] != 0, cost[1:] < cost[:-1])
        assert tuple(best.shape) == tuple(start.shape) and torch.equal(best[:-1], start[:-1])
        print(f"population_search(kge, fdc_share 0.5, {metric}): mean KGE {float(score[0].mean()):.4f} -> "
              f"{float(score[-1].mean()):.4f}, mean {metric} {float(score_fdc[0].mean()):.4f} -> {float(score_fdc[-1].mean()):.4f}")
        # the returned row through the call itself: the history's last scores
        cols = hist["columns"]
        st = population_fdc_stats(model, x, best, best[-1][:, cols].unsqueeze(0).contiguous(), obs)
        assert torch.equal(population_score(st, "kge")[0].cpu(), score[-1])
        assert torch.equal(population_fdc_score(st, metric)[0].cpu(), score_fdc[-1])
        again, hist2 = search(5, objective="kge", fdc_share=0.5, fdc_metric=metric)
        assert torch.equal(bits(again), bits(best)) and torch.equal(hist2["cost"], cost)
        assert torch.equal(hist2["score_fdc"], score_fdc)
