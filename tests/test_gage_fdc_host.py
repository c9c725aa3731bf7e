"""CPU tier: the flow-duration statistics of the hourly model's population calls without a GPU
(include/hbvx_gage_fdc.h, hydrodl2_amd/hourly_fdc.py).

The rules compiled for the host (tests/hosttest/gagefdc_host.cpp: hbvx_popk::FdcSlot fed hour by hour as a lane of
k_gp_fdc feeds its own; a plain std::sort for the quantiles) are held to numpy exactly -- a count is a count, a volume a
sequential float32 sum, a quantile a value of the series: there is nothing to bound.  Then the sortable key of the
kernel's sort, `hourly_fdc_score` against values written out here, what `hourly_population_fdc_stats` and
`hourly_routing_search` refuse before the model runs (host tensors), the observed side, the header's prototypes against
`_abi.GAGE_FDC_SIGNATURES`, the entry points' argument checks on the cross-compiled library (no launch), and
`population_fdc_score`'s bits on a saved dictionary."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi, hourly_fdc as hf
from hydrodl2_amd.hourly_events import hourly_routing_search
from hydrodl2_amd.hourly_fdc import hourly_fdc_score, hourly_population_fdc_stats
from hydrodl2_amd.population_fdc import DEFAULT_PROBS, fdc_thresholds, population_fdc_score

from .test_hourly_population_host import _model, _problem

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hosttest", "gagefdc_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libgagefdc_host.so")
HDR = os.path.join(ROOT, "hydrodl2_amd", "csrc", "hbv_pop.h")
NAN, INF = float("nan"), float("inf")


def load_fdclib():
    newest = max(os.path.getmtime(f) for f in (SRC, HDR))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    dll = C.CDLL(LIB)
    dll.gagefdc_host.argtypes = [C.c_int] * 3 + [C.c_void_p] * 5
    dll.gagefdc_host.restype = C.c_int
    dll.gagequant_host.argtypes = [C.c_int] * 3 + [C.c_void_p] * 4
    dll.gagequant_host.restype = C.c_int
    dll.gagequant_keys.argtypes = [C.c_int] + [C.c_void_p] * 3
    dll.gagequant_keys.restype = None
    return dll


@pytest.fixture(scope="module")
def fdclib():
    return load_fdclib()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_fdc(dll, series, scored, thr):
    """(count [K,G] int32, volume [K,G] float32) of gagefdc_host: series [T,G] float32, scored [T,G], thr [K,G]."""
    T, G = series.shape
    K = thr.shape[0]
    series, thr = (np.ascontiguousarray(a, dtype=np.float32) for a in (series, thr))
    scored = np.ascontiguousarray(scored, dtype=np.uint8)
    assert scored.shape == (T, G) and thr.shape == (K, G)
    count = np.full((K, G), -7, dtype=np.int32)
    volume = np.full((K, G), np.nan, dtype=np.float32)
    assert dll.gagefdc_host(T, G, K, series.ctypes.data, scored.ctypes.data, thr.ctypes.data, count.ctypes.data,
                            volume.ctypes.data) == 0
    return count, volume


def run_quant(dll, series, scored, rank):
    """quantile [K,G] float32 of gagequant_host: series [T,G] float32, scored [T,G], rank [K,G] int32."""
    T, G = series.shape
    K = rank.shape[0]
    series = np.ascontiguousarray(series, dtype=np.float32)
    scored = np.ascontiguousarray(scored, dtype=np.uint8)
    rank = np.ascontiguousarray(rank, dtype=np.int32)
    assert scored.shape == (T, G) and rank.shape == (K, G)
    q = np.full((K, G), -7.0, dtype=np.float32)
    assert dll.gagequant_host(T, G, K, series.ctypes.data, scored.ctypes.data, rank.ctypes.data, q.ctypes.data) == 0
    return q


def _hand_made():
    """T = 12, G = 5: gage 0 plain, gage 1 with a NaN hour and a masked hour above every threshold, gage 2 on a plateau
    AT a threshold, gage 3 of zeros of both signs against a +0 threshold, gage 4 without a scored hour."""
    rng = np.random.default_rng(5)
    T, G = 12, 5
    y = rng.gamma(2.0, 1.5, size=(T, G)).astype(np.float32)
    scored = np.ones((T, G), np.uint8)
    scored[[2, 7], 0] = 0
    y[4, 1] = np.nan
    y[9, 1] = 1e6
    scored[9, 1] = 0
    y[3:8, 2] = 2.5
    y[:, 3] = np.float32(0.0)
    y[::2, 3] = np.float32(-0.0)
    y[5, 3] = 1.0
    scored[:, 4] = 0
    thr = np.array([[0.5, 0.5, 2.5, 0.0, 0.5], [2.0, 2.0, 1.0, -1.0, 2.0], [100.0, 100.0, 2.5000002, 0.5, -INF]], np.float32)
    return y, scored, thr


def test_counts_are_numpys_and_volumes_a_float32_cumsum(fdclib):
    y, scored, thr = _hand_made()
    T, G = y.shape
    count, volume = run_fdc(fdclib, y, scored, thr)
    for k in range(thr.shape[0]):
        for g in range(G):
            with np.errstate(invalid="ignore"):
                above = (scored[:, g] != 0) & (y[:, g] > thr[k, g])
            assert count[k, g] == int(above.sum()), (k, g)
            # np.cumsum of a float32 array adds sequentially, one rounding per element; the leading +0 is the slot's start
            want = np.cumsum(np.concatenate([[np.float32(0.0)], y[above, g]]), dtype=np.float32)[-1]
            assert bits(volume[k, g]) == bits(np.float32(want)), (k, g)
    # the cases by hand: the NaN hour is above nothing and the masked 1e6 never enters
    assert count[2, 1] == 0 and volume[2, 1] == 0.0 and np.isfinite(volume[:, 1]).all()
    # an hour AT the threshold is not above it; the next float32 below it lets the plateau in
    assert count[0, 2] == int((y[:, 2] > 2.5).sum()) and count[0, 2] <= T - 5
    assert run_fdc(fdclib, y, scored, np.full((1, 5), np.nextafter(np.float32(2.5), np.float32(0)), np.float32))[0][0, 2] == \
        count[0, 2] + 5
    # -0 is not above +0 (nor +0): only the 1.0 counts; everything is above -1
    assert count[0, 3] == 1 and volume[0, 3] == 1.0 and count[1, 3] == T
    # a gage without a scored hour: 0 and +0 whatever the threshold, -inf included
    assert (count[:, 4] == 0).all() and (bits(volume[:, 4]) == 0).all()
    # a slot does not depend on K or on the order of the levels
    order = [2, 0, 1]
    c2, v2 = run_fdc(fdclib, y, scored, thr[order])
    assert np.array_equal(c2, count[order]) and np.array_equal(bits(v2), bits(volume[order]))
    c1, v1 = run_fdc(fdclib, y, scored, thr[1:2])
    assert np.array_equal(c1, count[1:2]) and np.array_equal(bits(v1), bits(volume[1:2]))
    assert fdclib.gagefdc_host(0, 1, 1, None, None, None, None, None) == -1


def test_quantiles_are_np_sort_descending_at_the_ranks(fdclib):
    rng = np.random.default_rng(6)
    T, G = 37, 5
    y = rng.normal(0.0, 2.0, size=(T, G)).astype(np.float32)
    y[3, 0] = y[9, 0]                                                   # a tie
    y[5, 2] = np.nan                                                    # a scored NaN: the column is NaN
    y[6, 3] = np.nan                                                    # a NaN that is masked: it never enters
    y[:, 1] = np.where(rng.random(T) < 0.5, np.float32(0.0), np.float32(-0.0))
    y[0, 1], y[1, 1], y[2, 1] = 3.0, -3.0, INF
    scored = (rng.random((T, G)) < 0.8).astype(np.uint8)
    scored[5, 2], scored[6, 3] = 1, 0
    scored[:, 4] = 0
    n = scored.sum(0).astype(np.int64)
    rank = np.stack([np.zeros(G), n // 2, n - 1, np.full(G, -1), n]).astype(np.int32)       # first, middle, last, -1, n
    q = run_quant(fdclib, y, scored, rank)
    for g in (0, 1, 3):
        col = y[scored[:, g] != 0, g]
        want = -np.sort(-col.astype(np.float64)).astype(np.float32)     # descending (np.sort leaves the zeros' signs alone)
        for k in range(3):
            assert q[k, g] == want[rank[k, g]], (k, g)
        assert np.isnan(q[3, g]) and np.isnan(q[4, g]), g               # rank -1 and rank n
    assert q[0, 1] == INF and q[2, 1] == -3.0
    # -0 sorts below +0: the zeros of gage 1 come as a run of +0 and then a run of -0
    col = y[scored[:, 1] != 0, 1]
    zeros = run_quant(fdclib, y, scored, np.tile(np.arange(2, len(col) - 1, dtype=np.int32)[:5, None], (1, G)))[:, 1]
    full = run_quant(fdclib, y, scored, np.tile(np.arange(32, dtype=np.int32)[:, None], (1, G)))[:, 1][:len(col)]
    sign = np.signbit(full[(full == 0)])
    assert sign.size > 4 and (np.diff(sign.astype(int)) >= 0).all() and sign[0] == False and sign[-1] == True   # noqa: E712
    assert (zeros == 0).all()
    # a value of the series, bit for bit
    assert set(bits(full[full == full]).tolist()) <= set(bits(col).tolist())
    assert np.isnan(q[:, 2]).all() and np.isnan(q[:, 4]).all()
    assert (bits(q[:, 4]) == 0x7FC00000).all()
    assert fdclib.gagequant_host(1, 0, 1, None, None, None, None) == -1


def test_the_sortable_key_orders_like_the_total_order(fdclib):
    vals = np.array([-INF, -3.5, -1e-45, -0.0, 0.0, 1e-45, 1.0, 1.0000001, 3e38, INF, NAN, -NAN], np.float32)
    key = np.zeros(len(vals), np.uint32)
    back = np.zeros(len(vals), np.float32)
    fdclib.gagequant_keys(len(vals), vals.ctypes.data, key.ctypes.data, back.ctypes.data)
    assert (np.diff(key[:10].astype(np.int64)) > 0).all()               # strictly ascending, -0 below +0
    assert key[:10].min() > 0                                           # nothing maps to the key of "not scored"
    assert key[10] == key[11] == 0xFFFFFFFF and key[:10].max() < 0xFFFFFFFF
    assert np.array_equal(bits(back[:10]), bits(vals[:10]))             # undone bit for bit
    rng = np.random.default_rng(7)
    r = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32).view(np.float32)
    r = r[~np.isnan(r)]
    key, back = np.zeros(len(r), np.uint32), np.zeros(len(r), np.float32)
    fdclib.gagequant_keys(len(r), r.ctypes.data, key.ctypes.data, back.ctypes.data)
    assert np.array_equal(bits(back), bits(r))
    order = np.argsort(key, kind="stable")
    assert (np.diff(r[order].astype(np.float64)) >= 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# hourly_fdc_score
def _stats(count, volume, quantile, thr, oc, ov, n, probs=(0.2, 0.5, 0.7)):
    t = lambda a, dt: torch.tensor(a, dtype=dt)      # noqa: E731
    f = dict(probs=t(probs, torch.float64), thresholds=t(thr, torch.float32), obs_count=t(oc, torch.int64),
             obs_volume=t(ov, torch.float64), n_hours=t(n, torch.int64), count=t(count, torch.int32),
             volume=t(volume, torch.float32))
    if quantile is not None:
        f["quantile"] = t(quantile, torch.float32)
    return {"fdc": f}


def test_fdc_scores_on_hand_made_dictionaries():
    # P = 2, K = 3, G = 2; gage 1 has a threshold of zero at k = 2
    thr = [[8.0, 4.0], [4.0, 2.0], [2.0, 0.0]]
    q = [[[8.0, 2.0], [2.0, 2.0], [1.0, 5.0]], [[16.0, 4.0], [4.0, 1.0], [2.0, 0.0]]]
    count = [[[10, 0], [50, 10], [70, 90]], [[20, 20], [50, 50], [70, 70]]]
    volume = [[[100.0, 0.0], [300.0, 50.0], [400.0, 90.0]], [[200.0, 10.0], [300.0, 50.0], [400.0, 0.0]]]
    oc = [[20, 20], [50, 50], [70, 70]]
    ov = [[200.0, 10.0], [300.0, 50.0], [400.0, 0.0]]
    st = _stats(count, volume, q, thr, oc, ov, [100, 100])
    got = hourly_fdc_score(st, "fdc_freq")
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, 2)
    # mean_k |count - obs_count| / n
    assert got.tolist() == [[(10 + 0 + 0) / 3 / 100, (20 + 40 + 20) / 3 / 100], [0.0, 0.0]]
    # mean over the k with obs_volume > 0 of |v - ov| / ov: gage 1 has two such k
    assert hourly_fdc_score(st, "fdc_vol").tolist() == [[(0.5 + 0 + 0) / 3, (1.0 + 0.0) / 2], [0.0, 0.0]]
    # mean over the k with tau > 0 of |q - tau| / tau: gage 1 has two such k
    assert hourly_fdc_score(st, "fdc_quantile").tolist() == [[(0 + 0.5 + 0.5) / 3, (0.5 + 0) / 2], [(1 + 0 + 0) / 3, (0 + 0.5) / 2]]
    # |s - s_obs| / |s_obs|, s = log q(0.2) - log q(0.7): gage 0 has s_obs = log 4; gage 1 has tau(0.7) = 0: NaN
    slope = hourly_fdc_score(st, "fdc_slope")
    np.testing.assert_allclose(slope[:, 0].numpy(), [abs(np.log(8.0) - np.log(4.0)) / np.log(4.0),
                                                     abs(np.log(8.0) - np.log(4.0)) / np.log(4.0)], rtol=1e-15)
    assert torch.isnan(slope[:, 1]).all()
    # other slope_probs; probabilities that are not sampled
    mid = hourly_fdc_score(st, "fdc_slope", slope_probs=(0.2, 0.5))
    np.testing.assert_allclose(mid[:, 0].numpy(), [abs(np.log(8.0 / 2.0) - np.log(2.0)) / np.log(2.0),
                                                   abs(np.log(16.0 / 4.0) - np.log(2.0)) / np.log(2.0)], rtol=1e-15)
    np.testing.assert_allclose(mid[:, 1].numpy(), [abs(0.0 - np.log(2.0)) / np.log(2.0), abs(np.log(4.0) - np.log(2.0)) / np.log(2.0)],
                               rtol=1e-15)
    with pytest.raises(ValueError, match="slope_probs .* must both be among probs"):
        hourly_fdc_score(st, "fdc_slope", slope_probs=(0.25, 0.7))
    with pytest.raises(ValueError, match="metric must be one of"):
        hourly_fdc_score(st, "kge")
    # without the quantiles (a call with thresholds=): the first two still score, the last two are refused
    bare = _stats(count, volume, None, thr, oc, ov, [100, 100])
    assert torch.equal(hourly_fdc_score(bare, "fdc_freq"), got)
    for metric in hf.QUANTILE_METRICS:
        with pytest.raises(ValueError, match="needs the simulated quantiles"):
            hourly_fdc_score(bare, metric)


def test_fdc_scores_nan_rules():
    one = lambda v: [[[v], [v], [v]]]       # noqa: E731
    base = dict(count=one(5), volume=one(5.0), quantile=[[[8.0], [4.0], [2.0]]], thr=[[4.0], [2.0], [1.0]], oc=[[5]] * 3,
                ov=[[5.0]] * 3, n=[10])

    def score(metric, **over):
        return float(hourly_fdc_score(_stats(**{**base, **over}), metric)[0, 0])

    # (log 8 - log 2 against log 4 - log 1: equal up to the rounding of the logarithms)
    assert score("fdc_quantile") == 1.0 and score("fdc_slope") < 1e-15 and score("fdc_freq") == 0.0
    # no scored hour: thresholds +inf, quantiles NaN
    assert np.isnan(score("fdc_freq", n=[0]))
    assert np.isnan(score("fdc_quantile", thr=[[INF]] * 3, quantile=one(NAN)))
    assert np.isnan(score("fdc_slope", thr=[[INF]] * 3, quantile=one(NAN)))
    # a NaN quantile (a NaN hour in the candidate's column) where the observed curve is fine
    assert np.isnan(score("fdc_quantile", quantile=[[[8.0], [NAN], [2.0]]]))
    assert np.isnan(score("fdc_slope", quantile=[[[NAN], [4.0], [2.0]]]))
    assert score("fdc_slope", quantile=[[[8.0], [NAN], [2.0]]]) < 1e-15        # 0.5 is not in the slope
    # no threshold above zero
    assert np.isnan(score("fdc_quantile", thr=[[0.0], [0.0], [-1.0]]))
    assert score("fdc_quantile", thr=[[4.0], [0.0], [-1.0]]) == 1.0
    # the slope: a flow that is not positive on either side, a flat observed segment
    assert np.isnan(score("fdc_slope", quantile=[[[8.0], [4.0], [0.0]]]))
    assert np.isnan(score("fdc_slope", thr=[[4.0], [2.0], [0.0]]))
    assert np.isnan(score("fdc_slope", thr=[[4.0], [2.0], [4.0]]))


def test_population_fdc_score_keeps_its_bits_on_a_saved_dictionary():
    """tests/golden/population_fdc_score.npz: a dictionary and what `population_fdc_score` gave on it before its body
    became the one `hourly_fdc_score` shares."""
    z = np.load(os.path.join(HERE, "golden", "population_fdc_score.npz"))
    f = {k: torch.from_numpy(z[k]) for k in ("count", "volume", "obs_count", "obs_volume", "n_days")}
    for metric in ("fdc_freq", "fdc_vol"):
        got = population_fdc_score({"fdc": f}, metric).numpy()
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), z[metric].view(np.uint64)), metric
    # and the hourly score on the same numbers under its own key
    g = dict(f, n_hours=f["n_days"])
    del g["n_days"]
    assert np.array_equal(hourly_fdc_score({"fdc": g}, "fdc_vol").numpy().view(np.uint64), z["fdc_vol"].view(np.uint64))
    with pytest.raises(ValueError, match="metric must be one of"):
        population_fdc_score({"fdc": f}, "fdc_quantile")                # the daily call has no quantiles


# ---------------------------------------------------------------------------------------------------------------------
# the observed side and the ranks
def test_the_ranks_are_the_index_of_the_thresholds():
    rng = np.random.default_rng(8)
    T, G = 200, 4
    obs = torch.from_numpy(rng.gamma(2.0, 1.0, size=(T, G)).astype(np.float32))
    scored = torch.from_numpy(rng.random((T, G)) < 0.9)
    scored[:, 2] = False
    scored[1:, 3] = False                                               # one scored hour
    n = scored.sum(0)
    rank = hf.fdc_ranks(n, DEFAULT_PROBS)
    assert rank.dtype == torch.int32 and tuple(rank.shape) == (15, G)
    assert (rank[:, 2] == -1).all() and (rank[:, 3] == 0).all()
    for g in (0, 1):
        for k, p in enumerate(DEFAULT_PROBS):
            assert int(rank[k, g]) == min(int(np.floor(p * int(n[g]))), int(n[g]) - 1)
    # reading the sorted observations at the ranks gives the thresholds: what makes `quantile == thresholds` on a series
    # equal to the observations
    thr = fdc_thresholds(torch.where(scored, obs, torch.zeros_like(obs)), scored, DEFAULT_PROBS)
    dll = load_fdclib()
    q = run_quant(dll, obs.numpy(), scored.numpy(), rank.numpy())
    assert np.array_equal(bits(q[:, [0, 1, 3]]), bits(thr.numpy()[:, [0, 1, 3]]))
    assert np.isnan(q[:, 2]).all() and torch.isinf(thr[:, 2]).all()


def test_the_hooks_observed_side():
    T, G = 48, 3
    m, x, params, cand, dcand, n_pair = _problem(T, 4, G, 3)
    gen = torch.Generator().manual_seed(2)
    tgt = torch.rand(T, G, generator=gen) + 0.5
    tgt[5, 0] = NAN
    w = torch.ones(T, G)
    w[7:10, 1] = 0.0
    dev = torch.device("cpu")
    hook = hf._FdcHook(x, tgt, w, None, (0.1, 0.5, 0.9), None, None)
    hook.check(T, G, dev)
    c = hook.curve
    assert set(c) == {"probs", "thresholds", "obs_count", "obs_volume", "n_hours", "rank"}
    assert c["n_hours"].tolist() == [47, 45, 48] and hook.scored.dtype == torch.uint8
    assert hook.scored.sum(0).tolist() == [47, 45, 48] and not hook.scored[5, 0] and not hook.scored[8, 1]
    assert hook.bytes == 8 * 3 * G + 4 * 3 * G + 4 * T * G
    assert "hbvx_gage_population_quantiles" in hook.exports
    # a second check keeps the curve (a search hands one hook to every round)
    hook.parts.append("stale")
    hook.check(T, G, dev)
    assert hook.curve is c and hook.parts == []
    # with a calendar the weights belong to the periods and do not enter; [T,G,1] and float64 are taken
    per = hf._FdcHook(x, tgt[:2], torch.ones(2, G), 24, (0.1, 0.5, 0.9), None, tgt.unsqueeze(-1).double())
    per.check(T, G, dev)
    assert per.curve["n_hours"].tolist() == [47, 48, 48]
    # thresholds: no ranks, no quantile export, the smaller footprint
    thr = hf._FdcHook(x, tgt, None, None, None, torch.ones(2, G), None)
    thr.check(T, G, dev)
    assert "rank" not in thr.curve and thr.curve["probs"] is None and thr.exports == ("hbvx_gage_population_fdc",)
    assert thr.bytes == 8 * 2 * G


# ---------------------------------------------------------------------------------------------------------------------
# refusals
def test_fdc_refusals_happen_before_anything_runs():
    """Host tensors and no library selected: a call that got as far as the module's forward would fail with the package's
    own 'no CPU path' error instead of the refusal under test."""
    T, U, G, P = 48, 4, 3, 3
    m, x, params, cand, dcand, n_pair = _problem(T, U, G, P)
    tgt = torch.rand(T, G, generator=torch.Generator().manual_seed(1)) + 0.5
    state = torch.get_rng_state()

    def stats(target=tgt, **kw):
        return hourly_population_fdc_stats(m, x, params, target, cand, dcand, **kw)

    # hourly_population_stats' own come first and are its own
    with pytest.raises(ValueError, match="needs candidates, distr_candidates or both"):
        hourly_population_fdc_stats(m, x, params, tgt)
    with pytest.raises(ValueError, match="target holds infinities"):
        stats(target=torch.full((T, G), INF))
    with pytest.raises(ValueError, match="max_candidates must be >= 1"):
        stats(max_candidates=0)
    with pytest.raises(ValueError, match="graph=True"):
        hourly_population_fdc_stats(_model(dyn=["parBETA"], graph=True), x, params, tgt, cand, dcand)
    # the levels
    with pytest.raises(ValueError, match="give probs or thresholds, not both"):
        stats(probs=(0.5,), thresholds=torch.ones(1, G))
    for bad in ((), (0.0, 0.5), (0.5, 1.0), (NAN,), [0.5] * 33):
        with pytest.raises(ValueError, match="hourly_population_fdc_stats: .*probs"):
            stats(probs=bad)
    with pytest.raises(ValueError, match="probs must be a sequence"):
        stats(probs=0.5)
    for bad, msg in ((torch.ones(G), r"thresholds must be \[K,3\]"), (torch.ones(2, G + 1), r"thresholds must be \[K,3\]"),
                     (torch.ones(0, G), r"thresholds must be \[K,3\]"), (torch.ones(33, G), "33 thresholds, at most 32"),
                     (torch.ones(2, G).double(), "thresholds must be float32"),
                     (torch.ones(2, G).to("meta"), "thresholds live on meta"),
                     (torch.full((2, G), INF), "thresholds must be finite"), ([[1.0] * G], r"thresholds must be \[K,3\]")):
        with pytest.raises(ValueError, match=msg):
            stats(thresholds=bad)
    # fdc_target
    with pytest.raises(ValueError, match=r"fdc_target must be \[48,3\]"):
        stats(fdc_target=tgt[:40])
    with pytest.raises(ValueError, match=r"fdc_target must be \[48,3\]"):
        stats(fdc_target=tgt[:, 0])
    with pytest.raises(ValueError, match=r"give the observed HOURLY series as fdc_target \[48,3\]"):
        stats(target=tgt[:2], periods=24)
    with pytest.raises(ValueError, match=r"fdc_target must be \[48,3\]"):
        stats(target=tgt[:2], periods=24, fdc_target=tgt[:2])
    assert torch.equal(torch.get_rng_state(), state)
    # what passes every check reaches the model, and host tensors end there
    for kw in (dict(), dict(probs=(0.2, 0.7)), dict(thresholds=torch.ones(32, G)), dict(fdc_target=tgt.unsqueeze(-1).double()),
               dict(target=tgt[:2], periods=24, fdc_target=tgt), dict(weights=torch.ones(T, G))):
        with pytest.raises(Exception) as err:
            stats(**kw)
        assert not isinstance(err.value, ValueError), err.value
    assert callable(m.population_fdc_stats)
    with pytest.raises(ValueError, match="give probs or thresholds, not both"):
        m.population_fdc_stats(x, params, tgt, cand, dcand, probs=(0.5,), thresholds=torch.ones(1, G))


def test_a_record_beyond_the_sorts_cap_is_refused_for_probs_alone():
    T, U, G, P = _abi.GAGE_QUANT_MAX_T + 1, 4, 3, 2
    m, x, params, cand, dcand, n_pair = _problem(T, U, G, P)
    tgt = torch.ones(T, G)
    with pytest.raises(ValueError, match="at most 16384 hours per column; the record has 16385"):
        hourly_population_fdc_stats(m, x, params, tgt, None, dcand)
    with pytest.raises(Exception) as err:
        hourly_population_fdc_stats(m, x, params, tgt, None, dcand, thresholds=torch.ones(2, G))
    assert not isinstance(err.value, ValueError), err.value


def test_search_refusals_of_the_fdc_term():
    T, U, G, P = 48, 4, 3, 3
    m, x, params, cand, dcand, n_pair = _problem(T, U, G, P, dyn=())
    tgt = torch.rand(T, G, generator=torch.Generator().manual_seed(1)) + 0.5
    from hydrodl2_amd.hourly_events import flood_events
    good = flood_events(tgt, 2, 2, 3)

    def search(target=tgt, **kw):
        return hourly_routing_search(m, x, params, target, **kw)

    for bad in (-0.1, 1.1, NAN):
        with pytest.raises(ValueError, match=r"fdc_share must lie in \[0, 1\]"):
            search(fdc_share=bad)
    with pytest.raises(ValueError, match="fdc_share > 0 together with event_share > 0"):
        search(fdc_share=0.5, event_share=0.5, events=good)
    for share in (0.0, 0.5):
        with pytest.raises(ValueError, match="fdc_metric must be one of"):
            search(fdc_share=share, fdc_metric="fdc")
    with pytest.raises(ValueError, match="give the observed HOURLY series as fdc_target"):
        search(fdc_share=0.5, target=tgt[:2], periods=24)
    # the front end's own, before the model runs
    with pytest.raises(ValueError, match=r"hourly_routing_search: probs must lie in \(0, 1\)"):
        search(fdc_share=0.5, fdc_probs=(0.5, 1.5))
    with pytest.raises(ValueError, match=r"fdc_target must be \[48,3\]"):
        search(fdc_share=0.5, fdc_target=tgt[:40])
    with pytest.raises(ValueError, match="target holds infinities"):
        search(fdc_share=0.5, target=torch.full((T, G), INF))
    # fdc_share == 0 does not look at fdc_probs or fdc_target at all; what passes reaches the model
    for kw in (dict(fdc_probs="not probabilities", fdc_target="no series"), dict(fdc_share=0.5),
               dict(fdc_share=1.0, fdc_metric="fdc_quantile", fdc_probs=(0.2, 0.7)),
               dict(fdc_share=0.5, target=tgt[:2], periods=24, fdc_target=tgt)):
        with pytest.raises(Exception) as err:
            search(**kw)
        assert not isinstance(err.value, ValueError), err.value


def test_a_library_without_the_exports_is_named_before_the_primal(monkeypatch):
    T, U, G, P = 48, 4, 3, 3
    m, x, params, cand, dcand, n_pair = _problem(T, U, G, P)
    tgt = torch.rand(T, G, generator=torch.Generator().manual_seed(1)) + 0.5
    import __graft_entry__ as ge
    from hydrodl2_amd import hourly_population as hp
    lib = _abi.Library(ge.build_hip())
    lib.missing.append("hbvx_gage_population_quantiles")        # a library that has the counts alone
    monkeypatch.setattr(hp, "get_library", lambda: lib)
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_gage_population_quantiles"):
        hourly_population_fdc_stats(m, x, params, tgt, cand, dcand)
    # with thresholds the quantile export is not asked for
    with pytest.raises(Exception) as err:
        hourly_population_fdc_stats(m, x, params, tgt, cand, dcand, thresholds=torch.ones(2, G))
    assert "hbvx_gage_population_quantiles" not in str(err.value)
    lib.missing.append("hbvx_gage_population_fdc")
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_gage_population_fdc"):
        hourly_population_fdc_stats(m, x, params, tgt, cand, dcand, thresholds=torch.ones(2, G))
    # the parent's call asks for neither
    with pytest.raises(Exception) as err:
        hydrodl2_amd.hourly_population_stats(m, x, params, tgt, cand, dcand)
    assert "hbvx_gage_population_fdc" not in str(err.value) and "hbvx_gage_population_quantiles" not in str(err.value)


# ---------------------------------------------------------------------------------------------------------------------
# the header, the table and the entry points' own refusals
def test_the_calls_are_exported():
    for name in ("hourly_population_fdc_stats", "hourly_fdc_score"):
        assert getattr(hydrodl2_amd, name) is getattr(hf, name) and name in hydrodl2_amd.__all__
    names = [row[0] for row in _abi.GAGE_FDC_SIGNATURES]
    assert names == ["hbvx_gage_fdc_sizeof", "hbvx_gage_population_fdc", "hbvx_gage_quantiles_workspace_bytes",
                     "hbvx_gage_population_quantiles"]
    assert not set(names) & set(_abi.EXPORTS + _abi.OPTIONAL_EXPORTS)       # a table of its own
    assert all(not row[1] for row in _abi.GAGE_FDC_SIGNATURES)
    assert _abi.ABI_VERSION == 10 and _abi.GAGE_FDC_ABI_VERSION == 1 and _abi.GAGE_QUANT_MAX_T == 16384


def _prototypes():
    with open(os.path.join(ROOT, "include", "hbvx_gage_fdc.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    found = {}
    for ret, name, args in re.findall(r"^(int|uint64_t)\s*(hbvx_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        assert name not in found, name
        found[name] = (ret, [a.strip() for a in " ".join(args.split()).split(",")])
    return found, text


def test_every_row_of_the_new_table_is_a_prototype_of_the_new_header():
    protos, text = _prototypes()
    returns = {"int": C.c_int, "uint64_t": C.c_uint64}
    assert sorted(protos) == sorted(row[0] for row in _abi.GAGE_FDC_SIGNATURES) and len(protos) == 4
    for name, required, restype, argtypes, layout in _abi.GAGE_FDC_SIGNATURES:
        ret, params = protos[name]
        assert len(params) == len(argtypes) and returns[ret] is restype and required is False, name
    assert protos["hbvx_gage_population_fdc"][1] == ["const hbvx_gage_fdc *gf", "void *stream"]
    assert re.search(r"#define HBVX_GAGE_FDC_ABI_VERSION\s+1\b", text)
    assert re.search(r"#define HBVX_GAGE_FDC_MAX_LEV\s+HBVX_POP_FDC_MAX_THR\b", text)       # one limit, not two
    assert re.search(r"#define HBVX_GAGE_QUANT_MAX_T\s+16384\b", text)
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    for name in protos:
        assert name not in lib.missing and hasattr(lib.dll, name), name
    assert lib.dll.hbvx_gage_fdc_sizeof(0) == C.sizeof(_abi.GageFdc) == 24 + 7 * 8
    assert lib.dll.hbvx_gage_fdc_sizeof(1) == 0 and lib.dll.hbvx_gage_fdc_sizeof(-1) == 0
    # the neighbours are what they were
    assert lib.dll.hbvx_gage_events_sizeof(0) == C.sizeof(_abi.GageEvents) and lib.dll.hbvx_version() == 10
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        assert "hbvx_gage_fdc.h" in f.read()                     # a change to the header rebuilds the library
    # the workspace: one series of keys; 0 for what the call refuses
    ws = lib.gage_quantiles_workspace_bytes
    assert ws(3, 40, 70) == 4 * 3 * 40 * 70 and ws(65535, 16384, 100) == 4 * 65535 * 16384 * 100
    assert ws(0, 40, 70) == ws(65536, 40, 70) == ws(3, 0, 70) == ws(3, 16385, 70) == ws(3, 40, 0) == 0


def _fdc_args(**kw):
    gf = _abi.GageFdc(abi_version=_abi.GAGE_FDC_ABI_VERSION, n_cand=4, T=100, G=3, n_lev=5, series=64, scored=64, thr=64,
                      count=64, volume=64, rank=64, quantile=64)
    for k, v in kw.items():
        setattr(gf, k, v)
    return gf


def test_the_abi_refuses_bad_arguments_before_any_launch():
    """Host-side checks (no launch): runs without a GPU on the cross-compiled library."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    big = 4 * 4 * 100 * 3

    def calls(gf, ws=64, ws_bytes=big):
        return (("hbvx_gage_population_fdc", lambda: lib.gage_population_fdc(gf, 0)),
                ("hbvx_gage_population_quantiles", lambda: lib.gage_population_quantiles(gf, ws, ws_bytes, 0)))

    def refused(code, msg, gf, only=None, **kw):
        for who, call in calls(gf, **kw):
            if only is None or only in who:
                with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*{who}: {msg}"):
                    call()

    refused(-1, "gf is NULL", None)
    for v in (0, 2):
        refused(-4, "gf abi_version mismatch", _fdc_args(abi_version=v))
    for n in (0, -1, 65536):
        refused(-2, r"n_cand must be in 1\.\.65535", _fdc_args(n_cand=n))
    for bad in (dict(T=0), dict(G=0), dict(T=-5)):
        refused(-2, "bad T/G", _fdc_args(**bad))
    for n in (0, -1, 33):
        refused(-2, r"n_lev must be in 1\.\.32", _fdc_args(n_lev=n))
    refused(-1, "series is NULL", _fdc_args(series=None))
    refused(-1, "scored is NULL", _fdc_args(scored=None))
    # each export asks for its own pointers and ignores the other's
    refused(-1, "thr is NULL", _fdc_args(thr=None, rank=None, quantile=None), only="fdc")
    for name in ("count", "volume"):
        refused(-1, "count / volume is NULL", _fdc_args(**{name: None}), only="fdc")
    refused(-1, "rank is NULL", _fdc_args(rank=None, thr=None, count=None, volume=None), only="quantiles")
    refused(-1, "quantile is NULL", _fdc_args(quantile=None), only="quantiles")
    # the cap of the sort, before the workspace is looked at; the counts have no such limit (nothing to refuse there
    # but a launch, which this tier does not make)
    refused(-3, "more than 16384 hours per column", _fdc_args(T=16385), only="quantiles", ws=None, ws_bytes=0)
    refused(-1, "workspace missing or too small", _fdc_args(), only="quantiles", ws=None)
    refused(-1, "workspace missing or too small", _fdc_args(), only="quantiles", ws_bytes=big - 1)
    for name in ("hbvx_gage_population_fdc", "hbvx_gage_population_quantiles"):
        lib.missing.append(name)
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_gage_population_fdc"):
        lib.gage_population_fdc(_fdc_args(), 0)
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_gage_population_quantiles"):
        lib.gage_population_quantiles(_fdc_args(), 64, big, 0)
