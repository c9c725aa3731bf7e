"""GPU tier: the flow-duration statistics of the hourly population (hbvx_gage_population_fdc and
hbvx_gage_population_quantiles, include/hbvx_gage_fdc.h; `hourly_population_fdc_stats`, `hourly_fdc_score`,
`hourly_routing_search(fdc_share=...)`) on the records 'tiles', 'short' and 'm16_muwts' of
tests/test_hourly_population_gpu.py with its P = 5 candidates, and on synthetic series handed to `ops.gage_fdc` and
`ops.gage_quantiles` directly.

  series only   P = 3, T = 40, G = 70 (two gage groups, the second a partial wave), K = 5, no model: a mask with holes, a
                NaN hour, a plateau AT a threshold, a gage fully masked, a gage whose series is all NaN -- every count,
                volume and quantile against the host restatement (tests/hosttest/gagefdc_host.cpp) bit for bit, the
                quantiles written into a buffer pre-filled with -7;  P = 2, G = 3 at T = 1, 65 (a padded column of 128)
                and 16384 (the cap): the quantiles `==` torch.sort(descending=True) at the ranks, a NaN for a NaN;
                T = 16385 is refused by the ABI with HBVX_E_UNSUPPORTED;
  own series    counts equal (series > tau).sum over the scored hours of the call's own [P,T,G] series exactly, volumes
                have the host restatement's bits, quantiles equal torch.sort of that series at the ranks, the four sums
                and the period means have `hourly_population_stats`' bits, hourly and with periods=24 + fdc_target; the
                observed series handed in as the series gives quantile == thresholds bit for bit;
  bit rules     two calls agree; a candidate alone or in another order; max_candidates 2 and 1; K = 1 against K = 15; the
                levels permuted; return_series on or off; `thresholds=` against `probs` at the same levels;
  module route  against P module forwards with the candidate substituted, tol_t = FLUX_ATOL + FLUX_RTOL |y_mod,t|
                (tests/abi_util.py).  A sort is 1-Lipschitz in the sup norm: |q_k - q_k,mod| <= max_t tol_t.  A count moves
                by at most the scored hours with |y_mod,t - tau_k| <= tol_t.  A volume by at most the sum of tol_t over
                the hours above tau_k on both routes plus the sum of |y_mod,t| + tol_t over the hours within tol_t of it.
                Nothing is skipped.  Largest measured shares of the three bounds on an MI355X (quantile / count /
                volume): 0 / 0 / 6.0e-3 on 'tiles', 0 / 0 / 5.7e-5 on 'short', 0 / 0 / 2.6e-4 on 'm16_muwts' -- the
                call's series has the module's bits, so the quantiles and counts are the module route's exactly and
                what is left of the volume is the float32 rounding of the ordered sum against a float64 one;
  search        'tiles', 8 candidates, 2 rounds, seeded: the cost never rises, the returned rows re-evaluated by a plain
                `hourly_population_fdc_stats` call reproduce history['cost'][-1], stage 1 never launches, fdc_share=0 is
                the existing search bit for bit with and without fdc_probs, fdc_share > 0 records history['score_fdc']."""
import numpy as np
import pytest
import torch

from hydrodl2_amd import _abi, ops
from hydrodl2_amd.hourly_events import hourly_routing_search
from hydrodl2_amd.hourly_fdc import fdc_ranks, hourly_fdc_score, hourly_population_fdc_stats
from hydrodl2_amd.population import _mixed_cost, _objective_cost, population_score
from hydrodl2_amd.population_fdc import DEFAULT_PROBS

from . import abi_util as au
from .test_gage_fdc_host import load_fdclib, run_fdc, run_quant
from .test_hourly_population_gpu import (DEV, KEYS, P, bits, call, case, hourly_target, kwargs_of, module_route, observations,
                                         staged)

pytestmark = pytest.mark.gpu

NAMES = ("tiles", "short", "m16_muwts")


@pytest.fixture(scope="module")
def fdclib():
    return load_fdclib()


def same(a, b):
    """torch.equal that takes a NaN for a NaN (the quantiles of a gage without a scored hour)."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


def sorted_at(series, scored, rank):
    """[P,K,G]: torch.sort(descending) of the scored hours of every [P,T,G] column at rank [K,G]; NaN where the rank is
    outside 0..n-1 or a scored hour of the column is NaN."""
    low = torch.full_like(series, -float("inf"))
    ranked = torch.where(scored.bool().unsqueeze(0), series, low).sort(1, descending=True).values
    n = scored.bool().sum(0)
    T = series.shape[1]
    idx = rank.long().clamp(0, T - 1).unsqueeze(0).expand(series.shape[0], -1, -1)
    q = ranked.gather(1, idx)
    bad = ((rank < 0) | (rank.long() >= n.unsqueeze(0))).unsqueeze(0) | \
        (torch.isnan(series) & scored.bool().unsqueeze(0)).any(1).unsqueeze(1)
    return torch.where(bad, torch.full_like(q, float("nan")), q)


def check_against_host(dll, series, scored, thr, rank, count, volume, quantile, what):
    sc, th = scored.cpu().numpy(), thr.cpu().numpy()
    for c in range(series.shape[0]):
        y = series[c].cpu().numpy()
        wc, wv = run_fdc(dll, y, sc, th)
        assert np.array_equal(count[c].cpu().numpy(), wc), f"{what}: count of candidate {c}"
        assert np.array_equal(volume[c].cpu().numpy().view(np.uint32), wv.view(np.uint32)), f"{what}: volume of candidate {c}"
        if quantile is not None:
            wq = run_quant(dll, y, sc, rank.cpu().numpy())
            assert np.array_equal(quantile[c].cpu().numpy().view(np.uint32), wq.view(np.uint32)), \
                f"{what}: quantile of candidate {c}"


def test_a_series_alone_through_the_ops_layer(hip_backend, fdclib):
    assert ops._POISON, "the GPU tier runs with poisoned output buffers"
    Pn, T, G, K = 3, 40, 70, 5
    rng = np.random.default_rng(71)
    series = np.round(rng.gamma(2.0, 1.5, size=(Pn, T, G)) * 4).astype(np.float32) / np.float32(4)     # ties are common
    scored = rng.random((T, G)) < 0.8                   # a mask with holes
    thr = np.quantile(series[0], [0.9, 0.5, 0.1, 0.99, 0.0], axis=0).astype(np.float32)                # any order
    series[0, 12, ::3] = np.nan                         # a NaN hour, scored at most of these gages
    scored[12, 0] = True
    series[1, 20:24, 5] = thr[1, 5]                     # a plateau AT a threshold
    scored[20:24, 5] = True
    scored[:, 65] = False                               # a gage of the partial wave fully masked
    series[2, :, 66] = np.nan                           # a gage whose whole series is NaN
    series[1, 3, 69], series[1, 4, 69] = np.float32(-0.0), np.float32(0.0)
    thr[4, 69] = np.float32(0.0)                        # -0 and +0 against a +0 threshold, in the last lane
    n = scored.sum(0).astype(np.int64)
    rank = np.stack([np.zeros(G, np.int64), n // 3, n - 1, np.full(G, -1), n]).astype(np.int32)
    ser, sc, th, rk = (torch.from_numpy(a).to(DEV) for a in (series, scored, thr, rank))
    count, volume = ops.gage_fdc(ser, sc, th)
    # the quantiles into a buffer of this test's own, pre-filled with -7: the poison of `ops` is a NaN, which a quantile
    # may be
    lib = hip_backend
    quantile = torch.full((Pn, K, G), -7.0, device=DEV)
    ws_bytes = lib.gage_quantiles_workspace_bytes(Pn, T, G)
    assert ws_bytes == 4 * Pn * T * G
    ws = torch.full((ws_bytes // 4,), float("nan"), device=DEV)
    sc8 = sc.to(torch.uint8)
    gf = _abi.GageFdc(abi_version=_abi.GAGE_FDC_ABI_VERSION, n_cand=Pn, T=T, G=G, n_lev=K, series=ser.data_ptr(),
                      scored=sc8.data_ptr(), rank=rk.data_ptr(), quantile=quantile.data_ptr())
    lib.gage_population_quantiles(gf, ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert tuple(count.shape) == (Pn, K, G) and count.dtype == torch.int32 and volume.dtype == torch.float32
    assert int((count < 0).sum()) == 0 and not bool(torch.isnan(volume).any()), "a slot was not written"
    assert not bool((quantile == -7.0).any()), "a quantile was not written"
    check_against_host(fdclib, ser, sc, th, rk, count, volume, quantile, "series only")
    viaops = ops.gage_quantiles(ser, sc, rk)
    assert torch.equal(bits(viaops), bits(quantile)), "ops.gage_quantiles against the direct call"
    # the cases by hand
    assert bool((count[:, :, 65] == 0).all()) and bool((volume[:, :, 65] == 0).all()) and bool(torch.isnan(quantile[:, :, 65]).all())
    assert bool((count[2, :, 66] == 0).all()) and bool(torch.isnan(quantile[2, :, 66]).all())
    assert bool(torch.isnan(quantile[0, :, 0]).all()) and bool(torch.isfinite(quantile[1, :3, 0]).all())
    assert bool(torch.isnan(quantile[:, 3:, :]).all())                          # rank -1 and rank n
    above = int(((series[1, :, 5] > thr[1, 5]) & scored[:, 5]).sum())
    assert int(count[1, 1, 5]) == above <= int(n[5]) - 4                        # the plateau is not above its threshold
    assert same(quantile, sorted_at(ser, sc, rk)), "torch.sort at the ranks"
    # bit rules at the ops layer: twice, a candidate alone, a level alone, the levels permuted
    again = ops.gage_fdc(ser, sc, th) + (ops.gage_quantiles(ser, sc8, rk),)
    alone = ops.gage_fdc(ser[1:2].contiguous(), sc, th) + (ops.gage_quantiles(ser[1:2].contiguous(), sc, rk),)
    order = [3, 0, 4, 2, 1]
    perm = ops.gage_fdc(ser, sc, th[order].contiguous()) + (ops.gage_quantiles(ser, sc, rk[order].contiguous()),)
    single = ops.gage_fdc(ser, sc, th[2:3].contiguous()) + (ops.gage_quantiles(ser, sc, rk[2:3].contiguous()),)
    for k, base in enumerate((count, volume, quantile)):
        assert torch.equal(bits(again[k]), bits(base)), "two calls"
        assert torch.equal(bits(alone[k]), bits(base[1:2])), "a candidate alone"
        assert torch.equal(bits(perm[k]), bits(base[:, order])), "the levels permuted"
        assert torch.equal(bits(single[k]), bits(base[:, 2:3])), "a level alone"
    # the ops layer's own checks
    with pytest.raises(TypeError, match="thresholds must be a torch.float32 tensor"):
        ops.gage_fdc(ser, sc, th.double())
    with pytest.raises(TypeError, match="rank must be a torch.int32 tensor"):
        ops.gage_quantiles(ser, sc, rk.long())
    with pytest.raises(TypeError, match="scored must be a bool or uint8 tensor"):
        ops.gage_fdc(ser, sc.float(), th)
    with pytest.raises(ValueError, match=r"scored must be a contiguous \[40,70\]"):
        ops.gage_fdc(ser, sc[:, :69].contiguous(), th)
    with pytest.raises(ValueError, match=r"thresholds must be a contiguous \[K,70\]"):
        ops.gage_fdc(ser, sc, th.cpu())
    with pytest.raises(ValueError, match=r"rank must be a contiguous \[K,70\]"):
        ops.gage_quantiles(ser, sc, rk.repeat(7, 1))
    with pytest.raises(ValueError, match=r"series must be a contiguous \[P,T,G\]"):
        ops.gage_fdc(ser.transpose(1, 2), sc, th)


@pytest.mark.parametrize("T", [1, 65, 16384])
def test_quantiles_against_torch_sort(hip_backend, T):
    Pn, G = 2, 3
    gen = torch.Generator().manual_seed(100 + T)
    ser = (torch.randn(Pn, T, G, generator=gen) * 3).to(DEV)
    sc = (torch.rand(T, G, generator=gen) < 0.9).to(DEV)
    sc[0] = torch.tensor([True, True, False], device=DEV)           # (T = 1: two columns of one hour, one of none)
    if T > 1:
        sc[:, 2] = True                                             # a full column: n = T, the padding alone below it
        ser[1, T // 2, 1] = float("nan")
        sc[T // 2, 1] = True                                        # a scored NaN in candidate 1 of gage 1
        ser[0, :2, 0] = torch.tensor([0.0, -0.0])
    n = sc.sum(0)
    rows = [torch.zeros_like(n), n // 2, n - 1, n, torch.full_like(n, -1), (n * 99) // 100, torch.full_like(n, T)]
    rk = torch.stack(rows).to(torch.int32).contiguous()
    got = ops.gage_quantiles(ser.contiguous(), sc, rk)
    want = sorted_at(ser, sc, rk)
    torch.cuda.synchronize()
    assert same(got, want), f"T = {T}"
    assert bool(torch.isnan(got[:, 3:5]).all()) and bool(torch.isnan(got[:, 6]).all())
    assert bool(torch.isfinite(got[0, :3, :2]).all())
    if T == 1:
        assert bool(torch.isnan(got[:, :, 2]).all()) and torch.equal(bits(got[:, 0, :2]), bits(ser[:, 0, :2]))
    if T > 1:
        assert bool(torch.isnan(got[1, :, 1]).all()) and bool(torch.isfinite(got[0, :3, 1]).all())
    # a value of the series, bit for bit
    pool = set(ser[0, :, 0].cpu().numpy().view(np.uint32).tolist())
    assert set(got[0, :3, 0].cpu().numpy().view(np.uint32).tolist()) <= pool


def test_a_record_beyond_the_cap_is_refused_by_the_abi(hip_backend):
    T, G = _abi.GAGE_QUANT_MAX_T + 1, 3
    ser = torch.ones(1, T, G, device=DEV)
    sc = torch.ones(T, G, dtype=torch.bool, device=DEV)
    rk = torch.zeros(1, G, dtype=torch.int32, device=DEV)
    with pytest.raises(_abi.HbvxError, match=r"\(-3\).*hbvx_gage_population_quantiles: more than 16384 hours per column"):
        ops.gage_quantiles(ser, sc, rk)
    # the counts and volumes have no such limit
    count, volume = ops.gage_fdc(ser, sc, torch.full((1, G), 0.5, device=DEV))
    assert bool((count == T).all()) and bool((volume == T).all())


def fdc_call(name, mode, cal, **kw):
    cs = case(name)
    tgt, w, _ = observations(name, cal)
    cs.prepare()
    args = kwargs_of(cs, mode)
    args.update(kw)
    if cal is not None:
        args.setdefault("fdc_target", hourly_target(name))
    return hourly_population_fdc_stats(cs.model, cs.xd, cs.p, tgt, weights=w, periods=cal, transform="none", **args)


def observed_side(name, cal):
    """(obs [T,G] float32, scored [T,G] bool) as the call forms them: hourly, the target's finite hours with a weight > 0;
    with a calendar, the finite hours of fdc_target."""
    if cal is None:
        tgt, w, _ = observations(name, None)
        return tgt.float(), torch.isfinite(tgt) & (w > 0)
    obs = hourly_target(name)
    return obs.float(), torch.isfinite(obs)


@pytest.mark.parametrize("name,mode", [(n, "both") for n in NAMES] + [("tiles", "routing")])
def test_the_curve_of_the_calls_own_series(hip_backend, fdclib, name, mode):
    cs = case(name)
    K = len(DEFAULT_PROBS)
    series = staged(name, mode, None, "none")[3]                    # [P,T,G]: the call's own hourly gage series
    first = None
    for cal in (None, 24):
        obs, scored = observed_side(name, cal)
        before = dict(ops.HOURLY_POP_LAUNCHES)
        got = fdc_call(name, mode, cal, return_series=True)
        launched = {k: ops.HOURLY_POP_LAUNCHES[k] - before[k] for k in before}
        assert launched == {"runoff": 0 if mode == "routing" else 1, "gage": 1}, launched
        f = got["fdc"]
        tau, rank = f["thresholds"], f["rank"]
        assert tuple(f["count"].shape) == (P, K, cs.G) and f["count"].dtype == torch.int32
        assert f["volume"].dtype == torch.float32 and f["quantile"].dtype == torch.float32 and rank.dtype == torch.int32
        assert torch.equal(f["n_hours"], scored.sum(0)) and torch.equal(rank, fdc_ranks(f["n_hours"], DEFAULT_PROBS))
        above = (series.unsqueeze(1) > tau.unsqueeze(0).unsqueeze(2)) & scored.unsqueeze(0).unsqueeze(0)    # [P,K,T,G]
        assert torch.equal(f["count"].long(), above.sum(2)), "count is not (series > tau).sum over the scored hours"
        check_against_host(fdclib, series, scored, tau, rank, f["count"], f["volume"], f["quantile"], f"{name} periods={cal}")
        assert same(f["quantile"], sorted_at(series, scored, rank)), "quantile is not torch.sort at the ranks"
        seen = f["n_hours"] > 0
        assert bool(torch.isfinite(f["quantile"][:, :, seen]).all()) and bool(torch.isnan(f["quantile"][:, :, ~seen]).all())
        assert bool((f["count"][:, :, ~seen] == 0).all()) and bool(torch.isinf(tau[:, ~seen]).all())
        # the observed series as the series: its own curve at the ranks IS the thresholds
        mine = ops.gage_quantiles(torch.where(scored, obs, torch.zeros_like(obs)).unsqueeze(0).contiguous(), scored, rank)
        assert torch.equal(bits(mine[0][:, seen]), bits(tau[:, seen])), "quantile != thresholds on the observed series"
        oc, ov = ops.gage_fdc(torch.where(scored, obs, torch.zeros_like(obs)).unsqueeze(0).contiguous(), scored, tau)
        assert torch.equal(oc[0].long(), f["obs_count"])
        for metric in ("fdc_freq", "fdc_vol", "fdc_quantile", "fdc_slope"):
            score = hourly_fdc_score(got, metric)
            assert tuple(score.shape) == (P, cs.G) and score.dtype == torch.float64
            assert bool(torch.isnan(score[:, ~seen]).all()), metric
            if metric != "fdc_slope":
                assert bool(torch.isfinite(score[:, seen]).all()), metric
        # the rest of the dictionary has hourly_population_stats' bits
        plain = call(name, mode, cal, "none", return_series=True)
        for k in KEYS + ("series",):
            assert torch.equal(bits(got[k]), bits(plain[k])), f"{k} under periods={cal}"
        assert sorted(set(got) - set(plain)) == ["fdc"]
        for k in plain["outputs"]:
            assert torch.equal(got["outputs"][k], plain["outputs"][k])
        first = first or got
    assert int(first["fdc"]["count"].sum()) > 0


def test_the_bit_rules(hip_backend):
    name, mode = "tiles", "both"
    cs = case(name)
    base = fdc_call(name, mode, 24, return_series=True)
    again = fdc_call(name, mode, 24)
    split = fdc_call(name, mode, 24, max_candidates=2)
    one = fdc_call(name, mode, 24, max_candidates=1)
    order = [3, 0, 4, 2, 1]
    shuffled = fdc_call(name, mode, 24, candidates=cs.cand[order].contiguous(), distr_candidates=cs.dcand[order].contiguous())
    alone = fdc_call(name, mode, 24, candidates=cs.cand[2:3].contiguous(), distr_candidates=cs.dcand[2:3].contiguous())
    assert "series" in base and "series" not in again
    slots = ("count", "volume", "quantile")
    for k in slots:
        b = base["fdc"][k]
        for other, what in ((again, "a second call, return_series off"), (split, "max_candidates=2"), (one, "max_candidates=1")):
            assert torch.equal(bits(other["fdc"][k]), bits(b)), f"{k}: {what}"
        assert torch.equal(bits(shuffled["fdc"][k]), bits(b[order])), f"{k}: another order"
        assert torch.equal(bits(alone["fdc"][k]), bits(b[2:3])), f"{k}: a candidate alone"
    for k in KEYS:
        for other in (again, split, one):
            assert torch.equal(bits(other[k]), bits(base[k])), k
        assert torch.equal(bits(shuffled[k]), bits(base[k][order])) and torch.equal(bits(alone[k]), bits(base[k][2:3]))
    # K = 1 against K = 15, and the levels permuted
    for j in (0, 7, 14):
        row = fdc_call(name, mode, 24, probs=(DEFAULT_PROBS[j],))
        for k in slots + ("thresholds", "rank"):
            full = base["fdc"][k]
            part = full[:, j:j + 1] if full.dim() == 3 else full[j:j + 1]
            assert torch.equal(bits(row["fdc"][k]), bits(part)), f"{k}: level {j} alone"
    lev = list(reversed(range(15)))
    lev[3], lev[9] = lev[9], lev[3]
    perm = fdc_call(name, mode, 24, probs=[DEFAULT_PROBS[j] for j in lev])
    for k in slots:
        assert torch.equal(bits(perm["fdc"][k]), bits(base["fdc"][k][:, lev])), f"{k}: the levels permuted"
    # thresholds= at the same levels: the same counts and volumes, and no quantiles
    thr = fdc_call(name, mode, 24, thresholds=torch.where(torch.isfinite(base["fdc"]["thresholds"]), base["fdc"]["thresholds"],
                                                          torch.zeros_like(base["fdc"]["thresholds"])))
    seen = base["fdc"]["n_hours"] > 0
    for k in ("count", "volume"):
        assert torch.equal(bits(thr["fdc"][k][:, :, seen]), bits(base["fdc"][k][:, :, seen])), f"{k}: thresholds= against probs"
    assert "quantile" not in thr["fdc"] and "rank" not in thr["fdc"] and thr["fdc"]["probs"] is None
    with pytest.raises(ValueError, match="needs the simulated quantiles"):
        hourly_fdc_score(thr, "fdc_quantile")
    # the method is the function
    tgt, w, _ = observations(name, 24)
    cs.prepare()
    meth = cs.model.population_fdc_stats(cs.xd, cs.p, tgt, cs.cand, cs.dcand, names=cs.names, weights=w, periods=24,
                                         fdc_target=hourly_target(name))
    for k in slots:
        assert torch.equal(bits(meth["fdc"][k]), bits(base["fdc"][k]))


@pytest.mark.parametrize("name", NAMES)
def test_fdc_against_the_module_route(hip_backend, name):
    """Largest shares of the three bounds measured on an MI355X (quantile / count / volume): 'tiles' 0 / 0 / 6.0e-3,
    'short' 0 / 0 / 5.7e-5, 'm16_muwts' 0 / 0 / 2.6e-4.  The test prints them."""
    cs = case(name)
    _, flow_want = module_route(name, "both")                       # [P,T,G] from P module forwards
    got = fdc_call(name, "both", None)
    own = staged(name, "both", None, "none")[3].double()            # the call's own series: "above on both routes"
    f = got["fdc"]
    _, scored = observed_side(name, None)
    y = flow_want.double()                                          # [P,T,G]
    tol = au.FLUX_ATOL + au.FLUX_RTOL * y.abs()
    sc = scored.unsqueeze(0)
    tau = f["thresholds"].double()                                  # [K,G]
    seen = f["n_hours"] > 0
    # quantiles: a sort is 1-Lipschitz in the sup norm
    q_mod = sorted_at(y, scored, f["rank"])
    q_bound = torch.where(sc, tol, torch.zeros_like(tol)).max(1).values.unsqueeze(1)           # [P,1,G]
    d_q = (f["quantile"].double() - q_mod).abs()[:, :, seen]
    assert bool(torch.isfinite(d_q).all())
    share_q = float((d_q / q_bound[:, :, seen]).max())
    assert bool((d_q <= q_bound[:, :, seen]).all()), share_q
    # counts and volumes, level by level
    share_c = share_v = 0.0
    for k in range(tau.shape[0]):
        t_k = tau[k].unsqueeze(0).unsqueeze(0)                      # [1,1,G]
        near = sc & ((y - t_k).abs() <= tol)
        above_mod = sc & (y > t_k)
        above_both = above_mod & (own > t_k) & ~near
        c_mod = above_mod.sum(1)
        c_bound = near.sum(1)
        d_c = (f["count"][:, k].long() - c_mod).abs()
        assert bool((d_c <= c_bound)[:, seen].all()), (name, k)
        v_mod = torch.where(above_mod, y, torch.zeros_like(y)).sum(1)
        v_bound = torch.where(above_both, tol, torch.zeros_like(tol)).sum(1) + \
            torch.where(near, y.abs() + tol, torch.zeros_like(tol)).sum(1)
        d_v = (f["volume"][:, k].double() - v_mod).abs()
        assert bool((d_v <= v_bound)[:, seen].all()), (name, k, float((d_v / v_bound.clamp_min(1e-300))[:, seen].max()))
        has = c_bound[:, seen] > 0
        if bool(has.any()):
            share_c = max(share_c, float((d_c[:, seen][has].double() / c_bound[:, seen][has].double()).max()))
        hasv = v_bound[:, seen] > 0
        if bool(hasv.any()):
            share_v = max(share_v, float((d_v[:, seen][hasv] / v_bound[:, seen][hasv]).max()))
    print(f"{name}: largest share of the bound -- quantile {share_q:.3g}, count {share_c:.3g}, volume {share_v:.3g}")


def test_the_routing_search_with_an_fdc_term(hip_backend):
    name = "tiles"
    cs = case(name)
    tgt, w, _ = observations(name, None)
    kw = dict(n_candidates=8, n_rounds=2, weights=w, objective="kge")
    seen = cs.observed_gages().cpu()

    def search(**more):
        cs.prepare()
        return hourly_routing_search(cs.model, cs.xd, cs.p, tgt, generator=torch.Generator().manual_seed(3), **kw, **more)

    before = dict(ops.HOURLY_POP_LAUNCHES)
    (_, _, p_plain), hist_plain = search()
    # fdc_share = 0 is the existing search bit for bit, with and without fdc_probs
    (_, _, p0), hist0 = search(fdc_share=0.0, fdc_probs=(0.2, 0.7), fdc_metric="fdc_slope")
    assert torch.equal(p0, p_plain) and sorted(hist0) == sorted(hist_plain) and all(same(hist_plain[k], hist0[k]) for k in hist0)
    assert "score_fdc" not in hist0
    for metric, probs in (("fdc_freq", None), ("fdc_quantile", (0.05, 0.2, 0.5, 0.7, 0.95))):
        gage_before = ops.HOURLY_POP_LAUNCHES["gage"]
        (p_dyn, p_sta, p_distr), hist = search(fdc_share=0.5, fdc_metric=metric, fdc_probs=probs)
        assert ops.HOURLY_POP_LAUNCHES["gage"] == gage_before + 2
        assert p_dyn is cs.p[0] and p_sta is cs.p[1] and tuple(p_distr.shape) == tuple(cs.p[2].shape)
        cost = hist["cost"]
        assert tuple(cost.shape) == (3, cs.G) and cost.dtype == torch.float64
        assert tuple(hist["score_fdc"].shape) == (3, cs.G) and hist["score_fdc"].dtype == torch.float64
        assert bool((cost[1:] <= cost[:-1]).all()), "a gage's cost rose"
        assert bool(torch.isfinite(cost[:, seen]).all()) and bool(torch.isinf(cost[:, ~seen]).all())
        mixed = 0.5 * (1.0 - hist["score"]) + 0.5 * hist["score_fdc"]
        assert torch.allclose(mixed[:, seen], cost[:, seen], rtol=1e-12, atol=0)
        assert same(hist["score"][0], hist_plain["score"][0])                   # the start is the start
        # the returned rows, evaluated by a plain call, have the cost the history ends on
        cs.prepare()
        st = hourly_population_fdc_stats(cs.model, cs.xd, cs.p, tgt, distr_candidates=p_distr.unsqueeze(0).contiguous(),
                                         weights=w, probs=probs)
        score = population_score(st, "kge")
        sf = hourly_fdc_score(st, metric)
        final = _mixed_cost(_objective_cost(score, "kge"), torch.where(torch.isnan(sf), torch.full_like(sf, float("inf")), sf),
                            0.5)[0].cpu()
        assert torch.equal(final[seen], cost[-1, seen])
        assert torch.equal(hist["score_fdc"][-1][seen], sf[0].cpu()[seen])
    assert ops.HOURLY_POP_LAUNCHES["runoff"] == before["runoff"], "stage 1 ran in a routing-only search"
