"""CPU tier: `population_fdc_stats` / `population_fdc_score` (hydrodl2_amd/population_fdc.py), the `fdc_share` term of
`population_search` and the exports of include/hbvx_pop_fdc.h without a GPU -- what the front end refuses before the
model runs (host tensors), the thresholds it derives from exceedance probabilities against their float64 definition,
the observed curve, the two scores against their definitions and NaN rules, the new header's prototypes against
`_abi.POP_FDC_SIGNATURES`, and the entry point's argument checks on the cross-compiled library (no launch)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi, population, population_fdc
from hydrodl2_amd.population import population_search
from hydrodl2_amd.population_fdc import (DEFAULT_PROBS, FDC_METRICS, _fdc_observations, fdc_thresholds,
                                         population_fdc_score, population_fdc_stats)

from .test_hbv_adj import host_math_backend  # noqa: F401  (fixture)
from .test_population_host import _desc, _model
from .test_step_math_host import steptest_lib  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_the_calls_are_exported():
    assert hydrodl2_amd.population_fdc_stats is population_fdc_stats
    assert hydrodl2_amd.population_fdc_score is population_fdc_score
    assert {"population_fdc_stats", "population_fdc_score"} <= set(hydrodl2_amd.__all__)
    names = [row[0] for row in _abi.POP_FDC_SIGNATURES]
    assert names == ["hbvx_pop_fdc_sizeof", "hbvx_population_fdc"]
    assert not set(names) & set(_abi.EXPORTS + _abi.OPTIONAL_EXPORTS) and not set(names) & set(_abi.POPULATION)
    assert all(not row[1] for row in _abi.POP_FDC_SIGNATURES)
    assert _abi.ABI_VERSION == 10 and _abi.POP_FDC_ABI_VERSION == 1 and _abi.POP_FDC_MAX_THR == 32
    assert FDC_METRICS == ("fdc_freq", "fdc_vol")
    assert DEFAULT_PROBS == (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98, 0.99)
    # the moment scores are what they were: the new metrics have a list and a function of their own
    assert population.METRICS == ("sse", "mse", "nse", "kge", "kge12", "r", "alpha", "beta", "pbias")
    assert population.OBJECTIVES == ("sse", "nse", "kge", "kge12")


def _problem(T=8, B=3, P=4):
    hbv = _model(dyn=["parBETA"])
    ny = hbv.learnable_param_count
    g = torch.Generator().manual_seed(3)
    return (hbv, {"x_phy": torch.zeros(T, B, 3)}, torch.zeros(T, B, ny), torch.zeros(P, B, ny - 2),
            torch.rand(T, B, generator=g) + 0.5)


def test_refusals_happen_before_anything_runs():
    """Host tensors: a call that got as far as the module's forward would fail with the package's own 'no CPU path'
    error instead of the refusal under test."""
    T, B, P = 8, 3, 4
    hbv, x, p, cand, tgt = _problem(T, B, P)
    state = torch.get_rng_state()

    def stats(model=hbv, pp=p, target=tgt, candidates=cand, **kw):
        return population_fdc_stats(model, x, pp, candidates, target, **kw)

    # what population_stats refuses
    hourly = hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")({"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}},
                                                                    torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="Hbv_2_hourly"):
        stats(model=hourly)
    hf = {"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}, "train_spatial_chunk_size": 4,
          "simulate_spatial_chunk_size": 4, "simulate_temporal_chunk_size": 4, "train_warmup": 1}
    mts = hydrodl2_amd.load_model("hbv_2_mts", "Hbv_2_mts")({"nmul": 2, "dynamic_params": {"Hbv_2": []}}, hf,
                                                            torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="Hbv_2_mts"):
        stats(model=mts)
    with pytest.raises(NotImplementedError, match="HbvAdj.*Newton"):
        stats(model=_model(("hbv_adj", "HbvAdj")), pp=torch.zeros(T, B, 12 * 2 + 2))
    with pytest.raises(ValueError, match="graph=True"):
        stats(model=_model(graph=True))
    with pytest.raises(ValueError, match="comprout"):
        stats(model=_model(nmul=1, comprout=True), pp=torch.zeros(T, B, 14), candidates=torch.zeros(P, B, 14))
    with pytest.raises(ValueError, match="dynamic parameter"):
        stats(names=["parBETA"])
    with pytest.raises(ValueError, match="target must be"):
        stats(target=tgt[:-1])
    with pytest.raises(ValueError, match="infinities"):
        stats(target=torch.full((T, B), INF))
    w = torch.ones(T, B)
    w[2, 1] = -1e-3
    with pytest.raises(ValueError, match="must not be negative"):
        stats(weights=w)
    with pytest.raises(ValueError, match="candidates must be"):
        stats(candidates=cand[:, :2])
    with pytest.raises(ValueError, match="float32"):
        stats(candidates=cand.double())
    with pytest.raises(ValueError, match="transform must be one of"):
        stats(transform="cube")
    with pytest.raises(ValueError, match="eps must be finite and > 0"):
        stats(transform="log", eps=0.0)
    with pytest.raises(ValueError, match="negative target has no square root"):
        stats(target=-tgt, transform="sqrt")
    # the levels
    thr = torch.ones(2, B)
    with pytest.raises(ValueError, match="probs or thresholds, not both"):
        stats(probs=(0.1, 0.5), thresholds=thr)
    for bad in ((0.0, 0.5), (0.5, 1.0), (-0.1,), (1.5,), (NAN,)):
        with pytest.raises(ValueError, match=r"probs must lie in \(0, 1\)"):
            stats(probs=bad)
    with pytest.raises(ValueError, match="at least one exceedance probability"):
        stats(probs=())
    with pytest.raises(ValueError, match="probs must be a sequence"):
        stats(probs=0.5)
    with pytest.raises(ValueError, match="33 probs, at most 32"):
        stats(probs=[(i + 1) / 40 for i in range(33)])
    with pytest.raises(ValueError, match="33 thresholds, at most 32"):
        stats(thresholds=torch.ones(33, B))
    for bad in (torch.ones(B), torch.ones(2, B + 1), torch.ones(2, B, 1), torch.ones(0, B), [[1.0] * B]):
        with pytest.raises(ValueError, match=rf"thresholds must be \[K,{B}\]"):
            stats(thresholds=bad)
    with pytest.raises(ValueError, match="thresholds must be float32"):
        stats(thresholds=thr.double())
    with pytest.raises(ValueError, match="thresholds live on meta"):
        stats(thresholds=thr.to("meta"))
    for bad in (NAN, INF, -INF):
        t = thr.clone()
        t[1, 2] = bad
        with pytest.raises(ValueError, match="thresholds must be finite"):
            stats(thresholds=t)
    # the search's term
    def search(**kw):
        return population_search(hbv, x, p, tgt, **kw)

    for bad in (-0.1, 1.5, NAN):
        with pytest.raises(ValueError, match=r"fdc_share must lie in \[0, 1\]"):
            search(objective="kge", fdc_share=bad)
    with pytest.raises(ValueError, match="objective 'sse'.*no scale to mix with"):
        search(fdc_share=0.3)
    with pytest.raises(ValueError, match="daily streamflow alone"):
        search(objective="kge", fdc_share=0.3, aux_target=tgt, aux_key="SWE")
    with pytest.raises(ValueError, match="daily streamflow alone"):
        search(objective="kge", fdc_share=0.3, periods=4)
    with pytest.raises(ValueError, match="daily streamflow alone"):
        search(objective="kge", fdc_share=0.3, aux_periods=4)
    with pytest.raises(ValueError, match="fdc_metric must be one of"):
        search(objective="kge", fdc_share=0.3, fdc_metric="fdc_mid")
    with pytest.raises(ValueError, match=r"probs must lie in \(0, 1\)"):
        search(objective="kge", fdc_share=0.3, fdc_probs=(0.5, 2.0))
    with pytest.raises(ValueError, match="dy_drop"):
        population_search(_model(dyn=["parBETA"], dy_drop=0.3), x, p, tgt, objective="kge", fdc_share=0.3)
    assert torch.equal(torch.get_rng_state(), state)            # nothing ran: no draw was made


def test_a_library_without_the_export_is_named_before_the_primal(host_math_backend, monkeypatch):  # noqa: F811
    """The host build of the math header has none of the population exports: the call names the first one it needs, before
    the module ran.  A library that has hbvx_population_stats and lacks the new one names the new one."""
    model = _model(dyn=["parBETA"], dy_drop=0.5)
    T, B = 6, 3
    ny = model.learnable_param_count
    xs, p, tgt = {"x_phy": torch.rand(T, B, 3)}, torch.randn(T, B, ny), torch.rand(T, B)
    plain = model.__class__({"nmul": 2, "dynamic_params": {"Hbv": []}}, torch.device("cpu"))
    state = torch.get_rng_state()
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_stats"):
        population_fdc_stats(model, xs, p, torch.zeros(2, B, ny - 2), tgt)
    lib = population.get_library()
    monkeypatch.setattr(lib, "missing", [n for n in lib.missing if n != "hbvx_population_stats"])
    assert "hbvx_population_fdc" in lib.missing
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_fdc"):
        population_fdc_stats(model, xs, p, torch.zeros(2, B, ny - 2), tgt)
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_fdc"):
        population_search(plain, xs, p, tgt, objective="kge", fdc_share=0.5)
    assert torch.equal(torch.get_rng_state(), state)


def test_the_default_search_touches_nothing_new(monkeypatch):
    """With the default fdc_* arguments the search does not reach population_fdc.py or ops.population_fdc: it goes on to
    run the module (which host tensors stop), as the search without the arguments does."""
    hbv, x, p, _, tgt = _problem()
    hbv = _model()
    p = torch.zeros(8, 3, hbv.learnable_param_count)

    def never(*a, **kw):
        raise AssertionError("the FDC path was entered")

    monkeypatch.setattr(population_fdc, "_fdc_request", never)
    monkeypatch.setattr(population_fdc, "_fdc_run", never)
    monkeypatch.setattr(hydrodl2_amd.ops, "population_fdc", never)
    for kw in ({}, {"objective": "kge"}, {"fdc_share": 0.0, "fdc_probs": (0.1, 0.5), "fdc_metric": "fdc_vol"}):
        with pytest.raises(Exception) as e:
            population_search(hbv, x, p, tgt, n_candidates=4, **kw)
        assert not isinstance(e.value, AssertionError), kw
    with pytest.raises(AssertionError, match="the FDC path was entered"):
        population_search(hbv, x, p, tgt, n_candidates=4, objective="kge", fdc_share=0.25)


# ---- thresholds and the observed curve -------------------------------------------------------------------------------

def thresholds64(obs, scored, probs):
    """The definition, basin by basin in Python: the scored observations sorted descending, index min(floor(p n), n - 1)
    with the product in float64; +inf without a scored day."""
    T, B = obs.shape
    out = np.full((len(probs), B), np.inf, dtype=np.float32)
    for b in range(B):
        v = np.sort(obs[scored[:, b], b])[::-1]
        n = len(v)
        for k, pk in enumerate(probs):
            if n:
                out[k, b] = v[min(int(math.floor(np.float64(pk) * np.float64(n))), n - 1)]
    return out


class _Req:
    def __init__(self, T_out, B):
        self.T_out, self.B = T_out, B


def test_thresholds_from_probabilities():
    rng = np.random.default_rng(5)
    T, B = 200, 7
    obs = (rng.gamma(2.0, 1.5, size=(T, B)) + 0.01).astype(np.float32)
    obs[:, 1] = np.round(obs[:, 1])                                  # ties, many of them
    obs[:, 2] = 3.25                                                 # one value
    w = rng.uniform(0.0, 2.0, size=(T, B)).astype(np.float32)
    w[rng.uniform(size=(T, B)) < 0.3] = 0.0
    w[:, 3] = 0.0                                                    # n = 0
    w[:, 4] = 0.0
    w[17, 4] = 1.0                                                   # n = 1
    tgt = obs.copy()
    tgt[rng.uniform(size=(T, B)) < 0.1] = np.nan
    tgt[17, 4] = 2.5
    probs = DEFAULT_PROBS + (0.001, 0.004, 0.999)                    # floor(p n) = 0 at 0.001 and 0.004; the last rank
    scored = np.isfinite(tgt) & (w > 0)
    assert scored[:, 3].sum() == 0 and scored[:, 4].sum() == 1 and 100 < scored[:, 0].sum() < 200
    x = {"x_phy": torch.zeros(T, B, 3)}
    got = _fdc_observations(_Req(T, B), x, torch.from_numpy(tgt).double().unsqueeze(-1), torch.from_numpy(w), probs, None)
    thr = got["thresholds"]
    assert thr.dtype == torch.float32 and tuple(thr.shape) == (len(probs), B)
    want = thresholds64(np.where(scored, tgt, 0).astype(np.float32), scored, probs)
    assert np.array_equal(thr.numpy().view(np.uint32), want.view(np.uint32))
    assert np.isinf(want[:, 3]).all() and (want[:, 4] == 2.5).all() and (want[:, 2][np.isfinite(want[:, 2])] == 3.25).all()
    n = scored.sum(0)
    assert torch.equal(got["n_days"], torch.from_numpy(n)) and got["n_days"].dtype == torch.int64
    assert got["probs"].dtype == torch.float64 and got["probs"].tolist() == list(probs)
    # the observed curve: the float32 comparison obs > tau on the scored days
    obs32 = np.where(scored, tgt, 0).astype(np.float32)
    above = (obs32[None] > want[:, None]) & scored[None]
    assert torch.equal(got["obs_count"], torch.from_numpy(above.sum(1))) and got["obs_count"].dtype == torch.int64
    vol = np.where(above, obs32[None].astype(np.float64), 0.0).sum(1)
    assert got["obs_volume"].dtype == torch.float64 and np.allclose(got["obs_volume"].numpy(), vol, rtol=1e-14, atol=0)
    # tie-free basins: exactly floor(p n) observations lie above tau_k (n - 1 at most)
    for b in (0, 5, 6):
        v = obs32[scored[:, b], b]
        assert len(np.unique(v)) == len(v)
        for k, pk in enumerate(probs):
            assert int(got["obs_count"][k, b]) == min(int(math.floor(pk * n[b])), n[b] - 1), (k, b)
    assert int(got["obs_count"][len(DEFAULT_PROBS), 0]) == 0         # floor(0.001 n) = 0: the largest observation, nothing above
    # with ties fewer lie above; without a scored day none; one value: none
    assert bool((got["obs_count"][:, 1] <= torch.floor(torch.tensor(probs, dtype=torch.float64) * n[1]).long()).all())
    assert got["obs_count"][:, 2].tolist() == [0] * len(probs) and got["obs_count"][:, 3].tolist() == [0] * len(probs)
    assert got["obs_count"][:, 4].tolist() == [0] * len(probs) and got["obs_volume"][:, 3].tolist() == [0.0] * len(probs)
    # without weights and NaNs every day is scored; the helper itself on a bare series
    plain = _fdc_observations(_Req(T, B), x, torch.from_numpy(obs), None, (0.5,), None)
    assert plain["n_days"].tolist() == [T] * B
    every = np.ones((T, B), dtype=bool)
    assert np.array_equal(plain["thresholds"].numpy(), thresholds64(obs, every, (0.5,)))
    assert torch.equal(fdc_thresholds(torch.from_numpy(obs), torch.from_numpy(every), (0.5,)), plain["thresholds"])
    # thresholds of the caller's own: passed through, probs None
    mine = torch.from_numpy(np.stack([obs.mean(0), obs.max(0), obs.min(0) - 1]).astype(np.float32))
    own = _fdc_observations(_Req(T, B), x, torch.from_numpy(obs), None, None, mine)
    assert own["probs"] is None and torch.equal(own["thresholds"], mine)
    assert own["obs_count"][1].tolist() == [0] * B and own["obs_count"][2].tolist() == [T] * B


# ---- the scores ------------------------------------------------------------------------------------------------------

def test_scores_against_their_definitions():
    rng = np.random.default_rng(9)
    P, K, B = 3, 5, 4
    n_days = np.array([100, 40, 0, 7])
    obs_count = rng.integers(0, 30, size=(K, B))
    obs_count[:, 2] = 0
    count = rng.integers(0, 40, size=(P, K, B)).astype(np.int32)
    obs_volume = rng.uniform(1.0, 50.0, size=(K, B))
    obs_volume[1, 0] = 0.0                                           # a level the observations never pass
    obs_volume[:, 1] = 0.0                                           # a basin where they pass none
    volume = rng.uniform(0.0, 60.0, size=(P, K, B)).astype(np.float32)
    volume[1, 3, 3] = np.inf
    volume[2, 0, 0] = np.nan
    stats = {"fdc": {"count": torch.from_numpy(count), "volume": torch.from_numpy(volume),
                     "obs_count": torch.from_numpy(obs_count), "obs_volume": torch.from_numpy(obs_volume),
                     "n_days": torch.from_numpy(n_days)}}
    freq = population_fdc_score(stats, "fdc_freq")
    assert freq.dtype == torch.float64 and tuple(freq.shape) == (P, B)
    for c in range(P):
        for b in range(B):
            if n_days[b] == 0:
                assert math.isnan(float(freq[c, b]))
            else:
                want = np.mean(np.abs(count[c, :, b].astype(np.float64) - obs_count[:, b])) / n_days[b]
                assert abs(float(freq[c, b]) - want) <= 1e-15 * max(want, 1.0), (c, b)
    vol = population_fdc_score(stats, "fdc_vol")
    assert vol.dtype == torch.float64 and tuple(vol.shape) == (P, B)
    for c in range(P):
        for b in range(B):
            ks = [k for k in range(K) if obs_volume[k, b] > 0]
            if not ks or not np.isfinite(volume[c, :, b]).all():
                assert math.isnan(float(vol[c, b])), (c, b)
            else:
                want = np.mean([abs(float(volume[c, k, b]) - obs_volume[k, b]) / obs_volume[k, b] for k in ks])
                assert abs(float(vol[c, b]) - want) <= 1e-14 * max(want, 1.0), (c, b)
    assert math.isnan(float(vol[1, 3])) and math.isnan(float(vol[2, 0])) and bool(torch.isnan(vol[:, 1]).all())
    assert bool(torch.isfinite(vol[0, [0, 2, 3]]).all())
    # a perfect candidate scores zero on both
    same = {"fdc": dict(stats["fdc"], count=torch.from_numpy(obs_count[None].astype(np.int32)),
                        volume=torch.from_numpy(obs_volume[None].astype(np.float32)))}
    same["fdc"]["obs_volume"] = same["fdc"]["volume"][0].double()
    assert population_fdc_score(same, "fdc_freq")[0, [0, 1, 3]].tolist() == [0.0, 0.0, 0.0]
    assert population_fdc_score(same, "fdc_vol")[0, [0, 2, 3]].tolist() == [0.0, 0.0, 0.0]
    for bad in ("kge", "fdc", ""):
        with pytest.raises(ValueError, match="metric must be one of"):
            population_fdc_score(stats, bad)
    with pytest.raises(ValueError, match="metric must be one of"):
        population.population_score(stats, "fdc_freq")               # the moment scores do not learn the new names


# ---- the ABI ---------------------------------------------------------------------------------------------------------

def _prototypes():
    with open(os.path.join(ROOT, "include", "hbvx_pop_fdc.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    found = {}
    for ret, name, args in re.findall(r"^(int|uint64_t|const char \*)\s*(hbvx_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        assert name not in found, name
        args = " ".join(args.split())
        found[name] = (ret, [] if args == "void" else [a.strip() for a in args.split(",")])
    return found, text


def test_every_row_of_the_new_table_is_a_prototype_of_the_new_header():
    protos, text = _prototypes()
    returns = {"int": C.c_int, "uint64_t": C.c_uint64}
    structs = {"hbvx_pop_fdc": _abi.PopFdc, "hbvx_desc": _abi.Desc}
    assert sorted(protos) == sorted(row[0] for row in _abi.POP_FDC_SIGNATURES) and len(protos) == 2
    for name, required, restype, argtypes, layout in _abi.POP_FDC_SIGNATURES:
        ret, params = protos[name]
        assert len(params) == len(argtypes), (name, params)
        assert returns[ret] is restype, name
        assert required is False
        for ptext, ct in zip(params, argtypes):
            named = re.fullmatch(r"const (hbvx_\w+) \*\w+", ptext)
            if named:
                assert ct == C.POINTER(structs[named.group(1)]), (name, ptext)
        if layout is not None:
            assert C.POINTER(layout[1]) in argtypes, name
    assert re.search(r"#define HBVX_POP_FDC_ABI_VERSION\s+1\b", text) and re.search(r"#define HBVX_POP_FDC_MAX_THR\s+32\b", text)
    # the struct's fields, in order, are the binding's
    body = re.search(r"typedef struct hbvx_pop_fdc \{(.*?)\} hbvx_pop_fdc;", text, flags=re.S).group(1)
    fields = [re.sub(r"^\**", "", part.strip().split()[-1]) for part in body.split(";") if part.strip()]
    assert fields == [f[0] for f in _abi.PopFdc._fields_] == ["abi_version", "n_thr", "flow", "thr", "count", "volume"]
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    for name in protos:
        assert name not in lib.missing and hasattr(lib.dll, name), name
    assert lib.dll.hbvx_pop_fdc_sizeof(0) == C.sizeof(_abi.PopFdc) == 8 + C.sizeof(_abi.PopStats) + 24
    assert lib.dll.hbvx_pop_fdc_sizeof(1) == 0 and lib.dll.hbvx_pop_fdc_sizeof(-1) == 0
    assert lib.dll.hbvx_version() == 10
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        assert "hbvx_pop_fdc.h" in f.read()                      # a change to the header rebuilds the library


def _fdc_args(**kw):
    pf = _abi.PopFdc(abi_version=_abi.POP_FDC_ABI_VERSION, n_thr=15, thr=64, count=64, volume=64)
    pf.flow.pop.n_cand, pf.flow.pop.t_first, pf.flow.pop.target, pf.flow.pop.cost = 4, 0, 64, 64
    pf.flow.transform, pf.flow.shift, pf.flow.s1, pf.flow.s2, pf.flow.s3 = 0, 64, 64, 64, 64
    for k, v in kw.items():
        obj, names = pf, k.split("__")
        for name in names[:-1]:
            obj = getattr(obj, name)
        setattr(obj, names[-1], v)
    return pf


def test_the_abi_refuses_bad_arguments_before_any_launch():
    """Host-side checks (no launch): runs without a GPU on the cross-compiled library."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    who = "hbvx_population_fdc: "

    def refused(code, msg, d, pf):
        with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*{msg}"):
            lib.population_fdc(d, pf, 0)

    refused(-1, "desc is NULL", None, _fdc_args())
    refused(-4, "abi_version", _desc(abi_version=9), _fdc_args())
    refused(-1, who + "pf is NULL", _desc(), None)
    for v in (0, 2):
        refused(-4, who + "pf abi_version mismatch", _desc(), _fdc_args(abi_version=v))
    for n in (0, -1, 33, 64):
        refused(-2, who + r"n_thr must be in 1\.\.32", _desc(), _fdc_args(n_thr=n))
    refused(-1, who + "thr is NULL", _desc(), _fdc_args(thr=None))
    refused(-1, who + "count / volume is NULL", _desc(), _fdc_args(count=None))
    refused(-1, who + "count / volume is NULL", _desc(), _fdc_args(volume=None))
    for model, n_param in ((_abi.MODEL_HBVADJ, 12), (_abi.MODEL_HOURLY, 19)):
        d = _desc(model=model, n_param=n_param, ac=64, elev=64)
        for i in range(12, n_param):
            d.p[i].sta, d.p[i].lo, d.p[i].hi = 64, 0.3, 5.0
        refused(-3, who + "HBV 1.0 / 1.1p / 2.0 only", d, _fdc_args())
    # hbvx_population_stats' own, under the new name
    refused(-1, who + "target is NULL", _desc(), _fdc_args(flow__pop__target=None))
    refused(-1, who + "cost is NULL", _desc(), _fdc_args(flow__pop__cost=None))
    for n in (0, 65536):
        refused(-2, who + "n_cand must be in 1..65535", _desc(), _fdc_args(flow__pop__n_cand=n))
    refused(-2, who + "t_first outside", _desc(), _fdc_args(flow__pop__t_first=20))
    for bad in (-1, 3):
        refused(-3, who + "transform must be", _desc(), _fdc_args(flow__transform=bad))
    refused(-1, who + "shift is NULL", _desc(), _fdc_args(flow__shift=None))
    refused(-1, who + "eps is NULL under HBVX_POP_T_LOG", _desc(), _fdc_args(flow__transform=_abi.POP_T_LOG))
    for name in ("s1", "s2", "s3"):
        refused(-1, who + "s1 / s2 / s3 is NULL", _desc(), _fdc_args(**{"flow__" + name: None}))
    lib.missing.append("hbvx_population_fdc")        # a library built before the export existed
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_fdc"):
        lib.population_fdc(_desc(), _fdc_args(), 0)
