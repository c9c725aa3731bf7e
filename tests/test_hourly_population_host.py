"""CPU tier: `hourly_population_stats` (hydrodl2_amd/hourly_population.py) and the exports of include/hbvx_gage_pop.h
without a GPU -- what the front end refuses before the model runs (host tensors), its observation side per gage against
a float64 restatement, its calendars, the entry points' argument checks on the cross-compiled library (no launch), the
new header's prototypes against `_abi.GAGE_POP_SIGNATURES`, `population_score` on a [P,G] result, and the host
restatement of the scorer (tests/hosttest/gagepop_host.cpp: PeriodMean and BasinStats::score over a [T,G] series)
against float64 with the bounds of tests/test_popstats_host.py and tests/test_popperiod_host.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi
from hydrodl2_amd.hourly_population import hourly_population_columns, hourly_population_stats
from hydrodl2_amd.population import _calendar, population_score

from .test_hbv_adj import host_math_backend  # noqa: F401  (fixture)
from .test_pop_host import gamma
from .test_popperiod_host import check_means
from .test_popstats_host import TRANSFORMS, bits, check_chains, observed
from .test_population_host import _desc
from .test_step_math_host import steptest_lib  # noqa: F401  (fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hosttest", "gagepop_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libgagepop_host.so")
HDR = os.path.join(ROOT, "hydrodl2_amd", "csrc", "hbv_pop.h")
NAN, INF = float("nan"), float("inf")


def _model(dyn=(), **cfg):
    cfg = {"nmul": 2, "dynamic_params": {"Hbv_2_hourly": list(dyn)}, **cfg}
    return hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")(cfg, torch.device("cpu"))


@pytest.fixture(scope="module")
def gagelib():
    newest = max(os.path.getmtime(f) for f in (SRC, HDR))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    dll = C.CDLL(LIB)
    dll.gagepop_host.argtypes = [C.c_int] * 4 + [C.c_void_p] * 9
    dll.gagepop_host.restype = C.c_int
    return dll


def run_host(dll, transform, ends, series, ot, w, shift, eps):
    """(period means [K,G], their transform [K,G], the four sums [4,G]) of tests/hosttest/gagepop_host.cpp."""
    T, G = series.shape
    K = len(ends)
    ends = np.ascontiguousarray(ends, dtype=np.int32)
    for arr in (series, ot, w, shift, eps):
        assert arr is None or (arr.flags["C_CONTIGUOUS"] and arr.dtype == np.float32)
    assert ot.shape == (K, G)
    mean, mean_t = (np.full((K, G), np.nan, dtype=np.float32) for _ in range(2))
    out = np.full((4, G), np.nan, dtype=np.float32)
    ptr = lambda arr: None if arr is None else arr.ctypes.data      # noqa: E731
    rc = dll.gagepop_host(T, G, K, TRANSFORMS[transform], ptr(ends), ptr(series), ptr(ot), ptr(w), ptr(shift), ptr(eps),
                          ptr(mean), ptr(mean_t), ptr(out))
    assert rc == 0
    return mean, mean_t, out


def test_the_call_is_exported():
    assert hydrodl2_amd.hourly_population_stats is hourly_population_stats
    assert {"hourly_population_stats", "hourly_population_columns"} <= set(hydrodl2_amd.__all__)
    names = [row[0] for row in _abi.GAGE_POP_SIGNATURES]
    assert not set(names) & set(_abi.EXPORTS + _abi.OPTIONAL_EXPORTS)       # a table of its own
    assert all(not row[1] for row in _abi.GAGE_POP_SIGNATURES)
    assert _abi.ABI_VERSION == 10 and _abi.GAGE_POP_ABI_VERSION == 1
    assert callable(_model().population_stats)


def test_the_columns_helper():
    m = _model(dyn=["parBETA", "parK0"])
    static = [n for n in m.parameter_bounds if n not in ("parBETA", "parK0")]
    assert hourly_population_columns(m) == list(range(2 * len(static)))
    assert hourly_population_columns(m, ["parFC"]) == [0, 1]                # parBETA is dynamic: parFC is static column 0
    i = static.index("parALPHA")
    assert hourly_population_columns(m, ["parALPHA", "parFC"]) == [2 * i, 2 * i + 1, 0, 1]
    with pytest.raises(ValueError, match="dynamic parameter"):
        hourly_population_columns(m, ["parBETA"])
    with pytest.raises(ValueError, match="unknown parameter name"):
        hourly_population_columns(m, ["route_a"])
    with pytest.raises(ValueError, match="listed twice"):
        hourly_population_columns(m, ["parFC", "parFC"])
    with pytest.raises(NotImplementedError, match="Hbv_2_hourly"):
        hourly_population_columns(hydrodl2_amd.load_model("hbv_2", "Hbv_2")({"nmul": 2, "dynamic_params": {"Hbv_2": []}}, torch.device("cpu")))


def _problem(T=48, U=4, G=3, P=3, dyn=("parBETA",), **cfg):
    m = _model(dyn=dyn, **cfg)
    topo = torch.tensor([[1, 1, 0, 0], [0, 1, 1, 1], [0, 0, 0, 1]], dtype=torch.float32)[:G, :U]
    x = {"x_phy": torch.zeros(T, U, 3), "ac_all": torch.ones(U), "elev_all": torch.ones(U), "outlet_topo": topo,
         "areas": torch.ones(U)}
    n_pair = int(topo.sum())
    params = (torch.zeros(T, U, m.learnable_param_count1), torch.zeros(U, m.learnable_param_count2),
              torch.zeros(n_pair, 3))
    C_all = len(hourly_population_columns(m))
    return m, x, params, torch.zeros(P, U, C_all), torch.zeros(P, n_pair, 3), n_pair


def test_refusals_happen_before_anything_runs():
    """Host tensors and no library selected: a call that got as far as the module's forward would fail with the package's
    own 'no CPU path' error instead of the refusal under test."""
    T, U, G, P = 48, 4, 3, 3
    m, x, params, cand, dcand, n_pair = _problem(T, U, G, P)
    tgt = torch.rand(T, G, generator=torch.Generator().manual_seed(1)) + 0.5
    tgt2 = tgt[:2].clone()
    state = torch.get_rng_state()

    def stats(model=m, target=tgt, candidates=cand, distr_candidates=dcand, **kw):
        return hourly_population_stats(model, x, params, target, candidates, distr_candidates, **kw)

    # the model and its modes
    daily = hydrodl2_amd.load_model("hbv_2", "Hbv_2")({"nmul": 2, "dynamic_params": {"Hbv_2": []}}, torch.device("cpu"))
    hf = {"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}, "train_spatial_chunk_size": 4,
          "simulate_spatial_chunk_size": 4, "simulate_temporal_chunk_size": 4, "train_warmup": 1}
    mts = hydrodl2_amd.load_model("hbv_2_mts", "Hbv_2_mts")({"nmul": 2, "dynamic_params": {"Hbv_2": []}}, hf,
                                                            torch.device("cpu"))
    for other, name in ((daily, "Hbv_2"), (mts, "Hbv_2_mts")):
        with pytest.raises(NotImplementedError, match=f"not {name}"):
            stats(model=other)
    with pytest.raises(ValueError, match="graph=True"):
        stats(model=_model(dyn=["parBETA"], graph=True))
    init = _model(dyn=["parBETA"])
    init.initialize = True
    with pytest.raises(ValueError, match="initialize mode"):
        stats(model=init)
    with pytest.raises(ValueError, match="cache_states=True"):
        stats(model=_model(dyn=["parBETA"], cache_states=True))
    with pytest.raises(ValueError, match="routing=True"):
        stats(model=_model(dyn=["parBETA"], routing=True))
    off = _model(dyn=["parBETA"])
    off.use_distr_routing = False
    with pytest.raises(ValueError, match="use_distr_routing=False"):
        stats(model=off)
    # the candidates
    with pytest.raises(ValueError, match="needs candidates, distr_candidates or both"):
        stats(candidates=None, distr_candidates=None)
    with pytest.raises(ValueError, match="dynamic parameter"):
        stats(names=["parBETA"])
    with pytest.raises(ValueError, match="unknown parameter name"):
        stats(names=["route_tau"])
    with pytest.raises(ValueError, match="names without candidates"):
        stats(candidates=None, names=["parFC"])
    for bad in (cand[0], cand[:, :3], cand[:, :, :5], cand[:0], cand.numpy()):
        with pytest.raises(ValueError, match=r"candidates must be \[P,4,"):
            stats(candidates=bad)
    with pytest.raises(ValueError, match="candidates must be float32"):
        stats(candidates=cand.double())
    with pytest.raises(ValueError, match="candidates lives on meta"):
        stats(candidates=cand.to("meta"))
    for bad in (dcand[0], dcand[:, :2], dcand[:, :, :2], dcand[:0]):
        with pytest.raises(ValueError, match=rf"distr_candidates must be \[P,{n_pair},3\]"):
            stats(distr_candidates=bad)
    with pytest.raises(ValueError, match="distr_candidates must be float32"):
        stats(distr_candidates=dcand.double())
    with pytest.raises(ValueError, match="distr_candidates lives on meta"):
        stats(distr_candidates=dcand.to("meta"))
    with pytest.raises(ValueError, match="candidates hold 3 sets, distr_candidates 2"):
        stats(distr_candidates=dcand[:2])
    for bad in (0, -1):
        with pytest.raises(ValueError, match="max_candidates must be >= 1"):
            stats(max_candidates=bad)
    # the observations
    for bad in (tgt[:-1], tgt[:, :2], tgt.unsqueeze(0)):
        with pytest.raises(ValueError, match=r"target must be \[48, 3\] or \[48, 3, 1\]"):
            stats(target=bad)
    with pytest.raises(ValueError, match="target must be float32 or float64"):
        stats(target=tgt.long())
    with pytest.raises(ValueError, match="target lives on meta"):
        stats(target=tgt.to("meta"))
    inf = tgt.clone()
    inf[3, 1] = INF
    with pytest.raises(ValueError, match="target holds infinities"):
        stats(target=inf)
    with pytest.raises(ValueError, match=r"weights must be \[48, 3\]"):
        stats(weights=torch.ones(T, G, 1))
    w = torch.ones(T, G)
    w[0, 0] = -1.0
    with pytest.raises(ValueError, match="weights must not be negative"):
        stats(weights=w)
    w[0, 0] = NAN
    with pytest.raises(ValueError, match="weights must be finite"):
        stats(weights=w)
    with pytest.raises(ValueError, match="transform must be one of"):
        stats(transform="cube")
    with pytest.raises(ValueError, match="eps must be finite and > 0"):
        stats(transform="log", eps=0.0)
    with pytest.raises(ValueError, match="negative target has no square root"):
        stats(target=-tgt, transform="sqrt")
    # the calendars: what population._calendar refuses, and a target that is not one row per period
    for bad in (0, -2, T + 1):
        with pytest.raises(ValueError, match=f"periods = {bad} days per period"):
            stats(target=tgt2, periods=bad)
    for bad in ([], [[1, 2]]):
        with pytest.raises(ValueError, match="periods must hold at least one closing day"):
            stats(target=tgt2, periods=bad)
    with pytest.raises(ValueError, match="periods must hold integers"):
        stats(target=tgt2, periods=[1.0, 2.0])
    for bad in ([5, 5], [9, 2], [-1, 4], [4, T]):
        with pytest.raises(ValueError, match=f"strictly ascending closing days in 0..{T - 1}"):
            stats(target=tgt2, periods=bad)
    with pytest.raises(ValueError, match=r"target must be \[2, 3\] or \[2, 3, 1\] \(the 2 periods"):
        stats(periods=24)
    with pytest.raises(ValueError, match=r"target must be \[3, 3\]"):
        stats(target=tgt2, periods=[0, 5, 47])
    assert torch.equal(torch.get_rng_state(), state)            # nothing ran


def test_the_generic_calls_keep_refusing_the_model():
    m, x, params, cand, _, _ = _problem()
    tgt = torch.zeros(48, 4)
    for call in (hydrodl2_amd.population_cost, hydrodl2_amd.population_stats):
        with pytest.raises(NotImplementedError, match="Hbv_2_hourly"):
            call(m, x, params, cand, tgt)
    with pytest.raises(NotImplementedError, match="Hbv_2_hourly"):
        hydrodl2_amd.population_period_stats(m, x, params, cand, tgt, 3)
    with pytest.raises(NotImplementedError, match="Hbv_2_hourly"):
        hydrodl2_amd.population_search(m, x, params, tgt)


def test_a_library_without_the_exports_is_named_before_the_primal(host_math_backend):  # noqa: F811
    m, x, params, cand, dcand, _ = _problem(dyn=("parBETA",), dy_drop=0.5)
    tgt = torch.rand(2, 3) + 0.5
    state = torch.get_rng_state()
    for kw in (dict(candidates=cand), dict(distr_candidates=dcand), dict(candidates=cand, distr_candidates=dcand)):
        with pytest.raises(_abi.HbvxError, match="missing export hbvx_hourly_population_runoff"):
            hourly_population_stats(m, x, params, tgt, periods=24, **kw)
    assert torch.equal(torch.get_rng_state(), state)            # no dy_drop draw: the module did not run


@pytest.mark.parametrize("transform", list(TRANSFORMS))
def test_the_observation_side_per_gage_against_float64(transform, monkeypatch):
    """What the front end hands to the kernel and to population_score -- target', weights, shift, eps, n_obs, W, e1, e2 --
    per GAGE, read off the call the front end makes to the library check that follows its observation side."""
    T, U, G, P = 48, 4, 3, 2
    m, x, params, cand, dcand, _ = _problem(T, U, G, P)
    K = 6
    g = torch.Generator().manual_seed(11)
    tgt = (torch.rand(K, G, generator=g) * 3 + 0.2).double()
    tgt[1, 0] = NAN
    tgt[:, 2] = NAN                                              # a gage without any observation
    w = torch.rand(K, G, generator=g)
    w[4, 1] = 0.0
    seen = {}

    import hydrodl2_amd.hourly_population as hp
    real = hp._observations

    def spy(*a, **kw):
        seen["ob"] = real(*a, **kw)
        raise RuntimeError("stop here")

    monkeypatch.setattr(hp, "_observations", spy)
    with pytest.raises(RuntimeError, match="stop here"):
        hourly_population_stats(m, x, params, tgt.unsqueeze(-1), cand, dcand, weights=w, periods=8, transform=transform)
    ob = seen["ob"]
    miss = torch.isnan(tgt)
    w8 = torch.where(miss, torch.zeros(K, G, dtype=torch.float64), w.float().double())
    o8 = torch.where(miss, torch.zeros_like(tgt), tgt.float().double())
    W = w8.sum(0)
    assert torch.equal(ob["n_obs"], (w8 > 0).sum(0)) and ob["n_obs"].tolist() == [5, 5, 0]
    assert torch.equal(ob["w"], w8.float()) and ob["target"].shape == (K, G) and ob["shift"].shape == (G,)
    if transform == "log":
        eps = torch.where(W > 0, 0.01 * (w8 * o8).sum(0) / W.clamp_min(1e-300), torch.ones(G, dtype=torch.float64)).float()
        assert torch.equal(ob["eps"], eps) and float(ob["eps"][2]) == 1.0
        ot8 = torch.log(o8 + eps.double())
    else:
        assert ob["eps"] is None
        ot8 = torch.sqrt(o8) if transform == "sqrt" else o8
    ot = torch.where(miss, torch.zeros(K, G), ot8.float())
    assert torch.equal(ob["target"], ot) and not bool(torch.isnan(ob["target"]).any())
    shift = torch.where(W > 0, (w8 * ot.double()).sum(0) / W.clamp_min(1e-300), torch.zeros(G, dtype=torch.float64)).float()
    assert torch.equal(ob["shift"], shift) and float(shift[2]) == 0.0
    e = ot.double() - shift.double()
    assert torch.equal(ob["obs"]["W"], W)
    assert torch.allclose(ob["obs"]["e1"], (w8 * e).sum(0), rtol=1e-14, atol=1e-300)
    assert torch.allclose(ob["obs"]["e2"], (w8 * e * e).sum(0), rtol=1e-14, atol=1e-300)


def test_the_calendars():
    cal = lambda p, T: _calendar(p, T, "periods", "hourly_population_stats").tolist()      # noqa: E731
    assert cal(None, 5) == [0, 1, 2, 3, 4]
    assert cal(24, 50) == [23, 47]                   # two days; the two hours left over are not scored
    assert cal(24, 48) == [23, 47]
    assert cal([5, 23, 40], 48) == [5, 23, 40] and cal(torch.tensor([3, 9]), 12) == [3, 9]


def _prototypes():
    with open(os.path.join(ROOT, "include", "hbvx_gage_pop.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    found = {}
    for ret, name, args in re.findall(r"^(int|uint64_t|const char \*)\s*(hbvx_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        assert name not in found, name
        args = " ".join(args.split())
        found[name] = (ret, [] if args == "void" else [a.strip() for a in args.split(",")])
    return found


def test_every_row_of_the_new_table_is_a_prototype_of_the_new_header():
    protos = _prototypes()
    returns = {"int": C.c_int, "uint64_t": C.c_uint64}
    structs = {"hbvx_pop_runoff": _abi.PopRunoff, "hbvx_gage_pop": _abi.GagePop, "hbvx_desc": _abi.Desc,
               "hbvx_gage_desc": _abi.GageDesc}
    assert sorted(protos) == sorted(row[0] for row in _abi.GAGE_POP_SIGNATURES) and len(protos) == 4
    for name, required, restype, argtypes, layout in _abi.GAGE_POP_SIGNATURES:
        ret, params = protos[name]
        assert len(params) == len(argtypes), (name, params)
        assert returns[ret] is restype, name
        assert required is False
        for text, ct in zip(params, argtypes):
            named = re.fullmatch(r"const (hbvx_\w+) \*\w+", text)
            if named:
                assert ct == C.POINTER(structs[named.group(1)]), (name, text)
        if layout is not None:
            assert C.POINTER(layout[1]) in argtypes, name
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    for name in protos:
        assert name not in lib.missing and hasattr(lib.dll, name), name
    assert lib.dll.hbvx_gage_pop_sizeof(0) == C.sizeof(_abi.PopRunoff)
    assert lib.dll.hbvx_gage_pop_sizeof(1) == C.sizeof(_abi.GagePop)
    assert lib.dll.hbvx_gage_pop_sizeof(2) == 0 and lib.dll.hbvx_gage_pop_sizeof(-1) == 0
    assert lib.dll.hbvx_version() == 10
    assert C.sizeof(_abi.PopRunoff) == 8 + _abi.MAX_PARAM * C.sizeof(_abi.PopSrc) + 8
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        assert "hbvx_gage_pop.h" in f.read()                     # a change to the header rebuilds the library


def _hourly_desc(**kw):
    d = _desc(model=_abi.MODEL_HOURLY, n_param=19, ac=64, elev=64)
    for i in range(12, 19):
        d.p[i].sta, d.p[i].sta_b_stride, d.p[i].lo, d.p[i].hi = 64, 24, 0.3, 5.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _runoff_args(**kw):
    pr = _abi.PopRunoff(abi_version=_abi.GAGE_POP_ABI_VERSION, n_cand=4, runoff=64)
    for k, v in kw.items():
        setattr(pr, k, v)
    return pr


def _gage_desc(**kw):
    r = _abi.GageDesc(abi_version=_abi.ABI_VERSION, T=100, U=5, G=3, NPAIR=7, L=72, lag_uh=1, pair_unit=64, gage_ptr=64,
                      pair_gage=64, unit_ptr=64, unit_pairs=64, areas=64, denom=64, dp=64, a_lo=0, a_hi=5, b_lo=0,
                      b_hi=12, tau_lo=0, tau_hi=48)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _gage_args(**kw):
    gp = _abi.GagePop(abi_version=_abi.GAGE_POP_ABI_VERSION, n_cand=4, runoff=64, runoff_c_stride=500, dp=64, uh=None,
                      transform=0, n_periods=4, period_end=64, target=64, shift=64, sse=64, s1=64, s2=64, s3=64)
    for k, v in kw.items():
        setattr(gp, k, v)
    return gp


def test_the_abi_refuses_bad_arguments_before_any_launch():
    """Host-side checks (no launch): runs without a GPU on the cross-compiled library."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())

    def refused(call, code, msg, *args):
        with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*{msg}"):
            call(*args)

    run, who = lambda d, pr: lib.hourly_population_runoff(d, pr, 0), "hbvx_hourly_population_runoff: "      # noqa: E731
    refused(run, -1, "desc is NULL", None, _runoff_args())
    refused(run, -4, "abi_version", _hourly_desc(abi_version=9), _runoff_args())
    refused(run, -3, who + "the hourly model", _desc(), _runoff_args())
    refused(run, -1, who + "pr is NULL", _hourly_desc(), None)
    refused(run, -4, who + "pr abi_version mismatch", _hourly_desc(), _runoff_args(abi_version=2))
    for n in (0, -1, 65536):
        refused(run, -2, who + "n_cand must be in 1..65535", _hourly_desc(), _runoff_args(n_cand=n))
    refused(run, -1, who + "runoff is NULL", _hourly_desc(), _runoff_args(runoff=None))
    extra = _runoff_args()
    extra.p[19].sta = 64
    refused(run, -2, who + "candidate values for a parameter slot the model lacks", _hourly_desc(), extra)

    big = 1 << 40
    st, who = lambda r, gp, ws=64, nb=big: lib.gage_population_stats(r, gp, ws, nb, 0), "hbvx_gage_population_stats: "  # noqa: E731
    refused(st, -1, who + "gage desc is NULL", None, _gage_args())
    refused(st, -4, who + "abi_version mismatch", _gage_desc(abi_version=9), _gage_args())
    for bad in (dict(T=0), dict(U=0), dict(G=-1), dict(NPAIR=-1)):
        refused(st, -2, who + "bad T/U/G/NPAIR", _gage_desc(**bad), _gage_args())
    refused(st, -2, who + r"L must be min\(T, 72\)", _gage_desc(L=71), _gage_args())
    refused(st, -2, who + r"L must be min\(T, 72\)", _gage_desc(T=50), _gage_args())
    refused(st, -2, who + "more than 65535", _gage_desc(G=65536), _gage_args())
    for name in ("pair_unit", "gage_ptr", "areas", "denom"):
        refused(st, -1, who + "gage routing pointer is NULL", _gage_desc(**{name: None}), _gage_args())
    refused(st, -1, who + "gp is NULL", _gage_desc(), None)
    refused(st, -4, who + "gp abi_version mismatch", _gage_desc(), _gage_args(abi_version=0))
    for n in (0, 65536):
        refused(st, -2, who + "n_cand must be in 1..65535", _gage_desc(), _gage_args(n_cand=n))
    refused(st, -1, who + "runoff is NULL", _gage_desc(), _gage_args(runoff=None))
    refused(st, -2, who + "runoff_c_stride is negative", _gage_desc(), _gage_args(runoff_c_stride=-1))
    refused(st, -1, who + "neither dp nor uh", _gage_desc(), _gage_args(dp=None))
    for bad in (-1, 3):
        refused(st, -3, who + "transform must be", _gage_desc(), _gage_args(transform=bad))
    for n in (0, -1, 101):
        refused(st, -2, who + "n_periods must be in 1..T", _gage_desc(), _gage_args(n_periods=n))
    for name in ("period_end", "target", "shift"):
        refused(st, -1, who + f"{name} is NULL", _gage_desc(), _gage_args(**{name: None}))
    refused(st, -1, who + "eps is NULL under HBVX_POP_T_LOG", _gage_desc(), _gage_args(transform=_abi.POP_T_LOG))
    for name in ("sse", "s1", "s2", "s3"):
        refused(st, -1, who + "sse / s1 / s2 / s3 is NULL", _gage_desc(), _gage_args(**{name: None}))
    # the workspace: [P,U,T] + [P,NPAIR,L] + [P,T,G] floats; a caller's series and one shared runoff take their parts out
    r = _gage_desc()
    need = lib.gage_population_workspace_bytes(r, _gage_args())
    assert need == 4 * 4 * (5 * 100 + 7 * 72 + 100 * 3)
    assert lib.gage_population_workspace_bytes(r, _gage_args(series=64)) == 4 * 4 * (5 * 100 + 7 * 72)
    assert lib.gage_population_workspace_bytes(r, _gage_args(runoff_c_stride=0)) == 4 * (5 * 100 + 4 * (7 * 72 + 100 * 3))
    assert lib.gage_population_workspace_bytes(r, _gage_args(dp=None, uh=64)) == 4 * 4 * (5 * 100 + 100 * 3)
    assert lib.gage_population_workspace_bytes(None, _gage_args()) == 0
    assert lib.gage_population_workspace_bytes(r, _gage_args(n_cand=0)) == 0
    refused(st, -1, who + "workspace missing or too small", r, _gage_args(), None)
    refused(st, -1, who + "workspace missing or too small", r, _gage_args(), 64, need - 1)
    lib.missing.append("hbvx_gage_population_stats")        # a library built before the export existed
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_gage_population_stats"):
        st(r, _gage_args())


def test_population_score_on_a_candidate_by_gage_result():
    """A hand-made [P,G] result in the layout the call returns: population_score reads gages as it reads basins."""
    rng = np.random.default_rng(3)
    K, G, P = 40, 3, 2
    o = rng.uniform(1.0, 3.0, size=(K, G))
    y = o[None] * rng.uniform(0.8, 1.2, size=(P, 1, G)) + 0.1 * rng.standard_normal((P, K, G))
    m = o.mean(0).astype(np.float32).astype(np.float64)
    d, e = y - m, (o - m)[None]
    stats = {"sse": torch.from_numpy(((y - o[None]) ** 2).sum(1)).float(), "s1": torch.from_numpy(d.sum(1)).float(),
             "s2": torch.from_numpy((d * d).sum(1)).float(), "s3": torch.from_numpy((d * e).sum(1)).float(),
             "shift": torch.from_numpy(m).float(), "n_obs": torch.full((G,), K, dtype=torch.int64),
             "obs": {"W": torch.full((G,), float(K), dtype=torch.float64), "e1": torch.from_numpy(e[0].sum(0)),
                     "e2": torch.from_numpy((e[0] ** 2).sum(0))}}
    nse = 1 - ((y - o[None]) ** 2).sum(1) / ((o - o.mean(0)) ** 2).sum(0)
    r = np.array([[np.corrcoef(y[c, :, g], o[:, g])[0, 1] for g in range(G)] for c in range(P)])
    alpha, beta = y.std(1) / o.std(0), y.mean(1) / o.mean(0)
    kge = 1 - np.sqrt((r - 1) ** 2 + (alpha - 1) ** 2 + (beta - 1) ** 2)
    for name, want in (("nse", nse), ("r", r), ("alpha", alpha), ("beta", beta), ("kge", kge)):
        got = population_score(stats, name)
        assert got.shape == (P, G) and got.dtype == torch.float64
        assert np.abs(got.numpy() - want).max() < 2e-5, name


def _series(T, G, seed):
    rng = np.random.default_rng(seed)
    y = (rng.gamma(2.0, 1.5, size=(T, G)) + 0.05).astype(np.float32)
    tgt = (y * rng.uniform(0.7, 1.3, size=(T, G)) + 0.02).astype(np.float32)
    w = rng.uniform(0.0, 2.0, size=(T, G)).astype(np.float32)
    w[rng.uniform(size=(T, G)) < 0.1] = 0.0
    return np.ascontiguousarray(y), np.ascontiguousarray(tgt), np.ascontiguousarray(w)


def per_period(daily, weights, ends):
    starts = np.concatenate([[0], ends[:-1] + 1])
    tgt = np.stack([daily[s:e + 1].astype(np.float64).mean(0) for s, e in zip(starts, ends)]).astype(np.float32)
    return np.ascontiguousarray(tgt), np.ascontiguousarray(weights[ends])


@pytest.mark.parametrize("transform", list(TRANSFORMS))
@pytest.mark.parametrize("T,G", [(1, 1), (50, 3), (400, 5), (1100, 7)])
def test_the_scorer_restated_on_the_host_against_float64(gagelib, transform, T, G):
    y, tgt, w = _series(T, G, 1000 * T + G)
    calendars = [None, 1] + ([24, [0] + list(range(7, T, 5))] if T >= 24 else [])
    hourly = None
    for cal in calendars:
        ends = _calendar(cal, T, "periods", "test").numpy().astype(np.int32)
        K = len(ends)
        tk, wk = per_period(tgt, w, ends)
        ot, shift, eps = observed(tk, wk, transform)
        what = f"{transform}, T {T}, calendar {cal}"
        mean, mean_t, out = run_host(gagelib, transform, ends, y, ot, wk, shift, eps)
        check_means(mean, y, ends, what)
        check_chains(out, mean_t, ot, wk, shift, K, 0, what)
        if cal in (None, 1):
            # a one-hour calendar equals no calendar bit for bit, and its period means are the hours themselves
            assert np.array_equal(bits(mean), bits(y)), what
            if hourly is None:
                hourly = out
            assert np.array_equal(bits(out), bits(hourly)), what
        # w = NULL is w = 1
        ot1, shift1, eps1 = observed(tk, None, transform)
        _, _, out1 = run_host(gagelib, transform, ends, y, ot1, None, shift1, eps1)
        _, _, out2 = run_host(gagelib, transform, ends, y, ot1, np.ones_like(wk), shift1, eps1)
        assert np.array_equal(bits(out1), bits(out2)), what
        # hours after the last closing hour reach no chain
        if ends[-1] + 1 < T:
            other = y.copy()
            other[ends[-1] + 1:] = 1e6
            again = run_host(gagelib, transform, ends, other, ot, wk, shift, eps)
            assert np.array_equal(bits(again[2]), bits(out)) and np.array_equal(bits(again[0]), bits(mean)), what
        # the period means as an hourly record of K hours: the same chains
        _, _, out_k = run_host(gagelib, transform, np.arange(K, dtype=np.int32), np.ascontiguousarray(mean), ot, wk, shift, eps)
        assert np.array_equal(bits(out_k), bits(out)), what
    assert gamma(T + 3) < 1e-3
