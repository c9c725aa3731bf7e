"""CPU tier: the particle filter's arithmetic and front end (hydrodl2_amd/ensemble.py) and the export of
include/hbvx_pop_ens.h without a GPU -- systematic resampling on fixed weights, the log-weight update against a float64
restatement (a particle with sse = inf, a basin with nothing finite), determinism under a seeded generator, the weighted
quantiles against numpy, what the front end refuses before the model runs (host tensors), the new header's prototype
and struct against `_abi.POP_ENS_SIGNATURES` / `_abi.PopEns`, and the entry point's argument checks on the
cross-compiled library (no launch)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi, ensemble
from hydrodl2_amd.ensemble import (EnsembleState, effective_sample_size, ensemble_forecast, ensemble_record, ensemble_step,
                                   particle_filter, systematic_resample, update_log_weights, weighted_quantiles)

from .test_hbv_adj import host_math_backend  # noqa: F401  (fixture)
from .test_population_host import _desc, _model, _route
from .test_step_math_host import steptest_lib  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_the_calls_are_exported():
    for name in ("EnsembleState", "ensemble_record", "ensemble_step", "particle_filter", "ensemble_forecast"):
        assert getattr(hydrodl2_amd, name) is getattr(ensemble, name) and name in hydrodl2_amd.__all__
    assert [row[0] for row in _abi.POP_ENS_SIGNATURES] == ["hbvx_population_ensemble"]
    assert "hbvx_population_ensemble" not in _abi.EXPORTS + _abi.OPTIONAL_EXPORTS + list(_abi.POPULATION)
    assert _abi.ABI_VERSION == 10 and _abi.POP_ENS_HIST == _abi.UH_MAXLEN - 1 == 14
    assert EnsembleState._fields == ("states", "history", "day", "weights")


# ---- resampling --------------------------------------------------------------------------------------------------------

def test_systematic_resampling_on_fixed_weights():
    P, B = 16, 6
    rng = np.random.default_rng(3)
    w = rng.gamma(0.5, 1.0, size=(P, B))
    w[:, 1] = 1.0                                       # uniform: every particle exactly once
    w[:, 2] = 0.0
    w[5, 2] = 1.0                                       # one particle holds everything
    w[:, 3] = 0.0
    w[2, 3], w[11, 3] = 0.75, 0.25                      # 12 and 4 offspring
    w = w / w.sum(0)
    log_w = torch.from_numpy(np.log(np.maximum(w, 1e-320)))
    log_w[torch.from_numpy(w == 0)] = -INF
    for u0 in (0.0, 0.37, 0.999999):
        u = torch.full((B,), u0, dtype=torch.float64)
        resample = torch.tensor([True, True, True, True, False, True])
        anc = systematic_resample(log_w, u, resample)
        assert anc.dtype == torch.int32 and tuple(anc.shape) == (P, B) and anc.is_contiguous()
        a = anc.numpy()
        assert (a >= 0).all() and (a < P).all()
        assert a[:, 4].tolist() == list(range(P)), "a basin that is not resampled keeps the identity"
        for b in (0, 1, 2, 3, 5):
            assert (np.diff(a[:, b]) >= 0).all(), "the ancestors ascend"
            counts = np.bincount(a[:, b], minlength=P)
            assert counts.sum() == P
            pw = P * w[:, b]
            assert ((counts >= np.floor(pw - 1e-9)) & (counts <= np.ceil(pw + 1e-9))).all(), (b, counts, pw)
        assert a[:, 1].tolist() == list(range(P)) and a[:, 2].tolist() == [5] * P
        assert np.bincount(a[:, 3], minlength=P)[[2, 11]].tolist() == [12, 4]
    # the definition, basin by basin: point (u + i) / P falls into the first particle whose running sum exceeds it
    u = torch.from_numpy(rng.random(B))
    a = systematic_resample(log_w, u, torch.ones(B, dtype=torch.bool)).numpy()
    for b in range(B):
        cum = np.cumsum(w[:, b]) / w[:, b].sum()
        want = [min(int(np.searchsorted(cum, (u[b].item() + i) / P, side="right")), P - 1) for i in range(P)]
        assert a[:, b].tolist() == want, b
    # the effective sample size that decides: 1 / sum w^2
    ess = effective_sample_size(log_w)
    assert np.allclose(ess.numpy(), 1.0 / (w ** 2).sum(0), rtol=1e-12)
    assert abs(float(ess[1]) - P) < 1e-9 and abs(float(ess[2]) - 1.0) < 1e-12


def test_the_log_weight_update_against_its_float64_restatement():
    P, B = 5, 4
    rng = np.random.default_rng(8)
    w0 = rng.random((P, B))
    w0 /= w0.sum(0)
    sse = rng.gamma(2.0, 3.0, size=(P, B)).astype(np.float32)
    sse[3, 0] = np.inf                                  # a particle whose flow had no transform: weight zero
    sse[1, 1] = np.nan
    sse[:, 2] = [np.inf, np.nan, np.inf, np.inf, np.nan]   # nothing finite: the basin keeps uniform weights
    sigma = np.array([0.5, 1.0, 2.0, 4.0])
    new, lse, degenerate = update_log_weights(torch.from_numpy(np.log(w0)), torch.from_numpy(sse), torch.from_numpy(sigma))
    assert new.dtype == torch.float64 and lse.dtype == torch.float64 and degenerate.tolist() == [False, False, True, False]
    for b in range(B):
        lik = np.array([math.exp(-0.5 * float(sse[c, b]) / sigma[b] ** 2) if np.isfinite(sse[c, b]) else 0.0 for c in range(P)])
        post = w0[:, b] * lik
        if b == 2:
            assert np.allclose(np.exp(new[:, b].numpy()), 1.0 / P, rtol=1e-15) and float(lse[b]) == 0.0
            continue
        assert np.allclose(np.exp(new[:, b].numpy()), post / post.sum(), rtol=1e-12, atol=0)
        assert abs(float(lse[b]) - math.log(post.sum())) <= 1e-12 * abs(math.log(post.sum())) + 1e-15
        assert abs(float(torch.logsumexp(new[:, b], 0))) < 1e-12
    assert float(new[3, 0]) == -INF and float(new[1, 1]) == -INF
    # a very small likelihood does not underflow the normalisation: 1e4 squared-error units at sigma 1
    big = torch.full((P, 1), 2.0e4, dtype=torch.float32)
    big[2, 0] = 2.0e4 - 2.0
    new, lse, degenerate = update_log_weights(torch.full((P, 1), -math.log(P), dtype=torch.float64), big, torch.ones(1, dtype=torch.float64))
    assert not bool(degenerate[0]) and abs(float(lse[0]) - (-1.0e4 + 1.0 + math.log((math.e ** -1 * 4 + 1) / P))) < 1e-9
    assert float(new[2, 0]) > float(new[0, 0])


def test_weighted_quantiles_against_numpy():
    rng = np.random.default_rng(5)
    P, T, B = 7, 3, 2
    v = rng.normal(size=(P, T, B)).astype(np.float32)
    k = rng.integers(0, 5, size=(P, B))                 # integer weights: the weighted sample is the sample with repeats
    k[0] += 1
    levels = (0.05, 0.33, 0.5, 0.81, 0.95, 1.0)
    got = weighted_quantiles(torch.from_numpy(v), torch.from_numpy(k.astype(np.float64)).unsqueeze(1), levels)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(levels), T, B)
    for t in range(T):
        for b in range(B):
            sample = np.repeat(v[:, t, b], k[:, b])
            for i, q in enumerate(levels):
                assert float(got[i, t, b]) == float(np.quantile(sample, q, method="inverted_cdf")), (t, b, q)
    plain = weighted_quantiles(torch.from_numpy(v), None, (0.5,))
    assert np.array_equal(plain[0].numpy(), np.quantile(v, 0.5, axis=0, method="inverted_cdf"))
    # a particle of weight zero is never a quantile
    w = torch.ones(P, 1, 1, dtype=torch.float64)
    w[int(v[:, 0, 0].argmin())] = 0.0
    assert float(weighted_quantiles(torch.from_numpy(v), w, (0.0,))[0, 0, 0]) > float(v[:, 0, 0].min())


def test_resampling_and_noise_are_deterministic_under_a_seed():
    P, B = 32, 3

    def draw(seed):
        g = torch.Generator().manual_seed(seed)
        z = ensemble._randn((P, 4, B), g, torch.device("cpu"))
        u = torch.rand((B,), generator=g, dtype=torch.float64)
        log_w = torch.log_softmax(z[:, 0].double() * 3, 0)
        return z, systematic_resample(log_w, u, effective_sample_size(log_w) < 0.5 * P)

    a, b, c = draw(11), draw(11), draw(12)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    assert a[0].dtype == torch.float32


# ---- the front end -------------------------------------------------------------------------------------------------------

def _problem(T=8, B=3):
    hbv = _model(dyn=["parBETA"])
    ny = hbv.learnable_param_count
    g = torch.Generator().manual_seed(3)
    return hbv, {"x_phy": torch.zeros(T, B, 3)}, torch.zeros(T, B, ny), torch.rand(T, B, generator=g) + 0.5


def test_refusals_happen_before_anything_runs():
    """Host tensors: a call that got as far as the module's forward would fail with the package's own 'no CPU path' error
    instead of the refusal under test."""
    T, B, P = 8, 3, 4
    hbv, x, p, tgt = _problem(T, B)
    ny = hbv.learnable_param_count
    state = torch.get_rng_state()
    st = EnsembleState(torch.zeros(P, 5, B, 2), torch.zeros(P, 14, B), 0)

    calls = {
        "ensemble_step": lambda model=hbv, pp=p, target=tgt, **kw: ensemble_step(model, x, pp, target, **{"n_particles": P, **kw}),
        "particle_filter": lambda model=hbv, pp=p, target=tgt, **kw: particle_filter(
            model, x, pp, target, kw.pop("n_particles", P), **{"obs_sigma": 1.0, **kw}),
        "ensemble_forecast": lambda model=hbv, pp=p, target=None, **kw: ensemble_forecast(model, x, pp, kw.pop("state", st), **kw),
        "ensemble_record": lambda model=hbv, pp=p, target=None, **kw: ensemble_record(model, x, pp),
    }
    hourly = hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")({"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}},
                                                                    torch.device("cpu"))
    hf = {"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}, "train_spatial_chunk_size": 4,
          "simulate_spatial_chunk_size": 4, "simulate_temporal_chunk_size": 4, "train_warmup": 1}
    mts = hydrodl2_amd.load_model("hbv_2_mts", "Hbv_2_mts")({"nmul": 2, "dynamic_params": {"Hbv_2": []}}, hf,
                                                            torch.device("cpu"))
    for what, call in calls.items():
        with pytest.raises(NotImplementedError, match="Hbv_2_hourly"):
            call(model=hourly)
        with pytest.raises(NotImplementedError, match="Hbv_2_mts"):
            call(model=mts)
        with pytest.raises(NotImplementedError, match="HbvAdj.*Newton"):
            call(model=_model(("hbv_adj", "HbvAdj")), pp=torch.zeros(T, B, 12 * 2 + 2))
        with pytest.raises(NotImplementedError):
            call(model=torch.nn.Identity())
        with pytest.raises(ValueError, match="graph=True"):
            call(model=_model(graph=True))
        with pytest.raises(ValueError, match="comprout"):
            call(model=_model(nmul=1, comprout=True), pp=torch.zeros(T, B, 14),
                 **({"state": EnsembleState(torch.zeros(P, 5, B, 1), None, 0)} if what == "ensemble_forecast" else {}))
    init = _model()
    init.initialize = True
    with pytest.raises(ValueError, match="initialize mode"):
        ensemble_step(init, x, torch.zeros(T, B, init.learnable_param_count), tgt, n_particles=P)
    step, pf, fc = calls["ensemble_step"], calls["particle_filter"], calls["ensemble_forecast"]
    for call in (step, pf):
        with pytest.raises(ValueError, match="target must be"):
            call(target=tgt[:-1])
        with pytest.raises(ValueError, match="infinities"):
            call(target=torch.full((T, B), INF))
        w = torch.ones(T, B)
        w[2, 1] = -1e-3
        with pytest.raises(ValueError, match="must not be negative"):
            call(weights=w)
        with pytest.raises(ValueError, match="transform must be one of"):
            call(transform="cube")
        with pytest.raises(ValueError, match="eps must be finite and > 0"):
            call(transform="log", eps=0.0)
        for bad in (0, -3, 2.5, True, None) if call is pf else (0, -3, 2.5, True):
            with pytest.raises(ValueError, match="n_particles must be an integer >= 1"):
                call(n_particles=bad)
    # ensemble_step's own
    cand = torch.zeros(P, B, ny - 2)
    with pytest.raises(ValueError, match="dynamic parameter"):
        step(candidates=cand, names=["parBETA"])
    with pytest.raises(ValueError, match="candidates must be"):
        step(candidates=cand[:, :2])
    with pytest.raises(ValueError, match="float32"):
        step(candidates=cand.double())
    with pytest.raises(ValueError, match="particle count must be given once and consistently"):
        step(candidates=cand[:3])
    with pytest.raises(ValueError, match="particle count must be given once and consistently"):
        ensemble_step(hbv, x, p, tgt)
    with pytest.raises(ValueError, match="prcp_mul must be a float32 tensor"):
        step(prcp_mul=torch.ones(P, B, dtype=torch.float64))
    with pytest.raises(ValueError, match="temp_add lives on meta"):
        step(temp_add=torch.ones(P, B, device="meta"))
    with pytest.raises(ValueError, match="ancestor must be a int32 tensor"):
        step(ancestor=torch.zeros(P, B, dtype=torch.int64))
    with pytest.raises(ValueError, match="state must be an EnsembleState"):
        step(state=(st.states, st.history, 0))
    with pytest.raises(ValueError, match=r"state.states must be \[P,5,B,M\]"):
        step(state=EnsembleState(torch.zeros(P, 4, B, 2), None, 0))
    with pytest.raises(ValueError, match="state.history must be"):
        step(state=EnsembleState(st.states, torch.zeros(P, 13, B), 0))
    with pytest.raises(ValueError, match="state.states must be a float32 tensor"):
        step(state=EnsembleState(st.states.double(), None, 0))
    with pytest.raises(ValueError, match="x_dict and parameters must be None"):
        ensemble_step(ensemble.EnsembleRecord(hbv, x, p, None, {}, None, 0), x, None, tgt)
    # the filter's own
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="window must be an integer >= 1"):
            pf(window=bad)
    for bad in (0.0, -1.0, NAN, INF, torch.tensor([1.0, 0.0, 1.0])):
        with pytest.raises(ValueError, match="obs_sigma must be finite and > 0"):
            pf(obs_sigma=bad)
    with pytest.raises(ValueError, match=r"obs_sigma must be a scalar or \[3\]"):
        pf(obs_sigma=torch.ones(4))
    for name in ("prcp_sigma", "temp_sigma", "state_sigma"):
        for bad in (-0.1, NAN, INF):
            with pytest.raises(ValueError, match=f"{name} must be finite and >= 0"):
                pf(**{name: bad})
    for bad in (-0.1, 1.1, NAN):
        with pytest.raises(ValueError, match=r"ess_threshold must lie in \[0, 1\]"):
            pf(ess_threshold=bad)
    # the forecast's own
    for bad in ((), (0.5, 1.5), (-0.1,), (NAN,)):
        with pytest.raises(ValueError, match=r"quantiles must lie in \[0, 1\]"):
            fc(quantiles=bad)
    with pytest.raises(ValueError, match="state must be an EnsembleState"):
        fc(state=None)
    with pytest.raises(ValueError, match=r"particle_weights must be \[4,3\]"):
        fc(particle_weights=torch.ones(3, B))
    assert torch.equal(torch.get_rng_state(), state)            # nothing ran: no draw was made


def test_a_library_without_the_export_is_named_before_the_primal(host_math_backend):  # noqa: F811
    """The host build of the math header has none of the population exports: every call names the one it needs before
    the module ran (dy_drop = 0.5: a run would have drawn masks)."""
    model = _model(dyn=["parBETA"], dy_drop=0.5)
    T, B = 6, 3
    ny = model.learnable_param_count
    xs, p, tgt = {"x_phy": torch.rand(T, B, 3)}, torch.randn(T, B, ny), torch.rand(T, B)
    state = torch.get_rng_state()
    st = EnsembleState(torch.zeros(2, 5, B, 2), None, 0)
    for call in (lambda: ensemble_step(model, xs, p, tgt, n_particles=2), lambda: ensemble_record(model, xs, p),
                 lambda: particle_filter(model, xs, p, tgt, 4, obs_sigma=1.0), lambda: ensemble_forecast(model, xs, p, st)):
        with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_ensemble"):
            call()
    assert torch.equal(torch.get_rng_state(), state)


# ---- the ABI -------------------------------------------------------------------------------------------------------------

def test_the_row_and_the_struct_are_the_headers():
    with open(os.path.join(ROOT, "include", "hbvx_pop_ens.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    found = re.findall(r"^(int|uint64_t)\s*(hbvx_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M)
    assert len(found) == 1, found
    ret, name, params = found[0][0], found[0][1], [a.strip() for a in " ".join(found[0][2].split()).split(",")]
    assert (ret, name) == ("int", "hbvx_population_ensemble")
    assert params == ["const hbvx_desc *d", "const hbvx_pop_ens *pe", "void *stream"]
    _, required, restype, argtypes, layout = _abi.POP_ENS_SIGNATURES[0]
    assert required is False and restype is C.c_int and layout == (14, _abi.PopEns)
    assert argtypes == [C.POINTER(_abi.Desc), C.POINTER(_abi.PopEns), C.c_void_p]
    assert re.search(r"#define HBVX_POP_ENS_HIST\s+14\b", text)
    body = re.search(r"typedef struct hbvx_pop_ens \{(.*?)\} hbvx_pop_ens;", text, flags=re.S).group(1)
    fields = []
    for part in body.split(";"):
        if part.strip():
            decl = part.strip()
            first, *more = decl.split(",")
            fields.append(re.sub(r"^\**", "", first.split()[-1]))
            fields += [re.sub(r"^\**", "", m.strip()) for m in more]
    assert fields == [f[0] for f in _abi.PopEns._fields_]
    # no index of hbvx_sizeof stands for two structs
    taken = {row[4][0]: row[4][1] for row in _abi.SIGNATURES if row[4] is not None}
    assert 14 not in taken
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    assert name not in lib.missing and hasattr(lib.dll, name)
    assert lib.dll.hbvx_sizeof(14) == C.sizeof(_abi.PopEns) == C.sizeof(_abi.PopStats) + 16 + 7 * 8 + 4 * 8
    assert lib.dll.hbvx_sizeof(15) == 0 and lib.dll.hbvx_sizeof(13) == C.sizeof(_abi.PopPeriod) and lib.dll.hbvx_version() == 10
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        assert "hbvx_pop_ens.h" in f.read()                      # a change to the header rebuilds the library


def _ens_args(**kw):
    pe = _abi.PopEns(t_begin=0, t_end=20, state_out=4096, hist_out=8192)
    pe.s.pop.n_cand, pe.s.pop.t_first, pe.s.pop.target, pe.s.pop.cost = 4, 0, 64, 64
    pe.s.transform, pe.s.shift, pe.s.s1, pe.s.s2, pe.s.s3 = 0, 64, 64, 64, 64
    for k, v in kw.items():
        obj, names = pe, k.split("__")
        for name in names[:-1]:
            obj = getattr(obj, name)
        setattr(obj, names[-1], v)
    return pe


def test_the_abi_refuses_bad_arguments_before_any_launch():
    """Host-side checks (no launch): runs without a GPU on the cross-compiled library.  _desc(): T = 20, B = 3, M = 2, so
    the storages of 4 particles are 4 * 30 floats and their histories 4 * 42."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    who = "hbvx_population_ensemble: "

    def refused(code, msg, d, pe):
        with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*{msg}"):
            lib.population_ensemble(d, pe, 0)

    refused(-1, "desc is NULL", None, _ens_args())
    refused(-4, "abi_version", _desc(abi_version=9), _ens_args())
    refused(-1, who + "pe is NULL", _desc(), None)
    for kw in (dict(t_begin=-1), dict(t_begin=20), dict(t_begin=7, t_end=7), dict(t_begin=8, t_end=7), dict(t_end=21),
               dict(t_end=0)):
        refused(-2, who + "the window must satisfy 0 <= t_begin < t_end <= T", _desc(), _ens_args(**kw))
    refused(-1, who + "state_out is NULL", _desc(), _ens_args(state_out=None))
    route = _route()
    refused(-1, who + "hist_out is NULL in a call that routes", _desc(), _ens_args(hist_out=None, s__pop__route=C.pointer(route)))
    for L in (1, 14, 16):       # min(d.T, 15) of the RECORD, whatever the window
        short = _route(L=L)
        refused(-2, who + r"route L must be min\(T, 15\)", _desc(), _ens_args(t_end=1, s__pop__route=C.pointer(short)))
    for model, n_param in ((_abi.MODEL_HBVADJ, 12), (_abi.MODEL_HOURLY, 19)):
        d = _desc(model=model, n_param=n_param, ac=64, elev=64)
        for i in range(12, n_param):
            d.p[i].sta, d.p[i].lo, d.p[i].hi = 64, 0.3, 5.0
        refused(-3, who + "HBV 1.0 / 1.1p / 2.0 only", d, _ens_args())
    # the sources an identity ancestor names
    for kw in (dict(n_src=3), dict(src_first=1), dict(n_src=-2), dict(src_first=-1), dict(n_src=8, src_first=5)):
        refused(-2, who + "n_src / src_first leave an identity ancestor outside", _desc(), _ens_args(**kw))
    # overlap of the outputs with the inputs, first and last element
    n_state, n_hist = 4 * 5 * 3 * 2, 4 * 14 * 3
    for s_in in (4096, 4096 + 4 * (n_state - 1), 4096 - 4 * (n_state - 1)):
        refused(-2, who + "state_out overlaps state_in", _desc(), _ens_args(state_in=s_in))
    for h_in in (8192, 8192 + 4 * (n_hist - 1), 8192 - 4 * (n_hist - 1)):
        refused(-2, who + "hist_out overlaps hist_in", _desc(), _ens_args(hist_in=h_in, s__pop__route=C.pointer(route)))
    # hbvx_population_stats' own, under the new name; the target only where the window scores a day
    refused(-1, who + "target is NULL", _desc(), _ens_args(s__pop__target=None))
    refused(-1, who + "target is NULL", _desc(), _ens_args(s__pop__target=None, s__pop__t_first=5, t_end=6))
    refused(-1, who + "cost is NULL", _desc(), _ens_args(s__pop__cost=None))
    for n in (0, 65536):
        refused(-2, who + "n_cand must be in 1..65535", _desc(), _ens_args(s__pop__n_cand=n))
    refused(-2, who + "t_first outside", _desc(), _ens_args(s__pop__t_first=20))
    for bad in (-1, 3):
        refused(-3, who + "transform must be", _desc(), _ens_args(s__transform=bad))
    refused(-1, who + "shift is NULL", _desc(), _ens_args(s__shift=None))
    refused(-1, who + "eps is NULL under HBVX_POP_T_LOG", _desc(), _ens_args(s__transform=_abi.POP_T_LOG))
    for name in ("s1", "s2", "s3"):
        refused(-1, who + "s1 / s2 / s3 is NULL", _desc(), _ens_args(**{"s__" + name: None}))
    lib.missing.append("hbvx_population_ensemble")        # a library built before the export existed
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_ensemble"):
        lib.population_ensemble(_desc(), _ens_args(), 0)
