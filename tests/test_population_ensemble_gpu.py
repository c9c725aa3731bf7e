"""GPU tier: `ensemble_step` / `ensemble_record` (hydrodl2_amd/ensemble.py) on hbvx_population_ensemble, the ensemble form
of k_pop (include/hbvx_pop_ens.h states the guarantees by number).

Records: 'hbv-m3-b5-t40-cutoff-subset' of tests/test_population_gpu.py (M = 3 padded to 4, B = 5 so the last wave is
partly empty, 50 descriptor days of which the first 10 are simulated and not scored, a routing column among the
candidates), its Hbv_1_1p and Hbv_2 siblings built here (Hbv_2 has no warm-up: 40 days, all scored), and that file's
'hbv11p-m16-b5-t40-muwts' (M = 16, ensemble weights, a warm-up PASS: t_first = 0 with carried-in storages).  P = 3
particles, candidate c's static values their difference, unless stated.

  same bits     (3) nothing new given: the four sums and the series are `population_stats`' bit for bit, every transform.
  resume        (4) windows 17|1|rest, one-day windows and 5|rest (t_first inside the second window) against one window,
                with precipitation noise per day and temperature noise per particle sliced per window: series, final
                storages and final history bit for bit; each window's chains against float64 sums over the window's own
                series with the measure and the bound of tests/test_population_stats_gpu.py (transform 'none': gamma(n + 2)
                sum w r^2 and its siblings, n the window's scored days).
  ancestors     a [P,B] index with repeats, different per basin, against the same call on host-gathered storages and
                history; the explicit identity against None; (2) P = 7 drawn from 3 sources against each particle alone.
  perturbations particle 0 with prcp_mul / temp_add, per day and per particle, against `population_stats` on a record whose
                x_phy was changed in torch by the same float32 multiply and add: series and sums bit for bit.  A None
                temp_add on a record with temperatures of -0.0 has `population_stats`' bits on that record (the add is
                absent from the instruction stream; -0.0 + 0.0 would be +0.0, which no output of the model can show, so
                this is the observable half of that statement).
  float64       three different wet starts as three particles of the routed WETR problems of tests/daily_sets.py against
                oracle/hbv_restate64.py in float64 per particle: series and storages under hourly_sets.admit at
                abi_util's flux tolerance, cap 2e-3, the float32 evaluations the C oracle's forward and the float32
                restatement (tests/test_ensemble_f64.py checks the float64 side and the cap on the CPU first).
  errors        every refusal of the launcher before a launch: the poisoned outputs stay poisoned."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from hydrodl2_amd import _abi, ops
from hydrodl2_amd.ensemble import EnsembleState, ensemble_record, ensemble_step
from hydrodl2_amd.population import population_stats

from . import abi_util as au
from . import hourly_sets as hs
from . import restate_util as ru
from . import test_population_gpu as suite
from .test_ensemble_f64 import PROBLEMS, particle_problems, want64
from .test_population_gpu import DEV, bits, gamma

KEYS = ("sse", "s1", "s2", "s3")
TRANSFORMS = ("none", "sqrt", "log")
BASE = "hbv-m3-b5-t40-cutoff-subset"
SIBLINGS = {
    "hbv11p-m3-b5-t40-cutoff-subset": dict(cls=("hbv_1_1p", "Hbv_1_1p"), M=3, B=5, T=50, warm_up=10, warm_up_states=False,
                                           P=3, names=["parFC", "parK1", "route_a"]),
    "hbv2-m3-b5-t40-subset": dict(cls=("hbv_2", "Hbv_2"), M=3, B=5, T=40, P=3, names=["parFC", "parK1", "route_a"]),
}
RECORDS = [BASE] + list(SIBLINGS) + ["hbv11p-m16-b5-t40-muwts"]


@functools.lru_cache(maxsize=None)
def case(name):
    """A record of the population suite, or one of SIBLINGS built by its `Case` (the entry is in that file's table only
    while the case is built: its own parametrisations do not see it)."""
    if name not in SIBLINGS:
        return suite.case(name)
    suite.CASES[name] = SIBLINGS[name]
    try:
        return suite.Case(name)
    finally:
        del suite.CASES[name]


@functools.lru_cache(maxsize=None)
def record(name):
    cs = case(name)
    cs.prepare()
    return ensemble_record(cs.model, cs.xd, cs.p)


def cands(name, P=None):
    """[P,B,C] candidates: the case's own, cycled to P."""
    cs = case(name)
    P = cs.P if P is None else P
    return cs.cand[[c % cs.P for c in range(P)]].contiguous()


def step(name, P=3, **kw):
    cs = case(name)
    kw.setdefault("candidates", cands(name, P))
    return ensemble_step(record(name), None, None, cs.target, names=cs.names, weights=cs.weights, **kw)


def noise(name, P):
    """(prcp_mul [P,T,B] around one, temp_add [P,B]) float32, fixed."""
    rec = record(name)
    T, B = rec.main.cfg.T, rec.main.cfg.B
    g = torch.Generator().manual_seed(17)
    pm = torch.exp(0.4 * torch.randn((P, T, B), generator=g) - 0.08).to(DEV)
    ta = (1.5 * torch.randn((P, B), generator=g)).to(DEV)
    return pm.contiguous(), ta.contiguous()


def same(a, b, what):
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (what, a.shape, b.shape)
    assert torch.equal(bits(a), bits(b)), f"{what}: other bits"


@pytest.mark.gpu
@pytest.mark.parametrize("name", RECORDS)
def test_nothing_new_given_is_population_stats_bit_for_bit(hip_backend, name):
    assert ops._POISON, "the GPU tier runs with NaN-poisoned output buffers"
    cs = case(name)
    for transform in TRANSFORMS:
        cs.prepare()
        want = population_stats(cs.model, cs.xd, cs.p, cs.cand, cs.target, cs.names, cs.weights, transform=transform,
                                return_series=True)
        cs.prepare()
        got = ensemble_step(cs.model, cs.xd, cs.p, cs.target, candidates=cs.cand, names=cs.names, weights=cs.weights,
                            transform=transform, return_series=True)
        for key in KEYS + ("series", "shift"):
            same(got[key], want[key], f"{name} {transform} {key}")
        assert bool(torch.isfinite(got["series"]).all()) and float(got["series"].max()) > 0.1
        assert torch.equal(got["n_obs"], want["n_obs"]) and got["columns"] == want["columns"]
        for k in ("W", "e1", "e2"):
            assert torch.allclose(got["obs"][k], want["obs"][k], rtol=1e-13, atol=1e-9)
        st = got["state"]
        M = cs.M
        assert isinstance(st, EnsembleState) and st.day == record(name).main.cfg.T
        assert tuple(st.states.shape) == (cs.P, 5, cs.B, M) and tuple(st.history.shape) == (cs.P, 14, cs.B)
        assert bool(torch.isfinite(st.states).all()) and bool(torch.isfinite(st.history).all()), "a poisoned element was left"
        # through the record: the same bits, the module is not run again
        again = step(name, cs.P, candidates=cs.cand, transform=transform, return_series=True)
        for key in KEYS + ("series",):
            same(again[key], want[key], f"{name} {transform} {key} through the record")
        same(again["state"].states, st.states, "state_out of a second call")
        same(again["state"].history, st.history, "hist_out of a second call")
        plain = step(name, cs.P, candidates=cs.cand, transform=transform)
        assert "series" not in plain and all(torch.equal(bits(plain[k]), bits(want[k])) for k in KEYS)
    # particle 0 has the module's own parameters: its final storages are the forward's, at the flux tolerance (the forward
    # may be another kernel family: bit equality with it is not promised)
    fwd = record(name).main.state_out.reshape(5, cs.B, M).double()
    assert bool(((st.states[0].double() - fwd).abs() <= au.FLUX_ATOL + au.FLUX_RTOL * fwd.abs()).all())


def splits(T, t_first):
    out = {"17|1|rest": [17, 1, T - 18], "one-day windows": [1] * T, "5|rest": [5, T - 5]}
    assert t_first == 0 or 5 < t_first < 17
    return out


def check_window_chains(got, rows, what):
    """The window's chains against float64 sums over its own series (transform 'none'): the measure and the bound of
    tests/test_population_stats_gpu.py with K = 0."""
    if rows == 0:
        for key in KEYS:
            assert not got[key].any() and not torch.signbit(got[key]).any(), f"{what}: an empty window's {key} is not +0"
        return
    y8 = got["series"].double()
    o8 = got["_target"].double()
    w8 = got["_w"].double()
    m8 = got["shift"].double()
    d, e, r = y8 - m8, o8 - m8, y8 - o8
    for key, terms, mags, n in (("sse", w8 * r * r, w8 * r * r, rows + 2), ("s1", w8 * d, w8 * d.abs(), rows + 1),
                                ("s2", w8 * d * d, w8 * d * d, rows + 3), ("s3", w8 * d * e, w8 * (d * e).abs(), rows + 3)):
        err = (got[key].double() - terms.sum(1)).abs()
        bound = gamma(n) * mags.sum(1)
        assert bool((err <= bound).all()), f"{what}: {key} misses the float64 sum of the window's own series"


@pytest.mark.gpu
@pytest.mark.parametrize("name", RECORDS)
def test_consecutive_windows_have_the_bits_of_one_window(hip_backend, name):
    cs = case(name)
    rec = record(name)
    T, t_first, P = rec.main.cfg.T, rec.t_first, 3
    pm, ta = noise(name, P)
    one = step(name, P, prcp_mul=pm, temp_add=ta, return_series=True)
    assert tuple(one["series"].shape) == (P, T - t_first, cs.B)
    from hydrodl2_amd.population import _observations
    ob = _observations(cs.req, cs.xd, cs.target, cs.weights, "none", None, "test")
    for label, pieces in splits(T, t_first).items():
        assert sum(pieces) == T
        state, at, series = None, 0, []
        for n in pieces:
            got = step(name, P, state=state, t_begin=at, t_end=at + n, prcp_mul=pm[:, at:at + n].contiguous(), temp_add=ta,
                       return_series=True)
            state = got["state"]
            assert state.day == at + n
            r0, r1 = max(at, t_first) - t_first, max(at + n, t_first) - t_first
            assert tuple(got["series"].shape) == (P, r1 - r0, cs.B), (label, at)
            got["_target"] = ob["target"][r0:r1]
            got["_w"] = torch.ones_like(got["_target"]) if ob["w"] is None else ob["w"][r0:r1]
            check_window_chains(got, r1 - r0, f"{name} {label} [{at},{at + n})")
            assert int(got["n_obs"].max()) <= r1 - r0
            series.append(got["series"])
            at += n
        same(torch.cat(series, 1), one["series"], f"{name} {label}: the series")
        same(state.states, one["state"].states, f"{name} {label}: the final storages")
        same(state.history, one["state"].history, f"{name} {label}: the final history")
    # the noise reaches the model, and differently per particle
    quiet = step(name, P, return_series=True)
    assert not torch.equal(bits(quiet["series"]), bits(one["series"]))
    # the history's meaning: entry 0 is the last day's un-routed mean; a second half started WITHOUT it differs
    half = step(name, P, t_begin=0, t_end=T // 2, prcp_mul=pm[:, :T // 2].contiguous(), temp_add=ta)["state"]
    cold = step(name, P, state=EnsembleState(half.states, None, half.day), prcp_mul=pm[:, T // 2:].contiguous(), temp_add=ta,
                return_series=True)
    assert not torch.equal(bits(cold["series"][:, :10]), bits(one["series"][:, T // 2 - t_first:][:, :10]))
    same(cold["state"].states, one["state"].states, "the storages do not depend on the routing history")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [BASE, "hbv11p-m16-b5-t40-muwts"])
def test_ancestors(hip_backend, name):
    cs = case(name)
    rec = record(name)
    T, B, P = rec.main.cfg.T, cs.B, 3
    pm, ta = noise(name, P)
    src = step(name, P, t_begin=0, t_end=20, prcp_mul=pm[:, :20].contiguous(), temp_add=ta)["state"]
    assert not torch.equal(src.states[0], src.states[1]) and not torch.equal(src.history[1], src.history[2])
    rest = dict(t_begin=20, t_end=T, prcp_mul=pm[:, 20:].contiguous(), temp_add=ta, return_series=True)

    def gathered(anc):
        idx = anc.long()
        Pn = idx.shape[0]
        return EnsembleState(src.states.gather(0, idx.view(Pn, 1, B, 1).expand(Pn, 5, B, cs.M)).contiguous(),
                             src.history.gather(0, idx.view(Pn, 1, B).expand(Pn, 14, B)).contiguous(), src.day)

    def agree(a, b, what):
        for key in KEYS + ("series",):
            same(a[key], b[key], f"{name} {what} {key}")
        same(a["state"].states, b["state"].states, f"{name} {what} storages")
        same(a["state"].history, b["state"].history, f"{name} {what} history")

    # a permutation with repeats, different per basin
    anc = torch.tensor([[(c + b) % P if b % 2 else (0 if c < 2 else 2) for b in range(B)] for c in range(P)],
                       dtype=torch.int32, device=DEV)
    assert len({tuple(anc[:, b].tolist()) for b in range(B)}) > 2
    by_index = step(name, P, state=src, ancestor=anc, **rest)
    by_gather = step(name, P, state=gathered(anc), **rest)
    agree(by_index, by_gather, "ancestor against host-gathered state")
    plain = step(name, P, state=src, **rest)
    assert not torch.equal(bits(plain["series"]), bits(by_index["series"]))
    ident = torch.arange(P, dtype=torch.int32, device=DEV).unsqueeze(1).expand(P, B).contiguous()
    agree(step(name, P, state=src, ancestor=ident, **rest), plain, "the explicit identity against None")
    # seven particles drawn from the three sources: each has the bits it has alone
    P7 = 7
    anc7 = torch.tensor([[(3 * c + 2 * b + c * b) % 3 for b in range(B)] for c in range(P7)], dtype=torch.int32, device=DEV)
    pm7, ta7 = noise(name, P7)
    rest7 = dict(t_begin=20, t_end=T, return_series=True)
    many = step(name, P7, state=src, ancestor=anc7, prcp_mul=pm7[:, 20:].contiguous(), temp_add=ta7, **rest7)
    cand7 = cands(name, P7)
    for c in (0, 3, 6):
        g = gathered(anc7[c:c + 1])
        alone = step(name, 1, candidates=cand7[c:c + 1].contiguous(), state=g, prcp_mul=pm7[c:c + 1, 20:].contiguous(),
                     temp_add=ta7[c:c + 1].contiguous(), **rest7)
        for key in KEYS + ("series",):
            same(alone[key][0], many[key][c], f"{name}: particle {c} of seven alone, {key}")
        same(alone["state"].states[0], many["state"].states[c], f"{name}: particle {c} of seven alone, storages")
        same(alone["state"].history[0], many["state"].history[c], f"{name}: particle {c} of seven alone, history")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [BASE, "hbv2-m3-b5-t40-subset"])
def test_perturbations_against_population_stats_on_a_changed_record(hip_backend, name):
    cs = case(name)
    rec = record(name)
    cfg = rec.main.cfg
    T, B = cfg.T, cs.B
    assert cfg.t0 == 0 and int(cs.xd["x_phy"].shape[0]) == T        # descriptor day t is row t of x_phy
    ch_p, ch_t, _ = cfg.channels
    pm, ta = noise(name, 3)
    c = 1
    cand = cs.cand[c:c + 1].contiguous()
    for label, pmul, tadd in (("per day", pm[c:c + 1], (ta[c:c + 1].unsqueeze(1) * torch.linspace(-1, 1, T, device=DEV).view(1, T, 1)).contiguous()),
                              ("per particle", pm[c:c + 1, 7].contiguous(), ta[c:c + 1])):
        x2 = cs.xd["x_phy"].clone()
        x2[..., ch_p] = x2[..., ch_p] * (pmul[0] if pmul.dim() == 3 else pmul[0].unsqueeze(0))
        x2[..., ch_t] = x2[..., ch_t] + (tadd[0] if tadd.dim() == 3 else tadd[0].unsqueeze(0))
        xd2 = dict(cs.xd, x_phy=x2)
        cs.prepare()
        want = population_stats(cs.model, xd2, cs.p, cand, cs.target, cs.names, cs.weights, transform="sqrt", return_series=True)
        got = step(name, 1, candidates=cand, prcp_mul=pmul.contiguous(), temp_add=tadd.contiguous(), transform="sqrt",
                   return_series=True)
        for key in KEYS + ("series",):
            same(got[key], want[key], f"{name} {label} {key}")
        base = step(name, 1, candidates=cand, transform="sqrt", return_series=True)
        assert not torch.equal(bits(base["series"]), bits(got["series"]))
    # temperatures of -0.0 and no temp_add: the record's own bits
    x3 = cs.xd["x_phy"].clone()
    x3[3::4, :, ch_t] = -0.0
    xd3 = dict(cs.xd, x_phy=x3)
    cs.prepare()
    want = population_stats(cs.model, xd3, cs.p, cand, cs.target, cs.names, cs.weights, return_series=True)
    cs.prepare()
    got = ensemble_step(cs.model, xd3, cs.p, cs.target, candidates=cand, names=cs.names, weights=cs.weights,
                        prcp_mul=torch.ones((1, B), device=DEV), return_series=True)
    for key in KEYS + ("series",):
        same(got[key], want[key], f"{name} -0.0 temperatures {key}")


@functools.lru_cache(maxsize=None)
def problem_record(model, name):
    """The ABI-level problem through the forward once, recorded."""
    prob = PROBLEMS[(model, name)]
    with ops.record_paths() as records:
        au.run_problem(prob, None, device="cuda:0", backward=False)
    return records[-1]


@pytest.mark.gpu
@pytest.mark.parametrize("model,name", list(PROBLEMS), ids=[f"{m}-{n}" for m, n in PROBLEMS])
def test_per_particle_storages_against_float64(hip_backend, oracle_path, model, name):
    prob = PROBLEMS[(model, name)]
    T, B, M = prob["T"], prob["B"], prob["M"]
    parts = particle_problems(model, name)
    P = len(parts)
    states = torch.from_numpy(np.stack([p["state_in"] for p in parts])).to(DEV).contiguous()
    assert P == 3 and not torch.equal(states[0], states[1]) and not torch.equal(states[1], states[2])
    rec = problem_record(model, name)
    zeros = torch.zeros((T, B), device=DEV)
    flow = ops.PopTerm(zeros, None, torch.zeros(B, device=DEV), None, "none")
    flow_out, (state_out, hist_out) = ops.population_ensemble(rec, {}, (None, None), flow, ops.EnsTerm(P, 0, T, states), 0, True)
    series = flow_out[4].cpu().numpy()
    assert tuple(series.shape) == (P, T, B) and tuple(state_out.shape) == (P, 5, B, M)
    for c, p in enumerate(parts):
        w = want64(model, name, c)
        oracle = au.run_problem(p, oracle_path, device="cpu", backward=False)
        f32 = functools.lru_cache(maxsize=None)(lambda p=p: ru.abi_daily(p, torch.float32, backward=False))
        for key, got, want, alts in (
                ("series", series[c], w["routed"][0], [oracle["routed"][0], lambda: f32()["routed"][0]]),
                ("state_out", state_out[c].cpu().numpy(), w["state_out"], [oracle["state_out"], lambda: f32()["state_out"]])):
            kept = hs.admit(f"ensemble-f64 {model} {name} particle {c} {key}", got, want, alts, hs._flux_tol)
            assert (np.abs(kept - want) <= hs._flux_tol(want)).all()
        assert float(np.abs(w["routed"][0]).max()) > 0.1


def _poisoned(shape, dtype=torch.float32):
    return torch.full(shape, float("nan") if dtype == torch.float32 else -7, dtype=dtype, device=DEV)


@pytest.mark.gpu
def test_refusals_come_before_any_launch(hip_backend):
    """The launcher's refusals on real device buffers: the error is reported, nothing is launched, the poisoned outputs
    stay poisoned (a launch would have written [P,B] sums and the storages)."""
    name = BASE
    cs = case(name)
    rec = record(name).main
    cfg = rec.cfg
    T, B, M, P = cfg.T, cfg.B, cfg.M, 3
    t_first = record(name).t_first
    desc = ops._fill_desc(cfg, rec.x, rec.state_in, rec.muwts, rec.ac, rec.elev, rec.ptensors)
    route = ops._route_desc(cfg, rec.ptensors, S=1)
    outs = {k: _poisoned((P, B)) for k in ("cost", "s1", "s2", "s3")}
    state_out, hist_out = _poisoned((P, 5, B, M)), _poisoned((P, 14, B))
    state_in, hist_in = torch.zeros((P, 5, B, M), device=DEV), torch.zeros((P, 14, B), device=DEV)
    target, shift = torch.zeros((T - t_first, B), device=DEV), torch.zeros(B, device=DEV)

    def args(**kw):
        pe = _abi.PopEns()
        pop = pe.s.pop
        pop.n_cand, pop.t_first, pop.route = P, t_first, C.pointer(route)
        pop.target, pop.cost = target.data_ptr(), outs["cost"].data_ptr()
        pe.s.transform, pe.s.shift = 0, shift.data_ptr()
        pe.s.s1, pe.s.s2, pe.s.s3 = (outs[k].data_ptr() for k in ("s1", "s2", "s3"))
        pe.t_begin, pe.t_end = 0, T
        pe.state_in, pe.hist_in = state_in.data_ptr(), hist_in.data_ptr()
        pe.state_out, pe.hist_out = state_out.data_ptr(), hist_out.data_ptr()
        for k, v in kw.items():
            obj, names = pe, k.split("__")
            for n in names[:-1]:
                obj = getattr(obj, n)
            setattr(obj, names[-1], v)
        return pe

    stream = torch.cuda.current_stream().cuda_stream
    who = "hbvx_population_ensemble: "
    cases = [(-2, "0 <= t_begin < t_end <= T", dict(t_begin=-1)), (-2, "0 <= t_begin < t_end <= T", dict(t_begin=5, t_end=5)),
             (-2, "0 <= t_begin < t_end <= T", dict(t_end=T + 1)), (-1, "state_out is NULL", dict(state_out=None)),
             (-1, "hist_out is NULL", dict(hist_out=None)), (-1, "target is NULL", dict(s__pop__target=None)),
             (-1, "cost is NULL", dict(s__pop__cost=None)), (-1, "shift is NULL", dict(s__shift=None)),
             (-1, "s1 / s2 / s3 is NULL", dict(s__s2=None)), (-3, "transform must be", dict(s__transform=5)),
             (-1, "eps is NULL", dict(s__transform=2)), (-2, "n_cand must be", dict(s__pop__n_cand=0)),
             (-2, "t_first outside", dict(s__pop__t_first=T)), (-2, "identity ancestor", dict(n_src=2)),
             (-2, "identity ancestor", dict(src_first=1)), (-2, "identity ancestor", dict(n_src=-1)),
             (-2, "state_out overlaps state_in", dict(state_in=state_out.data_ptr() + 4 * (P * 5 * B * M - 1))),
             (-2, "state_out overlaps state_in", dict(state_out=state_in.data_ptr() + 4 * B * M)),
             (-2, "hist_out overlaps hist_in", dict(hist_in=hist_out.data_ptr())),
             (-2, "hist_out overlaps hist_in", dict(hist_out=hist_in.data_ptr() + 4 * (P * 14 * B - 1)))]
    for code, msg, kw in cases:
        with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*{who}.*{msg}"):
            hip_backend.population_ensemble(desc, args(**kw), stream)
    bad_route = ops._route_desc(cfg, rec.ptensors, S=1)
    bad_route.L = 1                 # the window's length is not the record's: L stays min(T, 15)
    with pytest.raises(_abi.HbvxError, match=r"\(-2\).*route L must be min\(T, 15\)"):
        hip_backend.population_ensemble(desc, args(t_end=1, s__pop__route=C.pointer(bad_route)), stream)
    with pytest.raises(_abi.HbvxError, match=r"\(-1\).*pe is NULL"):
        hip_backend.population_ensemble(desc, None, stream)
    torch.cuda.synchronize()
    for t in list(outs.values()) + [state_out, hist_out]:
        assert bool(torch.isnan(t).all()), "a refused call wrote to its outputs"
    assert not state_in.any() and not hist_in.any()
    # a window before t_first needs no target; the same arguments otherwise run, and write everything
    hip_backend.population_ensemble(desc, args(t_end=t_first, s__pop__target=None), stream)
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert not t.any(), f"an empty window's {k} is not zero"
    assert bool(torch.isfinite(state_out).all()) and bool(torch.isfinite(hist_out).all())
    # ops refuses what it can see itself
    flow = ops.PopTerm(target, None, shift, None, "none")
    for bad, match in ((ops.EnsTerm(0, 0, T), "at least one particle"), (ops.EnsTerm(P, 3, 3), "the window must satisfy"),
                       (ops.EnsTerm(P, 0, T, state_in[:2]), "state_in must be"),
                       (ops.EnsTerm(P, 0, T, None, hist_in[:, :13].contiguous()), "hist_in must be"),
                       (ops.EnsTerm(P, 0, T, ancestor=torch.zeros((P, B + 1), dtype=torch.int32, device=DEV)), "ancestor must be"),
                       (ops.EnsTerm(P, 0, T, p_mul=torch.ones((P, T - 1, B), device=DEV)), "p_mul must be"),
                       (ops.EnsTerm(P, 0, T, t_add=torch.ones((P, B), device="cpu")), "t_add")):
        with pytest.raises((ValueError, RuntimeError), match=match):
            ops.population_ensemble(rec, {}, (None, None), flow, bad, t_first)
    with pytest.raises(TypeError, match="ancestor must be an int32"):
        ops.population_ensemble(rec, {}, (None, None), flow, ops.EnsTerm(P, 0, T, ancestor=torch.zeros((P, B), device=DEV)), t_first)
    # an ancestor outside the sources is clamped, not followed
    wild = torch.tensor([[-5, 0, 1, 2, 99]] * P, dtype=torch.int32, device=DEV)
    tame = wild.clamp(0, P - 1)
    st = torch.rand((P, 5, B, M), device=DEV) * 20
    a = ops.population_ensemble(rec, {}, (None, None), flow, ops.EnsTerm(P, 0, T, st, None, wild), t_first, True)
    b = ops.population_ensemble(rec, {}, (None, None), flow, ops.EnsTerm(P, 0, T, st, None, tame), t_first, True)
    same(a[0][4], b[0][4], "a clamped ancestor")
    same(a[1][0], b[1][0], "a clamped ancestor's storages")
