"""GPU tier: `enkf_filter` and `enkf_update` (hydrodl2_amd/enkf.py) end to end.

  twin experiment    examples/assimilate_enkf.py at its defaults (the set-up of examples/assimilate_pf.py: 8 basins x
                     nmul 4 x 150 days, 64 particles, one-day windows, seed 5): summed over the basins, the squared errors
                     of `forecast_mean` and of `analysis_mean` against the TRUTH over days 30 .. 149 are both below the open
                     loop's, and no (day, basin) pair has status 2 or 3.  No ratio to the particle filter is asserted; the
                     figures are printed and recorded in profiles/r31_enkf.md.
  determinism        T = 23, B = 5, M = 3, P = 16, windows of 1 and of 4, a NaN observation, both methods: two equally
                     seeded runs agree bit for bit in every output, another seed differs; shapes and dtypes.
  window agreement   window=4 with serial assimilation and window=1 agree in `forecast_mean` on day 0 (the same series bits; nothing has
                     been assimilated yet) and DIFFER later: window=1 restarts the model from the analysed storages every day,
                     window=4 carries the update of the window's later rows through the ensemble's covariances and moves the
                     storages at the window's end.  They are different filters; the test asserts the difference.
  spread             under 'sqrt' the spread of the analysed row is smaller than the forecast's, in every analysed basin.
  inactive filter    with every weight 0 `forecast_mean` has the bits of the mean of a plain `ensemble_step` series: the
                     analysis touches nothing.
  forecast           `ensemble_forecast` takes the returned state as it is; its quantiles are ordered."""
import importlib.util
import os
import sys

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import EnsembleState, enkf_filter, enkf_update, ensemble_forecast, ensemble_step

from . import synth
from .test_population_gpu import DEV, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, B, M, P = 23, 5, 3, 16


def _example():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        spec = importlib.util.spec_from_file_location("assimilate_enkf", os.path.join(ROOT, "examples", "assimilate_enkf.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "examples"))
    return mod


@pytest.mark.gpu
def test_twin_experiment(hip_backend):
    out = _example().twin_experiment(device=DEV)
    print("twin experiment:", out)
    assert out["basins"] == 8 and out["days"] == 150 and out["nmul"] == 4 and out["particles"] == 64 and out["window"] == 1
    assert out["seed"] == 5 and out["status_2_or_3"] == 0
    assert out["sse_forecast"] < out["sse_open_loop"], "the forecast mean is no closer to the truth than the open loop"
    assert out["sse_analysis"] < out["sse_open_loop"], "the analysis mean is no closer to the truth than the open loop"
    assert out["quantiles_ordered"] and 0.0 <= out["band_coverage"] <= 1.0


@pytest.fixture(scope="module")
def problem():
    model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "dynamic_params": {"Hbv": []}, "warm_up": 0}, DEV)
    x = {"x_phy": torch.from_numpy(synth.forcing(T, B, seed=71, day0=120.0)).to(DEV)}
    p = torch.from_numpy(synth.raw_parameters(T, B, model.learnable_param_count, seed=72)).to(DEV)
    with torch.no_grad():
        obs = model(x, p)["streamflow"][..., 0].clone() * 1.3 + 0.05
    obs[4, 2] = float("nan")                            # a missing observation
    return model, x, p, obs


def _run(problem, seed, window, method, **kw):
    model, x, p, obs = problem
    g = torch.Generator().manual_seed(seed)
    kw = {"obs_sigma": 0.2, "prcp_sigma": 0.5, "temp_sigma": 1.0, "state_sigma": 0.5, "state_add_sigma": 5.0,
          "inflation": 1.02, "return_series": True, **kw}
    return enkf_filter(model, x, p, obs, P, window=window, method=method, generator=g, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["sqrt", "perturbed"])
@pytest.mark.parametrize("window", [1, 4])
def test_two_equally_seeded_runs_agree_bit_for_bit(hip_backend, problem, window, method):
    a, b, c = _run(problem, 3, window, method), _run(problem, 3, window, method), _run(problem, 4, window, method)
    for key in ("forecast_mean", "analysis_mean", "spread", "innovation"):
        assert tuple(a[key].shape) == (T, B) and a[key].dtype == torch.float64, key
        assert torch.equal(a[key].view(torch.int64), b[key].view(torch.int64)), key
    assert tuple(a["status"].shape) == (T, B) and a["status"].dtype == torch.int32 and torch.equal(a["status"], b["status"])
    assert tuple(a["series"].shape) == (P, T, B) and a["series"].dtype == torch.float32
    assert torch.equal(bits(a["series"]), bits(b["series"]))
    assert a["windows"].tolist() == [[i, min(i + window, T)] for i in range(0, T, window)]
    st = a["state"]
    assert isinstance(st, EnsembleState) and st.day == T and st.weights is None
    assert tuple(st.states.shape) == (P, 5, B, M) and tuple(st.history.shape) == (P, 14, B)
    assert torch.equal(bits(st.states), bits(b["state"].states)) and torch.equal(bits(st.history), bits(b["state"].history))
    assert not torch.equal(a["forecast_mean"], c["forecast_mean"])
    # the missing observation is status 1 with a NaN innovation, every other pair was analysed
    want = torch.zeros((T, B), dtype=torch.int32, device=DEV)
    want[4, 2] = 1
    assert torch.equal(a["status"], want)
    assert bool(torch.isnan(a["innovation"][4, 2])) and int(torch.isnan(a["innovation"]).sum()) == 1
    assert bool(torch.isfinite(a["forecast_mean"]).all()) and bool(torch.isfinite(a["analysis_mean"]).all())
    assert bool((st.states >= 1e-5).all()) and bool((st.history >= 0).all())
    assert torch.allclose(a["forecast_mean"], a["series"].double().mean(0), rtol=1e-13, atol=0.0)
    # where nothing was analysed the analysed row is the forecast row
    assert torch.allclose(a["analysis_mean"][4, 2], a["forecast_mean"][4, 2], rtol=1e-12)


@pytest.mark.gpu
def test_windows_of_four_and_of_one_agree_on_day_zero_and_are_different_filters(hip_backend, problem):
    # no forcing noise: the draws of a window of four and of four windows of one come in another order
    kw = {"prcp_sigma": 0.0, "temp_sigma": 0.0}
    one, four = _run(problem, 3, 1, "sqrt", **kw), _run(problem, 3, 4, "sqrt", **kw)
    assert torch.equal(bits(one["series"][:, 0]), bits(four["series"][:, 0]))
    # (a mean over particles of a [P,1,B] and of a [P,4,B] tensor: the same values, possibly summed in another order)
    assert torch.allclose(one["forecast_mean"][0], four["forecast_mean"][0], rtol=1e-13, atol=0.0)
    assert torch.allclose(one["analysis_mean"][0], four["analysis_mean"][0], rtol=1e-13, atol=0.0)
    assert not torch.allclose(one["forecast_mean"][1:4], four["forecast_mean"][1:4], rtol=1e-6)
    assert not torch.equal(bits(one["state"].states), bits(four["state"].states))


@pytest.mark.gpu
def test_the_square_root_analysis_shrinks_the_spread(hip_backend, problem):
    model, x, p, obs = problem
    step = ensemble_step(model, x, p, obs, n_particles=P, t_begin=0, t_end=6, return_series=True,
                         prcp_mul=torch.exp(0.5 * torch.randn((P, 6, B), generator=torch.Generator().manual_seed(9))).to(DEV))
    y = step["series"][:, 5].contiguous()
    before = y.double().std(0)
    # an observation error as large as the spread (six days of rain noise move these flows by 1e-7 .. 1e-3): the
    # anomalies then shrink by 1 - alpha / 2 = 0.71, far from a float32 rounding; 1 where a basin has no spread at all
    sigma = torch.where(before > 0, before, torch.ones_like(before))
    out = enkf_update(step["state"], y, obs[5], sigma, extra=[y.unsqueeze(1)])
    assert not out["status"].any() and out["state"].day == 6 and out["state"].weights is None
    after = out["extra"][0][:, 0].double().std(0)
    print("spread before / after:", before.tolist(), after.tolist())
    live = before > 0                                   # (a basin under snow answers no rain: no spread, no gain)
    assert bool(live.any()) and bool((after[live] < 0.8 * before[live]).all()) and bool((after[live] > 0.6 * before[live]).all())
    assert torch.allclose(out["ybar"], y.double().mean(0), rtol=1e-12) and torch.allclose(out["yvar"], y.double().var(0), rtol=1e-10)
    assert torch.allclose(out["innovation"], obs[5].double() - y.double().mean(0), rtol=1e-9, atol=1e-12)
    # the inputs are not written: a new state comes back
    assert torch.equal(bits(step["series"][:, 5]), bits(y)) and out["state"].states.data_ptr() != step["state"].states.data_ptr()
    # the filter reports the same: its analysed row is narrower than its forecast row under 'sqrt'
    kf = _run(problem, 3, 1, "sqrt", inflation=1.0)
    pert = enkf_update(step["state"], y, obs[5], sigma, method="perturbed", generator=torch.Generator().manual_seed(1),
                       extra=[y.unsqueeze(1)])
    assert not pert["status"].any() and not torch.equal(bits(pert["state"].states), bits(out["state"].states))
    assert bool(torch.isfinite(kf["spread"]).all())


@pytest.mark.gpu
def test_a_filter_without_observations_is_the_plain_ensemble(hip_backend, problem):
    model, x, p, obs = problem
    kw = {"prcp_sigma": 0.0, "temp_sigma": 0.0, "state_sigma": 0.0, "state_add_sigma": 0.0}
    for window in (1, 4):
        kf = _run(problem, 3, window, "sqrt", weights=torch.zeros((T, B), device=DEV), **kw)
        plain = ensemble_step(model, x, p, obs, n_particles=P, return_series=True)
        assert torch.equal(bits(kf["series"]), bits(plain["series"]))
        # the mean over particles, taken window by window as the filter takes it
        want = torch.cat([plain["series"][:, a:b].double().mean(0) for a, b in kf["windows"].tolist()])
        assert torch.equal(kf["forecast_mean"].view(torch.int64), want.view(torch.int64))
        assert torch.allclose(kf["forecast_mean"], plain["series"].double().mean(0), rtol=1e-13, atol=0.0)
        assert bool((kf["status"] == 1).all()) and bool(torch.isnan(kf["innovation"]).all())
        assert torch.equal(bits(kf["state"].states), bits(plain["state"].states))
        assert torch.equal(bits(kf["state"].history), bits(plain["state"].history))


@pytest.mark.gpu
def test_the_forecast_takes_the_returned_state(hip_backend, problem):
    model, x, p, obs = problem
    kf = _run(problem, 3, 1, "sqrt")
    fx = {"x_phy": torch.from_numpy(synth.forcing(9, B, seed=73, day0=143.0)).to(DEV)}
    fc = ensemble_forecast(model, fx, p[:9].contiguous(), kf["state"])
    assert tuple(fc["series"].shape) == (P, 9, B) and tuple(fc["quantiles"].shape) == (3, 9, B)
    assert bool((fc["quantiles"][0] <= fc["quantiles"][1]).all()) and bool((fc["quantiles"][1] <= fc["quantiles"][2]).all())
    assert bool(torch.isfinite(fc["series"]).all()) and fc["state"].day == 9
