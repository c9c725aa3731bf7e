"""GPU tier: `particle_filter` and `ensemble_forecast` (hydrodl2_amd/ensemble.py) end to end.

  twin experiment   examples/assimilate_pf.py at its defaults (8 basins x nmul 4 x 150 days; truth from wet storages,
                    observations = truth + noise of 5 % of its mean, open loop from dry storages on 0.7 x the
                    precipitation, 64 particles, one-day windows, prcp_sigma 0.4, state_sigma 0.5, one seed): summed over
                    the basins, the squared error of the filtered mean flow against the TRUTH over days 30 .. 149 is below
                    the open loop's.  No ratio is fixed; the figures are printed and recorded in
                    profiles/r30_population_ensemble.md.
  determinism       two runs with equally seeded generators agree bit for bit in every output; another seed differs.
  bookkeeping       shapes and dtypes, ESS in [1, P], weights that sum to one, resampled basins reset to uniform weights,
                    a forecast whose quantiles are ordered and whose series starts from the filter's state."""
import importlib.util
import os

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import ensemble_forecast, particle_filter

from . import synth
from .test_population_gpu import DEV, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    spec = importlib.util.spec_from_file_location("assimilate_pf", os.path.join(ROOT, "examples", "assimilate_pf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_twin_experiment(hip_backend):
    out = _example().twin_experiment(device=DEV)
    print("twin experiment:", out)
    assert out["basins"] == 8 and out["days"] == 150 and out["nmul"] == 4 and out["particles"] == 64 and out["window"] == 1
    assert out["degenerate_windows"] == 0 and 1.0 <= out["mean_ess"] <= 64.0
    assert out["sse_filter"] < out["sse_open_loop"], "the filtered mean flow is no closer to the truth than the open loop"


@pytest.mark.gpu
def test_two_equally_seeded_runs_agree_bit_for_bit(hip_backend):
    T, B, M, P = 23, 5, 3, 16
    model = hydrodl2_amd.load_model("hbv", "Hbv")({"nmul": M, "dynamic_params": {"Hbv": []}, "warm_up": 0}, DEV)
    x = {"x_phy": torch.from_numpy(synth.forcing(T, B, seed=71, day0=120.0)).to(DEV)}
    p = torch.from_numpy(synth.raw_parameters(T, B, model.learnable_param_count, seed=72)).to(DEV)
    with torch.no_grad():
        obs = model(x, p)["streamflow"][..., 0].clone() * 1.3 + 0.05
    obs[4, 2] = float("nan")                            # a missing observation

    def run(seed, **kw):
        g = torch.Generator().manual_seed(seed)
        # ess_threshold = 1: every basin whose weights are not exactly uniform is resampled after every window, so the
        # ancestor index, its identity rows and the weight reset are all on the path, whatever the flows' size
        return particle_filter(model, x, p, obs, P, window=4, obs_sigma=0.2, prcp_sigma=0.5, temp_sigma=1.0,
                               state_sigma=0.5, ess_threshold=1.0, generator=g, return_series=True, **kw)

    a, b, c = run(3), run(3), run(4)
    n_win = (T + 3) // 4
    assert tuple(a["mean"].shape) == (T, B) and a["mean"].dtype == torch.float64
    assert tuple(a["ess"].shape) == tuple(a["resampled"].shape) == tuple(a["degenerate"].shape) == (n_win, B)
    assert tuple(a["series"].shape) == (P, T, B) and tuple(a["log_likelihood"].shape) == (B,)
    assert a["windows"].tolist() == [[i, min(i + 4, T)] for i in range(0, T, 4)]
    st = a["state"]
    assert st.day == T and tuple(st.states.shape) == (P, 5, B, M) and tuple(st.history.shape) == (P, 14, B)
    assert torch.allclose(st.weights.sum(0), torch.ones(B, dtype=torch.float64, device=DEV), rtol=1e-12)
    assert bool(((a["ess"] >= 1.0 - 1e-9) & (a["ess"] <= P + 1e-9)).all()) and bool(torch.isfinite(a["mean"]).all())
    assert bool(a["resampled"].any()), "no window resampled: the ancestor path is not exercised"
    last = a["resampled"][-1]
    assert torch.allclose(st.weights[:, last], torch.full_like(st.weights[:, last], 1.0 / P))
    for key in ("mean", "ess", "log_likelihood"):
        assert torch.equal(a[key].view(torch.int64), b[key].view(torch.int64)), key
    assert torch.equal(bits(a["series"]), bits(b["series"]))
    assert torch.equal(a["resampled"], b["resampled"]) and torch.equal(bits(st.states), bits(b["state"].states))
    assert torch.equal(bits(st.history), bits(b["state"].history)) and torch.equal(st.weights, b["state"].weights)
    assert not torch.equal(a["mean"], c["mean"])
    # the forecast from the filter's state: ordered quantiles, the particles' own series, weights respected
    fx = {"x_phy": torch.from_numpy(synth.forcing(9, B, seed=73, day0=143.0)).to(DEV)}
    fp = p[:9].contiguous()
    fc = ensemble_forecast(model, fx, fp, st)
    assert tuple(fc["series"].shape) == (P, 9, B) and tuple(fc["quantiles"].shape) == (3, 9, B)
    assert bool((fc["quantiles"][0] <= fc["quantiles"][1]).all()) and bool((fc["quantiles"][1] <= fc["quantiles"][2]).all())
    assert bool((fc["quantiles"][0] >= fc["series"].min(0).values).all()) and bool((fc["quantiles"][2] <= fc["series"].max(0).values).all())
    assert fc["state"].day == 9 and bool(torch.isfinite(fc["series"]).all())
    one = torch.zeros((P, B), dtype=torch.float64, device=DEV)
    one[5] = 1.0
    only = ensemble_forecast(model, fx, fp, st, particle_weights=one, quantiles=(0.1, 0.9))
    assert torch.equal(only["quantiles"][0], only["series"][5]) and torch.equal(only["quantiles"][1], only["series"][5])
    assert torch.equal(bits(only["series"]), bits(fc["series"]))
