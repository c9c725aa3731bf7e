"""CPU tier: the float64 side of tests/test_population_ensemble_gpu.py::test_per_particle_storages_against_float64, checked
before the kernel is: three particles of a routed wet problem of tests/daily_sets.py (WETR: storages carried in, raw
parameters spread over their ranges) that differ in their carried-in storages -- the problem's own and two more draws of
synth.wet_states -- each through oracle/hbv_restate64.py in float64 (restate_util.abi_daily) and through the C oracle's
forward.  The protocol, the tolerances and the cap are tests/test_daily_f64.py's, unchanged: daily_sets.compare_f64, i.e.
flux / traj / state_out under hourly_sets.admit at abi_util's flux tolerance with at most 2e-3 of an array admitted, the
routed rows whole.  The branches the wet starts are there for -- soil excess, fast runoff Q0 > 0, PERC = parPERC -- are
asserted on the float64 run of every particle."""
import functools

import pytest
import torch

from . import abi_util as au
from . import daily_sets as ds
from . import restate_util as ru
from . import synth

# (model, problem of daily_sets.ABI_PROBLEMS): routed, wet; the shortest per model, Hbv_2's with ensemble weights, and
# Hbv's all-dynamic one with drop masks and M = 16
NAMES = [("Hbv", "wet16"), ("Hbv", "wet63-all-drop"), ("Hbv_1_1p", "wet17"), ("Hbv_2", "wet15-muwts")]
PROBLEMS = {(m, n): ds.make(m, ds.ABI_PROBLEMS[m][n]) for m, n in NAMES}
N_PARTICLES = 3


@functools.lru_cache(maxsize=None)
def particle_problems(model, name):
    """The problem once per particle: particle 0 its own carried-in storages, the others new draws of them."""
    prob = PROBLEMS[(model, name)]
    assert prob["routing"] and "state_in" in prob
    out = [prob]
    for c in range(1, N_PARTICLES):
        p = dict(prob)
        p["state_in"] = synth.wet_states(prob["B"], prob["M"], 1000 + 37 * c).astype(prob["state_in"].dtype)
        assert p["state_in"].shape == prob["state_in"].shape
        out.append(p)
    return tuple(out)


_EVENTS = {}


@functools.lru_cache(maxsize=None)
def want64(model, name, c):
    """Particle c in float64 (forward only): run_problem's keys."""
    ev = {}
    res = ru.abi_daily(particle_problems(model, name)[c], torch.float64, backward=False, events=ev)
    _EVENTS[(model, name, c)] = ds.coverage(ev)
    return res


@pytest.mark.parametrize("model,name", NAMES, ids=[f"{m}-{n}" for m, n in NAMES])
def test_the_oracle_forward_matches_float64_on_every_particle(oracle_path, model, name):
    parts = particle_problems(model, name)
    for c, p in enumerate(parts):
        want = want64(model, name, c)
        got = au.run_problem(p, oracle_path, device="cpu", backward=False)
        ds.compare_f64(p, got, want, [lambda p=p: ru.abi_daily(p, torch.float32, backward=False)],
                       f"ensemble-f64 oracle {model} {name} particle {c}")
        cov = _EVENTS[(model, name, c)]
        print(f"{model} {name} particle {c}: Q0 {cov['Q0']:.5f} excs {cov['excs']:.5f} perc_par {cov['perc_par']:.5f}")
        assert min(cov["Q0"], cov["excs"], cov["perc_par"]) > 0, (model, name, c, cov)
    # the particles differ: their series are three series
    a, b, d = (want64(model, name, c)["routed"][0] for c in range(N_PARTICLES))
    assert abs(a - b).max() > 1e-3 and abs(b - d).max() > 1e-3
