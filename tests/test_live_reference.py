"""CPU tier: the CPU oracle against the reference on randomly drawn cases.

The committed fixtures pin the oracle on 39 hand-picked configurations; this test draws 40 more from a fixed seed list
(tests/golden_cases.py::live_case) -- model class, ensemble size, dynamic-parameter set, warm-up, dy_drop, routing, cold
start, parameter spread -- runs this package through the oracle, and compares every output, the final states and every
gradient at the stated tolerances (tests/helpers.py::compare) with what the reference itself computed on the same draw
(tests/golden/live_draws.npz, written by tests/golden/make_golden.py's `live` target).

One allowance the committed fixtures do not need: up to 0.5 % of a gradient tensor's elements (or four) may miss the per-GROUP
tolerance as long as they meet BASELINE.md's original proposal, 2e-6 of the TENSOR's largest entry.  Measured: draw 2 (Hbv,
4 members, static, cold start) -- the gradient of parFC for one lane is the sum of 40 daily terms of up to 1.9e-3 that
cancel to 1.3e-6, so float32 evaluations scatter around the float64 value 1.9462e-4: reference 1.9448e-4, a second torch
float32 evaluation of the same equations 1.8665e-4, the oracle 2.0047e-4; draw 138 (all 13 parameters dynamic, cold start)
-- parK2's per-day gradients of the first days, 5e-5 in a tensor whose largest entry is 22.6: reference -0.44 %, oracle
+0.34 %, second float32 evaluation +0.66 % from the float64 value.  (Seeds 0-299 under these rules: 297 agree; the other three are
single small elements of the same kind.  golden_cases.LIVE_SEEDS are the committed, deterministic set.)
"""
import os
import warnings

import numpy as np
import pytest

from . import golden_cases as gc
from .helpers import compare, run_case

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live_draws.npz")


class _Rec(dict):
    files = property(lambda self: list(self.keys()))


@pytest.fixture(scope="module")
def live_draws():
    with np.load(RECORD) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("seed", gc.LIVE_SEEDS)
def test_oracle_equals_the_live_reference_on_a_fresh_case(seed, live_draws, oracle_backend):
    name = f"_live_{seed}"
    gc.CASES[name] = gc.live_case(seed)
    try:
        ref = _Rec({k.split(":", 1)[1]: v for k, v in live_draws.items() if k.startswith(f"{seed}:")})
        assert ref, f"draw {seed} is not in {RECORD}"
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = run_case(name, "cpu")
        compare(name, res, ref, grad_outlier_frac=5e-3, grad_outlier_atol_rel=2e-6)
    finally:
        del gc.CASES[name]
