"""The regimes of tests/lstm_sets.py on the host: that they cover what they are for, that they are well conditioned,
and the oracle's LSTM restatement (oracle/hbv_oracle.c) on them.  The GPU tier is tests/test_lstm_f64_gpu.py.

Coverage: every regime at every shape of either tier is held to lstm_sets.FLOORS in a float64 unrolled run (whose
`out` is torch.nn.LSTM's float64 `out`, so the counts are of the model the references compute); the table is printed.

Condition: a float32 torch.nn.LSTM on the same numbers, in reverse mode and under forward_ad along one direction of
x, the state and every parameter, stays within HALF of each committed tolerance of float64 -- what the kernels are
then held to is a statement about them, not about float32.  Where a problem as first drawn did not (memory at T = 400,
the shapes with a state at T = 60, overflow on two layers), it was shortened or softened, never the tolerance:
lstm_sets.SHORTENED, GAIN and the comment above WITH_STATE.  Largest ratios to the half tolerance on this set: out
0.48 (saturated, two layers), c_n 0.57 (memory 120x33x7x256), gradients 0.08, tangents 0.06 (they vary with the
host's float32 kernels; the float32 LSTM is torch's own cell, not oneDNN's, which has no forward AD).

Each oracle case turns red when `cp` is dropped from the forget-gate term of the oracle's backward (every gradient
hundreds of times its bound, in every regime).

Oracle: its exports have no initial state and no tangent, so its zero-state reverse mode with the loss on `out` is
what runs here, through SeqLSTM(check=True) on the host, at the tolerances of the GPU tier.
"""
import pytest
import torch

from . import lstm_sets as ls

ALL = ls.cases(ls.SHAPES)


@pytest.mark.parametrize("regime,shape", ALL, ids=ls.case_id)
def test_regime_covers_what_it_is_for(regime, shape):
    prob = ls.problem(regime, shape)
    cov, out = ls.coverage(prob)
    print(ls.coverage_row(prob))
    ls.assert_covered(prob)
    # the unrolled run is the model of the reference
    want = ls.reference(prob)[0]["out"]
    assert (out - want).abs().max().item() <= 1e-12


def test_default_draw_meets_no_regime():
    """The inputs of every other LSTM test -- default initialisation, randn inputs, zero state -- counted the same
    way: no forget gate above 0.99, no |c| above 5, no pre-activation beyond |z| = 4."""
    key = ("memory", 120, 33, 7, 256, 1, False)
    plain = ls.make(*key)
    g = torch.Generator(device="cpu").manual_seed(0)
    k = plain.H ** -0.5
    sd = {n: (torch.rand(t.shape, generator=g) * 2 - 1) * k for n, t in plain.sd.items()}
    prob = ls.Problem(("default",) + key[1:], sd, torch.randn(plain.x.shape, generator=g), None, plain.w, plain.u, plain.v)
    cov = ls.coverage(prob)[0]
    print(" ".join(f"{c} {cov[c]:.3g}" for c in ls.COLUMNS))
    assert cov["f_hi"] == cov["c_big"] == cov["z_mid"] == cov["sig_exact"] == cov["g_ovf"] == 0
    assert cov["c_max"] < 1 and cov["z_max"] < 2


@pytest.mark.parametrize("regime,shape", ALL, ids=ls.case_id)
def test_float32_torch_keeps_half_of_every_tolerance(regime, shape):
    prob = ls.problem(regime, shape)
    ratios = ls.condition(prob)
    r64, r32 = ls.reference(prob)
    print(f"{prob.label:34s} float32 torch: out {ls._err(r32['out'], r64['out']).max().item():.3g}  c_n "
          f"{ls._err(r32['c_n'], r64['c_n']).max().item():.3g}  ratios to half the tolerance: "
          + " ".join(f"{k} {v:.2g}" for k, v in ratios.items()))
    over = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not over, (prob.label, over)


@pytest.mark.parametrize("regime,shape", ls.cases(ls.ORACLE), ids=ls.case_id)
def test_oracle_matches_float64(oracle_backend, regime, shape):
    prob = ls.problem(regime, shape)
    terms = (True, False, False)
    got = ls.reverse(prob, ls.module(prob, "cpu"), terms=terms)
    ls.compare_reverse(prob, got, label=f"oracle {prob.label}", terms=terms)
