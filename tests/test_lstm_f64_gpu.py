"""The LSTM kernels (csrc/lstm_seq.h: k_lstm_fwd, k_lstm_bwd, k_lstm_tan, k_lstm_dirs) against torch.nn.LSTM in float64
on the regimes of tests/lstm_sets.py -- forget gates at 0.99 and above, cell states in the tens, gates driven to
exactly 0 and 1, pre-activations beyond the overflow of the activations' exp2 -- where every other LSTM test draws
gates near 0.5 and |c| < 0.6.  What each regime covers is in lstm_sets.py's docstring and asserted on the host by
tests/test_lstm_f64.py, which also holds float32 torch to half of each tolerance on every problem used here.

(a) the gate functions themselves, through hbvx_lstm_forward / _forward_hx at T = 1, where the kernel adds nothing to
    the gx handed in; (b) reverse mode from a zero state, the kernel forms the host does not pick by itself included;
(c) with a state, c0 in +-50; (d) two layers; (e) forward mode, one direction (k_lstm_tan) and three in pieces of two
(k_lstm_dirs), and the batch recurrence against the one-direction one bit for bit on a regime's primal.

Tolerances: lstm_sets.py's docstring; none is added.  Every problem passes.  Measured on the MI355X (largest error
against float64; in brackets a float32 torch.nn.LSTM on the host on the same numbers), the module in 3.6 s:

  problem                      out                  c_n                  c_n ratio  worst gradient       worst tangent
  memory 320x17x5x64           5.9e-6 (2.1e-6)      9.8e-5 (4.0e-5)      2.42       3.7e-3 (1.0e-3)
  saturated 400x17x5x64        6.6e-7 (5.1e-7)      1.5e-4 (7.5e-5)      2.02       2.6e-4 (1.6e-4)
  overflow 400x17x5x64         4.1e-6 (3.8e-6)      2.2e-4 (1.7e-4)      1.30       3.6e-4 (2.6e-4)
  memory 120x33x7x128          4.8e-6 (4.5e-6)      5.2e-5 (3.4e-5)      1.54       5.8e-3 (4.1e-3)
  saturated 120x33x7x128       7.3e-7 (1.1e-6)      5.2e-5 (3.8e-5)      1.35       3.6e-4 (1.2e-4)
  overflow 120x33x7x128        2.7e-6 (2.4e-6)      1.0e-4 (7.8e-5)      1.29       6.4e-5 (7.8e-5)
  memory 120x33x7x256          5.1e-6 (3.3e-6)      6.1e-5 (3.8e-5)      1.62       7.4e-3 (3.9e-3)
  saturated 120x33x7x256       9.4e-7 (9.1e-7)      9.0e-5 (6.9e-5)      1.30       6.1e-4 (2.3e-4)
  overflow 120x33x7x256        2.3e-6 (2.0e-6)      1.1e-4 (1.0e-4)      1.07       2.7e-4 (2.6e-4)
  memory 120x33x7x64           4.7e-6 (3.2e-6)      5.6e-5 (2.6e-5)      2.13       1.7e-4 (1.3e-4)
  saturated 120x33x7x64        7.2e-7 (6.2e-7)      1.2e-5 (1.7e-5)      0.73       9.1e-5 (1.6e-5)
  overflow 120x33x7x64         2.9e-6 (2.8e-6)      6.9e-5 (6.2e-5)      1.12       2.0e-4 (1.5e-4)
  memory 24x19x7x64 hx         1.1e-6 (1.1e-6)      3.1e-5 (3.0e-5)      1.05       1.2e-4 (7.1e-5)      4.5e-5 (4.8e-5)
  saturated 24x19x7x64 hx      2.5e-6 (1.6e-6)      2.0e-5 (2.3e-5)      0.87       3.2e-6 (2.1e-6)      5.3e-5 (4.2e-5)
  overflow 24x19x7x64 hx       4.0e-6 (4.6e-6)      4.3e-5 (5.2e-5)      0.83       3.3e-6 (4.3e-6)      2.7e-4 (3.3e-4)
  memory 16x37x5x256 hx        1.2e-6 (8.9e-7)      3.8e-5 (2.6e-5)      1.47       1.4e-4 (1.1e-4)
  saturated 16x37x5x256 hx     2.9e-6 (2.2e-6)      2.5e-5 (2.7e-5)      0.93       8.8e-6 (3.6e-6)
  overflow 16x37x5x256 hx      2.6e-6 (2.9e-6)      2.0e-5 (2.0e-5)      1.00       8.5e-7 (7.2e-7)
  memory 16x21x9x64 L2 hx      1.4e-6 (1.0e-6)      3.1e-5 (2.8e-5)      1.14       1.9e-6 (1.9e-6)
  saturated 16x21x9x64 L2 hx   3.9e-6 (4.7e-6)      2.0e-5 (2.0e-5)      1.00       3.6e-4 (1.4e-4)
  overflow 16x21x9x64 L2 hx    3.2e-6 (2.6e-6)      2.6e-5 (2.6e-5)      1.01       1.7e-5 (2.1e-5)
  memory 16x21x5x256 hx        (forward mode only)                                                       3.4e-4 (2.1e-4)
  saturated 16x21x5x256 hx                                                                               4.9e-5 (5.1e-5)
  overflow 16x21x5x256 hx                                                                                1.4e-4 (1.1e-4)

(120x33x7x64 and 120x33x7x256 under HBVX_LSTM_UNITS=16 / HBVX_LSTM_WGS_PER_CU=3: the figures of the rows above to the
digits shown.)  No gradient or tangent uses more than 2.4 % of its bound, `out` at most 30 %: the kernels are as close
to float64 as float32 torch is.  c_n ratio: the kernel's largest c_n error over float32 torch's; the largest is 2.42
(memory 320x17x5x64), for the tangent of c_n 1.90, so lstm_sets.K_CN = 8 (twice 2.42, rounded up to a power of two).

Gate functions, (a): largest error 1.90e-7 (lstm_tanh; lstm_sigmoid 9.6e-8) against the 2e-7 that lstm_seq.h
documents -- the comment and the code agree, neither was changed; +-inf are exact.  The `1 - 2r` form of lstm_tanh
loses RELATIVE accuracy near zero by construction: 7.0e-4 of tanh(z) on 1e-4 <= |z| <= 1e-2 (printed, not bounded;
in absolute terms that is the same 1e-7).
"""
import time

import pytest
import torch

from hydrodl2_amd import _abi, lstm, ops

from . import lstm_sets as ls
from .test_lstm_jvp import _jvp

pytestmark = pytest.mark.gpu

_T0 = [None]


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    _T0[0] = time.time()
    yield
    print(f"\ntest_lstm_f64_gpu: {time.time() - _T0[0]:.1f} s for the module")
    worst = {}
    for label, name, e, bound, e32 in ls.FIGURES:
        kind = "grad" if name.startswith("d") and "=" not in name else ("tangent" if "=" in name else name)
        prob = label.split(" [")[0]
        w = worst.setdefault((prob, kind), (0.0, 0.0, 0.0))
        if e / bound >= w[0]:
            worst[(prob, kind)] = (e / bound, e, e32)
    for (prob, kind), (r, e, e32) in worst.items():
        print(f"worst  {prob:34s} {kind:8s} err {e:.3g} ({r:.3g} of its bound)  float32 torch {e32:.3g}")


def _reverse(prob, label=None):
    got = ls.reverse(prob, ls.module(prob, "cuda"), device="cuda")
    return ls.compare_reverse(prob, got, label=label)


# ------------------------------------------------------------------------------------------------ (a) the gate functions

GATE_TOL = 2e-7     # lstm_seq.h: "absolute error <= 2e-7 on values in [-1, 1]"


def _gate_inputs(B, H, seed):
    """[1, B, H, 4] float32 pre-activations in random order: +-0, +-1e-45 (a denormal), +-1e-8, +-1e-3, fine sweeps of
    +-[44, 45] and +-[88, 90] (lstm_tanh's and lstm_sigmoid's exp2 reach inf at 44.4 and 88.7), a logarithmic sweep of
    +-[1e-4, 1e-2], a dense sweep of [-120, 120] for the rest; then +-inf in every gate of two cells."""
    n = B * H * 4
    g = torch.Generator(device="cpu").manual_seed(seed)
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-8, -1e-8, 1e-3, -1e-3], dtype=torch.float32)
    fine = torch.cat([torch.linspace(44, 45, 1001), torch.linspace(88, 90, 1001)])
    small = torch.logspace(-4, -2, 512)
    parts = [special, fine, -fine, small, -small]
    parts.append(torch.linspace(-120, 120, n - sum(p.numel() for p in parts)))
    gx = torch.cat(parts).float()[torch.randperm(n, generator=g)].view(1, B, H, 4)
    inf = float("inf")
    gx[0, 0, 0] = torch.tensor([inf, -inf, inf, -inf])
    gx[0, B - 1, H - 1] = torch.tensor([-inf, inf, -inf, inf])
    return gx


def _check_gates(label, gx, c0, gates, c, h):
    """gx [1,B,H,4], c0 [B,H] or None, and what the kernel made of them (host tensors); the largest gate error."""
    z = gx.double()
    sig, tanh = torch.sigmoid(z), torch.tanh(z[..., 2])
    want = torch.stack([sig[..., 0], sig[..., 1], tanh, sig[..., 3]], -1)
    cp = torch.zeros(gx.shape[1:3], dtype=torch.float64) if c0 is None else c0.double()
    want_c = want[0, ..., 1] * cp + want[0, ..., 0] * want[0, ..., 2]
    want_h = want[0, ..., 3] * torch.tanh(want_c)
    for t in (gates, c, h):
        assert torch.isfinite(t).all(), label
    s3, tg = gates[..., [0, 1, 3]], gates[..., 2]
    assert s3.min() >= 0 and s3.max() <= 1 and tg.min() >= -1 and tg.max() <= 1, label
    err = (gates.double() - want).abs()
    e_sig, e_tanh = err[..., [0, 1, 3]].max().item(), err[..., 2].max().item()
    zt = gx[..., 2]
    mid = (zt.abs() >= 1e-4) & (zt.abs() <= 1e-2)
    rel = ((tg.double() - tanh).abs() / tanh.abs())[mid].max().item()
    e_c = ((c.double() - want_c).abs() / (1 + cp.abs())).max().item()
    e_h = (h.double() - want_h).abs().max().item()
    print(f"gates {label}: sigmoid {e_sig:.3g}  tanh {e_tanh:.3g}  (documented {GATE_TOL:g});  tanh relative on "
          f"1e-4 <= |z| <= 1e-2, {int(mid.sum())} points: {rel:.3g};  c / (1 + |c0|) {e_c:.3g}  h {e_h:.3g}")
    at_inf = torch.isinf(gx).nonzero().tolist()
    assert len(at_inf) == 8
    for idx in at_inf:                              # s(+inf) = 1, s(-inf) = 0, tanh(+-inf) = +-1, exactly
        exact = 1.0 if gx[tuple(idx)] > 0 else (-1.0 if idx[3] == 2 else 0.0)
        assert gates[tuple(idx)].item() == exact, (label, idx, gates[tuple(idx)].item(), exact)
    assert e_sig <= GATE_TOL and e_tanh <= GATE_TOL, (label, e_sig, e_tanh)
    assert e_c <= 5e-7, (label, e_c)
    assert e_h <= 2e-5, (label, e_h)
    return max(e_sig, e_tanh)


@pytest.mark.parametrize("B,H", [(1000, 64), (40, 256)])
def test_gate_functions_against_float64(hip_backend, B, H):
    """T = 1 and no h0: the kernel skips the matrix product, `gates` is (s(z_i), s(z_f), tanh(z_g), s(z_o)) of the gx
    handed in, c = f c0 + i g and h = o tanh(c).  Finite everywhere, the ranges kept, the documented 2e-7 against
    float64, the infinities exact, c within 5e-7 (1 + |c0|) (the gate error through f c0 + i g, and one rounding), h
    within 2e-5.  B = 1000: 63 row tiles, the last with 8 live rows."""
    lib = hip_backend
    p = ops._ptr
    st = torch.cuda.current_stream().cuda_stream
    gx = _gate_inputs(B, H, seed=B + H)
    g = torch.Generator(device="cpu").manual_seed(B)
    c0 = (torch.rand(B, H, generator=g) * 2 - 1) * 50
    c0[::7] = 0.0
    r = _abi.LstmDesc(abi_version=_abi.LSTM_ABI_VERSION, T=1, B=B, H=H)
    nb = lib.lstm_workspace_bytes(r)
    w_hh = torch.zeros(4 * H, H, device="cuda")
    gx_d = gx.cuda()
    worst = 0.0
    for state in (None, c0):
        ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device="cuda")
        gates, c_all, h_all = (torch.full(s, float("nan"), device="cuda") for s in ((1, B, H, 4), (1, B, H), (1, B, H)))
        if state is None:
            lib.lstm_forward(r, p(w_hh), p(gx_d), p(gates), p(c_all), p(h_all), p(ws), nb, st)
        else:
            c0_d = state.cuda()
            lib.lstm_forward_hx(r, p(w_hh), p(gx_d), None, p(c0_d), p(gates), p(c_all), p(h_all), p(ws), nb, st)
        lib.lstm_check(r, p(ws), st)
        worst = max(worst, _check_gates(f"B {B} H {H} {'zero state' if state is None else 'c0 in +-50'}", gx, state,
                                        gates.cpu(), c_all.cpu()[0], h_all.cpu()[0]))
    print(f"largest gate error B {B} H {H}: {worst:.3g}")


# ------------------------------------------------------------------------------------------------ (b) reverse mode, zero state

@pytest.mark.parametrize("regime,shape", ls.cases(ls.ZERO_STATE), ids=ls.case_id)
def test_reverse_mode_from_a_zero_state(hip_backend, regime, shape):
    """The loss is (out w).sum() + (c_n v).sum()."""
    _reverse(ls.problem(regime, shape))


FORMS = [(ls.OTHER_FORMS[0], {"HBVX_LSTM_UNITS": "16"}),             # the host picks 8 units there
         (ls.OTHER_FORMS[1], {"HBVX_LSTM_UNITS": "16"}), (ls.OTHER_FORMS[1], {"HBVX_LSTM_WGS_PER_CU": "3"})]


@pytest.mark.parametrize("shape,env", FORMS, ids=lambda v: ls.case_id(v) if isinstance(v, tuple) else "-".join(f"{k[10:]}{x}" for k, x in v.items()))
@pytest.mark.parametrize("regime", ls.REGIMES)
def test_reverse_mode_in_the_other_kernel_forms(hip_backend, monkeypatch, regime, shape, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = ls.problem(regime, shape)
    _reverse(prob, label=f"{prob.label} [{' '.join(f'{k[10:]}={v}' for k, v in env.items())}]")


# ------------------------------------------------------------------------------------------------ (c), (d) with a state

@pytest.mark.parametrize("regime,shape", ls.cases(ls.WITH_STATE), ids=ls.case_id)
def test_reverse_mode_with_a_state(hip_backend, regime, shape):
    """h0 uniform in +-1, c0 in +-50; the loss on out, h_n and c_n, gradients to h0 and c0 too."""
    _reverse(ls.problem(regime, shape))


@pytest.mark.parametrize("regime,shape", ls.cases(ls.TWO_LAYERS), ids=ls.case_id)
def test_reverse_mode_two_layers(hip_backend, regime, shape):
    _reverse(ls.problem(regime, shape))


# ------------------------------------------------------------------------------------------------ (e) forward mode

D = 3


def _on_gpu(prob):
    mod = ls.module(prob, "cuda")
    return mod, prob.x.cuda(), tuple(t.cuda() for t in prob.hx)


@pytest.mark.parametrize("regime,shape", ls.cases(ls.FORWARD_MODE), ids=ls.case_id)
def test_one_direction_under_forward_ad(hip_backend, regime, shape):
    """k_lstm_tan: x, h0, c0 and every parameter carry a tangent."""
    prob = ls.problem(regime, shape)
    mod, x, hx = _on_gpu(prob)
    dirs = {k: v[0].cuda() for k, v in ls.directions(prob, D).items()}
    _, got = _jvp(mod, x, hx, dirs)
    ls.compare_tangents(prob, got, 0, D, label=f"{prob.label} [fwAD]")


@pytest.mark.parametrize("regime,shape", ls.cases(ls.FORWARD_MODE), ids=ls.case_id)
def test_three_directions_in_pieces_of_two(hip_backend, regime, shape):
    """k_lstm_dirs through SeqLSTM.jvp_batch with max_directions = 2: every direction against float64 forward_ad."""
    prob = ls.problem(regime, shape)
    mod, x, hx = _on_gpu(prob)
    tans = {k: v.cuda() for k, v in ls.directions(prob, D).items()}
    _, (out_t, (hn_t, cn_t)) = mod.jvp_batch(x, hx, tangents=tans, max_directions=2)
    bad = []
    for d in range(D):
        try:
            ls.compare_tangents(prob, [out_t[d], hn_t[d], cn_t[d]], d, D, label=f"{prob.label} [batch]")
        except AssertionError as e:
            bad.append(e)
    assert not bad, bad


@pytest.mark.parametrize("regime,shape", ls.cases(ls.FORWARD_MODE), ids=ls.case_id)
def test_batch_slices_are_the_one_direction_bits(hip_backend, regime, shape):
    """hbvx_lstm_tangent_batch on the regime's primal (its gates, c_all and c0) against hbvx_lstm_tangent direction by
    direction on the same buffers: torch.equal, as tests/test_lstm_jvp_batch.py demands on synthetic gates."""
    prob = ls.problem(regime, shape)
    lib = hip_backend
    p = ops._ptr
    st = torch.cuda.current_stream().cuda_stream
    T, B, H = prob.T, prob.B, prob.H
    sd = {k: v.cuda() for k, v in prob.sd.items()}
    with torch.no_grad():
        _, _, w_hh, gates, c_all, _, _, _, c0 = lstm._primal(prob.x.cuda(), sd["weight_ih_l0"], sd["weight_hh_l0"], sd["bias_ih_l0"],
                                                              sd["bias_hh_l0"], True, prob.hx[0][0].cuda(), prob.hx[1][0].cuda())
    g = torch.Generator(device="cpu").manual_seed(T + B + H)
    gx_t, h0_t, c0_t = (torch.randn(*s, generator=g).cuda() for s in ((D, T, B, H, 4), (D, B, H), (D, B, H)))
    r = _abi.LstmDesc(abi_version=_abi.LSTM_ABI_VERSION, T=T, B=B, H=H)
    nb = lib.lstm_tangent_batch_workspace_bytes(r, D)
    ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device="cuda")
    h_t, c_t = torch.full((D, T, B, H), float("nan"), device="cuda"), torch.full((D, B, H), float("nan"), device="cuda")
    lib.lstm_tangent_batch(r, D, p(w_hh), p(gates), p(c0), p(c_all), p(gx_t), p(h0_t), p(c0_t), p(h_t), p(c_t), p(ws), nb, st)
    lib.lstm_check(r, p(ws), st)
    nb1 = lib.lstm_workspace_bytes(r)
    ws1 = torch.empty((nb1 + 3) // 4, dtype=torch.float32, device="cuda")
    for d in range(D):
        h1, c1 = torch.full((T, B, H), float("nan"), device="cuda"), torch.full((B, H), float("nan"), device="cuda")
        lib.lstm_tangent(r, p(w_hh), p(gates), p(c0), p(c_all), p(gx_t[d]), p(h0_t[d]), p(c0_t[d]), p(h1), p(c1), p(ws1), nb1, st)
        lib.lstm_check(r, p(ws1), st)
        assert torch.isfinite(h1).all() and torch.isfinite(c1).all(), d
        assert torch.equal(h_t[d], h1) and torch.equal(c_t[d], c1), d
