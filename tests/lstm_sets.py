"""Problem sets for the float64 tests of the sequence LSTM (tests/test_lstm_f64.py, tests/test_lstm_f64_gpu.py):
regimes of weights and inputs that a trained parameter network lives in and SeqLSTM's default draw never reaches,
their coverage counted in a float64 run, and the comparison against torch.nn.LSTM in float64.  No test in here.

A regime is a deterministic edit of a default-initialised state dict (uniform in +-1/sqrt(H), torch's creation
order) plus an input recipe.  Everything is drawn from explicit generator seeds and cast to float32 once, so that the
float64 reference, float32 torch and the kernels see the same numbers.  For two layers the edit goes to each layer
(layer 1 sees h in [-1, 1] as its input).

  memory     forget bias += linspace(2, 6, H), input bias += 1, W_ih rows of g x 4, x = randn + 0.5: a third of the
             forget gates above 0.99, cell states in the tens that live for the whole sequence -- c's float32
             rounding accumulates, and dc c_{t-1} f(1-f) is scaled by a large c_{t-1}.
  saturated  W_ih x 12, W_hh x 3, bias_ih += uniform(+-6): pre-activations spread over |z| up to 15, two thirds of
             them beyond |z| = 2 -- the cancellation region of s(1-s) and 1-g^2, not yet exact saturation.
  overflow   W_ih x 80, bias_ih += uniform(+-60): most sigmoids are exactly 0 or 1 in float32 (|z| > 17) and a fifth
             of the g pre-activations are beyond |z| = 45, where lstm_tanh's exp2 overflows.

Tolerances are the committed ones (tests/test_lstm.py, test_lstm_state.py, test_lstm_jvp.py) and none is added: out
and h_n 2e-5 absolute; every gradient (h0's and c0's too) and every tangent 2e-4 (3e-4 for two layers) of the
tensor's largest float64 entry; tensors are compared whole.  c_n and its tangent are the one exception -- float32
cannot hold a cell state of 100 to 2e-5 -- and get the larger of the committed bound (2e-5 + 1e-5 |ref|; the tangent:
the relative one) and K_CN times the largest error of a float32 torch.nn.LSTM on the same problem.
"""
import time

import torch

from hydrodl2_amd.lstm import SeqLSTM

from . import hourly_sets as hs
from .test_lstm_jvp import _directions, _jvp, _tol

REGIMES = ("memory", "saturated", "overflow")

# c_n: twice the largest ratio (kernel error / float32 torch error) measured over every problem of
# tests/test_lstm_f64_gpu.py, rounded up to a power of two; 16 at the most (the ratios are in that module's docstring)
K_CN = 8

OUT_TOL = 2e-5
CN_RTOL = 1e-5

# (T, B, I, H, L, state) of every problem the two tiers run, each in every regime.  The shapes with a state are short:
# c0 is uniform in +-50 and a cell whose forget gate is 1 walks from there through zero in |c0| steps, where the
# rounding it collected at |c| = 50 (4e-6 a step) stands against tanh'(0) = 1 -- in any float32 LSTM; at T = 60 float32
# torch itself is 1.1e-5 off float64 in `out` (H = 256; two layers: 2.6e-5), at these T it keeps within half of every
# tolerance (test_lstm_f64.py holds it to that).
ZERO_STATE = [(400, 17, 5, 64, 1, False), (120, 33, 7, 128, 1, False), (120, 33, 7, 256, 1, False)]
OTHER_FORMS = [(120, 33, 7, 256, 1, False), (120, 33, 7, 64, 1, False)]     # run under HBVX_LSTM_UNITS / _WGS_PER_CU
WITH_STATE = [(24, 19, 7, 64, 1, True), (16, 37, 5, 256, 1, True)]
TWO_LAYERS = [(16, 21, 9, 64, 2, True)]
FORWARD_MODE = [(24, 19, 7, 64, 1, True), (16, 21, 5, 256, 1, True)]
ORACLE = [(40, 19, 11, 64, 1, False), (120, 17, 5, 64, 1, False)]
SHAPES = list(dict.fromkeys(ZERO_STATE + OTHER_FORMS + WITH_STATE + TWO_LAYERS + FORWARD_MODE + ORACLE))

# Problems that float32 torch itself does not hold to half of the tolerances as drawn, shortened or softened until it
# does (floors unchanged).  memory at T = 400: one cell that wanders to |c| = 30 and back to zero puts float32 torch
# 2.2e-5 off in `out`; at T = 320 it is 2e-6 off.  overflow on two layers: layer 1 multiplies layer 0's rounding by
# W_ih x 80 wherever its gates are not saturated (float32 torch: c_n 1.7 times the half tolerance at T = 16); W_ih x 20
# there, the biases -- which alone put the gates where the regime wants them -- as they are.
SHORTENED = {("memory", 400, 17, 5, 64, 1, False): 320}
GAIN = {("overflow", 16, 21, 9, 64, 2, True): 20}


def cases(shapes):
    """(regime, shape) of every regime at every shape of the list: what the tests are parametrised over."""
    return [(regime, shape) for shape in shapes for regime in REGIMES]


def case_id(val):
    return val if isinstance(val, str) else "x".join(map(str, val[:4])) + (f"-L{val[4]}" if val[4] > 1 else "") + ("-hx" if val[5] else "")


def problem(regime, shape):
    """The Problem of a case, made on first use."""
    return make(regime, SHORTENED.get((regime,) + tuple(shape), shape[0]), *shape[1:])


class Problem:
    """key = (regime, T, B, I, H, L, state); sd: float32 state dict, x [T,B,I], hx = (h0, c0) [L,B,H] or None, loss
    weights w (out), u (h_n), v (c_n) -- all float32 host tensors, never written after they are made."""

    def __init__(self, key, sd, x, hx, w, u, v):
        self.key, self.sd, self.x, self.hx, self.w, self.u, self.v = key, sd, x, hx, w, u, v
        self.regime, self.T, self.B, self.I, self.H, self.L, self.state = key

    @property
    def label(self):
        return f"{self.regime} {self.T}x{self.B}x{self.I}x{self.H}" + (f" L{self.L}" if self.L > 1 else "") + \
            (" hx" if self.state else "")


def _seed(key):
    regime, T, B, I, H, L, state = key
    return ((((REGIMES.index(regime) * 1009 + T) * 1009 + B) * 1009 + I) * 1009 + H) * 4 + 2 * (L - 1) + int(state)


def _edit(regime, sd, layer, H, g, gain=None):
    """The regime's edit of one layer, in float64 (cast to float32 by the caller); gain: overflow's factor on W_ih."""
    w_ih, w_hh, b_ih = (sd[f"{n}_l{layer}"] for n in ("weight_ih", "weight_hh", "bias_ih"))
    if regime == "memory":
        b_ih[H:2 * H] += torch.linspace(2, 6, H, dtype=torch.float64)
        b_ih[:H] += 1
        w_ih[2 * H:3 * H] *= 4
    elif regime == "saturated":
        w_ih *= 12
        w_hh *= 3
        b_ih += (torch.rand(4 * H, generator=g, dtype=torch.float64) * 2 - 1) * 6
    elif regime == "overflow":
        w_ih *= 80 if gain is None else gain
        b_ih += (torch.rand(4 * H, generator=g, dtype=torch.float64) * 2 - 1) * 60
    else:
        raise KeyError(regime)


_PROBLEMS, _REF, _TAN, _COV = {}, {}, {}, {}


def make(regime, T, B, I, H, L=1, state=False):
    key = (regime, T, B, I, H, L, bool(state))
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    g = torch.Generator(device="cpu").manual_seed(_seed(key))
    k = H ** -0.5
    uni = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1)      # noqa: E731
    sd = {}
    for layer in range(L):                      # torch.nn.LSTM's creation order
        sd[f"weight_ih_l{layer}"] = uni(4 * H, I if layer == 0 else H) * k
        sd[f"weight_hh_l{layer}"] = uni(4 * H, H) * k
        sd[f"bias_ih_l{layer}"] = uni(4 * H) * k
        sd[f"bias_hh_l{layer}"] = uni(4 * H) * k
    for layer in range(L):
        _edit(regime, sd, layer, H, g, GAIN.get(key))
    x = torch.randn(T, B, I, generator=g, dtype=torch.float64) + (0.5 if regime == "memory" else 0.0)
    hx = (uni(L, B, H), uni(L, B, H) * 50) if state else None
    w, u, v = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((T, B, H), (L, B, H), (L, B, H)))
    f = lambda t: t.float()                                                          # noqa: E731
    _PROBLEMS[key] = Problem(key, {n: f(t) for n, t in sd.items()}, f(x), None if hx is None else (f(hx[0]), f(hx[1])),
                             f(w), f(u), f(v))
    return _PROBLEMS[key]


# ------------------------------------------------------------------------------------------------ coverage

def coverage(prob):
    """Shares of the regime's events in a float64 unrolled run (every layer pooled), and the float64 `out` of the
    last layer, which test_lstm_f64.py holds against torch.nn.LSTM's.  f_hi: forget gate above 0.99; c_big: |c| > 5;
    z_out: pre-activation with |z| >= 2 (the default draw: 0.25); z_mid: 4 <= |z| <= 15; sig_exact: sigmoid
    pre-activation beyond |z| = 17, where the float32 gate is exactly 0 or 1; g_ovf: g pre-activation beyond |z| = 45,
    where lstm_tanh's exp2 overflows; c_max, z_max: the largest |c| and |z|."""
    if prob.key in _COV:
        return _COV[prob.key]
    H, L = prob.H, prob.L
    inp = prob.x.double()
    n = dict(f_hi=0, c_big=0, z_out=0, z_mid=0, sig_exact=0, g_ovf=0)
    cells = gates = 0
    c_max = z_max = 0.0
    for layer in range(L):
        w_ih, w_hh, b_ih, b_hh = (prob.sd[f"{k}_l{layer}"].double() for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
        gx = inp @ w_ih.t() + (b_ih + b_hh)
        h = prob.hx[0][layer].double() if prob.state else torch.zeros(prob.B, H, dtype=torch.float64)
        c = prob.hx[1][layer].double() if prob.state else torch.zeros(prob.B, H, dtype=torch.float64)
        out = []
        for t in range(prob.T):
            z = gx[t] + h @ w_hh.t()
            zi, zf, zg, zo = z.split(H, dim=1)
            f = torch.sigmoid(zf)
            c = f * c + torch.sigmoid(zi) * torch.tanh(zg)
            h = torch.sigmoid(zo) * torch.tanh(c)
            out.append(h)
            a, zs = z.abs(), torch.cat([zi, zf, zo], 1).abs()
            n["f_hi"] += int((f > 0.99).sum())
            n["c_big"] += int((c.abs() > 5).sum())
            n["z_out"] += int((a >= 2).sum())
            n["z_mid"] += int(((a >= 4) & (a <= 15)).sum())
            n["sig_exact"] += int((zs > 17).sum())
            n["g_ovf"] += int((zg.abs() > 45).sum())
            c_max, z_max = max(c_max, float(c.abs().max())), max(z_max, float(a.max()))
        cells += prob.T * prob.B * H
        gates += prob.T * prob.B * 4 * H
        inp = torch.stack(out)
    cov = dict(f_hi=n["f_hi"] / cells, c_big=n["c_big"] / cells, z_out=n["z_out"] / gates, z_mid=n["z_mid"] / gates,
               sig_exact=n["sig_exact"] / (3 * cells), g_ovf=n["g_ovf"] / cells, c_max=c_max, z_max=z_max)
    _COV[prob.key] = (cov, inp)
    return _COV[prob.key]


# Floors: half of what the regimes were designed to (measured at (400,17,5,64), (120,33,7,128) and (120,33,7,256):
# memory f_hi 0.32-0.36, c_big 0.31-0.50, max |c| 45-93; saturated z_out 0.67, max |c| 87-106; overflow sig_exact
# 0.70-0.74, g_ovf 0.20-0.27, max |c| 120-398), hourly_sets.COVER_MIN where a share only has to be non-trivial.  max |c|
# is reached by accumulation, at most one per step: a short record is held to half of T / 4 instead (with a state, c0
# reaches 50 by itself).
FLOORS = {
    "memory": dict(f_hi=0.16, c_big=0.155, c_max=22.5),
    "saturated": dict(z_out=0.335, z_mid=hs.COVER_MIN, c_max=43.5),
    "overflow": dict(sig_exact=0.35, g_ovf=0.10, c_max=60.0),
}
COLUMNS = ("f_hi", "c_big", "z_out", "z_mid", "sig_exact", "g_ovf", "c_max", "z_max")


def floors(prob):
    fl = dict(FLOORS[prob.regime])
    fl["c_max"] = min(fl["c_max"], prob.T / 8)
    return fl


def assert_covered(prob):
    cov = coverage(prob)[0]
    missing = {k: (cov[k], lo) for k, lo in floors(prob).items() if cov[k] < lo}
    assert not missing, f"{prob.label}: the regime no longer does its job: (share, floor) {missing}"
    return cov


def coverage_row(prob):
    cov = coverage(prob)[0]
    return f"{prob.label:34s} " + " ".join(f"{k} {cov[k]:.3g}" for k in COLUMNS)


# ------------------------------------------------------------------------------------------------ references

def _plain_float32():
    """torch's own float32 LSTM cell on the host: the oneDNN one has no forward AD, and one float32 reference serves
    both modes."""
    return torch.backends.mkldnn.flags(enabled=False)


def torch_lstm(prob, dtype):
    ref = torch.nn.LSTM(prob.I, prob.H, num_layers=prob.L).to(dtype)
    ref.load_state_dict({k: v.to(dtype) for k, v in prob.sd.items()})
    return ref


def loss_terms(prob, terms=None):
    """Which of (out, h_n, c_n) carry loss weights: out and c_n without a state (and for a single layer), all three
    with one."""
    if terms is not None:
        return terms
    return (True, True, True) if prob.state else (True, False, True)


def reverse(prob, mod, device="cpu", dtype=torch.float32, terms=None):
    """Outputs and gradients of `mod` (a torch.nn.LSTM or a SeqLSTM holding prob's state dict) on the problem: a dict
    out, h_n, c_n and grads (name -> tensor: the parameters, x, and h0 / c0 with a state), detached."""
    cast = lambda t: t.to(device=device, dtype=dtype)                                 # noqa: E731
    leaf = lambda t: cast(t).detach().clone().requires_grad_(True)                    # noqa: E731
    x = leaf(prob.x)
    hx = tuple(leaf(t) for t in prob.hx) if prob.state else None
    for p in mod.parameters():
        p.grad = None
    out, (hn, cn) = mod(x, hx) if hx is not None else mod(x)
    sum((o * cast(wt)).sum() for o, wt, on in zip((out, hn, cn), (prob.w, prob.u, prob.v), loss_terms(prob, terms)) if on).backward()
    grads = {k: p.grad.detach().clone() for k, p in mod.named_parameters()}
    grads["x"] = x.grad
    if hx is not None:
        grads["h0"], grads["c0"] = hx[0].grad, hx[1].grad
    return dict(out=out.detach(), h_n=hn.detach(), c_n=cn.detach(), grads=grads)


def reference(prob, terms=None):
    """(float64 result, float32 result) of torch.nn.LSTM on the host, once per problem and loss."""
    key = (prob.key, loss_terms(prob, terms))
    if key not in _REF:
        t = time.time()
        r64 = reverse(prob, torch_lstm(prob, torch.float64), dtype=torch.float64, terms=terms)
        with _plain_float32():
            r32 = reverse(prob, torch_lstm(prob, torch.float32), dtype=torch.float32, terms=terms)
        print(f"{prob.label}: torch.nn.LSTM float64 + float32, forward + backward {time.time() - t:.1f} s")
        _REF[key] = (r64, r32)
    return _REF[key]


def module(prob, device):
    mod = SeqLSTM(prob.I, prob.H, check=True, num_layers=prob.L)
    mod.load_state_dict(prob.sd)
    return mod.to(device)


def directions(prob, D):
    """D draws of test_lstm_jvp.py's direction set "all" (x, the state, every parameter), float32 on the host:
    name -> [D, ...] with the state tangents [D, L, B, H]."""
    mod = module(prob, "cpu")
    per = [_directions(mod, prob.x, prob.hx, "all", seed=_seed(prob.key) % 100003 + 17 * d) for d in range(D)]
    return {k: torch.stack([p[k] for p in per]) for k in per[0]}


def tangents(prob, D):
    """(float64, float32): per direction the tangents [out', h_n', c_n'] of torch.nn.LSTM under forward_ad on the
    host, once per problem."""
    key = (prob.key, D)
    if key not in _TAN:
        t = time.time()
        dirs = directions(prob, D)
        res = []
        for dtype in (torch.float64, torch.float32):
            ref = torch_lstm(prob, dtype)
            with _plain_float32():
                res.append([_jvp(ref, prob.x, prob.hx, {k: v[d] for k, v in dirs.items()}, dtype=dtype, device="cpu")[1]
                            for d in range(D)])
        print(f"{prob.label}: torch.nn.LSTM forward_ad float64 + float32, {D} directions {time.time() - t:.1f} s")
        _TAN[key] = tuple(res)
    return _TAN[key]


# ------------------------------------------------------------------------------------------------ comparison

FIGURES = []        # (label, tensor name, error, bound, float32 torch's error): what the docstrings quote


def _err(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs()


def compare_reverse(prob, got, label=None, terms=None, k_cn=None):
    """`got` (reverse()'s dict, from the code under test) against float64 at the committed tolerances; prints every
    figure, then asserts all of them.  Returns {tensor name: (error, bound, float32 torch's error)}."""
    r64, r32 = reference(prob, terms)
    label = label or prob.label
    k_cn = K_CN if k_cn is None else k_cn
    gtol = _tol(prob.L)
    rows, bad = {}, []
    for name in ("out", "h_n", "c_n"):
        a, b = got[name], r64[name]
        assert a.shape == b.shape, (label, name, a.shape, b.shape)
        assert torch.isfinite(a).all(), (label, name, "not finite")
        err, e32 = _err(a, b), _err(r32[name], b).max().item()
        if name == "c_n":
            bound = torch.clamp(OUT_TOL + CN_RTOL * b.abs(), min=k_cn * e32)
        else:
            bound = torch.full_like(err, OUT_TOL)
        worst = (err / bound).argmax()              # c_n: the element nearest its bound, not always the largest error
        rows[name] = (err.flatten()[worst].item(), bound.flatten()[worst].item(), e32)
        if name == "c_n":
            e_cn = err.max().item()
        if not torch.all(err <= bound):
            bad.append(name)
    for name, b in r64["grads"].items():
        a = got["grads"].get(name)
        assert a is not None and a.shape == b.shape, (label, name)
        assert torch.isfinite(a).all(), (label, name, "not finite")
        bound = gtol * max(b.abs().max().item(), 1e-3)
        rows["d" + name] = (_err(a, b).max().item(), bound, _err(r32["grads"][name], b).max().item())
        if rows["d" + name][0] > bound:
            bad.append("d" + name)
    for name, (e, bound, e32) in rows.items():
        print(f"{label:40s} {name:16s} err {e:.3g} bound {bound:.3g} ratio {e / bound:.3g}  float32 torch {e32:.3g}"
              + (f"  largest err {e_cn:.3g} kernel/torch {e_cn / e32:.3g}" if name == "c_n" and e32 > 0 else ""))
        FIGURES.append((label, name, e, bound, e32))
    assert not bad, (label, {n: rows[n] for n in bad})
    return rows


def compare_tangents(prob, got, d, D, label=None, k_cn=None):
    """Direction d's tangents `got` = [out', h_n', c_n'] against float64 forward_ad; as compare_reverse."""
    t64, t32 = tangents(prob, D)
    label = label or prob.label
    k_cn = K_CN if k_cn is None else k_cn
    rows, bad = {}, []
    for name, a, b, c in zip(("out'", "h_n'", "c_n'"), got, t64[d], t32[d]):
        assert a is not None and a.shape == b.shape, (label, d, name)
        assert torch.isfinite(a).all(), (label, d, name, "not finite")
        e32 = _err(c, b).max().item()
        bound = _tol(prob.L) * max(b.abs().max().item(), 1e-3)
        if name == "c_n'":
            bound = max(bound, k_cn * e32)
        rows[name] = (_err(a, b).max().item(), bound, e32)
        if rows[name][0] > bound:
            bad.append(name)
    for name, (e, bound, e32) in rows.items():
        print(f"{label:40s} d={d} {name:12s} err {e:.3g} bound {bound:.3g} ratio {e / bound:.3g}  float32 torch {e32:.3g}")
        FIGURES.append((label, f"d={d} {name}", e, bound, e32))
    assert not bad, (label, d, {n: rows[n] for n in bad})
    return rows


def condition(prob, D=1):
    """float32 torch.nn.LSTM against float64, reverse mode and forward_ad, as ratios of HALF of each committed
    tolerance: {tensor name: ratio}; a well-conditioned problem keeps every one at or below 1."""
    r64, r32 = reference(prob)
    gtol = _tol(prob.L)
    out = {}
    for name in ("out", "h_n"):
        out[name] = _err(r32[name], r64[name]).max().item() / (0.5 * OUT_TOL)
    out["c_n"] = (_err(r32["c_n"], r64["c_n"]) / (0.5 * (OUT_TOL + CN_RTOL * r64["c_n"].abs()))).max().item()
    for name, b in r64["grads"].items():
        out["d" + name] = _err(r32["grads"][name], b).max().item() / (0.5 * gtol * max(b.abs().max().item(), 1e-3))
    t64, t32 = tangents(prob, D)
    for d in range(D):
        for name, b, c in zip(("out'", "h_n'", "c_n'"), t64[d], t32[d]):
            r = _err(c, b).max().item() / (0.5 * gtol * max(b.abs().max().item(), 1e-3))
            out[name] = max(out.get(name, 0.0), r)
    return out
