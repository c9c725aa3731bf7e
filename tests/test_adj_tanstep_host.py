"""CPU tier: the implicit scheme's day-level tangent, `adj_tanstep` of hydrodl2_amd/csrc/hbv_adj_step.h, compiled for
the host (tests/hosttest/adj_tan_host.cpp) and checked on random lane-days, both BETAET instances,

(a) against the adjoint of the same header: one-day duality
        <a, x_dot> + gQ Q_dot == <dL/dx_t, xt_dot> + <gp, p_dot>
    with (dL/dx_t, gp) from adj_backstep.  Both sides are float32 results summed in float64; the bound is
    DUALITY_EPS * eps32 * (sum of the magnitudes of all terms of both sides).  DUALITY_EPS = 8 comes from the length
    of the chain between the inputs and either side: about 40 roundings in the flux partials and 20 in the
    substitution, independent in sign (sqrt(60) ~ 8), and every pivot of I/dt - F is at least 1/dt, so nothing
    amplifies them.  Needed on the 400 lane-days per instance below: 0.88 (BETAET), 0.75 (without).
(b) against float64: `rhs` of oracle/hbv_adj_oracle.py under autograd, x_dot = -J^-1 dG/d(x_t, theta, clim) . direction
    at the same state, forcing tangents included; rtol 2e-3 + 2e-4 x max.

The state of a lane-day need not be a solved one for either check (the implicit-function derivative is linear algebra
on df/dx at whatever state it is given); the draws cover dry soil below its clamp, SM > FC, SUZ on both sides of UZL,
Tf on both sides of TT and an empty snowpack."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from .test_hbv_adj import _close, adj_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hosttest", "adj_tan_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libadj_tan_host.so")
CSRC = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "hbv_step.h"), os.path.join(CSRC, "hbv_adj_step.h")]

N_ROWS = 400
EPS32 = float(np.finfo(np.float32).eps)
DUALITY_EPS = 8.0
NAMES13 = list(adj_oracle.BOUNDS)


@pytest.fixture(scope="module")
def tanlib():
    newest = max(os.path.getmtime(f) for f in DEPS)
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    dll = C.CDLL(LIB)
    fp = C.c_void_p
    dll.adj_tan_rows.argtypes = [C.c_int, C.c_int] + [fp] * 8
    dll.adj_tan_rows.restype = None
    dll.adj_back_rows.argtypes = [C.c_int, C.c_int] + [fp] * 6
    dll.adj_back_rows.restype = None
    return dll


def _ptr(a):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def _rows(betaet: bool, seed: int):
    """Random lane-days: float32 arrays for the header, the same numbers for the oracle."""
    rng = np.random.default_rng(seed)
    n = N_ROWS
    lo = np.array([adj_oracle.BOUNDS[k][0] for k in NAMES13], dtype=np.float64)
    hi = np.array([adj_oracle.BOUNDS[k][1] for k in NAMES13], dtype=np.float64)
    p = (lo + rng.random((n, 13)) * (hi - lo)).astype(np.float32)
    FC, UZL, TT = p[:, 1], p[:, 7], p[:, 8]
    u = rng.random((n, 8))
    x = np.empty((n, 5), dtype=np.float32)
    x[:, 0] = np.where(u[:, 0] < 0.3, 0.0, rng.random(n) * 80.0)                   # empty snowpack
    x[:, 1] = np.where(u[:, 1] < 0.3, 0.0, rng.random(n) * 10.0)
    sm = (0.05 + 0.95 * rng.random(n)) * FC
    sm = np.where(u[:, 2] < 0.15, rng.random(n) * 2e-8 - 1e-8, sm)                  # dry soil, either side of the clamp
    sm = np.where(u[:, 2] > 0.75, FC * (1.0 + 0.2 * rng.random(n)), sm)              # above field capacity
    x[:, 2] = sm
    x[:, 3] = np.where(u[:, 3] < 0.1, -rng.random(n), rng.random(n) * (2.0 * UZL + 5.0))
    x[:, 4] = rng.random(n) * 50.0
    clim = np.empty((n, 3), dtype=np.float32)
    clim[:, 0] = np.where(u[:, 4] < 0.3, 0.0, rng.random(n) * 20.0)
    clim[:, 1] = TT + (rng.random(n) * 16.0 - 8.0)
    clim[:, 2] = rng.random(n) * 8.0
    xt_dot = rng.standard_normal((n, 5)).astype(np.float32)
    p_dot = (rng.standard_normal((n, 13)) * 0.05 * (hi - lo)).astype(np.float32)
    if not betaet:
        p_dot[:, 12] = 0.0
    c_dot = rng.standard_normal((n, 3)).astype(np.float32)
    a = rng.standard_normal((n, 5)).astype(np.float32)
    gq = rng.standard_normal(n).astype(np.float32)
    # the regimes the docstring names are all drawn
    assert (x[:, 2] < 1e-8).any() and (x[:, 2] > FC).any() and (x[:, 0] == 0).any()
    assert (x[:, 3] > UZL).any() and ((x[:, 3] < UZL) & (x[:, 3] > 0)).any()
    assert (clim[:, 1] < TT).any() and (clim[:, 1] >= TT).any()
    return dict(p=p, x=x, clim=clim, xt_dot=xt_dot, p_dot=p_dot, c_dot=c_dot, a=a, gq=gq, lo=lo, hi=hi)


def _tangent(dll, betaet, r, c_dot=None):
    n = N_ROWS
    x_dot = np.full((n, 5), np.nan, dtype=np.float32)
    q_dot = np.full(n, np.nan, dtype=np.float32)
    cd = r["c_dot"] if c_dot is None else c_dot
    dll.adj_tan_rows(int(betaet), n, _ptr(r["p"]), _ptr(r["clim"]), _ptr(r["x"]), _ptr(r["xt_dot"]), _ptr(r["p_dot"]),
                     _ptr(cd), _ptr(x_dot), _ptr(q_dot))
    return x_dot, q_dot


@pytest.mark.parametrize("betaet", [True, False], ids=["betaet", "plain"])
def test_one_day_duality_with_the_adjoint(tanlib, betaet):
    r = _rows(betaet, 11 if betaet else 12)
    n = N_ROWS
    x_dot, q_dot = _tangent(tanlib, betaet, r, np.zeros((n, 3), dtype=np.float32))   # the adjoint has no forcing gradient
    a_t = r["a"].copy()
    gp = np.full((n, 13), np.nan, dtype=np.float32)
    tanlib.adj_back_rows(int(betaet), n, _ptr(r["p"]), _ptr(r["clim"]), _ptr(r["x"]), _ptr(r["gq"]), _ptr(a_t), _ptr(gp))
    npar = 13 if betaet else 12
    f8 = np.float64
    left = [r["a"].astype(f8) * x_dot, (r["gq"].astype(f8) * q_dot)[:, None]]
    right = [a_t.astype(f8) * r["xt_dot"], gp[:, :npar].astype(f8) * r["p_dot"][:, :npar]]
    lhs = sum(t.sum(1) for t in left)
    rhs = sum(t.sum(1) for t in right)
    mag = sum(np.abs(t).sum(1) for t in left + right)
    assert np.isfinite(lhs).all() and np.isfinite(rhs).all()
    need = np.abs(lhs - rhs) / (EPS32 * mag)
    print(f"duality, betaet={betaet}: multiple of eps32 * sum|terms| needed {need.max():.2f}")
    assert (need <= DUALITY_EPS).all(), f"worst row {int(need.argmax())}: {need.max():.1f} eps"


@pytest.mark.parametrize("betaet", [True, False], ids=["betaet", "plain"])
def test_one_day_tangent_against_float64(tanlib, betaet):
    r = _rows(betaet, 21 if betaet else 22)
    x_dot, q_dot = _tangent(tanlib, betaet, r)
    names = NAMES13 if betaet else NAMES13[:12]
    k = len(names)
    span = torch.from_numpy(r["hi"] - r["lo"])[:k]
    f8 = torch.float64
    y = torch.from_numpy(r["x"]).to(f8)
    theta = (torch.from_numpy(r["p"]).to(f8)[:, :k] - torch.from_numpy(r["lo"])[:k]) / span
    theta_dot = torch.from_numpy(r["p_dot"]).to(f8)[:, :k] / span
    clim = torch.from_numpy(r["clim"]).to(f8)
    clim_dot = torch.from_numpy(r["c_dot"]).to(f8)
    # explicit part: d(f, Q)/d(theta, clim) . direction at fixed y
    _, (f_dot, q_exp) = torch.autograd.functional.jvp(lambda th, cl: adj_oracle.rhs(y, th, cl, names), (theta, clim),
                                                      (theta_dot, clim_dot))
    yy = y.clone().requires_grad_(True)
    f, Q = adj_oracle.rhs(yy, theta, clim, names)
    dfdy = torch.stack([torch.autograd.grad(f[:, i].sum(), yy, retain_graph=True)[0] for i in range(5)], dim=1)
    dQdy = torch.autograd.grad(Q.sum(), yy)[0]
    J = torch.eye(5, dtype=f8) - dfdy                                   # dG/dx with dt = 1
    g = torch.from_numpy(r["xt_dot"]).to(f8) + f_dot                     # -dG/d(x_t, theta, clim) . direction
    want_x = torch.linalg.solve(J, g.unsqueeze(-1)).squeeze(-1)
    want_q = (dQdy * want_x).sum(1) + q_exp
    _close("x_dot", x_dot, want_x.numpy(), 2e-3, 2e-4)
    _close("Q_dot", q_dot, want_q.numpy(), 2e-3, 2e-4)
