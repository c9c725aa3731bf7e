"""CPU tier: the tangent of one HBV day (hbvx::Step::tan, hydrodl2_amd/csrc/hbv_step.h) compiled for the host is the
transpose of its adjoint (Step::bwd) on the same intermediates: <w, J v> == <J^T w, v> over random days of HBV 1.0,
1.1p and 2.0, including cold days (SM = 0) and days with forced ties (parPERC == SUZ1, T == TT, an empty snowpack)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from . import synth

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hosttest", "step_tan_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libhbvx_steptan.so")
STEP_H = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_step.h")

NP = 19      # NPARAM_MAX
P_BETA, P_FC, P_K0, P_K1, P_K2, P_LP, P_PERC, P_UZL, P_TT, P_CFMAX, P_CFR, P_CWH, P_BETAET, P_C, P_RT, P_AC = range(16)
BOUNDS = [(1.0, 6.0), (50, 1000), (0.05, 0.9), (0.01, 0.5), (0.001, 0.2), (0.2, 1), (0, 10), (0, 100), (-2.5, 2.5),
          (0.5, 10), (0, 0.1), (0, 0.2), (0.3, 5), (0, 1), (0, 20), (0, 2500)]
MODELS = [(0, 0, 12), (0, 1, 13), (1, 1, 14), (2, 1, 16)]     # (model, BETAET, n_param)


@pytest.fixture(scope="module")
def lib():
    deps = [SRC, STEP_H, os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_step_hourly.h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    d = C.CDLL(LIB)
    d.steptan_day.restype = C.c_int
    return d


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _day(lib, model, betaet, st, p, x, nz, ac, elev, tie, v, w):
    ds, dp, dx = (_f(a) for a in v)
    a, g = (_f(b) for b in w)
    out = [np.zeros(n, np.float32) for n in (5, 12, 5, NP, 3, 17)]
    rc = lib.steptan_day(model, betaet, _ptr(_f(st)), _ptr(_f(p)), _ptr(_f(x)), C.c_float(nz), C.c_float(ac),
                         C.c_float(elev), tie, _ptr(ds), _ptr(dp), _ptr(dx), _ptr(a), _ptr(g), *map(_ptr, out))
    assert rc == 0
    return out


def _random_day(seed, n_param, kind):
    u = lambda n, s: synth.uniform((n,), seed, s).astype(np.float64)
    p = np.zeros(NP)
    pu = u(16, 1)
    for i in range(n_param):
        lo, hi = BOUNDS[i]
        p[i] = pu[i] * (hi - lo) + lo
    su = u(5, 2)
    st = np.array([40 * su[0] * (su[0] > 0.4), 5 * su[1], 400 * su[2], 60 * su[3], 80 * su[4]])
    xu = u(3, 3)
    x = np.array([30 * xu[0] * (xu[0] > 0.3), 40 * xu[1] - 15, 6 * xu[2]])
    if kind == "cold":
        st[2] = 0.0
        x[0] = 0.0
    if kind == "tie":
        st[0] = 0.0                 # empty snowpack: min(melt potential, SP1) at 0 == 0
        x[1] = np.float32(p[P_TT])  # T == TT: the melt and refreeze clamps at 0
    ac = 3000.0 * u(1, 4)[0]
    elev = 3000.0 * u(1, 5)[0]
    return st, p, x, ac, elev


def _dirs(seed, n_param):
    nl = lambda n, s: synth.normalish((n,), seed, s).astype(np.float64)
    dp = np.zeros(NP)
    dp[:n_param] = nl(n_param, 11) * np.array([(hi - lo) for lo, hi in BOUNDS[:n_param]]) * 0.1
    v = (nl(5, 10), dp, nl(3, 12))
    w = (nl(5, 13), nl(12, 14))
    return v, w


@pytest.mark.parametrize("model,betaet,n_param", MODELS, ids=["hbv10", "hbv10-betaet", "hbv11p", "hbv20"])
@pytest.mark.parametrize("kind", ["warm", "cold", "tie"])
def test_tangent_is_transpose_of_adjoint(lib, model, betaet, n_param, kind):
    worst = 0.0
    for k in range(200):
        seed = 1000 * model + 100 * betaet + 7 * k + {"warm": 0, "cold": 1, "tie": 2}[kind]
        st, p, x, ac, elev = _random_day(seed, n_param, kind)
        v, w = _dirs(seed, n_param)
        jv_s, jv_f, jtw_s, jtw_p, jtw_x, prim = _day(lib, model, betaet, st, p, x, 1e-5, ac, elev,
                                                     1 if kind == "tie" else 0, v, w)
        assert np.isfinite(prim).all()
        if model == 0:
            jv_f[11] = 0.0
            assert jtw_p[P_C] == 0.0 and jtw_p[P_RT] == 0.0 and jtw_p[P_AC] == 0.0
        ds, dp, dx = (_f(a).astype(np.float64) for a in v)
        a, g = (_f(b).astype(np.float64) for b in w)
        terms_l = np.concatenate([a * jv_s, g * jv_f])
        terms_r = np.concatenate([jtw_s * ds, jtw_p * dp, jtw_x * dx])
        lhs, rhs = terms_l.sum(), terms_r.sum()
        scale = max(np.abs(terms_l).sum(), np.abs(terms_r).sum(), 1e-30)
        err = abs(lhs - rhs) / scale
        worst = max(worst, err)
        assert err <= 1e-5, (k, lhs, rhs, scale)
    print(f"worst relative <w,Jv> - <J^T w,v>: {worst:.2e}")


def test_tie_day_takes_half_weights(lib):
    """On a forced parPERC == SUZ1 tie the percolation tangent is the mean of the two branches (torch.minimum)."""
    st, p, x, ac, elev = _random_day(4242, 12, "warm")
    st[3] = 30.0
    zero = (np.zeros(5), np.zeros(NP), np.zeros(3))
    w0 = (np.zeros(5), np.zeros(12))
    dp = np.zeros(NP)
    dp[P_PERC] = 1.0
    _, jv_f, _, _, _, prim = _day(lib, 0, 0, st, p, x, 1e-5, ac, elev, 1, (np.zeros(5), dp, np.zeros(3)), w0)
    assert jv_f[10] == pytest.approx(0.5, abs=0)
    ds = np.zeros(5)
    ds[3] = 1.0
    _, jv_f2, _, _, _, _ = _day(lib, 0, 0, st, p, x, 1e-5, ac, elev, 1, (ds, np.zeros(NP), np.zeros(3)), w0)
    assert jv_f2[10] == pytest.approx(0.5, abs=0)
    _, jv_f0, _, _, _, _ = _day(lib, 0, 0, st, p, x, 1e-5, ac, elev, 1, zero, w0)
    assert not jv_f0.any()
