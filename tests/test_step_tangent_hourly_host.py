"""CPU tier: the tangent of one hour of the hourly model (hbvx::Step<MODEL_HOURLY>::tan,
hydrodl2_amd/csrc/hbv_step_hourly.h) compiled for the host is the transpose of its adjoint (Step::bwd) on the same
intermediates: <w, J v> == <J^T w, v> over random hours -- warm, cold (SM = 0, P = 0), tied (an empty pack with
T == TT and parPERC * dt == SUZ1) and storm hours (rain above the infiltration capacity, IE > 0), with `ac` and
`elev` drawn on both sides of 2500 and 2000."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from . import synth

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hosttest", "step_tan_hourly_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libhbvx_steptan_hourly.so")
CSRC = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc")

NP = 19      # NPARAM_MAX
(P_BETA, P_FC, P_K0, P_K1, P_K2, P_LP, P_PERC, P_UZL, P_TT, P_CFMAX, P_CFR, P_CWH, P_BETAET, P_C, P_RT, P_AC, P_F0,
 P_FMIN, P_ALPHA) = range(19)
BOUNDS = [(1.0, 6.0), (50, 1000), (0.05, 0.9), (0.01, 0.5), (0.001, 0.2), (0.2, 1), (0, 10), (0, 100), (-2.5, 2.5),
          (0.5, 10), (0, 0.1), (0, 0.2), (0.3, 5), (0, 1), (0, 20), (0, 2500), (120.0, 2880.0), (0.0, 1.0), (0.5, 5.0)]
KINDS = {"warm": 0, "cold": 0, "tie": 1, "storm": 2}      # the harness's mode bits
F_PERC = 10


@pytest.fixture(scope="module")
def lib():
    deps = [SRC, os.path.join(CSRC, "hbv_step.h"), os.path.join(CSRC, "hbv_step_hourly.h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    d = C.CDLL(LIB)
    d.steptan_hour.restype = C.c_int
    return d


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _hour(lib, st, p, x, nz, ac, elev, mode, v, w):
    ds, dp, dx = (_f(a) for a in v)
    a, g = (_f(b) for b in w)
    out = [np.zeros(n, np.float32) for n in (5, 12, 5, NP, 3, 17)]
    reached = lib.steptan_hour(_ptr(_f(st)), _ptr(_f(p)), _ptr(_f(x)), C.c_float(nz), C.c_float(ac), C.c_float(elev),
                               mode, _ptr(ds), _ptr(dp), _ptr(dx), _ptr(a), _ptr(g), *map(_ptr, out))
    assert reached >= 0
    return out, reached


def _random_hour(seed, kind):
    u = lambda n, s: synth.uniform((n,), seed, s).astype(np.float64)
    pu = u(NP, 1)
    p = np.array([pu[i] * (hi - lo) + lo for i, (lo, hi) in enumerate(BOUNDS)])
    su = u(5, 2)
    st = np.array([40 * su[0] * (su[0] > 0.4), 5 * su[1], 400 * su[2], 60 * su[3], 80 * su[4]])
    xu = u(3, 3)
    x = np.array([3 * xu[0] * (xu[0] > 0.3), 40 * xu[1] - 15, 0.3 * xu[2]])      # depths per hour
    if kind == "cold":
        st[2] = 0.0
        x[0] = 0.0
    if kind == "tie":
        st[0] = 0.0                 # empty snowpack: min(melt potential, SP1) at 0 == 0
        x[1] = np.float32(p[P_TT])  # T == TT: the melt and refreeze clamps at 0 (where elev < 2000)
    ac = 5000.0 * u(1, 4)[0]        # both sides of 2500
    elev = 4000.0 * u(1, 5)[0]      # both sides of 2000
    return st, p, x, ac, elev


def _dirs(seed):
    nl = lambda n, s: synth.normalish((n,), seed, s).astype(np.float64)
    dp = nl(NP, 11) * np.array([(hi - lo) for lo, hi in BOUNDS]) * 0.1
    v = (nl(5, 10), dp, nl(3, 12) * np.array([0.1, 1.0, 0.02]))
    w = (nl(5, 13), nl(12, 14))
    return v, w


@pytest.mark.parametrize("kind", list(KINDS))
def test_tangent_is_transpose_of_adjoint(lib, kind):
    worst, tied, storms, sides = 0.0, 0, 0, set()
    for k in range(200):
        seed = 9000 + 7 * k + list(KINDS).index(kind)
        st, p, x, ac, elev = _random_hour(seed, kind)
        v, w = _dirs(seed)
        (jv_s, jv_f, jtw_s, jtw_p, jtw_x, prim), reached = _hour(lib, st, p, x, 1e-5, ac, elev, KINDS[kind], v, w)
        assert np.isfinite(prim).all()
        tied += reached & 1
        storms += (reached >> 1) & 1
        sides.add((ac >= 2500.0, elev >= 2000.0))
        ds, dp, dx = (_f(a).astype(np.float64) for a in v)
        a, g = (_f(b).astype(np.float64) for b in w)
        terms_l = np.concatenate([a * jv_s, g * jv_f])
        terms_r = np.concatenate([jtw_s * ds, jtw_p * dp, jtw_x * dx])
        lhs, rhs = terms_l.sum(), terms_r.sum()
        scale = max(np.abs(terms_l).sum(), np.abs(terms_r).sum(), 1e-30)
        err = abs(lhs - rhs) / scale
        worst = max(worst, err)
        assert err <= 1e-5, (k, lhs, rhs, scale)
    print(f"worst relative <w,Jv> - <J^T w,v>: {worst:.2e}; tied {tied}, storms {storms} of 200")
    assert len(sides) == 4                      # ac and elev on both sides of their thresholds
    if kind == "tie":
        assert tied >= 100                      # the rounded product parPERC * dt reaches SUZ1 for most draws
    if kind == "storm":
        assert storms == 200


def _tied_hour(lib):
    zero_w = (np.zeros(5), np.zeros(12))
    zero_v = (np.zeros(5), np.zeros(NP), np.zeros(3))
    for seed in range(4242, 4262):
        st, p, x, ac, elev = _random_hour(seed, "warm")
        st[3] = 30.0
        _, reached = _hour(lib, st, p, x, 1e-5, ac, elev, 1, zero_v, zero_w)
        if reached & 1:
            return st, p, x, ac, elev
    raise AssertionError("no draw reached parPERC * dt == SUZ1")


def test_tie_hour_takes_half_weights(lib):
    """On a forced min(SUZ1, parPERC * dt) tie the percolation tangent is the mean of the two branches
    (torch.minimum): d PERC / d parPERC = 1/2, d PERC / d SUZ = 1/2 / dt."""
    st, p, x, ac, elev = _tied_hour(lib)
    w0 = (np.zeros(5), np.zeros(12))
    dp = np.zeros(NP)
    dp[P_PERC] = 1.0
    (_, jv_f, _, _, _, _), reached = _hour(lib, st, p, x, 1e-5, ac, elev, 1, (np.zeros(5), dp, np.zeros(3)), w0)
    assert reached & 1
    assert jv_f[F_PERC] == pytest.approx(0.5, rel=1e-6)
    ds = np.zeros(5)
    ds[3] = 1.0
    (_, jv_f2, _, _, _, _), _ = _hour(lib, st, p, x, 1e-5, ac, elev, 1, (ds, np.zeros(NP), np.zeros(3)), w0)
    assert jv_f2[F_PERC] == pytest.approx(12.0, rel=1e-6)


def test_zero_direction_gives_zeros(lib):
    for kind in KINDS:
        st, p, x, ac, elev = _random_hour(77, kind)
        zero = (np.zeros(5), np.zeros(NP), np.zeros(3))
        (jv_s, jv_f, _, _, _, _), _ = _hour(lib, st, p, x, 1e-5, ac, elev, KINDS[kind], zero,
                                            (np.zeros(5), np.zeros(12)))
        assert not jv_s.any() and not jv_f.any()
