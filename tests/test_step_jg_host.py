"""CPU tier: the parameter-Jacobian application of one HBV 1.0 day (hbvx::Step::jt_gp, hydrodl2_amd/csrc/hbv_step.h),
which the one-pass static adjoint (hbv_chunked.h, k_bwd_chunk_onepass) runs on every vector it carries through a
chunk, compiled for the host.  For each of the four vector kinds -- the snow-block unit adjoints (level 0), the soil
one (level 1), the full ones (level 2) and the affine offset with its runoff sources -- its gp[] must equal what
Step::bwd() adds for the same vector (1e-6 of each element, plus a floor of FLOOR x the vector's largest), over random warm, cold and tie days (empty snowpack with T == TT,
parPERC == SUZ1), with and without parBETAET; and the vector it propagates must be jt_unit's / jt_affine's bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from . import synth
from .test_step_tangent_host import NP, P_BETAET, _random_day

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hosttest", "step_jg_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libhbvx_stepjg.so")
STEP_H = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_step.h")
SNOW = [8, 9, 10, 11]                  # TT CFMAX CFR CWH
SOIL = [0, 1, 5]                       # BETA FC LP (+ BETAET)
# Floor of the comparison, as a fraction of the vector's largest gp: the worst difference measured over these draws is
# 2.9e-6 of it (level 1 vectors on cold and tie days; see the comment in the test).
FLOOR = 5e-6


@pytest.fixture(scope="module")
def lib():
    deps = [SRC, STEP_H, os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_step_hourly.h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    d = C.CDLL(LIB)
    d.stepjg_day.restype = C.c_int
    return d


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _reached(level, betaet):
    """Parameters a vector of this kind can reach (the sparsity the kernel's accumulators rely on)."""
    if level == 0:
        return SNOW
    if level == 1:
        return SNOW + SOIL + ([P_BETAET] if betaet else [])
    return list(range(13 if betaet else 12))


@pytest.mark.parametrize("betaet", [False, True])
@pytest.mark.parametrize("kind", ["warm", "cold", "tie"])
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_jt_gp_equals_bwd_gp(lib, betaet, kind, level):
    n_param = 13 if betaet else 12
    reach = _reached(level, betaet)
    worst = 0.0
    for k in range(300):
        seed = 5000 + 100 * betaet + 11 * k + {"warm": 0, "cold": 1, "tie": 2}[kind] + 3 * level
        st, p, x, _, _ = _random_day(seed, n_param, kind)
        a = synth.normalish((5,), seed, 21).astype(np.float64)
        if level <= 1:
            a[2 + level:] = 0.0
        src = synth.normalish((3,), seed, 22).astype(np.float64) if level == 3 else np.zeros(3)
        out = [np.zeros(n, np.float32) for n in (NP, 5, NP, 5, 5)]
        assert lib.stepjg_day(int(betaet), _ptr(_f(st)), _ptr(_f(p)), _ptr(_f(x)), C.c_float(1e-5),
                              1 if kind == "tie" else 0, level, _ptr(_f(a)), _ptr(_f(src)), *map(_ptr, out)) == 0
        gp_new, a_new, gp_ref, a_ref, a_jt = out
        assert np.array_equal(a_new, a_jt), (k, a_new, a_jt)
        assert np.isfinite(gp_ref).all() and np.isfinite(gp_new).all()
        off = [i for i in range(NP) if i not in reach]
        assert not gp_new[off].any() and not gp_ref[off].any(), (k, off)
        ref, new = gp_ref.astype(np.float64), gp_new.astype(np.float64)
        # Per element: 1e-6 of its own value, plus a floor of FLOOR x the vector's largest gp.  The floor is there
        # because jt_unit / jt_affine propagate the vector in another association than bwd() (the a-propagation the
        # two-pass map already uses; its soil factor kap is a difference that cancels), and where a parameter's own
        # terms cancel (parTT: refreeze against melt) that rounding shows against the small sum.
        tol = 1e-6 * np.abs(ref) + FLOOR * np.abs(ref).max()
        excess = np.abs(new - ref) - tol
        worst = max(worst, float((np.abs(new - ref) / max(np.abs(ref).max(), 1e-30)).max()))
        assert (excess <= 0).all(), (k, excess.argmax(), new, ref)
    print(f"level {level}: worst |gp difference| / max|gp| {worst:.2e}")
