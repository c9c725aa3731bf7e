"""CPU tier: the unit hydrograph's per-tap arithmetic (hbvx_popk::gamma_denom / gamma_tap, hydrodl2_amd/csrc/hbv_pop.h),
which k_uh_gamma runs with one thread per (basin, tap), compiled for the host without fused contraction and put
together in the kernel's order (tests/hosttest/uh_tap_host.cpp): the 15 values of a basin summed in ascending k, zeros
from L on included, each divided by the sum.  It must give the bits of gamma_taps, the whole-basin restatement the
population kernels run (the two keep separate texts, hbv_pop.h), and the sum and the divide must be the ones NumPy
forms in float32 in that order.  Route parameters below zero (the relu), at zero and up to the reference's bounds;
L = 1, 8 and 15 taps."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_pop.h")
SRC = os.path.join(HERE, "hosttest", "uh_tap_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libhbvx_uh_tap.so")
UH = 15


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in (SRC, HDR)):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    return C.CDLL(LIB)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("L", [1, 8, 15])
def test_taps_in_kernel_order_are_gamma_taps(lib, L):
    rng = np.random.default_rng(70 + L)
    n = 4000
    a = rng.uniform(-0.5, 2.9, n).astype(np.float32)
    bb = rng.uniform(-0.5, 6.5, n).astype(np.float32)
    a[:3], bb[:3] = (0.0, 2.9, -0.25), (0.0, 6.5, -0.25)
    raw, uh, ref = (np.full((n, UH), np.nan, np.float32) for _ in range(3))
    lib.uh_by_taps(n, _ptr(a), _ptr(bb), L, _ptr(raw), _ptr(uh))
    lib.uh_by_gamma_taps(n, _ptr(a), _ptr(bb), L, _ptr(ref))
    assert np.isfinite(uh).all() and (raw[:, L:] == 0).all() and (uh[:, L:] == 0).all()
    assert (uh.view(np.uint32) == ref.view(np.uint32)).all()
    s = np.zeros(n, np.float32)
    for k in range(UH):
        s = s + raw[:, k]
    want = raw / s[:, None]
    assert want.dtype == np.float32
    assert (uh[:, :L].view(np.uint32) == np.ascontiguousarray(want[:, :L]).view(np.uint32)).all()
