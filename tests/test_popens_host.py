"""CPU tier: the routing window of hbvx_population_ensemble across calls -- hbvx_popk::Basin::load_history /
save_history (hydrodl2_amd/csrc/hbv_pop.h) compiled for the host (tests/hosttest/popens_host.cpp).

A 40-day series is pushed in one go and in the splits 17|1|22 and 1|1|...|1, each piece handed the history the piece
before it saved: the routed values and the final history agree BIT FOR BIT with the one run, with 15 taps and with
L = 7 (a record shorter than the window: taps 7..14 are zero, the window still carries 14 days).  The history's
meaning is checked too: entry k after day t is the un-routed value of day t - k, and a NULL history is zeros, which is
what a call that starts the record has.  The routed values of the one run are held to the float64 convolution with the
bound of tests/test_pop_host.py, so that "the same bits" is not the same mistake twice."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from .test_pop_host import gamma

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hosttest", "popens_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libpopens_host.so")
HDR = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_pop.h")

UH, HIST, T, B = 15, 14, 40, 9
SPLITS = {"17|1|22": [17, 1, 22], "forty one-day windows": [1] * 40, "15|25": [15, 25], "39|1": [39, 1]}


@pytest.fixture(scope="module")
def enslib():
    newest = max(os.path.getmtime(f) for f in (SRC, HDR))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    dll = C.CDLL(LIB)
    dll.popens_host.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
    dll.popens_host.restype = None
    return dll


def draw(seed):
    rng = np.random.default_rng(seed)
    q = (rng.gamma(0.7, 3.0, size=(T, B)) * 10.0 ** rng.uniform(-1, 1, size=(1, B))).astype(np.float32)
    q[rng.random((T, B)) < 0.15] = 0.0
    q[3, 2] = -0.0                                      # a negative zero travels through the history as itself
    a = rng.uniform(0.0, 2.9, size=B).astype(np.float32)
    bb = rng.uniform(0.0, 6.5, size=B).astype(np.float32)
    return q, a, bb


def run(dll, q, a, bb, L, hist):
    n = q.shape[0]
    q = np.ascontiguousarray(q)
    y = np.full((n, B), np.nan, dtype=np.float32)
    out = np.full((HIST, B), np.nan, dtype=np.float32)
    dll.popens_host(n, B, L, a.ctypes.data, bb.ctypes.data, q.ctypes.data, None if hist is None else hist.ctypes.data,
                    y.ctypes.data, out.ctypes.data)
    return y, out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("L", [15, 7])
def test_a_split_run_has_the_bits_of_one_run(enslib, L):
    q, a, bb = draw(11 + L)
    y_one, h_one = run(enslib, q, a, bb, L, None)
    assert np.isfinite(y_one).all() and np.isfinite(h_one).all()
    # the history after the last day: entry k is the un-routed value of day T - 1 - k
    assert np.array_equal(bits(h_one), bits(q[::-1][:HIST]))
    # NULL is zeros
    y_zero, h_zero = run(enslib, q, a, bb, L, np.zeros((HIST, B), dtype=np.float32))
    assert np.array_equal(bits(y_zero), bits(y_one)) and np.array_equal(bits(h_zero), bits(h_one))
    for name, pieces in SPLITS.items():
        assert sum(pieces) == T
        hist, at, ys = None, 0, []
        for n in pieces:
            y, hist = run(enslib, q[at:at + n], a, bb, L, hist)
            ys.append(y)
            at += n
            k = min(at, HIST)
            assert np.array_equal(bits(hist[:k]), bits(q[:at][::-1][:k])), (name, at)
            assert not hist[k:].any(), (name, at)           # days before the record: zeros
        assert np.array_equal(bits(np.concatenate(ys)), bits(y_one)), f"L = {L}, {name}: other routed bits"
        assert np.array_equal(bits(hist), bits(h_one)), f"L = {L}, {name}: other final history"


@pytest.mark.parametrize("L", [15, 7])
def test_the_one_run_is_the_convolution(enslib, L):
    """float64 over the float32 taps the first day alone reveals (day 0 of a zero history: y = uh[0] q[0], and the taps
    follow from unit impulses): |y - exact| <= gamma(16) sum_k |uh_k q_{t-k}| (tests/test_pop_host.py)."""
    q, a, bb = draw(23 + L)
    imp = np.zeros((UH, B), dtype=np.float32)
    imp[0] = 1.0
    uh, _ = run(enslib, imp, a, bb, L, None)                # the response to a unit impulse: the taps themselves
    assert not uh[L:].any() and np.allclose(uh.astype(np.float64).sum(0), 1.0, atol=1e-5)
    y, _ = run(enslib, q, a, bb, L, None)
    q8, u8 = q.astype(np.float64), uh.astype(np.float64)
    exact, mag = np.zeros((T, B)), np.zeros((T, B))
    for t in range(T):
        for k in range(min(t + 1, UH)):
            exact[t] += u8[k] * q8[t - k]
            mag[t] += np.abs(u8[k] * q8[t - k])
    assert (np.abs(y - exact) <= gamma(16) * mag).all()
    # a history that is not zero enters: the same days after 20 others differ from the same days from nothing
    _, h = run(enslib, q[:20], a, bb, L, None)
    y_cont, _ = run(enslib, q[20:], a, bb, L, h)
    y_cold, _ = run(enslib, q[20:], a, bb, L, None)
    assert np.array_equal(bits(y_cont), bits(y[20:])) and not np.array_equal(bits(y_cont[:L - 1]), bits(y_cold[:L - 1]))
