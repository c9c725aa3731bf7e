"""CPU tier: the per-threshold arithmetic of hbvx_population_fdc (hydrodl2_amd/csrc/hbv_pop.h: FdcSlot), compiled for
the host (tests/hosttest/popfdc_host.cpp feeds one FdcSlot per (threshold, basin) day by day, as a lane of the kernel
does) and held to numpy exactly: the counts are integer counts, the volumes a sequential float32 sum over ascending
days, bit for bit -- there is nothing to bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hosttest", "popfdc_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libpopfdc_host.so")
HDR = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_pop.h")
NAN, INF = float("nan"), float("inf")


def load_fdclib():
    newest = max(os.path.getmtime(f) for f in (SRC, HDR))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    dll = C.CDLL(LIB)
    dll.popfdc_host.argtypes = [C.c_int] * 3 + [C.c_void_p] * 5
    dll.popfdc_host.restype = C.c_int
    return dll


@pytest.fixture(scope="module")
def fdclib():
    return load_fdclib()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(dll, y, enter, thr):
    """(count [K,B] int32, volume [K,B] float32) of tests/hosttest/popfdc_host.cpp: y [T,B] float32, enter [T,B] bool or
    None, thr [K,B] float32."""
    T, B = y.shape
    K = thr.shape[0]
    y, thr = np.ascontiguousarray(y, dtype=np.float32), np.ascontiguousarray(thr, dtype=np.float32)
    en = None if enter is None else np.ascontiguousarray(enter, dtype=np.uint8)
    assert thr.shape == (K, B) and (en is None or en.shape == (T, B))
    count = np.full((K, B), -1, dtype=np.int32)
    volume = np.full((K, B), np.nan, dtype=np.float32)
    rc = dll.popfdc_host(T, B, K, y.ctypes.data, None if en is None else en.ctypes.data, thr.ctypes.data,
                         count.ctypes.data, volume.ctypes.data)
    assert rc == 0
    return count, volume


def restated(y, enter, thr):
    """The same in numpy: integer counts, and the float32 sum of the flows above the threshold in day order (np.cumsum
    of a float32 array adds sequentially, one rounding per element; the zeros of the other days change nothing but the
    sign of a zero sum, which the first term fixes: the slot starts from +0)."""
    T, B = y.shape
    en = np.ones((T, B), dtype=bool) if enter is None else enter.astype(bool)
    with np.errstate(invalid="ignore"):
        above = (y[None] > thr[:, None]) & en[None]                                    # [K,T,B]
    count = above.sum(1).astype(np.int32)
    terms = np.where(above, y[None], np.float32(0.0)).astype(np.float32)
    volume = np.cumsum(np.concatenate([np.zeros((thr.shape[0], 1, B), np.float32), terms], 1), axis=1, dtype=np.float32)[:, -1]
    return count, volume


@pytest.mark.parametrize("T,B,K", [(1, 1, 1), (7, 3, 2), (400, 5, 15), (7300, 4, 32)])
def test_counts_and_volumes_are_numpys(fdclib, T, B, K):
    rng = np.random.default_rng(100 * T + K)
    y = (rng.gamma(2.0, 1.5, size=(T, B)) + 0.01).astype(np.float32)
    thr = np.quantile(y, rng.uniform(0.02, 0.98, size=K), axis=0).astype(np.float32)
    thr[0] = y[rng.integers(T)]                                     # a threshold that IS a day's flow: not above itself
    enter = rng.uniform(size=(T, B)) > 0.2
    for en in (None, enter):
        count, volume = run(fdclib, y, en, thr)
        want_n, want_v = restated(y, en, thr)
        assert np.array_equal(count, want_n), (T, B, K)
        assert np.array_equal(bits(volume), bits(want_v)), (T, B, K)
        assert count.min() >= 0 and not np.isnan(volume).any()
    if T >= 400:
        assert 0 < count.min() and count.max() < T                  # the thresholds cut the record: nothing is vacuous
    # a slot depends on its own threshold alone: any subset, any order
    order = rng.permutation(K)
    c2, v2 = run(fdclib, y, enter, thr[order])
    assert np.array_equal(c2, count[order]) and np.array_equal(bits(v2), bits(volume[order]))
    c1, v1 = run(fdclib, y, enter, thr[K - 1:])
    assert np.array_equal(c1[0], count[K - 1]) and np.array_equal(bits(v1[0]), bits(volume[K - 1]))


def test_edge_cases(fdclib):
    y = np.array([[1.0], [2.0], [2.0], [3.0], [NAN], [0.0], [-0.0], [INF]], dtype=np.float32)
    T = y.shape[0]
    thr = np.array([[2.0], [0.0], [-0.0], [-1.0], [1e30], [INF], [3.0]], dtype=np.float32)
    count, volume = run(fdclib, y, None, thr)
    #   thr 2:    3 and inf are above; a day AT the threshold is not
    #   thr +-0:  1, 2, 2, 3, inf; neither zero is above either zero
    #   thr -1:   everything but the NaN day
    #   thr 1e30: inf alone;  thr inf: nothing, not even inf;  thr 3: inf alone
    assert count[:, 0].tolist() == [2, 5, 5, 7, 1, 0, 1]
    assert volume[5, 0] == 0.0 and not np.signbit(volume[5, 0])
    assert np.isinf(volume[[0, 1, 2, 3, 4, 6], 0]).all()
    # without the infinite day: plain sums, and a NaN flow is above nothing (it reaches no volume)
    count, volume = run(fdclib, y[:-1], None, thr)
    assert count[:, 0].tolist() == [1, 4, 4, 6, 0, 0, 0]
    assert volume[:, 0].tolist() == [3.0, 8.0, 8.0, 8.0, 0.0, 0.0, 0.0]
    # never above / always above, and days that do not enter
    flat = np.full((50, 2), 1.5, dtype=np.float32)
    count, volume = run(fdclib, flat, None, np.array([[1.5, 1.0]], dtype=np.float32))
    assert count.tolist() == [[0, 50]] and volume.tolist() == [[0.0, 75.0]]
    enter = np.zeros((50, 2), dtype=bool)
    enter[::5] = True
    count, volume = run(fdclib, flat, enter, np.array([[1.0, 1.0]], dtype=np.float32))
    assert count.tolist() == [[10, 10]] and volume.tolist() == [[15.0, 15.0]]
    count, _ = run(fdclib, flat, np.zeros((50, 2), dtype=bool), np.array([[1.0, 1.0]], dtype=np.float32))
    assert count.tolist() == [[0, 0]]
    assert T == 8


def test_the_slot_count_is_bounded(fdclib):
    y = np.ones((3, 1), dtype=np.float32)
    for K in (0, 33):
        out = np.zeros(64, dtype=np.float32)
        assert fdclib.popfdc_host(3, 1, K, y.ctypes.data, None, out.ctypes.data, out.ctypes.data, out.ctypes.data) == -1
