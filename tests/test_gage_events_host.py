"""CPU tier: the per-slot arithmetic of hbvx_gage_population_events (hydrodl2_amd/csrc/hbv_pop.h: EventSlot), compiled
for the host (tests/hosttest/gageevents_host.cpp feeds one EventSlot per (event, gage) hour by hour, as a lane of the
kernel does) and held to numpy exactly: the peak is a maximum, the hour its first argmax, the volume a sequential float32
sum over ascending hours, bit for bit -- there is nothing to bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hosttest", "gageevents_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libgageevents_host.so")
HDR = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_pop.h")
NAN, INF = float("nan"), float("inf")


def load_eventlib():
    newest = max(os.path.getmtime(f) for f in (SRC, HDR))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    dll = C.CDLL(LIB)
    dll.gageevents_host.argtypes = [C.c_int] * 3 + [C.c_void_p] * 6
    dll.gageevents_host.restype = C.c_int
    return dll


@pytest.fixture(scope="module")
def eventlib():
    return load_eventlib()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(dll, series, start, end):
    """(peak [E,G] float32, hour [E,G] int32, volume [E,G] float32) of tests/hosttest/gageevents_host.cpp: series [T,G]
    float32, start / end [E,G] int32."""
    T, G = series.shape
    E = start.shape[0]
    series = np.ascontiguousarray(series, dtype=np.float32)
    start, end = (np.ascontiguousarray(a, dtype=np.int32) for a in (start, end))
    assert start.shape == (E, G) and end.shape == (E, G)
    peak = np.full((E, G), np.nan, dtype=np.float32)
    hour = np.full((E, G), -7, dtype=np.int32)
    volume = np.full((E, G), np.nan, dtype=np.float32)
    rc = dll.gageevents_host(T, G, E, series.ctypes.data, start.ctypes.data, end.ctypes.data, peak.ctypes.data,
                             hour.ctypes.data, volume.ctypes.data)
    assert rc == 0
    return peak, hour, volume


def restated(series, start, end):
    """The same in numpy, window by window: the maximum of the hours that are not NaN and the first hour that equals it
    (-inf and -1 where there is none above -inf), and the float32 sum in hour order from +0 (np.cumsum of a float32
    array adds sequentially, one rounding per element; the leading +0 is the slot's start)."""
    T, G = series.shape
    E = start.shape[0]
    peak = np.full((E, G), -np.inf, dtype=np.float32)
    hour = np.full((E, G), -1, dtype=np.int32)
    volume = np.zeros((E, G), dtype=np.float32)
    for e in range(E):
        for g in range(G):
            s, f = int(start[e, g]), min(int(end[e, g]), T - 1)
            if s < 0 or f < s:
                continue
            w = series[s:f + 1, g]
            seen = w[~np.isnan(w)]
            if seen.size and seen.max() > -np.inf:
                first = int(np.flatnonzero(w == seen.max())[0])
                peak[e, g] = w[first]               # (the hour's own value: np.max does not say which zero it returns)
                hour[e, g] = s + first
            volume[e, g] = np.cumsum(np.concatenate([np.zeros(1, np.float32), w]), dtype=np.float32)[-1]
    return peak, hour, volume


@pytest.mark.parametrize("T,G,E", [(1, 1, 1), (9, 3, 2), (400, 5, 6), (2160, 4, 10)])
def test_peaks_hours_and_volumes_are_numpys(eventlib, T, G, E):
    rng = np.random.default_rng(10 * T + E)
    series = (rng.gamma(2.0, 1.5, size=(T, G)) + 0.01).astype(np.float32)
    series = np.round(series * 4) / np.float32(4)                      # quarter steps: the maximum of a window is often tied
    length = max(1, T // (2 * E))
    start = np.stack([np.sort(rng.choice(np.arange(0, T, length), size=E, replace=False)) for _ in range(G)], 1).astype(np.int32)
    end = (start + rng.integers(0, length, size=(E, G))).astype(np.int32)
    start[0, 0], end[-1, -1] = 0, T - 1                                 # a window at hour 0 and one ending at T - 1
    if E > 1:
        end[0, 0] = start[0, 0]                                         # a one-hour window
    if E > 2:
        start[E - 1, 0] = end[E - 1, 0] = -1                            # an absent slot
    peak, hour, volume = run(eventlib, series, start, end)
    want = restated(series, start, end)
    assert np.array_equal(bits(peak), bits(want[0])) and np.array_equal(hour, want[1])
    assert np.array_equal(bits(volume), bits(want[2]))
    present = start >= 0
    assert (hour[present] >= start[present]).all() and (hour[present] <= np.minimum(end, T - 1)[present]).all()
    assert np.array_equal(series[hour[present], np.nonzero(present)[1]], peak[present])
    if T >= 400:
        ties = sum(int((series[start[e, g]:end[e, g] + 1, g] == peak[e, g]).sum() > 1) for e, g in zip(*np.nonzero(present)))
        assert ties > 0, "no window has a tied maximum: the first-argmax rule is not exercised"
    # a slot depends on its own window alone: any subset of the events, any order
    order = rng.permutation(E)
    p2, h2, v2 = run(eventlib, series, start[order], end[order])
    assert np.array_equal(bits(p2), bits(peak[order])) and np.array_equal(h2, hour[order])
    assert np.array_equal(bits(v2), bits(volume[order]))
    p1, h1, v1 = run(eventlib, series, start[E - 1:], end[E - 1:])
    assert np.array_equal(bits(p1[0]), bits(peak[E - 1])) and np.array_equal(h1[0], hour[E - 1])
    assert np.array_equal(bits(v1[0]), bits(volume[E - 1]))


def test_edge_cases(eventlib):
    #                 0    1    2    3    4    5     6     7    8    9    10   11
    y = np.array([[1.0, 3.0, 3.0, 2.0, NAN, 0.0, -0.0, -0.0, 0.0, NAN, NAN, 5.0]], dtype=np.float32).T
    T = y.shape[0]
    windows = [(0, 3),      # a plateau at hours 1 and 2: the FIRST hour
               (3, 3),      # a one-hour window
               (0, 0),      # a window at hour 0
               (11, 11),    # ... and one ending at T - 1
               (3, 5),      # a NaN inside: the peak and its hour ignore it, the volume does not
               (9, 10),     # NaNs alone: -inf, -1
               (5, 8),      # +0, -0, -0, +0: -0 is not above +0 and +0 not above -0, the first hour stays
               (6, 8),      # -0, -0, +0: the first -0 stays
               (-1, -1),    # an absent slot
               (-3, 5),     # start < 0 with an end: absent all the same
               (7, 4),      # end < start: absent
               (10, 99),    # end clamped to T - 1
               (12, 20)]    # a start past the record: nothing to read, absent
    start = np.array([[w[0]] for w in windows], dtype=np.int32)
    end = np.array([[w[1]] for w in windows], dtype=np.int32)
    peak, hour, volume = run(eventlib, y, start, end)
    assert hour[:, 0].tolist() == [1, 3, 0, 11, 3, -1, 5, 6, -1, -1, -1, 11, -1]
    assert peak[:5, 0].tolist() == [3.0, 2.0, 1.0, 5.0, 2.0] and peak[11, 0] == 5.0
    assert np.isneginf(peak[[5, 8, 9, 10, 12], 0]).all()
    assert peak[6, 0] == 0.0 and not np.signbit(peak[6, 0])              # the +0 of hour 5
    assert peak[7, 0] == 0.0 and np.signbit(peak[7, 0])                  # the -0 of hour 6
    assert volume[:4, 0].tolist() == [9.0, 2.0, 1.0, 5.0]
    assert np.isnan(volume[[4, 5, 11], 0]).all()
    for k in (6, 7, 8, 9, 10, 12):                                       # +0 + -0 = +0; the absent slots hold +0
        assert volume[k, 0] == 0.0 and not np.signbit(volume[k, 0]), k
    want = restated(y, start, end)
    assert np.array_equal(bits(peak), bits(want[0])) and np.array_equal(hour, want[1])
    assert np.array_equal(bits(volume)[~np.isnan(volume)], bits(want[2])[~np.isnan(want[2])])
    assert np.array_equal(np.isnan(volume), np.isnan(want[2]))
    # an infinite flow is a peak like any other; -inf is above nothing, not even the start
    z = np.array([[-INF, -INF, 1.0, INF, INF]], dtype=np.float32).T
    peak, hour, volume = run(eventlib, z, np.array([[0], [0], [2]], np.int32), np.array([[1], [2], [4]], np.int32))
    assert hour[:, 0].tolist() == [-1, 2, 3] and np.isneginf(peak[0, 0]) and peak[1, 0] == 1.0 and np.isposinf(peak[2, 0])
    assert np.isneginf(volume[0, 0]) and np.isposinf(volume[2, 0])
    assert T == 12


def test_the_shapes_are_bounded(eventlib):
    y = np.ones((3, 1), dtype=np.float32)
    out = np.zeros(8, dtype=np.int32)
    for T, G, E in ((0, 1, 1), (3, 0, 1), (3, 1, 0)):
        assert eventlib.gageevents_host(T, G, E, y.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data,
                                        out.ctypes.data, out.ctypes.data) == -1
