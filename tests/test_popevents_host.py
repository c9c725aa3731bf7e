"""CPU tier: the event part of hbvx_population_events (hydrodl2_amd/csrc/hbv_pop.h: EventCursor + EventSlot), compiled
for the host (tests/hosttest/popevents_host.cpp walks the scored days of every basin with the statements of k_pop's event
form) and held to a numpy restatement of the cursor rule of include/hbvx_pop_events.h, exactly: a max, a first-argmax
and a sequential float32 sum -- there is nothing to bound.  On well-formed windows, on malformed ones (overlap,
descending, start < 0 mid-list, end >= T_out, E = 1, a basin with no live row), with every slot defined and at most E
cursor steps per basin."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hosttest", "popevents_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libpopevents_host.so")
HDR = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_pop.h")
NAN, INF = float("nan"), float("inf")


def load_eventlib():
    newest = max(os.path.getmtime(f) for f in (SRC, HDR))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    dll = C.CDLL(LIB)
    dll.popevents_host.argtypes = [C.c_int] * 3 + [C.c_void_p] * 7
    dll.popevents_host.restype = C.c_int
    return dll


@pytest.fixture(scope="module")
def eventlib():
    return load_eventlib()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(dll, y, start, end):
    """(peak, day, volume [E,B], steps [B]) of tests/hosttest/popevents_host.cpp on y [T_out,B] float32 and the [E,B]
    int32 windows; the outputs are prefilled with poison."""
    T, B = y.shape
    E = start.shape[0]
    y = np.ascontiguousarray(y, dtype=np.float32)
    start, end = np.ascontiguousarray(start, dtype=np.int32), np.ascontiguousarray(end, dtype=np.int32)
    assert start.shape == end.shape == (E, B)
    peak = np.full((E, B), 12345.0, dtype=np.float32)
    day = np.full((E, B), -2 ** 31, dtype=np.int32)
    volume = np.full((E, B), 12345.0, dtype=np.float32)
    steps = np.full(B, -1, dtype=np.int32)
    rc = dll.popevents_host(T, B, E, y.ctypes.data, start.ctypes.data, end.ctypes.data, peak.ctypes.data, day.ctypes.data,
                            volume.ctypes.data, steps.ctypes.data)
    assert rc == 0
    return peak, day, volume, steps


def restated(y, start, end):
    """The cursor rule of include/hbvx_pop_events.h in numpy: (peak, day, volume, live) [E,B].  Rows in order with
    last = -1; f = min(end, T_out - 1); live iff start > last and f >= start; a live row is the slot's rule on
    y[start .. f] -- the first day at the maximum among the days that are not NaN (the day's own value: a maximum of
    zeros has either sign), the float32 sum in day order from +0 (np.cumsum of float32 adds sequentially) -- and sets
    last = f; any other row holds -inf, -1, +0."""
    T, B = y.shape
    E = start.shape[0]
    peak = np.full((E, B), -np.inf, dtype=np.float32)
    day = np.full((E, B), -1, dtype=np.int32)
    volume = np.zeros((E, B), dtype=np.float32)
    live = np.zeros((E, B), dtype=bool)
    for b in range(B):
        last = -1
        for e in range(E):
            s, f = int(start[e, b]), min(int(end[e, b]), T - 1)
            if not (s > last and f >= s):
                continue
            live[e, b] = True
            last = f
            w = y[s:f + 1, b]
            ranked = np.where(np.isnan(w), np.float32(-np.inf), w)
            if ranked.max() > -np.inf:
                first = int(ranked.argmax())
                peak[e, b], day[e, b] = w[first], s + first
            volume[e, b] = np.cumsum(np.concatenate([np.zeros(1, np.float32), w]), dtype=np.float32)[-1]
    return peak, day, volume, live


def same(got, want):
    peak, day, volume = got[:3]
    assert np.array_equal(bits(peak), bits(want[0]))
    assert np.array_equal(day, want[1])
    assert np.array_equal(bits(volume), bits(want[2]))


def well_formed(rng, T, B, E, width):
    """A basin's windows strictly ascending and disjoint in its first rows, (-1, -1) below; basins differ in their
    count, basin 0 has none where B > 1."""
    start = np.full((E, B), -1, dtype=np.int32)
    end = np.full((E, B), -1, dtype=np.int32)
    for b in range(B):
        n = 0 if (b == 0 and B > 1) else int(rng.integers(1, E + 1))
        t = 0 if b == 1 else int(rng.integers(0, 3))
        for e in range(n):
            f = t + int(rng.integers(0, width))
            if f > T - 1:
                break
            start[e, b], end[e, b] = t, f
            t = f + 1 + int(rng.integers(0, 4))
    return start, end


@pytest.mark.parametrize("T,B,E,width", [(1, 1, 1, 1), (7, 3, 2, 3), (40, 5, 6, 5), (400, 67, 9, 12), (7300, 4, 20, 11)])
def test_well_formed_windows_are_numpys(eventlib, T, B, E, width):
    from hydrodl2_amd.hourly_events import _observed_events
    rng = np.random.default_rng(100 * T + E)
    y = (rng.gamma(2.0, 1.5, size=(T, B)) + 0.01).astype(np.float32)
    start, end = well_formed(rng, T, B, E, width)
    got = run(eventlib, y, start, end)
    want = restated(y, start, end)
    same(got, want)
    assert np.array_equal(want[3], start >= 0)                  # every present row is live
    assert (got[3] == E).all()                                  # every row is offered once
    # the rule the Python layer applies to the observed side is the same rule
    op, od, ov, _ = _observed_events(y, start, end)
    same(got, (op, od, ov))
    absent = start < 0
    assert np.isneginf(got[0][absent]).all() and (got[1][absent] == -1).all()
    assert (got[2][absent] == 0).all() and not np.signbit(got[2][absent]).any()
    if T >= 40:
        assert (start >= 0).sum() > B                           # nothing is vacuous
    # a slot depends on the rows up to its own alone: rows appended behind, and the list cut after any row
    more_s = np.concatenate([start, np.full((2, B), T // 2, np.int32)])
    more_e = np.concatenate([end, np.full((2, B), T - 1, np.int32)])
    if E + 2 <= T:
        p2, d2, v2, _ = run(eventlib, y, more_s, more_e)
        same((p2[:E], d2[:E], v2[:E]), want)
    p1, d1, v1, _ = run(eventlib, y, start[:1], end[:1])
    same((p1, d1, v1), tuple(a[:1] for a in want[:3]))


def test_malformed_windows_follow_the_cursor_rule(eventlib):
    T = 30
    rng = np.random.default_rng(7)
    y = (rng.gamma(2.0, 1.5, size=(T, 8)) + 0.01).astype(np.float32)
    cols = {
        # overlap: the second row starts inside the first -> absent; the third is ahead again -> live
        "overlap": [(2, 6), (5, 9), (7, 8), (12, 12)],
        # descending: only rows ahead of the last live one
        "descending": [(20, 22), (10, 12), (3, 4), (23, 25)],
        # start < 0 mid-list, then a live row behind it
        "negative-mid": [(0, 1), (-1, -1), (-5, 3), (4, 4)],
        # end beyond the record: clamped to T - 1; a row after it can never be ahead
        "end-clamped": [(25, 99), (29, 29), (28, 40), (-1, -1)],
        # end < start, start beyond the record, start == last (not ahead)
        "empty": [(5, 4), (30, 35), (3, 7), (7, 9)],
        # no live row at all
        "none": [(-1, -1), (-1, 5), (9, 2), (-2 ** 31, 2 ** 31 - 1)],
        # extreme values: nothing overflows, nothing is touched
        "extreme": [(2 ** 31 - 1, 2 ** 31 - 1), (0, 2 ** 31 - 1), (1, 1), (-2 ** 31, -2 ** 31)],
        # adjacent windows: a row that starts on the day after the last live one is live
        "adjacent": [(0, 0), (1, 1), (2, 5), (6, 29)],
    }
    start = np.array([[w[e][0] for w in cols.values()] for e in range(4)], dtype=np.int64).astype(np.int32)
    end = np.array([[w[e][1] for w in cols.values()] for e in range(4)], dtype=np.int64).astype(np.int32)
    got = run(eventlib, y, start, end)
    want = restated(y, start, end)
    same(got, want)
    live = {name: want[3][:, i].tolist() for i, name in enumerate(cols)}
    assert live == {"overlap": [True, False, True, True], "descending": [True, False, False, True],
                    "negative-mid": [True, False, False, True], "end-clamped": [True, False, False, False],
                    "empty": [False, False, True, False], "none": [False] * 4,
                    "extreme": [False, True, False, False], "adjacent": [True] * 4}
    # every slot is defined: no poison is left, absent rows hold -inf, -1, +0
    assert not (got[0] == 12345.0).any() and not (got[2] == 12345.0).any() and (got[1] > -2 ** 31).all()
    absent = ~want[3]
    assert np.isneginf(got[0][absent]).all() and (got[1][absent] == -1).all()
    assert (got[2][absent] == 0).all() and not np.signbit(got[2][absent]).any()
    assert (got[3] == 4).all()                                  # E cursor steps per basin, whatever the rows hold
    # E = 1, live and absent
    p, d, v, steps = run(eventlib, y[:, :2], np.array([[3, -1]], np.int32), np.array([[3, -1]], np.int32))
    assert p[0, 0] == y[3, 0] and d[0].tolist() == [3, -1] and v[0, 0] == y[3, 0]
    assert np.isneginf(p[0, 1]) and v[0, 1] == 0 and steps.tolist() == [1, 1]


def test_slot_edge_cases(eventlib):
    y = np.array([[1.0], [3.0], [3.0], [NAN], [0.0], [-0.0], [NAN], [NAN], [-INF], [INF]], dtype=np.float32)
    start = np.array([[0], [3], [4], [6], [8], [9]], dtype=np.int32)
    end = np.array([[2], [3], [5], [7], [8], [20]], dtype=np.int32)
    peak, day, volume, _ = run(eventlib, y, start, end)
    same((peak, day, volume), restated(y, start, end))
    #   a plateau keeps its first day; a NaN day is above nothing and poisons the volume; +0 before -0 keeps day 4;
    #   -inf is not above -inf: day -1 with a volume of -inf; the last window is clamped to the record
    assert peak[:, 0].tolist()[:1] == [3.0] and day[:, 0].tolist() == [1, -1, 4, -1, -1, 9]
    assert np.isnan(volume[1, 0]) and np.isneginf(peak[1, 0])
    assert peak[2, 0] == 0 and not np.signbit(peak[2, 0]) and volume[2, 0] == 0 and not np.signbit(volume[2, 0])
    assert np.isnan(volume[3, 0]) and np.isneginf(volume[4, 0]) and np.isposinf(peak[5, 0])


def test_sizes_are_checked(eventlib):
    y = np.ones((3, 1), dtype=np.float32)
    w = np.zeros((1, 1), dtype=np.int32)
    out = np.zeros(4, dtype=np.float32)
    for T, B, E in ((0, 1, 1), (3, 0, 1), (3, 1, 0)):
        assert eventlib.popevents_host(T, B, E, y.ctypes.data, w.ctypes.data, w.ctypes.data, out.ctypes.data,
                                       out.ctypes.data, out.ctypes.data, None) == -1
