"""CPU tier: the per-lane arithmetic, the packed-factor indexing and the tiling of hbvx_quadform
(hydrodl2_amd/csrc/hbv_quadform.h), compiled for the host (tests/hosttest/quadform_host.cpp: the two passes of
quadform.hip with the lanes as loops, over a NaN-filled workspace).

Definition, per (t, b), in float32:
    y_e = chain over ascending c = 0..e:   acc = fmaf(m[b,e,c], s[c,t,b], acc)
    q   = chain over ascending e = 0..C-1: q = fmaf(y_e, y_e, q)

Bound against float64 on the same float32 inputs (gamma_n = n u / (1 - n u), u = 2^-24; Higham, Accuracy and Stability
of Numerical Algorithms, ch. 3):
  * y_e is a chain of at most C fused multiply-adds, one rounding each, so |fl(y_e) - y_e| <= gamma_C m_e with
    m_e = sum_{c<=e} |m_ec s_c|, and |fl(y_e)| <= (1 + gamma_C) m_e;
  * hence |fl(y_e)^2 - y_e^2| <= (2 gamma_C + gamma_C^2) m_e^2;
  * the chain over e is C more fused multiply-adds on non-negative terms: a relative gamma_C on every term, and
    (1 + gamma_C)(1 + 2 gamma_C + gamma_C^2) - 1 = 3 gamma_C + 3 gamma_C^2 + gamma_C^3 <= gamma_{3C+4}
    (gamma_j + gamma_k + gamma_j gamma_k <= gamma_{j+k}; the four spare units cover the cross terms).
So |q - q64| <= gamma_n * sum_e m_e^2 with n = 3C + 4, the sums of magnitudes taken in float64.  An indexing mistake (a
wrong column, row, day or basin; an element of the packed factor misplaced) misses it by orders of magnitude.

Also: bit-equality with a direct scalar evaluation of the two chains, q >= 0, a NaN upper triangle changes nothing,
and q of a day slice or a basin subset has the bits of the full call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hosttest", "quadform_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libquadform_host.so")
HDR = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_quadform.h")

# (33, 130, 70): C above one workgroup's span of factor rows; (12, 5, 194): the column count of the flagship Jacobian
SHAPES = [(1, 1, 1), (5, 3, 7), (9, 65, 9), (257, 67, 17), (33, 130, 70), (12, 5, 194)]
IDS = [f"{t}x{b}x{c}" for t, b, c in SHAPES]
U = 2.0 ** -24


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


@pytest.fixture(scope="module")
def qflib():
    newest = max(os.path.getmtime(f) for f in (SRC, HDR))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    dll = C.CDLL(LIB)
    for fn in (dll.quadform_host, dll.quadform_direct):
        fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong] + [C.c_void_p] * 3
        fn.restype = None
    return dll


def draw(T, B, Cn, seed, pad=0, nan_upper=False):
    """series [C, T*B + pad] (series_stride = T*B + pad) with columns of different scale, as a Jacobian's; a
    lower-triangular factor [B,C,C] whose upper triangle is zero or NaN; float32."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((Cn, T * B + pad)).astype(np.float32)
    s *= (10.0 ** rng.uniform(-2, 2, size=(Cn, 1))).astype(np.float32)
    m = np.tril(rng.standard_normal((B, Cn, Cn))).astype(np.float32)
    m *= (10.0 ** rng.uniform(-1, 1, size=(B, 1, Cn))).astype(np.float32)
    if nan_upper:
        m[:, np.triu_indices(Cn, 1)[0], np.triu_indices(Cn, 1)[1]] = np.nan
    return s, m


def run(fn, T, B, Cn, s, m):
    q = np.full((T, B), np.nan, dtype=np.float32)
    assert s.flags["C_CONTIGUOUS"] and m.flags["C_CONTIGUOUS"] and s.dtype == m.dtype == np.float32
    fn(T, B, Cn, s.shape[1], s.ctypes.data, m.ctypes.data, q.ctypes.data)
    return q


def reference(T, B, Cn, s, m):
    """float64 value and the float64 sum of magnitudes that scales the bound."""
    s8 = s[:, :T * B].reshape(Cn, T, B).astype(np.float64)
    m8 = np.tril(np.nan_to_num(m.astype(np.float64), nan=0.0))
    y = np.einsum("bec,ctb->etb", m8, s8)
    mag = np.einsum("bec,ctb->etb", np.abs(m8), np.abs(s8))
    return (y * y).sum(0), (mag * mag).sum(0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("T,B,Cn", SHAPES, ids=IDS)
def test_against_float64_and_the_direct_chains(qflib, T, B, Cn):
    s, m = draw(T, B, Cn, seed=T + 7 * B + 13 * Cn, pad=5 if Cn % 2 else 0)
    q = run(qflib.quadform_host, T, B, Cn, s, m)
    assert np.isfinite(q).all() and (q >= 0).all()
    want, mag = reference(T, B, Cn, s, m)
    err = np.abs(q.astype(np.float64) - want)
    bound = gamma(3 * Cn + 4) * mag
    need = (err / np.where(bound > 0, bound, 1.0)).max()
    print(f"worst error / bound {need:.3f}")
    assert (err <= bound).all(), f"error {err.max():.3e} exceeds the bound by {need:.2f}x"
    direct = run(qflib.quadform_direct, T, B, Cn, s, m)
    assert np.array_equal(bits(q), bits(direct)), "the tiled passes do not give the bits of the definition"


@pytest.mark.parametrize("T,B,Cn", SHAPES, ids=IDS)
def test_the_upper_triangle_is_not_read(qflib, T, B, Cn):
    s, m = draw(T, B, Cn, seed=5)
    s2, m2 = draw(T, B, Cn, seed=5, nan_upper=True)
    assert Cn == 1 or np.isnan(m2).any()
    q, q2 = run(qflib.quadform_host, T, B, Cn, s, m), run(qflib.quadform_host, T, B, Cn, s2, m2)
    assert np.isfinite(q2).all() and np.array_equal(bits(q), bits(q2))


@pytest.mark.parametrize("T,B,Cn", [(257, 67, 17), (33, 130, 70), (12, 5, 194)])
def test_bits_of_a_day_and_a_basin_depend_on_nothing_else(qflib, T, B, Cn):
    s, m = draw(T, B, Cn, seed=99)
    q = run(qflib.quadform_host, T, B, Cn, s, m)
    s3 = s.reshape(Cn, T, B)
    # a day slice that starts and ends inside a wave's group of days
    t0, t1 = 3, min(T, 20)
    part = np.ascontiguousarray(s3[:, t0:t1]).reshape(Cn, -1)
    assert np.array_equal(bits(run(qflib.quadform_host, t1 - t0, B, Cn, part, m)), bits(q[t0:t1]))
    # a basin subset with its factors: other lanes, another group of 64, another width of the packed rows
    sel = [b for b in (0, 2, 4, 63, 64, 66, B - 1) if b < B]
    sel = sorted(set(sel))
    part = np.ascontiguousarray(s3[:, :, sel]).reshape(Cn, -1)
    got = run(qflib.quadform_host, T, len(sel), Cn, part, np.ascontiguousarray(m[sel]))
    assert np.array_equal(bits(got), bits(q[:, sel]))
