"""CPU tier: the composition of the one-pass static adjoint's chunk maps (hbvx::onepass_compose,
hydrodl2_amd/csrc/hbv_onepass_compose.h), which k_bwd_chunk_onepass runs to fold the chunks of a workgroup into one map,
compiled for the host in its double instantiation.  Random maps with the kernel's sparsity (units 0 and 1 stay in the
snow block, unit 2 reaches snow and soil; a parameter p is reached by the units k >= kmin(p)), for 12 and 13 parameters,
chains of 1 to 7 chunks and a random incoming adjoint:

  route A hops chunk by chunk, last chunk first, and sums G_c a_c + g0_c per chunk;
  route B composes the chain into one map and applies it once.

Both give the gradient and the adjoint leaving the chain, and must agree to 1e-12 of the largest element: pure double
arithmetic reassociated over at most 7 x 5 terms.  The composite must also equal the dense matrix composition numpy
forms without any knowledge of the patterns, and its entries outside the patterns must be exactly zero."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc")
SRC = os.path.join(HERE, "hosttest", "onepass_compose_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libhbvx_onepass_compose.so")
# BETA FC K0 K1 K2 LP PERC UZL TT CFMAX CFR CWH BETAET: the first unit adjoint that reaches the parameter
KMIN = [2, 2, 3, 3, 3, 2, 3, 3, 0, 0, 0, 0, 2]
REACH = [2, 2, 3, 5, 5]            # unit k propagates into the storages i < REACH[k]
TOL = 1e-12


@pytest.fixture(scope="module")
def lib():
    deps = [SRC, os.path.join(CSRC, "hbv_onepass_compose.h"), os.path.join(CSRC, "hbv_step.h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
    d = C.CDLL(LIB)
    d.onepass_chain.restype = C.c_int
    return d


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_the_patterns_are_the_kernels(lib):
    assert [lib.onepass_pattern_kmin(p) for p in range(13)] == KMIN
    assert [lib.onepass_pattern_reach(k) for k in range(5)] == REACH


def _draw(rng, n, npar, nmax):
    Phi = rng.standard_normal((n, 5, 5))
    phi = rng.standard_normal((n, 5))
    G = rng.standard_normal((n, 6, nmax))
    for k in range(5):
        Phi[:, k, REACH[k]:] = 0.0
    G[:, :, npar:] = 0.0
    for p in range(npar):
        G[:, :KMIN[p], p] = 0.0        # (row 5, g0, is never masked: KMIN <= 3)
    return Phi, phi, G


def _dense_composite(Phi, phi, G):
    """The chain as one map by dense matrix products, last chunk first; no use of the patterns."""
    n = Phi.shape[0]
    cP, cp, cG, cg = Phi[n - 1].copy(), phi[n - 1].copy(), G[n - 1, :5].copy(), G[n - 1, 5].copy()
    for c in range(n - 2, -1, -1):
        cg = cg + G[c, 5] + cp @ G[c, :5]
        cG = cG + cP @ G[c, :5]
        cp = phi[c] + cp @ Phi[c]
        cP = cP @ Phi[c]
    return cP, cp, cG, cg


@pytest.mark.parametrize("npar", [12, 13])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7])
def test_composed_chain_equals_the_hops(lib, npar, n):
    nmax = lib.onepass_chain(0, 0, *([None] * 11))    # an unknown parameter count: -1
    assert nmax == -1
    worst = 0.0
    for draw in range(50):
        rng = np.random.default_rng(9000 + 100 * npar + 10 * n + 1000 * draw)
        a_in = rng.standard_normal(5)
        nmax = 19
        Phi, phi, G = _draw(rng, n, npar, nmax)
        out = [np.full(s, np.nan) for s in (nmax, 5, nmax, 5, 25, 5, 6 * nmax)]
        assert lib.onepass_chain(npar, n, _ptr(Phi), _ptr(phi), _ptr(G), _ptr(a_in), *map(_ptr, out)) == nmax
        g_hop, a_hop, g_one, a_one, cPhi, cphi, cG = out
        cPhi, cG = cPhi.reshape(5, 5), cG.reshape(6, nmax)
        assert all(np.isfinite(o).all() for o in out)
        for name, x, y in (("gradient", g_hop[:npar], g_one[:npar]), ("adjoint", a_hop, a_one)):
            err = np.abs(x - y).max() / max(np.abs(x).max(), np.abs(y).max())
            worst = max(worst, err)
            assert err <= TOL, (draw, name, err)
        # the composite itself, against the dense composition, and its zeros
        dP, dp, dG, dg = _dense_composite(Phi, phi, G)
        for name, x, y in (("Phi", cPhi, dP), ("phi", cphi, dp), ("G", cG[:5], dG), ("g0", cG[5], dg)):
            assert np.abs(x - y).max() <= TOL * max(np.abs(y).max(), 1e-300), (draw, name)
        for k in range(5):
            assert not cPhi[k, REACH[k]:].any() and not dP[k, REACH[k]:].any(), (draw, k)
        assert not cG[:, npar:].any()
        for p in range(npar):
            assert not cG[:KMIN[p], p].any() and not dG[:KMIN[p], p].any(), (draw, p)
    print(f"NP {npar}, {n} chunks: worst difference of the two routes {worst:.2e} of the largest element")
