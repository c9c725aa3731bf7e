"""What the ensemble Kalman tests share: the host build of hydrodl2_amd/csrc/hbv_enkf.h (tests/hosttest/enkf_host.cpp), a
float64 numpy restatement of the update written from the formulas of include/hbvx_enkf.h, the error bound both are held to,
and the input sets.

THE BOUND.  The kernel body and the restatement evaluate the same real-number formulas in float64 from the same float32
inputs (exact in float64); they differ in the order of the sums.  With u = 2^-53 and first-order error analysis (a sum of P
terms carries at most P u times the sum of the magnitudes; each further +, -, *, /, sqrt one more u of its result), writing
D(q) for the error of a computed q against the exact value:

    Yabs = mean|y_p|, Xabs = mean|x_p|, Eabs = mean|e_p|, dy_p = y_p - ybar
    D(ybar)  <= P u Yabs
    D(dy_p)  <= D(ybar) + u |dy_p|
    D(c)     <= [ sum_p |x_p| D(dy_p) + (P + 2) u sum_p |x_p| |dy_p| ] / (P - 1)
    D(v)     <= [ 2 sum_p |dy_p| D(dy_p) + (P + 2) u sum_p dy_p^2 ] / (P - 1);        D(s) <= D(v) + u s
    D(K)     <= D(c) / s + |c| D(s) / s^2 + u |K|
    D(xbar)  <= P u Xabs;   D(ebar) <= P u Eabs
    D(d)     <= D(ybar) + D(ebar) + 2 u (|o| + |ebar| + |d|)                            (ebar = 0 for method 1)
    D(m)     <= D(xbar) + D(K) |d| + |K| D(d) + u |K d| + u |m|
  method 0:  i_p = (o + e_p) - y_p,  D(i_p) <= 2 u (|o| + |e_p| + |i_p|)
    D(xa_p)  <= D(K) |i_p| + |K| D(i_p) + u |K i_p| + u |xa_p|
  method 1:  D(alpha) <= D(s) / (2 s) + 4 u      (alpha = 1 / (1 + sqrt(R / s)) lies in (1/2, 1), d alpha / alpha <= d s / 2 s)
    D(aK)    <= D(alpha) |K| + D(K) + u |K|
    t_p = (x_p - xbar) - aK dy_p,  D(t_p) <= D(xbar) + u |x_p - xbar| + D(aK) |dy_p| + |aK| D(dy_p) + u |aK dy_p| + u |t_p|
    D(xa_p)  <= D(m) + D(t_p) + u |xa_p|
  inflation: D(xa'_p) <= D(m) + rho (D(xa_p) + D(m)) + 2 u rho |xa_p - m| + u |xa'_p|
  the floor is monotone with slope <= 1 and adds nothing.

Every term has the shape  P u |x| |y - ybar| |innovation| / s  or is smaller.  The kernel and the restatement each lie within
D of the exact value, so they lie within 2 D of each other; second-order terms are below 1e-13 of D at P <= 200.  The
kernel then rounds ONCE to float32: |float32(q) - q| <= 2^-24 |q| + 2^-150.  So
    |kernel - restatement| <= 2 D + 2^-24 (|xa| + 2 D) + 2^-150,
`bound` below, nothing in it fitted to what the code gives."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hosttest", "enkf_host.cpp")
LIB = os.path.join(HERE, "hosttest", "libenkf_host.so")
HDR = os.path.join(os.path.dirname(HERE), "hydrodl2_amd", "csrc", "hbv_enkf.h")
U = 2.0 ** -53

_dll = None


def host_library():
    """tests/hosttest/libenkf_host.so, rebuilt when its source or the header is newer."""
    global _dll
    if _dll is None:
        newest = max(os.path.getmtime(f) for f in (SRC, HDR))
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", LIB, SRC])
        _dll = C.CDLL(LIB)
        _dll.enkf_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int64] + [C.c_void_p] * 8 + \
            [C.c_int64, C.c_int, C.c_float, C.c_int, C.c_int]
        _dll.enkf_host.restype = None
    return _dll


def _p(a):
    return None if a is None else a.ctypes.data


def host_update(y, obs, obs_var, arrays, method, rho=1.0, eps=None, active=None, form=0, inplace=False):
    """The host build on numpy arrays: y [P,B] float32 (C-contiguous), arrays a list of (x [P,...] float32, M, lo).
    Returns (outs, status [B] int32, stats [3,B] float64); the first array leads, as in the library."""
    dll = host_library()
    P, B = y.shape
    status = np.full(B, -7, dtype=np.int32)
    stats = np.full((3, B), 123.0)
    act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
    outs = []
    for i, (x, M, lo) in enumerate(arrays):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = x if inplace else np.full_like(x, np.nan)
        dll.enkf_host(P, B, method, float(rho), _p(y), y.strides[0] // 4, _p(obs), _p(obs_var), _p(act), _p(eps),
                      _p(status), _p(stats), _p(x), _p(out), x.size // P, M, float(lo), int(i == 0), form)
        outs.append(out)
    return outs, status, stats


def basin_of(shape, B, M):
    """[n] the basin of every element of an array of `shape` [P,...] whose elements per particle run [..., B, M]."""
    n = int(np.prod(shape[1:]))
    return (np.arange(n) // M) % B


def restate(y, obs, obs_var, x, M, lo, method, rho=1.0, eps=None, active=None):
    """The update of ONE array in float64 numpy, from the formulas of include/hbvx_enkf.h: (xa [P,...] float64 -- NOT
    rounded to float32; skipped basins and copied elements hold x --, status [B], stats [3,B], bound [P,...] float64 (the
    docstring's 2 D + float32 rounding; 0 where a copy is expected), floored [P,...] bool: where the floor was reached)."""
    P, B = y.shape
    y8, o8, R = y.astype(np.float64), obs.astype(np.float64), obs_var.astype(np.float64)
    e8 = np.zeros((P, B)) if method == 1 else eps.astype(np.float64)
    X = x.astype(np.float64).reshape(P, -1)
    bas = basin_of(x.shape, B, M)
    with np.errstate(all="ignore"):
        ybar = y8.sum(0) / P
        dyb = y8 - ybar
        v = (dyb * dyb).sum(0) / (P - 1)
        s = v + R
        ebar = e8.sum(0) / P
        d = (o8 + ebar) - ybar if method == 0 else o8 - ybar
        status = np.zeros(B, dtype=np.int32)
        bad = ~(np.isfinite(R) & (R > 0)) | ~np.isfinite(ybar) | ~np.isfinite(v) | ~np.isfinite(s)
        if method == 0:
            bad |= ~np.isfinite(e8).all(0)
        status[bad] = 2
        off = np.isnan(o8) if active is None else (np.isnan(o8) | (np.asarray(active) == 0))
        status[off] = 1
        stats = np.stack([ybar, v, d])
        stats[2, status == 2] = np.nan
        stats[:, status == 1] = np.nan

        Y, E, DY = y8[:, bas], e8[:, bas], dyb[:, bas]                  # [P,n]
        ybar_e, s_e, R_e, o_e, d_e = ybar[bas], s[bas], R[bas], o8[bas], d[bas]
        c = (X * DY).sum(0) / (P - 1)
        K = c / s_e
        xbar = X.sum(0) / P
        m = xbar + K * d_e
        if method == 0:
            inn = (o_e + E) - Y
            xa = X + K * inn
        else:
            alpha = 1.0 / (1.0 + np.sqrt(R_e / s_e))
            aK = alpha * K
            t = (X - xbar) - aK * DY
            xa = m + t
        if rho != 1.0:
            pre = xa
            xa = m + rho * (xa - m)
        raw = xa
        lo8 = float(np.float32(lo))                                     # the float32 of the ABI, widened
        xa = np.maximum(xa, lo8)
        floored = raw < lo8

        # the bound (docstring)
        Yabs, Xabs, Eabs = np.abs(y8).mean(0)[bas], np.abs(X).mean(0), np.abs(e8).mean(0)[bas]
        D_ybar = P * U * Yabs
        D_dy = D_ybar + U * np.abs(DY)
        D_c = ((np.abs(X) * D_dy).sum(0) + (P + 2) * U * (np.abs(X) * np.abs(DY)).sum(0)) / (P - 1)
        D_v = ((2 * np.abs(dyb) * (P * U * np.abs(y8).mean(0) + U * np.abs(dyb))).sum(0) + (P + 2) * U * (dyb * dyb).sum(0)) / (P - 1)
        D_s = (D_v + U * s)[bas]
        D_K = D_c / s_e + np.abs(c) * D_s / s_e ** 2 + U * np.abs(K)
        D_xbar = P * U * Xabs
        D_d = D_ybar + P * U * Eabs + 2 * U * (np.abs(o_e) + np.abs(ebar[bas]) + np.abs(d_e))
        D_m = D_xbar + D_K * np.abs(d_e) + np.abs(K) * D_d + U * np.abs(K * d_e) + U * np.abs(m)
        if method == 0:
            D_i = 2 * U * (np.abs(o_e) + np.abs(E) + np.abs(inn))
            D_xa = D_K * np.abs(inn) + np.abs(K) * D_i + U * np.abs(K * inn) + U * np.abs(X + K * inn)
        else:
            D_alpha = D_s / (2 * s_e) + 4 * U
            D_aK = D_alpha * np.abs(K) + D_K + U * np.abs(K)
            D_t = D_xbar + U * np.abs(X - xbar) + D_aK * np.abs(DY) + np.abs(aK) * D_dy + U * np.abs(aK * DY) + U * np.abs(t)
            D_xa = D_m + D_t + U * np.abs(m + t)
        if rho != 1.0:
            D_xa = D_m + rho * (D_xa + D_m) + 2 * U * rho * np.abs(pre - m) + U * np.abs(raw)
        bound = 2 * D_xa + 2.0 ** -24 * (np.abs(xa) + 2 * D_xa) + 2.0 ** -150

        copy = (status != 0)[bas] | ~np.isfinite(K) | ~np.isfinite(raw).all(0) | \
            ~np.isfinite(xa.astype(np.float32)).all(0)
        status3 = np.zeros(B, dtype=bool)
        np.logical_or.at(status3, bas, copy & (status == 0)[bas])
        status[status3] = 3
        xa = np.where(copy, X, xa)
        bound = np.where(copy, 0.0, bound)
        floored = floored & ~copy
    return xa.reshape(x.shape), status, stats, bound.reshape(x.shape), floored.reshape(x.shape)


def inputs(P, B, M, seed, kind="wet"):
    """y [P,B], obs, obs_var [B], eps [P,B], and the three array kinds: storages [P,5,B,M] (floor 1e-5), history [P,14,B]
    (floor 0) and an extra [P,3,B] (no floor) -- all float32, correlated with y so that the gains are not noise.
    kind 'dry': storages within a few floors of the floor and an observation one spread BELOW ybar, so that the update drives a
    share of them onto the floor."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-1, 1, size=B)
    z = rng.standard_normal((P, B))
    y = (scale * (3.0 + z)).astype(np.float32)
    obs_var = ((0.3 * scale) ** 2).astype(np.float32)
    if kind == "dry":
        obs = (scale * (3.0 - 1.0 + 0.1 * rng.standard_normal(B))).astype(np.float32)
        base = 1e-5 * (1.0 + 3.0 * rng.random((P, 5, B, M)))
        states = (base * (1.0 + 0.8 * np.clip(z, -1, 3)[:, None, :, None] * rng.random((1, 5, B, M)))).astype(np.float32)
        states = np.maximum(states, np.float32(1e-5))
    else:
        obs = (scale * (3.0 + 0.7 * rng.standard_normal(B))).astype(np.float32)
        states = (20.0 * rng.random((1, 5, B, M)) * np.exp(0.3 * z[:, None, :, None] * rng.uniform(-1, 1, (1, 5, B, M))
                                                          + 0.2 * rng.standard_normal((P, 5, B, M)))).astype(np.float32)
    hist = np.maximum(scale * (3.0 + 0.6 * z[:, None, :] * rng.random((1, 14, B)) + 0.5 * rng.standard_normal((P, 14, B))),
                      0.0).astype(np.float32)
    extra = (scale * (3.0 + z[:, None, :] * rng.uniform(-1, 1, (1, 3, B)) + 0.3 * rng.standard_normal((P, 3, B)))).astype(np.float32)
    eps = (np.sqrt(obs_var) * rng.standard_normal((P, B))).astype(np.float32)
    return {"y": y, "obs": obs, "obs_var": obs_var, "eps": eps,
            "arrays": [(states, M, 1e-5), (hist, 1, 0.0), (extra, 1, -np.inf)]}
