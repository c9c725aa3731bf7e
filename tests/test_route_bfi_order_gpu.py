"""GPU tier: the order of every sum in the routing and baseflow-index kernels (csrc/hbvx.hip: k_uh_gamma, k_route_fwd,
k_route_bwd, k_route_bwd_params, k_bfi) through the C ABI, against NumPy restatements of the documented order.  The
library is built without fused contraction, so float32 multiply-then-add in NumPy reproduces the kernels bit for bit;
a product of two floats is exact in float64, so `gw + g0 * q` in float64 is the adjoint's `fma`.

Shapes: the smallest at which the thread mappings can go wrong.  T in {8, 15, 33, 65, 129, 130, 257}: fewer days than
taps, one day past a forward wave's 32 days, a forward workgroup's 128 days and an adjoint chunk of 64, both sides of
k_bfi's `t + 64 < T` edge, chunk counts that are no multiple of 4 (k_route_bwd_params' four parts).  B in {1, 17, 65,
130}: no multiple of 16 or 64.  S in {1, 4}.

What is held, per (T, B, S):
  uh        to a float64 restatement at the golden fixture's tolerance (rtol 1e-4, atol 1e-7: device powf / lgammaf are
            not NumPy's); every row sums to 1 within 2 ulp of 1 (the float32 taps summed in float64)
  y         bit-equal to the restatement fed with the uh the library returned
  gq        bit-equal; the per-chunk tap-gradient doubles in the workspace bit-equal
  ga / gb   float64 restatement of k_route_bwd_params (parts c = p mod 4 ascending, (p0 + p1) + (p2 + p3)) at 1e-6
            relative: its log is the only operation NumPy does not reproduce
  rows      hbvx_route_backward_rows into a NaN-filled [4,T,B]: rows S..3 exactly zero, rows 0..S-1 the bits of
            hbvx_route_backward
  bfi       the two per-basin sums in the slice order (a over t = sl, sl + 128, ..; c over t = sl + 64, ..; a + c;
            sl = 0..63 in sequence), then 100 * (s2 / (s0 + nearzero)): bit-equal -- the device's float32 division is
            correctly rounded, as NumPy's is."""
import math

import numpy as np
import pytest
import torch

from hydrodl2_amd import _abi

from . import synth

pytestmark = pytest.mark.gpu

TS = (8, 15, 33, 65, 129, 130, 257)
BS = (1, 17, 65, 130)
SS = (1, 4)
UH = _abi.UH_MAXLEN
CHUNK_BWD = 64
f32 = np.float32


def _inputs(T, B, S):
    a = synth.uniform((B,), 31, 1) * f32(2.9)
    b = synth.uniform((B,), 31, 2) * f32(6.5)
    q = (synth.uniform((S * T, B), 31, 3) * f32(5.0)).reshape(S, T, B)
    g = synth.loss_weights((S * T, B, 1), 31, 4).reshape(S, T, B).astype(f32)
    return a.astype(f32), b.astype(f32), np.ascontiguousarray(q, f32), np.ascontiguousarray(g)


def _desc(T, B, S, a, b):
    r = _abi.RouteDesc()
    r.abi_version = _abi.ABI_VERSION
    r.T, r.B, r.S = T, B, S
    r.L = min(T, UH)
    r.raw_sigmoid = 0
    r.ra, r.rb, r.r_stride = a.data_ptr(), b.data_ptr(), 1
    r.a_lo, r.a_hi, r.b_lo, r.b_hi = 0.0, 1.0, 0.0, 1.0
    return r


def _run(lib, T, B, S):
    dev = torch.device("cuda:0")
    a_h, b_h, q_h, g_h = _inputs(T, B, S)
    a, b, q, g = (torch.from_numpy(v).to(dev) for v in (a_h, b_h, q_h, g_h))
    r = _desc(T, B, S, a, b)
    L = r.L
    stream = torch.cuda.current_stream().cuda_stream
    uh = torch.full((B, L), float("nan"), device=dev)
    y = torch.full((S, T, B), float("nan"), device=dev)
    lib.route_forward(r, q.data_ptr(), uh.data_ptr(), y.data_ptr(), stream)
    nchunk = (T + CHUNK_BWD - 1) // CHUNK_BWD
    nbytes = lib.route_workspace_bytes(r)
    assert nbytes == nchunk * L * B * 8
    out = {"a": a_h, "b": b_h, "q": q_h, "g": g_h, "L": L, "nchunk": nchunk}
    for tag, rows in (("plain", S), ("rows", 4)):
        gq = torch.full((rows, T, B), float("nan"), device=dev)
        ga, gb = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
        ws = torch.full((nchunk * L * B,), float("nan"), dtype=torch.float64, device=dev)
        if tag == "plain":
            lib.route_backward(r, q.data_ptr(), uh.data_ptr(), g.data_ptr(), gq.data_ptr(), ga.data_ptr(), gb.data_ptr(),
                               ws.data_ptr(), nbytes, stream)
        else:
            lib.route_backward_rows(r, q.data_ptr(), uh.data_ptr(), g.data_ptr(), gq.data_ptr(), rows, ga.data_ptr(),
                                    gb.data_ptr(), ws.data_ptr(), nbytes, stream)
        torch.cuda.synchronize()
        out[tag] = {"gq": gq.cpu().numpy(), "ga": ga.cpu().numpy(), "gb": gb.cpu().numpy(),
                    "ws": ws.cpu().numpy().reshape(nchunk, L, B)}
    out["uh"], out["y"] = uh.cpu().numpy(), y.cpu().numpy()
    return out


def _taps15(uh, L):
    w = np.zeros((uh.shape[0], UH), f32)
    w[:, :L] = uh
    return w


def _conv_fwd(q, w):
    """acc = 0; acc += w[k] * q[t - k] for k = 0..14, float32, zero history."""
    S, T, B = q.shape
    pad = np.zeros((S, T + UH - 1, B), f32)
    pad[:, UH - 1:] = q
    acc = np.zeros((S, T, B), f32)
    for k in range(UH):
        acc = acc + w[None, None, :, k] * pad[:, UH - 1 - k:UH - 1 - k + T]
    return acc


def _conv_bwd(g, w):
    """acc = 0; acc += w[k] * gy[t + k] for k = 0..14, float32, zero from T on."""
    S, T, B = g.shape
    pad = np.zeros((S, T + UH - 1, B), f32)
    pad[:, :T] = g
    acc = np.zeros((S, T, B), f32)
    for k in range(UH):
        acc = acc + w[None, None, :, k] * pad[:, k:k + T]
    return acc


def _tap_partials(q, g, L):
    """ws[c, k, b]: from 0, series by series, the chunk's days ascending: gw = fma(gy[s,t,b], q[s,t-k,b], gw) in double."""
    S, T, B = q.shape
    nchunk = (T + CHUNK_BWD - 1) // CHUNK_BWD
    q64 = np.zeros((S, T + UH - 1, B))
    q64[:, UH - 1:] = q
    g64 = g.astype(np.float64)
    ws = np.zeros((nchunk, L, B))
    for s in range(S):
        for t in range(T):
            win = q64[s, t + UH - 1 - np.arange(L)]          # q[s, t - k, :], k = 0..L-1
            ws[t // CHUNK_BWD] = ws[t // CHUNK_BWD] + g64[s, t][None, :] * win
    return ws


def _params(ws, uh, a, b, L):
    """k_route_bwd_params in float64 (de-scaled inputs, bounds [0, 1]: the chain to the raw inputs is the identity)."""
    nchunk, _, B = ws.shape
    n4 = nchunk & ~3
    parts = []
    for p in range(4):
        acc = np.zeros((L, B))
        for c in range(p, n4, 4):
            acc = acc + ws[c]
        if p == 0:
            for c in range(n4, nchunk):
                acc = acc + ws[c]
        parts.append(acc)
    red = (parts[0] + parts[1]) + (parts[2] + parts[3])
    gw = np.zeros((UH, B))
    gw[:L] = red
    w = np.zeros((UH, B))
    w[:L] = uh.T.astype(np.float64)
    theta = (np.maximum(b, f32(0.0)) + f32(0.5)).astype(f32)
    th2 = theta.astype(np.float64) * theta.astype(np.float64)
    tk = np.arange(UH) + 0.5
    mlt, mt = np.zeros(B), np.zeros(B)
    for j in range(UH):
        mlt = mlt + w[j] * math.log(tk[j])
        mt = mt + w[j] * tk[j]
    gaa, gth = np.zeros(B), np.zeros(B)
    for j in range(UH):
        gaa = gaa + gw[j] * w[j] * (math.log(tk[j]) - mlt)
        gth = gth + gw[j] * w[j] * ((tk[j] - mt) / th2)
    ga = np.where(a > 0, gaa.astype(f32), f32(0.0))
    gb = np.where(b > 0, gth.astype(f32), f32(0.0))
    return ga, gb


def _uh64(a, b, L):
    aa = np.maximum(a.astype(np.float64), 0.0) + np.float64(f32(0.1))
    theta = np.maximum(b.astype(np.float64), 0.0) + 0.5
    t = np.arange(L)[None, :] + 0.5
    lg = np.array([math.lgamma(v) for v in aa])
    w = np.exp(-lg)[:, None] / theta[:, None] ** aa[:, None] * t ** (aa[:, None] - 1.0) * np.exp(-t / theta[:, None])
    return w / w.sum(1, keepdims=True)


def _same_bits(name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    iv = np.uint32 if got.dtype == np.float32 else np.uint64
    diff = got.view(iv) != want.view(iv)
    if diff.any():
        i = np.argwhere(diff)[0]
        raise AssertionError(f"{name}: {int(diff.sum())} of {diff.size} elements differ in bits, first at {tuple(i)}: "
                             f"{got[tuple(i)]!r} vs {want[tuple(i)]!r}")


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("T", TS)
def test_routing_sums_run_in_the_documented_order(T, B, hip_backend):
    for S in SS:
        res = _run(hip_backend, T, B, S)
        L, uh = res["L"], res["uh"]
        who = f"T={T} B={B} S={S}"
        assert np.isfinite(uh).all(), who
        ref_uh = _uh64(res["a"], res["b"], L)
        err = np.abs(uh - ref_uh)
        rowsum = np.abs(uh.astype(np.float64).sum(1) - 1.0)
        print(f"{who}: uh max err {err.max():.3e}, worst |row sum - 1| {rowsum.max():.3e} ({rowsum.max() / 2.0 ** -23:.2f} ulp)")
        assert (err <= 1e-7 + 1e-4 * np.abs(ref_uh)).all(), who
        assert (rowsum <= 2.0 * 2.0 ** -23).all(), (who, float(rowsum.max()))
        w = _taps15(uh, L)
        _same_bits(f"{who} y", res["y"], _conv_fwd(res["q"], w))
        want_gq = _conv_bwd(res["g"], w)
        want_ws = _tap_partials(res["q"], res["g"], L)
        want_ga, want_gb = _params(want_ws, uh, res["a"], res["b"], L)
        for tag in ("plain", "rows"):
            got = res[tag]
            _same_bits(f"{who} {tag} gq", got["gq"][:S], want_gq)
            _same_bits(f"{who} {tag} ws", got["ws"], want_ws)
            for k, want in (("ga", want_ga), ("gb", want_gb)):
                rel = np.abs(got[k].astype(np.float64) - want) / np.maximum(np.abs(want), 1e-300)
                rel = np.where(got[k] == want, 0.0, rel)
                print(f"{who} {tag} {k}: worst relative difference {rel.max():.3e}")
                assert (rel <= 1e-6).all(), (who, tag, k, float(rel.max()))
        # the padded call: the rows without a series are zero, the others are the plain call's
        _same_bits(f"{who} rows gq[:S]", res["rows"]["gq"][:S], res["plain"]["gq"])
        assert (res["rows"]["gq"][S:].view(np.uint32) == 0).all(), who
        _same_bits(f"{who} rows ga", res["rows"]["ga"], res["plain"]["ga"])
        _same_bits(f"{who} rows gb", res["rows"]["gb"], res["plain"]["gb"])


def test_rows_call_refuses_fewer_rows_than_series(hip_backend):
    dev = torch.device("cuda:0")
    a, b = torch.ones(3, device=dev), torch.ones(3, device=dev)
    r = _desc(20, 3, 2, a, b)
    buf = torch.zeros(2 * 20 * 3, device=dev)
    with pytest.raises(_abi.HbvxError):
        hip_backend.route_backward_rows(r, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, None, None,
                                        None, 0, torch.cuda.current_stream().cuda_stream)


def _slice_sums(x):
    """k_bfi's per-basin sum of x [T,B]."""
    T, B = x.shape
    tot = np.zeros(B, f32)
    for sl in range(64):
        a, c = np.zeros(B, f32), np.zeros(B, f32)
        for t in range(sl, T, 128):
            a = a + x[t]
        for t in range(sl + 64, T, 128):
            c = c + x[t]
        tot = tot + (a + c)
    return tot


# .. and records long enough for the walk with eight rows in flight (from 960 + sl days on); 4 096 basins and more run
# the kernel's 16-basin blocks, fewer its 4-basin blocks with a chain per thread
BFI_CASES = [(T, B) for T in TS + (1100, 2200) for B in BS] + [(T, B) for T in (129, 130, 1100) for B in (4065, 4081)]


@pytest.mark.parametrize("T,B", BFI_CASES)
def test_bfi_sums_run_in_the_documented_order(T, B, hip_backend):
    dev = torch.device("cuda:0")
    qs = (synth.uniform((T, B), 33, 1) * f32(5.0)).astype(f32)
    q2 = (synth.uniform((T, B), 33, 2) * qs).astype(f32)
    nz = 1e-5
    out = torch.full((B,), float("nan"), device=dev)
    tq, t2 = torch.from_numpy(qs).to(dev), torch.from_numpy(q2).to(dev)
    hip_backend.bfi(T, B, tq.data_ptr(), t2.data_ptr(), nz, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    s0, s2 = _slice_sums(qs), _slice_sums(q2)
    want = f32(100.0) * (s2 / (s0 + f32(nz)))
    assert want.dtype == np.float32
    _same_bits(f"bfi T={T} B={B}", out.cpu().numpy(), want)
