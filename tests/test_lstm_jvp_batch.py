"""Forward-mode AD of SeqLSTM along many directions per call (SeqLSTM.jvp_batch / hydrodl2_amd.lstm_jvp_batch,
include/hbvx_lstm.h's hbvx_lstm_tangent_batch).

Two references.  The recurrence: hbvx_lstm_tangent, direction by direction on the same buffers -- bit for bit, since
a (direction, row tile) pair of the batch kernel runs the one-direction kernel's operations in its order.  The module
level: torch.nn.LSTM in float64 on the host under forward_ad, one call per direction, at test_lstm_jvp.py's
tolerances (2e-4 of the tangent's largest entry for one layer, 3e-4 for two), every element of every direction; the
time-parallel terms are formed by other library calls than LstmSeq.jvp's (products written into a direction's slice,
accumulating products) and may round differently, so the comparison with D one-direction forward_ad calls of the
module is at that tolerance too.  What must not depend on the company a direction is in -- pieces of a request
against the whole -- is compared bit for bit.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import hydrodl2_amd
from hydrodl2_amd import _abi
from hydrodl2_amd.lstm import SeqLSTM, lstm_jvp_batch

from .test_lstm_jvp import DIRS_1, _directions, _jvp, _tol, _torch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hydrodl2_amd", "csrc", "libhbvx.so")
NEW = ("hbvx_lstm_tangent_batch", "hbvx_lstm_tangent_batch_workspace_bytes")


def _stacked(mod, x, hx, which, D, seed):
    """name -> [D, ...]: D draws of test_lstm_jvp.py's direction set `which`."""
    per = [_directions(mod, x, hx, which, seed=seed + 17 * d) for d in range(D)]
    return {k: torch.stack([p[k] for p in per]) for k in per[0]}


def _slice(tangents, d):
    return {k: v[d] for k, v in tangents.items()}


def _flat(res):
    """(out, (h_n, c_n)) -> [out, h_n, c_n]"""
    return [res[0], res[1][0], res[1][1]]


def _case(T, B, I, H, L, seed, state=True, **kw):
    torch.manual_seed(seed)
    mod = SeqLSTM(I, H, check=True, num_layers=L, **kw).cuda()
    x = torch.randn(T, B, I, device="cuda")
    hx = (0.5 * torch.randn(L, B, H, device="cuda"), torch.randn(L, B, H, device="cuda")) if state else None
    return mod, x, hx


def _assert_close_per_direction(got, want_of, D, L, label):
    """got: [out_t, h_n_t, c_n_t] with the direction axis; want_of(d): the three reference tangents of direction d."""
    for d in range(D):
        want = want_of(d)
        for name, a, b in zip(("out", "h_n", "c_n"), got, want):
            a = a[d]
            assert a.shape == b.shape, (label, d, name, a.shape, b.shape)
            assert torch.isfinite(a).all(), (label, d, name)
            err = (a.cpu().double() - b.cpu().double()).abs().max().item()
            ref = b.abs().max().item()
            print(f"{label} d={d} {name}: err {err:.3g} ref {ref:.3g} ratio {err / (_tol(L) * max(ref, 1e-3)):.3g}")
            assert err <= _tol(L) * max(ref, 1e-3), (label, d, name, err, ref)


# ------------------------------------------------------------------------------------------------ CPU tier

@pytest.fixture(scope="module")
def hip_lib():
    import __graft_entry__ as ge
    return _abi.Library(ge.build_hip())


def test_the_library_exports_the_batch_entry_points(hip_lib):
    for name in NEW:
        assert name in _abi.OPTIONAL_EXPORTS
        assert name not in hip_lib.missing
    assert hydrodl2_amd.lstm_jvp_batch is lstm_jvp_batch


def test_batch_entry_point_validates_its_arguments(hip_lib):
    """Refused before anything touches a device, like hbvx_lstm_tangent."""
    lib = hip_lib
    r = _abi.LstmDesc(abi_version=0, T=4, B=2, H=64)
    big = 1 << 40

    def tan(r, n_dir=3, w_hh=1, gates=1, c_all=1, gx_t=1, h_t=1, ws=1, nb=big):
        lib.lstm_tangent_batch(r, n_dir, w_hh, gates, None, c_all, gx_t, None, None, h_t, None, ws, nb, 0)
    with pytest.raises(_abi.HbvxError, match="abi_version"):
        tan(r)
    r.abi_version = _abi.LSTM_ABI_VERSION
    r.H = 48
    with pytest.raises(_abi.HbvxError, match="hidden size"):
        tan(r)
    r.H = 64
    for n_dir in (0, -2):
        with pytest.raises(_abi.HbvxError, match="n_dir"):
            tan(r, n_dir=n_dir)
    with pytest.raises(_abi.HbvxError, match="workspace"):
        tan(r, nb=16)
    with pytest.raises(_abi.HbvxError, match="workspace"):          # enough for two directions, asked for three
        tan(r, nb=lib.lstm_tangent_batch_workspace_bytes(r, 2))
    with pytest.raises(_abi.HbvxError, match="workspace"):
        tan(r, ws=None)
    for k in ("w_hh", "gates", "c_all", "gx_t", "h_t"):
        with pytest.raises(_abi.HbvxError, match="NULL"):
            tan(r, **{k: None})
    # more (direction, row tile) pairs than a launch's grid can count
    r.B = 16 * 1024
    with pytest.raises(_abi.HbvxError, match="out of range"):
        tan(r, n_dir=1 << 16)


def test_batch_workspace_size(hip_lib):
    lib = hip_lib
    r = _abi.LstmDesc(abi_version=_abi.LSTM_ABI_VERSION, T=37, B=100, H=256)
    assert lib.lstm_tangent_batch_workspace_bytes(r, 0) == 0
    assert lib.lstm_tangent_batch_workspace_bytes(r, -1) == 0
    for bad in (dict(T=0), dict(B=0), dict(H=0)):
        kw = dict(abi_version=_abi.LSTM_ABI_VERSION, T=37, B=100, H=256)
        kw.update(bad)
        assert lib.lstm_tangent_batch_workspace_bytes(_abi.LstmDesc(**kw), 4) == 0
    size = [lib.lstm_tangent_batch_workspace_bytes(r, n) for n in (1, 2, 3, 16)]
    slab = 37 * 7 * 256 * 16 * 4                       # T x row tiles x H x 16 rows, float: one direction's slabs
    assert size[1] - size[0] == size[2] - size[1] == slab
    assert size[3] - size[0] == 15 * slab
    assert 0 < size[0] - slab <= 4096                  # the error word's line
    assert size[0] <= lib.lstm_workspace_bytes(r)      # one direction: no more than the one-direction calls take


def test_jvp_batch_on_a_library_without_the_export_names_it(oracle_backend):
    """The CPU restatement under oracle/ lacks hbvx_lstm_tangent_batch: the call raises an error naming the export
    (before it runs anything), and a plain forward still runs on that library."""
    torch.manual_seed(0)
    mod = SeqLSTM(4, 8, num_layers=2)
    x = torch.randn(5, 3, 4)
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_lstm_tangent_batch"):
        mod.jvp_batch(x, tangents={"x": torch.randn(2, 5, 3, 4)})
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_lstm_tangent_batch"):
        lstm_jvp_batch(mod, x, None, {"weight_hh_l1": torch.randn(3, 32, 8)})
    out, (hn, cn) = mod(x)
    assert out.shape == (5, 3, 8) and cn.shape == (2, 3, 8)


def test_tangents_are_validated_on_the_host():
    """Names, the shared leading axis and the shapes behind it: ValueError before any library is asked for."""
    torch.manual_seed(0)
    mod = SeqLSTM(4, 8, num_layers=2)
    T, B = 5, 3
    x = torch.randn(T, B, 4)
    hx = (torch.randn(2, B, 8), torch.randn(2, B, 8))
    with pytest.raises(ValueError, match="at least one tangent"):
        mod.jvp_batch(x, tangents={})
    with pytest.raises(ValueError, match="at least one tangent"):
        mod.jvp_batch(x)
    with pytest.raises(ValueError, match="unknown tangent names"):
        mod.jvp_batch(x, tangents={"weight_ih_l2": torch.randn(2, 32, 8)})
    with pytest.raises(ValueError, match="leading direction axis"):
        mod.jvp_batch(x, tangents={"x": torch.randn(2, T, B, 4), "bias_ih_l0": torch.randn(3, 32)})
    with pytest.raises(ValueError, match="'x' must be"):
        mod.jvp_batch(x, tangents={"x": torch.randn(2, T, B, 5)})
    with pytest.raises(ValueError, match="'x' must be"):
        mod.jvp_batch(x, tangents={"x": torch.randn(T, B, 4)})          # no direction axis
    with pytest.raises(ValueError, match="'weight_hh_l1' must be"):
        mod.jvp_batch(x, tangents={"weight_hh_l1": torch.randn(2, 8, 32)})
    with pytest.raises(ValueError, match="'h0' must be"):
        mod.jvp_batch(x, hx, tangents={"h0": torch.randn(2, B, 8)})      # [D,L,B,H] wanted
    with pytest.raises(ValueError, match="hx"):
        mod.jvp_batch(x, tangents={"c0": torch.randn(2, 2, B, 8)})       # a state tangent without a state
    with pytest.raises(ValueError, match="float32"):
        mod.jvp_batch(x, tangents={"x": torch.randn(2, T, B, 4, dtype=torch.float64)})
    with pytest.raises(ValueError, match="no direction"):
        mod.jvp_batch(x, tangents={"x": torch.randn(0, T, B, 4)})
    with pytest.raises(ValueError, match="max_directions"):
        mod.jvp_batch(x, tangents={"x": torch.randn(2, T, B, 4)}, max_directions=0)


def test_the_batch_kernels_keep_the_one_direction_resources_and_prefetch():
    """Every k_lstm_dirs instance: no scratch, no spilled VGPR, the registers, LDS and waves per SIMD of its
    k_lstm_tan sibling (the host's residency arithmetic is the same for both), and in the time loop no s_waitcnt vmcnt
    between either prefetch batch (gx', gates, c of the next step) and the step's barrier -- the method of
    test_lstm_jvp.py::test_the_tangent_prefetch_is_not_waited_for_before_the_barrier."""
    if not os.path.exists(LIB):
        pytest.skip("libhbvx.so not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    table = {r["name"].split("(")[0]: r for r in kernel_resources.kernel_table(LIB)}
    names = [n for n in table if "k_lstm_dirs<" in n]
    assert len(names) == 6, names
    for n in names:
        r, one = table[n], table[n.replace("k_lstm_dirs<", "k_lstm_tan<")]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert r["waves_per_simd"] >= 3, (n, r)                          # launch_lstm puts up to 3 workgroups on a CU
        for k in ("vgpr", "agpr", "lds", "waves_per_simd"):
            assert r[k] == one[k], (n, k, r[k], one[k])
    dis = kernel_resources.disassemble_addr(LIB, ["k_lstm_dirs"])
    assert len(dis) == 6, sorted(dis)
    for sym, ins in dis.items():
        h, b = max(kernel_resources.loops_of(ins), key=lambda hb: hb[1] - hb[0])     # the time loop
        body = [x for _, x in ins[h:b + 1]]
        batches = [i for i in range(len(body)) if body[i].startswith("global_load_dword ") and
                   sum(x.startswith("global_load_dwordx4") for x in body[max(0, i - 6):i]) == 2]
        assert len(batches) == 2, (sym, batches)
        for i in batches:
            end = next(k for k in range(i, len(body)) if body[k].startswith("s_barrier"))
            waits = [x for x in body[i:end] if x.startswith("s_waitcnt") and "vmcnt" in x]
            assert not waits, f"{sym}: {waits} between the prefetch at loop instruction {i} and the barrier"


# ------------------------------------------------------------------------------------------------ GPU tier

def _abi_buffers(T, B, H, D, state, with_c0, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()                 # noqa: E731
    buf = dict(w_hh=rnd(4 * H, H) / H ** 0.5, gates=torch.sigmoid(rnd(T, B, H, 4)), c_all=rnd(T, B, H),
               gx_t=rnd(D, T, B, H, 4), c0=rnd(B, H) if with_c0 else None,
               h0_t=rnd(D, B, H) if state else None, c0_t=rnd(D, B, H) if state else None)
    buf["gates"][..., 2] = 2 * buf["gates"][..., 2] - 1                  # g is a tanh
    return buf


@pytest.mark.gpu
@pytest.mark.parametrize("units", ["8", "16"])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_batch_recurrence_is_bit_identical_to_the_one_direction_entry(hip_backend, monkeypatch, units, H):
    """hbvx_lstm_tangent_batch on [D, ...] buffers against D calls of hbvx_lstm_tangent on their slices, the kernel
    form pinned on both sides: torch.equal of every h'[d] and c'_{T-1}[d].  D in {1, 3, 7}, T in {1, 2, 37}, B not a
    multiple of 16, with and without the state tangents and c0."""
    from hydrodl2_amd import ops
    monkeypatch.setenv("HBVX_LSTM_UNITS", units)
    lib = hip_backend
    st = torch.cuda.current_stream().cuda_stream
    p = ops._ptr
    k = 0
    for D in (1, 3, 7):
        for T, B in ((1, 21), (2, 37), (37, 19)):
            for state, with_c0 in ((True, True), (False, False), (True, False)):
                k += 1
                b = _abi_buffers(T, B, H, D, state, with_c0, seed=1000 * H + k)
                r = _abi.LstmDesc(abi_version=_abi.LSTM_ABI_VERSION, T=T, B=B, H=H)
                nb = lib.lstm_tangent_batch_workspace_bytes(r, D)
                ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device="cuda")
                h_t = torch.full((D, T, B, H), float("nan"), device="cuda")
                c_t = torch.full((D, B, H), float("nan"), device="cuda")
                lib.lstm_tangent_batch(r, D, p(b["w_hh"]), p(b["gates"]), p(b["c0"]), p(b["c_all"]), p(b["gx_t"]),
                                       p(b["h0_t"]), p(b["c0_t"]), p(h_t), p(c_t), p(ws), nb, st)
                lib.lstm_check(r, p(ws), st)
                nb1 = lib.lstm_workspace_bytes(r)
                ws1 = torch.empty((nb1 + 3) // 4, dtype=torch.float32, device="cuda")
                for d in range(D):
                    h1 = torch.full((T, B, H), float("nan"), device="cuda")
                    c1 = torch.full((B, H), float("nan"), device="cuda")
                    lib.lstm_tangent(r, p(b["w_hh"]), p(b["gates"]), p(b["c0"]), p(b["c_all"]), p(b["gx_t"][d]),
                                     p(b["h0_t"][d]) if state else None, p(b["c0_t"][d]) if state else None,
                                     p(h1), p(c1), p(ws1), nb1, st)
                    lib.lstm_check(r, p(ws1), st)
                    label = (units, H, D, T, B, state, with_c0, d)
                    assert torch.isfinite(h1).all() and torch.isfinite(c1).all(), label
                    assert torch.equal(h_t[d], h1), label
                    assert torch.equal(c_t[d], c1), label


# every direction set of the one-direction tests ("all" among them) with a state; without one, those that need none
# (a state tangent without a state is refused: test_tangents_are_validated_on_the_host)
SETS = [(w, True) for w in DIRS_1] + [(w, False) for w in DIRS_1 if w not in ("h0", "c0", "state")]


@pytest.mark.gpu
@pytest.mark.parametrize("which,hx_given", SETS)
@pytest.mark.parametrize("L,T,B,I,H", [(1, 37, 19, 7, 64), (1, 2, 33, 12, 128), (2, 37, 21, 5, 256), (2, 1, 7, 3, 256)])
def test_batch_tangents_match_torch(hip_backend, which, hx_given, L, T, B, I, H):
    """Five directions per call against torch.nn.LSTM in float64 under forward_ad, direction by direction."""
    D = 5
    mod, x, hx = _case(T, B, I, H, L, seed=T * 100 + B + L, state=hx_given)
    tans = _stacked(mod, x, hx, which, D, seed=len(which) + H)
    _, got = mod.jvp_batch(x, hx, tangents=tans)
    ref = _torch_ref(mod)
    _assert_close_per_direction(_flat(got), lambda d: _jvp(ref, x, hx, _slice(tans, d), dtype=torch.float64,
                                                            device="cpu")[1], D, L, f"{which} L{L} {T}x{B}x{H}")


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2])
def test_batch_tangents_match_one_direction_forward_ad(hip_backend, L):
    """Against D one-direction forward_ad calls of the same module, at the float64 comparison's tolerance (the
    time-parallel terms may round differently; the recurrence does not: the bit-identity test above)."""
    D = 5
    mod, x, hx = _case(37, 40, 8, 128, L, seed=31 + L)
    tans = _stacked(mod, x, hx, "all", D, seed=3)
    _, got = mod.jvp_batch(x, hx, tangents=tans)
    _assert_close_per_direction(_flat(got), lambda d: _jvp(mod, x, hx, _slice(tans, d))[1], D, L, f"fwAD L{L}")


@pytest.mark.gpu
def test_more_pairs_than_one_launch_holds_and_pieces_equal_the_whole(hip_backend):
    """T 12, B 1000, H 256, D 3: 189 (direction, row tile) pairs x 16 workgroups against 3 x 256 CUs -- several
    launches, each with its rows of every direction's buffers; and D above max_directions runs in pieces on the one
    primal run whose results are the bits of the whole."""
    D = 3
    mod, x, hx = _case(12, 1000, 8, 256, 1, seed=4)
    tans = _stacked(mod, x, hx, "all", D, seed=4)
    prim, got = mod.jvp_batch(x, hx, tangents=tans)
    ref = _torch_ref(mod)
    _assert_close_per_direction(_flat(got), lambda d: _jvp(ref, x, hx, _slice(tans, d), dtype=torch.float64,
                                                            device="cpu")[1], D, 1, "launches")
    for md in (1, 2):
        prim_p, got_p = mod.jvp_batch(x, hx, tangents=tans, max_directions=md)
        for a, b in zip(_flat(prim) + _flat(got), _flat(prim_p) + _flat(got_p)):
            assert a.shape == b.shape and torch.equal(a, b), md
    # two layers, pieces of two out of five
    mod, x, hx = _case(20, 50, 6, 64, 2, seed=8)
    tans = _stacked(mod, x, hx, "all", 5, seed=8)
    whole, pieces = mod.jvp_batch(x, hx, tangents=tans), mod.jvp_batch(x, hx, tangents=tans, max_directions=2)
    for a, b in zip(_flat(whole[0]) + _flat(whole[1]), _flat(pieces[0]) + _flat(pieces[1])):
        assert a.shape == b.shape and torch.equal(a, b)


@pytest.mark.gpu
def test_batch_weight_dropout_draws_one_mask_for_primal_and_directions(hip_backend):
    """dr > 0 in training mode: the masks are drawn once, in the module's order, for the primal and every direction,
    and mask the weight tangents; torch's LSTM on the masked weights and masked weight tangents (the same masks,
    drawn from the same seed) is the reference, and the primal is the plain training-mode call from that seed."""
    L, T, B, I, H, p, D = 2, 25, 19, 6, 64, 0.5, 4
    torch.manual_seed(3)
    mod = SeqLSTM(I, H, check=True, num_layers=L, dr=p).cuda().train()
    x = torch.randn(T, B, I, device="cuda")
    tans = _stacked(mod, x, None, "all", D, seed=9)
    torch.manual_seed(11)
    prim, got = mod.jvp_batch(x, tangents=tans)
    torch.manual_seed(11)
    with torch.no_grad():
        plain = mod(x)
    for a, b in zip(_flat(prim), _flat(plain)):
        assert torch.equal(a, b)
    torch.manual_seed(11)
    masks = {}
    for layer in range(L):                      # the module's draw order: W_ih, then W_hh, layer by layer
        for k in (f"weight_ih_l{layer}", f"weight_hh_l{layer}"):
            w = getattr(mod, k)
            masks[k] = torch.nn.functional.dropout(torch.ones_like(w), p, training=True)
    assert any((m == 0).any() for m in masks.values())
    ref = _torch_ref(mod)
    with torch.no_grad():
        for k, m in masks.items():
            getattr(ref, k).copy_((getattr(mod, k).detach() * m).double().cpu())

    def want(d):
        rdirs = {k: (v * masks[k] if k in masks else v) for k, v in _slice(tans, d).items()}
        return _jvp(ref, x, None, rdirs, dtype=torch.float64, device="cpu")[1]
    _assert_close_per_direction(_flat(got), want, D, L, "dropout")


@pytest.mark.gpu
def test_batch_adjoint_consistency_at_the_dmg_shape(hip_backend):
    """Per direction d: |<w, J v_d> - <J^T w, v_d>| <= 1e-4 |w| |J v_d| against the existing backward, at T 730,
    B 100, H 256, D = 4, every input carrying a direction, the loss weights on out, h_n and c_n; dot products in
    float64."""
    T, B, I, H, D = 730, 100, 16, 256, 4
    mod, x, hx = _case(T, B, I, H, 1, seed=21)
    tans = _stacked(mod, x, hx, "all", D, seed=21)
    _, got = mod.jvp_batch(x, hx, tangents=tans)
    jv = _flat(got)
    g = torch.Generator(device="cpu").manual_seed(22)
    w = [torch.randn(t.shape[1:], generator=g).cuda() for t in jv]
    xl = x.clone().requires_grad_(True)
    h0, c0 = (s.clone().requires_grad_(True) for s in hx)
    for p in mod.parameters():
        p.grad = None
    out, (hn, cn) = mod(xl, (h0, c0))
    sum((o * ww).sum() for o, ww in zip((out, hn, cn), w)).backward()
    grads = dict((k, p.grad) for k, p in mod.named_parameters())
    grads.update(x=xl.grad, h0=h0.grad, c0=c0.grad)
    nw = sum((t.double() ** 2).sum().item() for t in w) ** 0.5
    for d in range(D):
        lhs = sum((a.double() * b[d].double()).sum().item() for a, b in zip(w, jv))
        rhs = sum((grads[k].double() * v[d].double()).sum().item() for k, v in tans.items())
        njv = sum((t[d].double() ** 2).sum().item() for t in jv) ** 0.5
        print(f"adjoint d={d}: lhs {lhs:.9g} rhs {rhs:.9g} ratio {abs(lhs - rhs) / (1e-4 * nw * njv):.3g}")
        assert abs(lhs - rhs) <= 1e-4 * nw * njv, (d, lhs, rhs, nw * njv)


@pytest.mark.gpu
def test_batch_primal_is_a_plain_call_and_the_call_is_deterministic(hip_backend):
    mod, x, hx = _case(80, 100, 16, 256, 2, seed=6)
    with torch.no_grad():
        plain = mod(x, hx)
        plain0 = mod(x)
    tans = _stacked(mod, x, hx, "all", 3, seed=6)
    prim1, tan1 = mod.jvp_batch(x, hx, tangents=tans)
    prim2, tan2 = mod.jvp_batch(x, hx, tangents=tans)
    for a, b in zip(_flat(prim1), _flat(plain)):
        assert torch.equal(a, b)
    for a, b in zip(_flat(prim1) + _flat(tan1), _flat(prim2) + _flat(tan2)):
        assert torch.equal(a, b)
    assert not any(t.requires_grad for t in _flat(prim1) + _flat(tan1))
    prim0, _ = lstm_jvp_batch(mod, x, None, {"x": tans["x"]})          # the zero-state call
    for a, b in zip(_flat(prim0), _flat(plain0)):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_streamflow_sensitivity_to_every_input_channel(hip_backend):
    """Linear -> ReLU -> SeqLSTM -> Linear -> Hbv, one direction per input channel of the network (every basin and
    day at once): SeqLSTM.jvp_batch feeds hydrodl2_amd.jvp_batch a full-form parameter tangent, and
    tan['streamflow'][d] is compared with the same chain in float64 (torch's LSTM and oracle/hbv_restate64.py) at
    _assert_tangent_close's defaults, for every channel."""
    from . import restate_util as ru
    from . import synth
    from .test_jvp_gpu import _assert_tangent_close
    from .golden_cases import PHY_NAMES
    T, B, n_in, H = 120, 37, 6, 64
    ny = len(PHY_NAMES["Hbv"]) + 2
    cfg = dict(nmul=1, dynamic_params={"Hbv": ["parBETA", "parK0"]}, warm_up=0)
    torch.manual_seed(1)
    lin_in, lin_out = torch.nn.Linear(n_in, H).cuda(), torch.nn.Linear(H, ny).cuda()
    lstm = SeqLSTM(H, H, check=True).cuda()
    z = torch.randn(T, B, n_in, device="cuda")
    z_t = torch.zeros(n_in, T, B, n_in, device="cuda")
    for ch in range(n_in):
        z_t[ch, :, :, ch] = 1.0                    # d/d(input channel ch), every basin and day
    x_phy = torch.from_numpy(synth.forcing(T, B, 7)).cuda()
    model = hydrodl2_amd.load_model("hbv", "Hbv")(cfg, torch.device("cuda"))
    with torch.no_grad():
        pre = lin_in(z)
        (h, _), (h_t, _) = lstm.jvp_batch(torch.relu(pre), tangents={"x": (pre > 0) * (z_t @ lin_in.weight.T)})
        raw, raw_t = lin_out(h), h_t @ lin_out.weight.T
        out, tan = hydrodl2_amd.jvp_batch(model, {"x_phy": x_phy}, raw, {"parameters": raw_t}, keys=("streamflow",))
        plain = model({"x_phy": x_phy}, lin_out(lstm(torch.relu(lin_in(z)))[0]))["streamflow"]
    assert torch.equal(out["streamflow"], plain)
    got = tan["streamflow"].double().cpu().numpy()
    assert got.shape[0] == n_in

    li64, lo64 = (torch.nn.Linear(m.in_features, m.out_features).double() for m in (lin_in, lin_out))
    li64.load_state_dict({k: v.double().cpu() for k, v in lin_in.state_dict().items()})
    lo64.load_state_dict({k: v.double().cpu() for k, v in lin_out.state_dict().items()})
    ref = _torch_ref(lstm)
    kw = ru.config_kwargs("Hbv", cfg)
    for ch in range(n_in):
        with fwAD.dual_level():
            zz = fwAD.make_dual(z.double().cpu(), z_t[ch].double().cpu())
            hh, _ = ref(torch.relu(li64(zz)))
            q64 = ru.restate().run("Hbv", x_phy.double().cpu(), lo64(hh), **kw)[0]["streamflow"]
            want = fwAD.unpack_dual(q64).tangent.detach().numpy()
        assert np.abs(want).max() > 0
        _assert_tangent_close(f"lstm-jvp-batch-e2e:streamflow:ch{ch}", got[ch], want)
