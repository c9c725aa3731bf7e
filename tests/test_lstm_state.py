"""Sequence LSTM from an initial state (h0, c0): `SeqLSTM(x, hx)`, include/hbvx_lstm.h's *_hx entry points.
torch.nn.LSTM's float64 CPU LSTM on the same state dict and state is the reference; tolerances are those of
tests/test_lstm.py (outputs 2e-5 absolute, gradients 2e-4 relative to each gradient's largest entry; the
two-layer ones there for two layers)."""
import pytest
import torch

from hydrodl2_amd import _abi
from hydrodl2_amd.lstm import LstmSeq, SeqLSTM


def _tol(L):
    return (2e-4, 0.0) if L == 1 else (3e-4, 1e-4)      # (gradient, output rtol)


def _torch_reference(mod: SeqLSTM, x, h0, c0, g):
    ref = torch.nn.LSTM(mod.input_size, mod.hidden_size, num_layers=mod.num_layers).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in mod.state_dict().items()})
    xr, h0r, c0r = (t.detach().cpu().double().requires_grad_(True) for t in (x, h0, c0))
    out, (hn, cn) = ref(xr, (h0r, c0r))
    sum((o * w.cpu().double()).sum() for o, w in zip((out, hn, cn), g) if w is not None).backward()
    grads = {k: p.grad for k, p in ref.named_parameters()}
    grads.update(x=xr.grad, h0=h0r.grad, c0=c0r.grad)
    return (out, hn, cn), grads


def _case(T, B, I, H, L=1, seed=0, terms=(True, True, True), h0_zero=False, c0_zero=False):
    """Random x, h0, c0 (requiring grad) and loss weights g1..g3 on out, h_n, c_n (None: that term left out)."""
    torch.manual_seed(seed)
    mod = SeqLSTM(I, H, check=True, num_layers=L).cuda()
    x = torch.randn(T, B, I, device="cuda", requires_grad=True)
    h0 = (torch.zeros if h0_zero else torch.randn)(L, B, H, device="cuda").requires_grad_(True)
    c0 = (torch.zeros if c0_zero else torch.randn)(L, B, H, device="cuda").requires_grad_(True)
    shapes = ((T, B, H), (L, B, H), (L, B, H))
    g = [torch.randn(s, device="cuda") if on else None for s, on in zip(shapes, terms)]
    return mod, x, h0, c0, g


def _check(mod, x, h0, c0, g, L=1):
    out, (hn, cn) = mod(x, (h0, c0))
    assert cn.requires_grad
    sum((o * w).sum() for o, w in zip((out, hn, cn), g) if w is not None).backward()
    want, gw = _torch_reference(mod, x, h0, c0, g)
    gtol, rtol = _tol(L)
    for name, got, ref in zip(("out", "h_n", "c_n"), (out, hn, cn), want):
        assert got.shape == ref.shape
        err = (got.detach().cpu().double() - ref.detach()).abs()
        assert torch.all(err <= 2e-5 + rtol * ref.detach().abs()), (name, err.max().item())
    got = {k: p.grad for k, p in mod.named_parameters()}
    got.update(x=x.grad, h0=h0.grad, c0=c0.grad)
    for k, ref in gw.items():
        assert got[k] is not None, k
        err = (got[k].cpu().double() - ref).abs().max().item()
        assert err <= gtol * max(ref.abs().max().item(), 1e-3), (k, err, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------ CPU tier

def test_hx_entry_points_validate_their_arguments():
    """Mirror of tests/test_lstm.py::test_lstm_descriptor_validation for the *_hx calls (every call is refused
    before anything touches a device)."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    assert not lib.missing
    r = _abi.LstmDesc(abi_version=0, T=4, B=2, H=64)
    big = 1 << 30
    fwd = lambda r, w_hh=1, gx=1, gates=1, c_all=1, h_all=1, ws=1, nb=big: lib.lstm_forward_hx(   # noqa: E731
        r, w_hh, gx, 1, 1, gates, c_all, h_all, ws, nb, 0)
    bwd = lambda r, w_hh=1, gates=1, c_all=1, gh=1, gg=2, ws=1, nb=big: lib.lstm_backward_hx(      # noqa: E731
        r, w_hh, gates, 1, c_all, gh, 1, gg, 1, ws, nb, 0)
    for call in (fwd, bwd):
        with pytest.raises(_abi.HbvxError, match="abi_version"):
            call(r)
    r.abi_version = _abi.LSTM_ABI_VERSION
    r.H = 48
    for call in (fwd, bwd):
        with pytest.raises(_abi.HbvxError, match="hidden size"):
            call(r)
    r.H = 64
    for call in (fwd, bwd):
        with pytest.raises(_abi.HbvxError, match="workspace"):
            call(r, nb=16)
        with pytest.raises(_abi.HbvxError, match="workspace"):
            call(r, ws=None)
    for k in ("w_hh", "gx", "gates", "c_all", "h_all"):
        with pytest.raises(_abi.HbvxError, match="NULL"):
            fwd(r, **{k: None})
    for k in ("w_hh", "gates", "c_all", "gh", "gg"):
        with pytest.raises(_abi.HbvxError, match="NULL"):
            bwd(r, **{k: None})
    with pytest.raises(_abi.HbvxError, match="alias"):
        bwd(r, gates=7, gg=7)


def test_stateful_call_on_a_library_without_hx_names_the_export(oracle_backend):
    """The CPU restatement under oracle/ exports ABI version 1 only: it still loads, the zero-state call still runs
    on it, and a stateful call raises an error that names the missing export."""
    torch.manual_seed(0)
    mod = SeqLSTM(4, 8, num_layers=2)
    x = torch.randn(5, 3, 4)
    out, (hn, cn) = mod(x)
    assert out.shape == (5, 3, 8) and cn.shape == (2, 3, 8)
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_lstm_forward_hx"):
        mod(x, (torch.zeros(2, 3, 8), torch.zeros(2, 3, 8)))


def test_c_n_carries_gradient(oracle_backend):
    torch.manual_seed(0)
    _, (hn, cn) = SeqLSTM(4, 8)(torch.randn(5, 3, 4))
    assert hn.requires_grad and cn.requires_grad


@pytest.mark.parametrize("bad", ["shape", "layers", "dtype", "device", "arity"])
def test_bad_state_is_refused_before_any_launch(oracle_backend, bad):
    torch.manual_seed(0)
    mod = SeqLSTM(4, 8, num_layers=2)
    x = torch.randn(5, 3, 4)
    h0, c0 = torch.zeros(2, 3, 8), torch.zeros(2, 3, 8)
    hx = {"shape": (h0, torch.zeros(2, 4, 8)), "layers": (torch.zeros(1, 3, 8), c0),
          "dtype": (h0.double(), c0), "device": (h0, torch.zeros(2, 3, 8, device="meta")), "arity": (h0,)}[bad]
    with pytest.raises(ValueError):
        mod(x, hx)


# ------------------------------------------------------------------------------------------------ GPU tier

@pytest.mark.gpu
@pytest.mark.parametrize("L,T,B,I,H", [(1, 30, 19, 7, 64), (1, 25, 33, 12, 128), (1, 40, 37, 5, 256),
                                       (2, 20, 21, 9, 64), (2, 16, 5, 6, 128), (2, 12, 40, 8, 256),
                                       (1, 1, 7, 3, 64), (2, 1, 17, 4, 256)])
def test_state_matches_torch(hip_backend, L, T, B, I, H):
    mod, x, h0, c0, g = _case(T, B, I, H, L=L, seed=T * 1000 + B)
    _check(mod, x, h0, c0, g, L=L)


@pytest.mark.gpu
@pytest.mark.parametrize("units", ["8", "16"])
def test_state_both_forward_kernel_forms(hip_backend, monkeypatch, units):
    monkeypatch.setenv("HBVX_LSTM_UNITS", units)
    for k, (T, B, I, H) in enumerate([(20, 37, 5, 64), (30, 100, 12, 256)]):
        mod, x, h0, c0, g = _case(T, B, I, H, seed=11 + k)
        _check(mod, x, h0, c0, g)


@pytest.mark.gpu
def test_state_more_row_tiles_than_one_launch_holds(hip_backend):
    # 63 row tiles x 16 workgroups > 3 x 256 CUs: two launches, each with its rows of h0 / c0 / grad_c0
    mod, x, h0, c0, g = _case(12, 1000, 8, 256, seed=4)
    _check(mod, x, h0, c0, g)


@pytest.mark.gpu
@pytest.mark.parametrize("zero", ["c0", "h0"])
def test_state_with_one_half_zero(hip_backend, zero):
    mod, x, h0, c0, g = _case(20, 21, 6, 128, seed=8, h0_zero=zero == "h0", c0_zero=zero == "c0")
    _check(mod, x, h0, c0, g)


@pytest.mark.gpu
@pytest.mark.parametrize("given", ["h0", "c0"])
def test_function_with_one_state_tensor(hip_backend, given):
    """LstmSeq with only h0 or only c0 (the other None = zeros) against the module with a zero tensor in its place."""
    torch.manual_seed(2)
    T, B, I, H = 15, 19, 6, 64
    mod = SeqLSTM(I, H).cuda()
    x = torch.randn(T, B, I, device="cuda")
    s = torch.randn(B, H, device="cuda", requires_grad=True)
    z = torch.zeros(B, H, device="cuda")
    w = [getattr(mod, n) for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    h0, c0 = (s, None) if given == "h0" else (None, s)
    out, _, cn = LstmSeq.apply(x, *w, True, h0, c0, True)
    (out.sum() + cn.sum()).backward()
    got = s.grad.clone()
    s.grad = None
    out2, (_, cn2) = mod(x, (s[None], z[None]) if given == "h0" else (z[None], s[None]))
    (out2.sum() + cn2.sum()).backward()
    assert torch.equal(out, out2) and torch.equal(cn, cn2[0])
    assert torch.equal(got, s.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("term", ["c_n", "h_n"])
def test_loss_on_one_final_state_alone(hip_backend, term):
    mod, x, h0, c0, g = _case(25, 23, 7, 256, seed=9, terms=(False, term == "h_n", term == "c_n"))
    _check(mod, x, h0, c0, g)


@pytest.mark.gpu
def test_zero_state_is_the_zero_state_call(hip_backend):
    """SeqLSTM(x) and SeqLSTM(x, (zeros, zeros)): the same bits in the outputs and in the gradients of x and the
    weights (the stateful path multiplies a zero h0 into gx and adds a zero step-0 term to grad_W_hh)."""
    res = []
    for state in (False, True):
        torch.manual_seed(6)
        mod = SeqLSTM(11, 256, num_layers=2).cuda()
        x = torch.randn(60, 37, 11, device="cuda", requires_grad=True)
        gh = torch.randn(60, 37, 256, device="cuda")
        z = torch.zeros(2, 37, 256, device="cuda")
        out, (hn, cn) = mod(x, (z, z)) if state else mod(x)
        (out * gh).sum().backward()
        res.append([out, hn, cn, x.grad] + [p.grad for p in mod.parameters()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def _abi_forward(lib, w_hh, gx, h0, c0):
    T, B = gx.shape[:2]
    H = w_hh.shape[1]
    r = _abi.LstmDesc(abi_version=_abi.LSTM_ABI_VERSION, T=T, B=B, H=H)
    nb = lib.lstm_workspace_bytes(r)
    ws = torch.empty(nb // 4 + 1, device="cuda")
    gates = torch.empty(T, B, H, 4, device="cuda")
    c_all, h_all = torch.empty(T, B, H, device="cuda"), torch.empty(T, B, H, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()     # noqa: E731
    lib.lstm_forward_hx(r, w_hh.data_ptr(), gx.data_ptr(), ptr(h0), ptr(c0), gates.data_ptr(), c_all.data_ptr(),
                        h_all.data_ptr(), ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
    lib.lstm_check(r, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return h_all, c_all


@pytest.mark.gpu
@pytest.mark.parametrize("units", ["8", "16"])
@pytest.mark.parametrize("H", [64, 256])
def test_resume_is_exact(hip_backend, monkeypatch, units, H):
    """One gx run as [0, T), and as [0, T1) then [T1, T) from (h_all[T1-1], c_all[T1-1]): the same bits."""
    monkeypatch.setenv("HBVX_LSTM_UNITS", units)
    torch.manual_seed(H)
    T, T1, B = 50, 23, 37
    w_hh = torch.empty(4 * H, H, device="cuda").uniform_(-H ** -0.5, H ** -0.5)
    gx = torch.randn(T, B, H, 4, device="cuda")
    h, c = _abi_forward(hip_backend, w_hh, gx, None, None)
    h1, c1 = _abi_forward(hip_backend, w_hh, gx[:T1].contiguous(), None, None)
    h2, c2 = _abi_forward(hip_backend, w_hh, gx[T1:].contiguous(), h1[-1], c1[-1])
    torch.cuda.synchronize()
    assert torch.equal(h, torch.cat([h1, h2])) and torch.equal(c, torch.cat([c1, c2]))


@pytest.mark.gpu
def test_resume_is_differentiable(hip_backend):
    """Module level, the sequence split at T1 with the state carried over.  Attached: the one-shot gradients (to x,
    the weights, h0 and c0); detached (truncated back-propagation): the one-shot outputs."""
    T, T1 = 40, 17
    mod, x, h0, c0, g = _case(T, 29, 6, 128, L=2, seed=12)
    out, (hn, cn) = mod(x, (h0, c0))
    sum((o * w).sum() for o, w in zip((out, hn, cn), g)).backward()
    want = [t.grad.clone() for t in (x, h0, c0)] + [p.grad.clone() for p in mod.parameters()]
    for t in [x, h0, c0] + list(mod.parameters()):
        t.grad = None
    o1, s1 = mod(x[:T1], (h0, c0))
    o2, (hn2, cn2) = mod(x[T1:], s1)
    sum((o * w).sum() for o, w in zip((torch.cat([o1, o2]), hn2, cn2), g)).backward()
    got = [t.grad for t in (x, h0, c0)] + [p.grad for p in mod.parameters()]
    for a, b in zip(got, want):
        assert (a - b).abs().max().item() <= 2e-4 * max(b.abs().max().item(), 1e-3)
    with torch.no_grad():
        o1, s1 = mod(x[:T1], (h0, c0))
        o2, (hn2, cn2) = mod(x[T1:], (s1[0].detach(), s1[1].detach()))
        for a, b in ((torch.cat([o1, o2]), out), (hn2, hn), (cn2, cn)):
            assert (a - b).abs().max().item() <= 2e-5


@pytest.mark.gpu
def test_stateful_calls_are_deterministic(hip_backend):
    res = []
    for _ in range(2):
        mod, x, h0, c0, g = _case(80, 100, 16, 256, seed=21)
        out, (hn, cn) = mod(x, (h0, c0))
        sum((o * w).sum() for o, w in zip((out, hn, cn), g)).backward()
        res.append([out, hn, cn, x.grad, h0.grad, c0.grad] + [p.grad for p in mod.parameters()])
    for a, b in zip(*res):
        assert torch.equal(a, b)
