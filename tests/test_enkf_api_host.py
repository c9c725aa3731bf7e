"""CPU tier: the front end and the binding of the ensemble Kalman update -- every refusal of `enkf_update` and `enkf_filter`
on host tensors (a call that got as far as the library would fail with the package's own 'no CPU path' error instead of
the refusal under test), the `_abi` row and structs against include/hbvx_enkf.h, the struct sizes against the
cross-compiled library, and the launcher's own refusals, which happen before anything is launched and so run without a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

import hydrodl2_amd
from hydrodl2_amd import _abi, enkf
from hydrodl2_amd.ensemble import EnsembleState

from .test_hbv_adj import host_math_backend  # noqa: F401  (fixture)
from .test_population_host import _model
from .test_step_math_host import steptest_lib  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_the_calls_are_exported():
    assert hydrodl2_amd.enkf_update is enkf.enkf_update and hydrodl2_amd.enkf_filter is enkf.enkf_filter
    assert {"enkf_update", "enkf_filter"} <= set(hydrodl2_amd.__all__)
    assert [row[0] for row in _abi.ENKF_SIGNATURES] == ["hbvx_enkf_sizeof", "hbvx_enkf_update"]
    assert callable(_abi.Library.enkf_update)


def test_enkf_update_refuses_before_any_library_call():
    P, B, M = 4, 3, 2
    st = EnsembleState(torch.ones(P, 5, B, M), torch.ones(P, 14, B), 7)
    y, o = torch.ones(P, B), torch.ones(B)
    state = torch.get_rng_state()

    def call(state=st, predicted=y, observed=o, obs_sigma=1.0, **kw):
        return hydrodl2_amd.enkf_update(state, predicted, observed, obs_sigma, **kw)

    with pytest.raises(ValueError, match="state must be an EnsembleState"):
        call(state=(st.states, st.history, 0))
    with pytest.raises(ValueError, match="state.states must be a float32 tensor"):
        call(state=EnsembleState(st.states.double(), None, 0))
    with pytest.raises(ValueError, match="state.states must be a float32 tensor"):
        call(state=EnsembleState(None, None, 0))
    with pytest.raises(ValueError, match=r"state.states must be \[P,5,B,M\]"):
        call(state=EnsembleState(torch.ones(P, 4, B, M), None, 0))
    with pytest.raises(ValueError, match="state.history must be"):
        call(state=EnsembleState(st.states, torch.ones(P, 13, B), 0))
    with pytest.raises(ValueError, match=r"state.history must be \[4,14,3\]"):
        call(state=EnsembleState(st.states, torch.ones(P, 14, B + 1), 0))
    with pytest.raises(ValueError, match="state.history lives on meta"):
        call(state=EnsembleState(st.states, torch.ones(P, 14, B, device="meta"), 0))
    with pytest.raises(ValueError, match="at least 2 particles"):
        call(state=EnsembleState(torch.ones(1, 5, B, M), None, 0), predicted=torch.ones(1, B))
    with pytest.raises(ValueError, match="predicted must be a float32 tensor"):
        call(predicted=y.double())
    with pytest.raises(ValueError, match=r"predicted must be \[4,3\]"):
        call(predicted=torch.ones(P, B + 1))
    with pytest.raises(ValueError, match=r"predicted must be \[4,3\]"):
        call(predicted=None)
    with pytest.raises(ValueError, match="predicted lives on meta"):
        call(predicted=torch.ones(P, B, device="meta"))
    with pytest.raises(ValueError, match=r"observed must be a float32 or float64 \[3\] tensor"):
        call(observed=torch.ones(B + 1))
    with pytest.raises(ValueError, match=r"observed must be a float32 or float64 \[3\] tensor"):
        call(observed=torch.ones(B, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"observed must be a float32 or float64 \[3\] tensor"):
        call(observed=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="observed lives on meta"):
        call(observed=torch.ones(B, device="meta"))
    with pytest.raises(ValueError, match="infinities"):
        call(observed=torch.tensor([1.0, INF, 1.0]))
    for bad in (0.0, -1.0, NAN, INF, torch.tensor([1.0, 0.0, 1.0])):
        with pytest.raises(ValueError, match="obs_sigma must be finite and > 0"):
            call(obs_sigma=bad)
    with pytest.raises(ValueError, match=r"obs_sigma must be a scalar or \[3\]"):
        call(obs_sigma=torch.ones(4))
    with pytest.raises(ValueError, match="method must be one of"):
        call(method="etkf")
    for bad in (0.0, -1.0, NAN, INF, "x"):
        with pytest.raises(ValueError, match="inflation must be"):
            call(inflation=bad)
    for bad in (NAN, INF, None):
        with pytest.raises(ValueError, match="floor must be finite"):
            call(floor=bad)
    with pytest.raises(ValueError, match="eps must be a float32 tensor"):
        call(method="perturbed", eps=torch.ones(P, B, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"eps must be \[4,3\]"):
        call(method="perturbed", eps=torch.ones(P + 1, B))
    with pytest.raises(ValueError, match="at most 2 extra arrays"):
        call(extra=[torch.ones(P, 1, B)] * 3)
    with pytest.raises(ValueError, match=r"extra\[1\] must be \[4,k,3\]"):
        call(extra=[torch.ones(P, 1, B), torch.ones(P, B)])
    with pytest.raises(ValueError, match=r"extra\[0\] must be a float32 tensor"):
        call(extra=[torch.ones(P, 1, B, dtype=torch.float64)])
    with pytest.raises(ValueError, match=r"extra\[0\] must be a float32 tensor"):
        call(extra=[None])
    with pytest.raises(ValueError, match=r"active must be a bool \[3\] tensor"):
        call(active=torch.ones(B))
    with pytest.raises(ValueError, match=r"active must be a bool \[3\] tensor"):
        call(active=torch.ones(B + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="active lives on meta"):
        call(active=torch.ones(B, dtype=torch.bool, device="meta"))
    # a valid call gets as far as the library, which has no CPU path -- and 'perturbed' has drawn by then
    with pytest.raises(RuntimeError, match="no CPU path"):
        call()
    assert torch.equal(torch.get_rng_state(), state)            # nothing above made a draw


def test_enkf_filter_refuses_before_the_model_runs():
    T, B, P = 8, 3, 4
    hbv = _model(dyn=["parBETA"])
    ny = hbv.learnable_param_count
    x, p = {"x_phy": torch.zeros(T, B, 3)}, torch.zeros(T, B, ny)
    tgt = torch.rand(T, B, generator=torch.Generator().manual_seed(3)) + 0.5
    state = torch.get_rng_state()

    def call(model=hbv, pp=p, target=tgt, n_particles=P, **kw):
        return hydrodl2_amd.enkf_filter(model, x, pp, target, n_particles, **{"obs_sigma": 1.0, **kw})

    hourly = hydrodl2_amd.load_model("hbv_2_hourly", "Hbv_2_hourly")({"nmul": 2, "dynamic_params": {"Hbv_2_hourly": []}},
                                                                    torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="Hbv_2_hourly"):
        call(model=hourly)
    with pytest.raises(NotImplementedError, match="HbvAdj.*Newton"):
        call(model=_model(("hbv_adj", "HbvAdj")), pp=torch.zeros(T, B, 12 * 2 + 2))
    with pytest.raises(NotImplementedError):
        call(model=torch.nn.Identity())
    with pytest.raises(ValueError, match="graph=True"):
        call(model=_model(graph=True))
    with pytest.raises(ValueError, match="comprout"):
        call(model=_model(nmul=1, comprout=True), pp=torch.zeros(T, B, 14))
    with pytest.raises(ValueError, match="target must be"):
        call(target=tgt[:-1])
    with pytest.raises(ValueError, match="infinities"):
        call(target=torch.full((T, B), INF))
    w = torch.ones(T, B)
    w[2, 1] = -1e-3
    with pytest.raises(ValueError, match="must not be negative"):
        call(weights=w)
    with pytest.raises(ValueError, match="transform must be one of"):
        call(transform="cube")
    with pytest.raises(ValueError, match="eps must be finite and > 0"):
        call(transform="log", eps=0.0)
    for bad in (1, 0, -3, 2.5, True, None):
        with pytest.raises(ValueError, match="n_particles must be an integer >= [12]"):
            call(n_particles=bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="window must be an integer >= 1"):
            call(window=bad)
    for bad in (0.0, -1.0, NAN, INF, torch.tensor([1.0, 0.0, 1.0])):
        with pytest.raises(ValueError, match="obs_sigma must be finite and > 0"):
            call(obs_sigma=bad)
    with pytest.raises(ValueError, match=r"obs_sigma must be a scalar or \[3\]"):
        call(obs_sigma=torch.ones(4))
    for name in ("prcp_sigma", "temp_sigma", "state_sigma", "state_add_sigma"):
        for bad in (-0.1, NAN, INF):
            with pytest.raises(ValueError, match=f"{name} must be finite and >= 0"):
                call(**{name: bad})
    with pytest.raises(ValueError, match="method must be one of"):
        call(method="pf")
    for bad in (0.0, -2.0, NAN, INF):
        with pytest.raises(ValueError, match="inflation must be finite and > 0"):
            call(inflation=bad)
    assert torch.equal(torch.get_rng_state(), state)


def test_a_library_without_the_export_is_named_before_the_primal(host_math_backend):  # noqa: F811
    """The host build of the math header has neither export: the filter names what it lacks before the module ran
    (dy_drop = 0.5: a run would have drawn masks), and so does the update."""
    model = _model(dyn=["parBETA"], dy_drop=0.5)
    T, B = 6, 3
    xs, p, tgt = {"x_phy": torch.rand(T, B, 3)}, torch.randn(T, B, model.learnable_param_count), torch.rand(T, B)
    state = torch.get_rng_state()
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_population_ensemble"):
        hydrodl2_amd.enkf_filter(model, xs, p, tgt, 4, obs_sigma=1.0)
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_enkf_update"):
        hydrodl2_amd.enkf_update(EnsembleState(torch.ones(2, 5, B, 2), None, 0), torch.ones(2, B), torch.ones(B), 1.0)
    assert torch.equal(torch.get_rng_state(), state)


def _fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    fields = []
    for part in body.split(";"):
        if part.strip():
            first, *more = part.strip().split(",")
            fields.append(re.sub(r"^\**|\[.*\]$", "", first.split()[-1]))
            fields += [re.sub(r"^\**|\[.*\]$", "", m.strip()) for m in more]
    return fields


def test_the_rows_and_the_structs_are_the_header():
    with open(os.path.join(ROOT, "include", "hbvx_enkf.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    found = {name: (ret, [] if not args.strip() else [a.strip() for a in " ".join(args.split()).split(",")])
             for ret, name, args in re.findall(r"^(int|uint64_t)\s*(hbvx_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M)}
    assert found == {"hbvx_enkf_sizeof": ("uint64_t", ["int which"]),
                     "hbvx_enkf_update": ("int", ["const hbvx_enkf *e", "void *stream"])}
    returns = {"int": C.c_int, "uint64_t": C.c_uint64}
    for name, required, restype, argtypes, layout in _abi.ENKF_SIGNATURES:
        ret, params = found[name]
        assert required is False and restype is returns[ret] and len(argtypes) == len(params), name
    assert _abi.ENKF_SIGNATURES[1][3] == [C.POINTER(_abi.Enkf), C.c_void_p] and _abi.ENKF_SIGNATURES[1][4] == (0, _abi.Enkf)
    assert re.search(r"#define HBVX_ENKF_MAX_ARRAYS\s+4\b", text) and _abi.ENKF_MAX_ARRAYS == 4
    assert re.search(r"#define HBVX_ENKF_PERTURBED\s+0\b", text) and re.search(r"#define HBVX_ENKF_SQRT\s+1\b", text)
    assert _abi.ENKF_METHODS == {"perturbed": 0, "sqrt": 1}
    assert _fields(text, "hbvx_enkf") == [f[0] for f in _abi.Enkf._fields_]
    assert _fields(text, "hbvx_enkf_array") == [f[0].rstrip("_") for f in _abi.EnkfArray._fields_]
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    assert not {"hbvx_enkf_sizeof", "hbvx_enkf_update"} & set(lib.missing)
    assert lib.dll.hbvx_enkf_sizeof(0) == C.sizeof(_abi.Enkf) == 16 + 8 + 8 * 8 + 4 * 32
    assert lib.dll.hbvx_enkf_sizeof(1) == C.sizeof(_abi.EnkfArray) == 32 and lib.dll.hbvx_enkf_sizeof(2) == 0
    assert lib.dll.hbvx_version() == 10                         # additive: the ABI version stands
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        assert "hbvx_enkf.h" in f.read()                        # a change to the header rebuilds the library


def _args(**kw):
    e = _abi.Enkf(P=4, B=3, method=1, n_arrays=2, inflation=1.0, y=1 << 20, y_stride=3, obs=64, obs_var=128, eps=None)
    e.a[0] = _abi.EnkfArray(in_=4096, out=4096, n=30, M=2, lo=1e-5)                 # [4,5,3,2] in place
    e.a[1] = _abi.EnkfArray(in_=8192, out=16384, n=42, M=1, lo=0.0)                 # [4,14,3]
    for k, v in kw.items():
        obj, names = e, k.split("__")
        if names[0] in ("a0", "a1"):
            obj, names = e.a[int(names[0][1])], names[1:]
        setattr(obj, names[-1], v)
    return e


def test_the_abi_refuses_bad_arguments_before_any_launch():
    """Host-side checks: no pointer is followed and nothing is launched, so this runs without a GPU."""
    import __graft_entry__ as ge
    lib = _abi.Library(ge.build_hip())
    who = "hbvx_enkf_update: "

    def refused(code, msg, e):
        with pytest.raises(_abi.HbvxError, match=rf"\({code}\).*{who}{msg}"):
            lib.enkf_update(e, 0)

    refused(-1, "e is NULL", None)
    for P in (1, 0, -2):
        refused(-2, "P must be at least 2", _args(P=P))
    refused(-2, "B must be at least 1", _args(B=0))
    for n in (0, 5, -1):
        refused(-2, r"n_arrays must be in 1\.\.4", _args(n_arrays=n))
    for m in (-1, 2):
        refused(-3, "method must be 0", _args(method=m))
    for rho in (0.0, -1.0, NAN, INF):
        refused(-2, "inflation must be finite and > 0", _args(inflation=rho))
    refused(-1, "y is NULL", _args(y=None))
    refused(-2, "y_stride is below B", _args(y_stride=2))
    refused(-1, "obs is NULL", _args(obs=None))
    refused(-1, "obs_var is NULL", _args(obs_var=None))
    refused(-1, "eps is NULL under method 0", _args(method=0))
    refused(-1, "an array's in is NULL", _args(a1__in_=None))
    refused(-1, "an array's out is NULL", _args(a0__out=None))
    for kw in (dict(a0__n=31), dict(a0__M=0), dict(a1__n=0), dict(a1__M=4), dict(a0__n=-30)):
        refused(-2, "an array's n must be a positive multiple", _args(**kw))
    refused(-2, "an array's lo is NaN", _args(a0__lo=NAN))
    # out == in exactly is allowed; a partial overlap is not: first and last element
    n0, n1, ny = 4 * 30, 4 * 42, 3 * 3 + 3
    for out in (4096 + 4, 4096 + 4 * (n0 - 1), 4096 - 4 * (n0 - 1)):
        refused(-2, "an array's out overlaps its in", _args(a0__out=out))
    for y in (16384, 16384 + 4 * (n1 - 1), 16384 - 4 * (ny - 1)):
        refused(-2, "an array's out overlaps y", _args(y=y))
    refused(-2, "an array's out overlaps another array's in", _args(a1__in_=4096 + 4 * (n0 - 1)))
    refused(-2, "an array's out overlaps another array's", _args(a1__out=4096 - 4 * (n1 - 1)))
    lib.missing.append("hbvx_enkf_update")                      # a library built before the export existed
    with pytest.raises(_abi.HbvxError, match="missing export hbvx_enkf_update"):
        lib.enkf_update(_args(), 0)
