"""CPU tier: hbvx_backward_live (include/hbvx_live_rows.h) in the binding's tables -- the row is the header's
prototype, the built library exports it, a library without it (the CPU restatement) lists it as missing -- and the
range of n_live4: the library, the binding and ops.py each refuse anything outside 1 .. 4.  No GPU: the library
answers a bad count before it looks at anything else."""
import ctypes as C
import os
import re

import pytest

import __graft_entry__ as ge
import hydrodl2_amd
from hydrodl2_amd import _abi, ops

EXPORT = "hbvx_backward_live"
E_SHAPE = -2


def _prototype():
    root = os.path.dirname(os.path.dirname(os.path.abspath(hydrodl2_amd.__file__)))
    with open(os.path.join(root, "include", "hbvx_live_rows.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    found = re.findall(r"^(int|uint64_t)\s*(hbvx_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M)
    assert len(found) == 1, found
    ret, name, args = found[0]
    return ret, name, [a.strip() for a in " ".join(args.split()).split(",")]


def test_the_row_is_the_prototype_of_the_header():
    ret, name, params = _prototype()
    assert (ret, name) == ("int", EXPORT)
    assert params == ["const hbvx_desc *d", "const hbvx_bwd_io *io", "int32_t n_live4", "void *stream"]
    assert [row[0] for row in _abi.LIVE_ROWS_SIGNATURES] == [EXPORT]
    _, required, restype, argtypes, layout = _abi.LIVE_ROWS_SIGNATURES[0]
    assert required is False and restype is C.c_int and layout is None
    assert argtypes == [C.POINTER(_abi.Desc), C.POINTER(_abi.BwdIO), C.c_int32, C.c_void_p]
    assert EXPORT not in _abi.EXPORTS                 # optional: the ABI version stays
    assert _abi.ABI_VERSION == 10


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(ge.HIP_LIB):
        pytest.skip("libhbvx.so not built")
    return _abi.Library(ge.HIP_LIB)


def test_the_built_library_exports_it_and_the_restatement_does_not(built, oracle_path):
    assert EXPORT not in built.missing and hasattr(built.dll, EXPORT)
    assert built.dll.hbvx_backward_live.argtypes == _abi.LIVE_ROWS_SIGNATURES[0][3]
    cpu = _abi.Library(oracle_path)
    assert EXPORT in cpu.missing
    with pytest.raises(_abi.HbvxError, match=EXPORT):
        cpu.backward_live(_abi.Desc(), _abi.BwdIO(), 1, 0)


@pytest.mark.parametrize("n", [0, 5, -1, 1 << 20])
def test_the_library_and_the_binding_refuse_a_count_outside_1_to_4(n, built):
    rc = built.dll.hbvx_backward_live(None, None, n, None)
    assert rc == E_SHAPE, rc
    assert b"n_live4" in built.dll.hbvx_last_error()
    with pytest.raises(ValueError, match="n_live4"):
        built.backward_live(_abi.Desc(), _abi.BwdIO(), n, 0)


@pytest.mark.parametrize("n", [0, 5, -3, 2.0, None])
def test_ops_refuses_a_count_outside_1_to_4(n):
    with pytest.raises(ValueError, match="n_live4"):
        ops._live_rows(n)


def test_ops_passes_the_counts_that_exist():
    assert [ops._live_rows(n) for n in (1, 2, 3, 4)] == [1, 2, 3, 4]
