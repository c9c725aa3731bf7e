"""CPU tier: the binding's signature table (hydrodl2_amd/_abi.py, SIGNATURES) against the prototypes of include/hbvx.h
and include/hbvx_lstm.h -- every row is a prototype with as many parameters and the same kind of return value, the
export lists are the table, and every population entry takes the struct its prototype names."""
import ctypes as C
import os
import re

import hydrodl2_amd
from hydrodl2_amd import _abi

RETURNS = {"int": C.c_int, "uint64_t": C.c_uint64, "const char *": C.c_char_p}
POP_STRUCTS = {"hbvx_pop": _abi.Pop, "hbvx_pop_stats": _abi.PopStats, "hbvx_pop_joint": _abi.PopJoint,
               "hbvx_pop_period": _abi.PopPeriod}


def _prototypes():
    """{name: (return type, [parameter, ...])} of every hbvx_* function the two headers declare."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(hydrodl2_amd.__file__)))
    found = {}
    for header in ("hbvx.h", "hbvx_lstm.h"):
        with open(os.path.join(root, "include", header)) as f:
            text = f.read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        for ret, name, args in re.findall(r"^(int|uint64_t|const char \*)\s*(hbvx_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
            assert name not in found, name
            args = " ".join(args.split())
            found[name] = (ret, [] if args == "void" else [a.strip() for a in args.split(",")])
    return found


def test_the_headers_parse():
    protos = _prototypes()
    assert len(protos) == 56
    assert protos["hbvx_version"] == ("int", []) and protos["hbvx_sizeof"] == ("uint64_t", ["int which"])
    assert protos["hbvx_zero_rest"][1] == ["void *ptr", "uint64_t bytes", "const void *zero_state", "void *stream"]


def test_every_row_is_a_prototype_of_the_headers():
    protos = _prototypes()
    names = [row[0] for row in _abi.SIGNATURES]
    assert len(set(names)) == len(names)
    for name, required, restype, argtypes, layout in _abi.SIGNATURES:
        assert name in protos, name
        ret, params = protos[name]
        assert len(params) == len(argtypes), (name, params)
        assert RETURNS[ret] is restype, (name, ret, restype)
        assert isinstance(required, bool)
        if layout is not None:
            which, st = layout
            assert isinstance(which, int) and issubclass(st, C.Structure), name
            assert C.POINTER(st) in argtypes, name


def test_the_export_lists_are_the_table():
    names = [row[0] for row in _abi.SIGNATURES]
    assert sorted(_abi.EXPORTS + _abi.OPTIONAL_EXPORTS) == sorted(names)
    assert not set(_abi.EXPORTS) & set(_abi.OPTIONAL_EXPORTS)
    assert _abi.EXPORTS == [row[0] for row in _abi.SIGNATURES if row[1]]
    assert _abi.OPTIONAL_EXPORTS == [row[0] for row in _abi.SIGNATURES if not row[1]]
    assert isinstance(_abi.EXPORTS, list) and isinstance(_abi.OPTIONAL_EXPORTS, list)
    # a library without one of these used to die with an AttributeError; now it is refused like any other
    assert {"hbvx_zero_in_launch", "hbvx_zero_rest", "hbvx_last_dispatch"} <= set(_abi.EXPORTS)
    # an index of hbvx_sizeof stands for one struct
    structs = {}
    for name, _, _, _, layout in _abi.SIGNATURES:
        if layout is not None:
            assert structs.setdefault(layout[0], layout[1]) is layout[1], name


def test_every_population_entry_takes_the_struct_its_prototype_names():
    protos = _prototypes()
    rows = {row[0]: row for row in _abi.SIGNATURES}
    assert sorted(_abi.POPULATION) == sorted(n for n in protos if "population" in n)
    for entry, info in _abi.POPULATION.items():
        params = protos[entry][1]
        named = re.fullmatch(r"const (hbvx_pop\w*) \*\w+", params[1])
        assert named and POP_STRUCTS[named.group(1)] is info.struct, (entry, params[1])
        _, required, restype, argtypes, layout = rows[entry]
        assert not required and restype is C.c_int
        assert argtypes == [C.POINTER(_abi.Desc), C.POINTER(info.struct), C.c_void_p] and layout[1] is info.struct
        assert info.implicit == entry.startswith("hbvx_adj_")
        assert (info.aux_series is None) == (info.struct in (_abi.Pop, _abi.PopStats))
        assert callable(getattr(_abi.Library, entry[len("hbvx_"):]))
