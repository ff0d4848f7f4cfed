"""CPU tier of the matches calls (the similar frames a live handle matched): the three entry points are declared in the header
with the documented signatures, exported, bound and listed, the ABI version stays 4, each refuses a null handle with a message
and leaves its destinations alone, and the Python layer has the documented surface."""
import ctypes as C
import inspect
import re

import numpy as np

import repet
from repet import _native
from test_abi import HEADER, declared_functions

P, I64P = C.c_void_p, C.POINTER(C.c_int64)
SIGNATURES = {
    "repet_online_match_capacity": ("repet_online* h, int32_t* capacity", [P, C.POINTER(C.c_int32)]),
    "repet_online_last_matches": ("repet_online* h, int32_t* count_out, int32_t* age_out, float* similarity_out, "
                                  "int64_t capacity_rows, int64_t* n_rows", [P, P, P, P, C.c_int64, I64P]),
    "repet_online_last_matches_device": ("repet_online* h, void* count_dst, void* age_dst, void* similarity_dst, void* signal_stream",
                                         [P, P, P, P, P]),
}


def test_new_names_are_declared_exported_and_bound():
    lib = _native.lib()
    declared = declared_functions()
    for name, (_, argtypes) in SIGNATURES.items():
        assert name in declared, f"{name} is not declared in repet_hip.h"
        assert name in _native.EXPORTED_SYMBOLS and name in _native._SIGNATURES
        assert getattr(lib, name).argtypes == _native._SIGNATURES[name][1] == argtypes
        assert getattr(lib, name).restype is C.c_int
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4


def test_the_header_declares_the_documented_signatures():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (args, _) in SIGNATURES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} has no declaration returning int"
        assert re.sub(r"\s+", " ", m.group(1)).strip() == args, name


def test_null_handles_are_refused_with_a_message():
    lib = _native.lib()
    count, age = np.full(4, 7, dtype=np.int32), np.full(16, 7, dtype=np.int32)
    sim = np.full(16, 7.0, dtype=np.float32)
    k, rows = C.c_int32(5), C.c_int64(6)
    for call in (lambda: lib.repet_online_match_capacity(None, C.byref(k)),
                 lambda: lib.repet_online_last_matches(None, _native.ptr(count), _native.ptr(age), _native.ptr(sim), 4, C.byref(rows)),
                 lambda: lib.repet_online_last_matches(None, None, None, None, 0, C.byref(rows)),
                 lambda: lib.repet_online_last_matches_device(None, _native.ptr(count), _native.ptr(age), _native.ptr(sim), None)):
        assert call() == _native.ERR_BAD_ARG
        assert lib.repet_last_error()
    assert (count == 7).all() and (age == 7).all() and (sim == 7.0).all() and (k.value, rows.value) == (5, 6)


def test_python_surface():
    for cls in (_native.OnlineStreams, _native.OnlineSeparator):
        params = inspect.signature(cls.last_matches).parameters
        assert list(params) == ["self", "out"] and params["out"].default is None
        assert isinstance(inspect.getattr_static(cls, "match_capacity"), property)
    assert repet.Matches is _native.Matches and repet.Matches._fields == ("count", "age", "similarity")
    assert tuple(repet.Matches(1, 2, 3)) == (1, 2, 3)
    for text in (repet.online_streams.__doc__, repet.online.__doc__):
        assert "last_matches" in text and "match_capacity" in text
