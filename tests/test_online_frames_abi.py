"""CPU tier of the frames calls (the spectra of a live handle's last frames, whole or in bands): the five entry points are
declared in the header with the documented signatures, exported, bound and listed, the ABI version stays 4, each refuses a
null handle with a message and leaves its destinations alone, and the Python layer refuses what it can before the library is
called."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import repet
from repet import _native
from test_abi import HEADER, declared_functions

P, I64P = C.c_void_p, C.POINTER(C.c_int64)
SIGNATURES = {
    "repet_online_last_frame_range": ("repet_online* h, int64_t* first_frame, int64_t* n_frames", [P, I64P, I64P]),
    "repet_online_last_frames": ("repet_online* h, int which, float* out, int64_t capacity_floats, int64_t* n_written",
                                 [P, C.c_int, P, C.c_int64, I64P]),
    "repet_online_last_frames_device": ("repet_online* h, int which, void* dst, const int64_t dst_strides[4], void* signal_stream",
                                        [P, C.c_int, P, P, P]),
    "repet_online_last_band_energies": ("repet_online* h, int which, const int32_t* edges, int32_t n_bands, "
                                        "double* out, int64_t capacity_doubles, int64_t* n_written",
                                        [P, C.c_int, P, C.c_int32, P, C.c_int64, I64P]),
    "repet_online_last_band_energies_device": ("repet_online* h, int which, const int32_t* edges, int32_t n_bands, "
                                               "void* dst, void* signal_stream", [P, C.c_int, P, C.c_int32, P, P]),
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
    assert re.search(r"^#define REPET_MAX_BANDS 128\b", open(HEADER).read(), flags=re.M)


def test_null_handles_are_refused_with_a_message():
    lib = _native.lib()
    out = np.full(16, 7.0)
    edges = np.array([0, 1, 2], dtype=np.int32)
    strides = (C.c_int64 * 4)(8, 4, 2, 1)
    a, b = C.c_int64(5), C.c_int64(6)
    for call in (lambda: lib.repet_online_last_frame_range(None, C.byref(a), C.byref(b)),
                 lambda: lib.repet_online_last_frames(None, 1, _native.ptr(out), out.size, C.byref(a)),
                 lambda: lib.repet_online_last_frames(None, 1, None, 0, C.byref(a)),
                 lambda: lib.repet_online_last_frames_device(None, 1, _native.ptr(out), strides, None),
                 lambda: lib.repet_online_last_band_energies(None, 1, _native.ptr(edges), 2, _native.ptr(out), out.size, C.byref(a)),
                 lambda: lib.repet_online_last_band_energies_device(None, 1, _native.ptr(edges), 2, _native.ptr(out), None)):
        assert call() == _native.ERR_BAD_ARG
        assert lib.repet_last_error()
    assert (out == 7.0).all() and (a.value, b.value) == (5, 6)


def test_python_surface(monkeypatch):
    for cls in (_native.OnlineStreams, _native.OnlineSeparator):
        params = inspect.signature(cls.last_frames).parameters
        assert list(params) == ["self", "which", "bands", "out"]
        assert (params["which"].default, params["bands"].default, params["out"].default) == ("foreground", None, None)
        assert isinstance(inspect.getattr_static(cls, "last_frame_range"), property)
    assert list(inspect.signature(repet.band_edges).parameters) == ["sampling_frequency", "number_bands", "f_min", "f_max"]
    for text in (repet.online_streams.__doc__, repet.online.__doc__):
        assert "last_frames" in text
    # what the Python layer can refuse is refused before the library is called
    monkeypatch.setattr(_native, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    for bands in ([0], [0.0, 4.0], "ab", [[0, 1], [1, 2]], [0, 2 ** 40], None):
        with pytest.raises(ValueError):
            _native._last_frames(None, 0, ((1,), 1), 257, "both" if bands is None else "foreground", bands, None, False)
    assert _native.band_edge_array([0, 3, 3, 257]).dtype == np.int32
    assert _native.band_edge_array(np.array([5, 9], dtype=np.int64)).tolist() == [5, 9]
