"""CPU tier of the foreground / mixture selector (``which``): the new entry points are declared, exported, bound and listed
together, the ABI version stays 4, each refuses a null handle and an unknown selector before it could reach a device, and
the Python methods take ``which`` and reject an unknown value with ValueError before they touch a device."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import repet
from repet import _native
from test_abi import HEADER, declared_functions

NEW = ["repet_online_set_output", "repet_online_also_emit", "repet_online_last_emission", "repet_online_last_emission_device",
       "repet_ctx_select_result", "repet_select_run_result"]


def test_new_names_are_declared_exported_and_bound():
    lib = _native.lib()
    declared = declared_functions()
    for name in NEW:
        assert name in declared, f"{name} is not declared in repet_hip.h"
        assert name in _native.EXPORTED_SYMBOLS and name in _native._SIGNATURES
        assert getattr(lib, name).argtypes == _native._SIGNATURES[name][1]
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4


def test_selector_constants_match_the_header():
    text = open(HEADER).read()
    for name, value in (("BACKGROUND", _native.OUT_BACKGROUND), ("FOREGROUND", _native.OUT_FOREGROUND), ("MIXTURE", _native.OUT_MIXTURE)):
        assert int(re.search(rf"#define REPET_OUT_{name}\s+(\d+)", text).group(1)) == value
    assert _native.which_codes("both") == (_native.OUT_BACKGROUND, _native.OUT_FOREGROUND)
    assert [_native.which_codes(w) for w in ("background", "foreground", "mixture")] == [(0,), (1,), (2,)]


def test_null_handles_are_refused():
    lib = _native.lib()
    n = C.c_int64(5)
    strides = (C.c_int64 * 3)(2, 2, 1)
    buf = (C.c_double * 4)()
    assert lib.repet_online_set_output(None, 0) == _native.ERR_BAD_ARG and lib.repet_last_error()
    assert lib.repet_online_also_emit(None, 1, buf, _native.F64, strides) == _native.ERR_BAD_ARG
    assert lib.repet_online_last_emission(None, 1, buf, 4, C.byref(n)) == _native.ERR_BAD_ARG
    assert lib.repet_online_last_emission_device(None, 1, buf, _native.F64, strides, None, C.byref(n)) == _native.ERR_BAD_ARG
    assert lib.repet_ctx_select_result(None, 1) == _native.ERR_BAD_ARG and lib.repet_last_error()


@pytest.mark.parametrize("which", [-1, 3, 99])
def test_unknown_selectors_are_refused(which):
    """Without a device there is no handle to try them on: the one entry that takes none must refuse by value alone, and the
    text must name the selector (the handle forms are tried on a live handle in the GPU tier)."""
    lib = _native.lib()
    assert lib.repet_select_run_result(0, which) == _native.ERR_BAD_ARG
    assert b"which" in lib.repet_last_error()


class NoDevice:
    """Stands where the device handle would be: any use of it is a failure of the order of the checks."""

    def __getattr__(self, name):
        raise AssertionError(f"the handle was used ({name}) before `which` was checked")

    def __bool__(self):
        raise AssertionError("the handle was used before `which` was checked")


def bare(cls):
    h = object.__new__(cls)
    h._h = NoDevice()
    return h


@pytest.mark.parametrize("bad", ["vocals", "", None, 1, "Foreground"])
def test_python_methods_reject_an_unknown_which_before_any_device_work(bad, monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    chunk = np.zeros((3, 100, 2))
    streams, single = bare(_native.OnlineStreams), bare(_native.OnlineSeparator)
    try:
        for call in (lambda: streams.push(chunk, which=bad), lambda: streams.finish(which=bad),
                     lambda: streams.finish_stream(0, which=bad), lambda: streams.last_emission(bad),
                     lambda: single.push(chunk[0], which=bad), lambda: single.finish(which=bad),
                     lambda: repet.separate("sim", chunk, 8000, which=bad)):
            with pytest.raises(ValueError, match="which"):
                call()
    finally:
        streams._h = single._h = None               # (their __del__ must find nothing to close)


def test_which_is_an_argument_with_the_background_as_default():
    for fn in (_native.OnlineStreams.push, _native.OnlineStreams.finish, _native.OnlineStreams.finish_stream,
               _native.OnlineSeparator.push, _native.OnlineSeparator.finish, repet.separate):
        assert inspect.signature(fn).parameters["which"].default == "background", fn
    for name in ("original", "extended", "adaptive", "sim", "simonline"):       # the reference's two-argument signatures stay
        assert list(inspect.signature(getattr(repet, name)).parameters) == ["audio_signal", "sampling_frequency"]


def test_out_pair_checks():
    with pytest.raises(ValueError):
        _native.out_pair(np.zeros(3))
    with pytest.raises(ValueError):
        _native.out_pair((1, 2, 3))
    assert _native.out_pair(None) == (None, None)
