"""CPU tier of the background gain (a chosen share of the background kept in the foreground): the four entry points are
declared, exported, bound and listed together, the ABI version stays 4, each refuses a null handle or context with a message,
the entry that takes no handle refuses a bad value by the value alone, and the Python layer rejects a bad gain (or a gain
beside a signal it does not change) with ValueError before it touches a device."""
import ctypes as C
import inspect

import numpy as np
import pytest

import repet
from repet import _native
from test_abi import declared_functions
from test_online_foreground_abi import bare

NEW = ["repet_online_set_background_gain", "repet_online_background_gain", "repet_ctx_set_background_gain",
       "repet_set_run_background_gain"]


def test_new_names_are_declared_exported_and_bound():
    lib = _native.lib()
    declared = declared_functions()
    for name in NEW:
        assert name in declared, f"{name} is not declared in repet_hip.h"
        assert name in _native.EXPORTED_SYMBOLS and name in _native._SIGNATURES
        assert getattr(lib, name).argtypes == _native._SIGNATURES[name][1]
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4


def test_null_handles_are_refused_with_a_message():
    lib = _native.lib()
    gains = (C.c_float * 2)(0.5, 0.25)
    slots = (C.c_int32 * 2)(0, 1)
    out = C.c_float(7.0)
    for call in (lambda: lib.repet_online_set_background_gain(None, slots, 2, gains),
                 lambda: lib.repet_online_set_background_gain(None, None, 0, gains),
                 lambda: lib.repet_online_background_gain(None, 0, C.byref(out)),
                 lambda: lib.repet_ctx_set_background_gain(None, 0.5)):
        assert call() == _native.ERR_BAD_ARG
        assert lib.repet_last_error()
    assert out.value == 7.0


@pytest.mark.parametrize("gain", [-0.1, 1.5, float("nan"), float("inf"), float("-inf")])
def test_the_run_form_refuses_a_bad_gain_by_its_value(gain):
    """Without a device there is no context to set it on: the value is checked before one is made."""
    lib = _native.lib()
    assert lib.repet_set_run_background_gain(0, gain) == _native.ERR_BAD_ARG
    assert b"[0, 1]" in lib.repet_last_error()


def test_gain_values_of_the_python_layer():
    g = _native.background_gains(0.25)
    assert g.dtype == np.float32 and g.tolist() == [0.25]
    assert _native.background_gains(0.5, 3).tolist() == [0.5] * 3
    assert _native.background_gains([0.0, 1.0], 2).tolist() == [0.0, 1.0]
    g = _native.background_gains(10 ** (-12 / 20))
    assert g[0] == np.float32(10 ** (-12 / 20))
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "loud", None, [0.5, 0.5]):
        with pytest.raises(ValueError, match="background_gain"):
            _native.background_gains(bad)
    with pytest.raises(ValueError):
        _native.background_gains([0.5, 0.5, 0.5], 2)
    with pytest.raises(ValueError, match="background_gain"):
        _native.background_gains([0.5, 2.0], 2)


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan"), float("inf")])
def test_python_methods_reject_a_bad_gain_before_any_device_work(bad, monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    streams, single, ctx = bare(_native.OnlineStreams), bare(_native.OnlineSeparator), bare(_native.Context)
    streams._streams = 3
    chunk = np.zeros((100, 2))
    try:
        for call in (lambda: streams.set_background_gain(bad), lambda: streams.set_background_gain(bad, slots=[0, 2]),
                     lambda: streams.set_background_gain([0.5, bad], slots=[0, 2]), lambda: single.set_background_gain(bad),
                     lambda: ctx.set_background_gain(bad),
                     lambda: repet.separate("sim", chunk, 8000, which="foreground", background_gain=bad)):
            with pytest.raises(ValueError, match="background_gain"):
                call()
        with pytest.raises(ValueError):
            streams.set_background_gain(0.5, slots=[3])                    # a slot out of range
        with pytest.raises(ValueError):
            streams.set_background_gain([0.5, 0.5, 0.5], slots=[0, 1])     # three values for two slots
    finally:
        streams._h = single._h = ctx._h = None          # (their __del__ must find nothing to close)


@pytest.mark.parametrize("which", ["background", "mixture"])
def test_separate_refuses_a_gain_beside_a_signal_it_does_not_change(which, monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    with pytest.raises(ValueError, match="background_gain"):
        repet.separate("sim", np.zeros((100, 2)), 8000, which=which, background_gain=0.5)


def test_the_gain_is_an_optional_argument_and_the_drop_in_functions_are_unchanged():
    assert inspect.signature(repet.separate).parameters["background_gain"].default is None
    assert inspect.signature(_native.OnlineStreams.set_background_gain).parameters["slots"].default is None
    assert list(inspect.signature(_native.OnlineSeparator.set_background_gain).parameters) == ["self", "gain"]
    for name in ("original", "extended", "adaptive", "sim", "simonline"):
        assert list(inspect.signature(getattr(repet, name)).parameters) == ["audio_signal", "sampling_frequency"]
