"""CPU tier of the many-stream streaming handle (repet_online_open_streams and its companions): the new names are exported
and bound, and the handle refuses bad arguments before it opens a device. The arithmetic of repet_online_emit_count needs
a handle, hence a device: tests/test_gpu_online_streams.py runs it."""
import ctypes

import pytest

import repet
from repet import _native

NEW_NAMES = ["repet_online_open_streams", "repet_online_emit_count", "repet_online_push_streams", "repet_online_push_device",
             "repet_online_finish_streams", "repet_online_finish_device"]


def test_new_names_are_exported_and_bound():
    lib = _native.lib()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS, name
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4
    assert callable(repet.online_streams)


def open_streams(n_streams, n_channels, params, max_push=0):
    h = ctypes.c_void_p()
    rc = _native.lib().repet_online_open_streams(0, n_streams, n_channels, ctypes.byref(params), max_push, ctypes.byref(h))
    return rc, h


@pytest.mark.parametrize("n_streams,n_channels", [(0, 2), (-3, 2), (4, 0), (4, -1), (0, 0)])
def test_open_refuses_counts_before_a_device(n_streams, n_channels):
    rc, h = open_streams(n_streams, n_channels, repet.derive_params(8000))
    assert rc == _native.ERR_BAD_ARG and not h.value
    assert b"at least one" in _native.lib().repet_last_error() or b"streams" in _native.lib().repet_last_error()


@pytest.mark.parametrize("field,value", [("step_length", 100), ("buffer_frames", 1), ("sim_number", 0),
                                         ("sim_distance_frames", -1), ("flags", 1 << 7)])
def test_open_refuses_bad_parameters_before_a_device(field, value):
    p = repet.derive_params(8000)
    setattr(p, field, value)
    rc, h = open_streams(4, 2, p)
    assert rc == _native.ERR_BAD_ARG and not h.value


def test_open_refuses_a_negative_push_size_and_null_arguments():
    lib = _native.lib()
    rc, h = open_streams(2, 2, repet.derive_params(8000), max_push=-1)
    assert rc == _native.ERR_BAD_ARG and not h.value
    p = repet.derive_params(8000)
    assert lib.repet_online_open_streams(0, 2, 2, ctypes.byref(p), 0, None) == _native.ERR_BAD_ARG
    assert lib.repet_online_open_streams(0, 2, 2, None, 0, ctypes.byref(ctypes.c_void_p())) == _native.ERR_BAD_ARG
    n = ctypes.c_int64()
    assert lib.repet_online_emit_count(None, 10, 0, ctypes.byref(n)) == _native.ERR_BAD_ARG
    assert lib.repet_online_push_streams(None, None, _native.F32, 0, None, 0, ctypes.byref(n)) == _native.ERR_BAD_ARG
    assert lib.repet_online_finish_streams(None, None, 0, ctypes.byref(n)) == _native.ERR_BAD_ARG


def test_python_constructor_refuses_counts():
    with pytest.raises(ValueError):
        repet.online_streams(8000, 2, 0)
    with pytest.raises(ValueError):
        repet.online_streams(8000, 0, 4)
