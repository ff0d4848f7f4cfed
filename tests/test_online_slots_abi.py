"""CPU tier of the per-slot lifecycle of the many-stream streaming handle (restart / release / finish_stream of single
slots): the five names are exported, bound with argument types and listed, and each refuses a null handle before any device
is touched. What the calls compute needs a handle, hence a device: tests/test_gpu_online_slots.py."""
import ctypes

import repet
from repet import _native

NEW_NAMES = ["repet_online_restart_streams", "repet_online_release_streams", "repet_online_stream_emit_count",
             "repet_online_finish_stream", "repet_online_finish_stream_device"]


def test_new_names_are_exported_bound_and_listed():
    lib = _native.lib()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name
    # additive: the version the existing callers check has not moved
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4


def test_each_refuses_a_null_handle():
    lib = _native.lib()
    n = ctypes.c_int64(7)
    slots = (ctypes.c_int32 * 2)(0, 1)
    strides = (ctypes.c_int64 * 2)(2, 1)
    assert lib.repet_online_restart_streams(None, slots, 2) == _native.ERR_BAD_ARG
    assert lib.repet_online_release_streams(None, slots, 2) == _native.ERR_BAD_ARG
    assert lib.repet_online_stream_emit_count(None, 0, ctypes.byref(n)) == _native.ERR_BAD_ARG
    assert lib.repet_online_finish_stream(None, 0, None, 0, ctypes.byref(n)) == _native.ERR_BAD_ARG
    assert lib.repet_online_finish_stream_device(None, 0, None, _native.F64, strides, None, ctypes.byref(n)) == _native.ERR_BAD_ARG
    assert lib.repet_last_error()


def test_python_surface():
    for name in ("restart", "release", "finish_stream", "stream_emit_count", "stream_samples", "samples_pushed"):
        assert hasattr(_native.OnlineStreams, name), name
    assert "restart" in repet.online_streams.__doc__ and "finish_stream" in repet.online_streams.__doc__
