"""CPU tier of ``start_frames`` (separation that starts before the 10-s buffer is full): the three names are exported by the
built library, bound with argument types and listed in the header, each refuses null arguments before any device is touched, and
the Python surface is there. What the calls compute needs a device: tests/test_gpu_online_start.py."""
import ctypes
import inspect
import os

import repet
from repet import _native

NEW_NAMES = ["repet_online_set_start_frames", "repet_online_start_frames", "repet_ctx_set_online_start"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "repet_hip.h")


def test_new_names_are_exported_bound_and_listed():
    lib = _native.lib()
    header = open(HEADER).read()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS and name in _native._SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _native._SIGNATURES[name][1], name
        assert ("int %s(" % name) in header, name
    # additive: the version the existing callers check has not moved
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4
    assert "#define REPET_ABI_VERSION 4" in header


def test_each_refuses_null_arguments():
    lib = _native.lib()
    out = ctypes.c_int32(7)
    assert lib.repet_online_set_start_frames(None, 40) == _native.ERR_BAD_ARG
    assert lib.repet_online_start_frames(None, ctypes.byref(out)) == _native.ERR_BAD_ARG
    assert lib.repet_ctx_set_online_start(None, 40) == _native.ERR_BAD_ARG
    assert lib.repet_last_error()
    assert out.value == 7


def test_start_length_in_frames():
    p = repet.derive_params(8000)
    assert (p.step_length, p.buffer_frames) == (256, 312)
    f = _native.start_frames_for
    assert f(p, 8000, None) is None                                  # the default path makes no call
    assert f(p, 8000, 33 * 256 / 8000) == 33
    assert f(p, 8000, 0.0) == 1 and f(p, 8000, 0.001) == 1          # below one hop
    assert f(p, 8000, 10.0) == 312 and f(p, 8000, 60.0) == 312       # round(312.5) = 312, as buffer_frames; clamped above
    assert f(p, 8000, 2.5 * 256 / 8000) == 2                         # Python's round: half to even


def test_python_surface():
    for fn in (repet.online, repet.online_streams):
        par = inspect.signature(fn).parameters
        assert "start_length" in par and par["start_length"].default is None, fn.__name__
        assert "start_length" in fn.__doc__ and "similarity_distance" in fn.__doc__, fn.__name__
    assert list(inspect.signature(repet.online_streams).parameters)[:4] == [
        "sampling_frequency", "number_channels", "number_streams", "max_push_samples"]
    for cls in (_native.OnlineSeparator, _native.OnlineStreams):
        assert isinstance(inspect.getattr_static(cls, "start_frames"), property), cls.__name__
    assert callable(_native.Context.set_online_start)
    assert not hasattr(repet, "start_length")                        # no new module global
