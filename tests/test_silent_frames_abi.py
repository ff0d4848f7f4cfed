"""CPU tier of ``silent_frames`` (REPET_FLAG_SILENT_FRAMES_ZERO: live streams and ``simonline`` separated through digital silence
instead of answering it with NaN): the define and the symbol are in the header and the built library, the bit passes the
parameter check and is refused for the four other variants before any device is touched, and the Python keyword refuses what
it must without a GPU. What the rule computes needs a device: tests/test_gpu_silent_frames.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import repet
from repet import _native

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "repet_hip.h")


def test_define_and_symbol():
    lib = _native.lib()
    header = open(HEADER).read()
    assert re.search(r"^#define REPET_FLAG_SILENT_FRAMES_ZERO 4\b", header, flags=re.M)
    assert _native.FLAG_SILENT_FRAMES_ZERO == 4
    assert _native.SILENT_FRAMES == {"reference": 0, "zero": 4}
    name = "repet_silent_frames_supported"
    assert hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS and name in _native._SIGNATURES
    fn = getattr(lib, name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == []
    assert "int %s(void)" % name in header
    assert fn() == 1
    # additive: the version the existing callers check has not moved
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4
    assert "#define REPET_ABI_VERSION 4" in header


def test_the_other_variants_refuse_the_bit_before_any_device():
    """repet_run checks the parameters and the variant before it uploads anything: the refusal needs no device and names the bit."""
    lib = _native.lib()
    x = np.zeros((4096, 2))
    out = np.full((4096, 2), 7.0)
    p = repet.derive_params(8000)
    p.flags |= _native.FLAG_SILENT_FRAMES_ZERO
    for algo in ("original", "extended", "adaptive", "sim"):
        rc = lib.repet_run(_native.ALGO_IDS[algo], _native.ptr(x), _native.F64, 4096, 2, p, _native.ptr(out), 10 ** 6, None)
        assert rc == _native.ERR_BAD_ARG and b"REPET_FLAG_SILENT_FRAMES_ZERO" in lib.repet_last_error(), algo
        assert (out == 7.0).all()
    # simonline takes it: the call gets as far as the device, which does not exist
    rc = lib.repet_run(_native.ALGO_IDS["simonline"], _native.ptr(x), _native.F64, 4096, 2, p, _native.ptr(out), 10 ** 6, None)
    assert rc != 0 and b"REPET_FLAG_SILENT_FRAMES_ZERO" not in lib.repet_last_error() and b"unknown bits" not in lib.repet_last_error()
    p.flags |= 8                                                     # an unknown bit is still unknown
    rc = lib.repet_run(_native.ALGO_IDS["simonline"], _native.ptr(x), _native.F64, 4096, 2, p, _native.ptr(out), 10 ** 6, None)
    assert rc == _native.ERR_BAD_ARG and b"unknown bits" in lib.repet_last_error()
    assert (out == 7.0).all()


def test_keyword_values():
    f = _native.silent_frames_flag
    assert f("reference") == 0 and f("zero") == 4
    assert f("reference", "sim") == 0 and f("zero", "simonline") == 4
    for bad in ("Zero", "nan", "", None, 0, 4, True):
        with pytest.raises(ValueError, match="silent_frames"):
            f(bad)
    for algo in ("original", "extended", "adaptive", "sim"):
        with pytest.raises(ValueError, match="simonline"):
            f("zero", algo)


def test_python_surface_and_refusals_without_a_device():
    for fn in (repet.online, repet.online_streams, repet.separate):
        par = inspect.signature(fn).parameters
        assert "silent_frames" in par and par["silent_frames"].default == "reference", fn.__name__
        # appended -- in `separate` in front of the band-gain pair, which stays last: all three are passed by keyword
        assert list(par)[-1 if fn is not repet.separate else -3] == "silent_frames", fn.__name__
        assert "silent_frames" in fn.__doc__, fn.__name__
    for cls in (_native.OnlineSeparator, _native.OnlineStreams):
        assert isinstance(inspect.getattr_static(cls, "silent_frames"), property), cls.__name__
    assert not hasattr(repet, "silent_frames")                       # no new module global
    assert "silent_frames" not in inspect.signature(repet.simonline).parameters
    assert repet.derive_params(8000).flags & _native.FLAG_SILENT_FRAMES_ZERO == 0
    x = np.zeros((4096, 2))                                          # not a tensor: the keyword is judged first
    with pytest.raises(ValueError, match="simonline"):
        repet.separate("sim", x, 8000, silent_frames="zero")
    with pytest.raises(ValueError, match="silent_frames"):
        repet.separate("simonline", x, 8000, silent_frames="mute")
    # band gains passed as the ninth positional argument of `separate`, where the new keyword now sits: told what to do
    with pytest.raises(ValueError, match="background_band_gains and band_edges of repet.separate by keyword"):
        repet.separate("sim", x, 8000, None, "foreground", None, False, None, np.zeros(257, dtype=np.float32))
    with pytest.raises(ValueError, match="silent_frames"):
        repet.online(8000, 2, silent_frames="mute")
    with pytest.raises(ValueError, match="silent_frames"):
        repet.online_streams(8000, 2, 3, silent_frames=None)
