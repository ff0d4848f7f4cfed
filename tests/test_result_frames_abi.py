"""CPU tier of the spectra of a tensor call (``repet.separate(..., frames=...)``; include/repet_hip.h: repet_ctx_request_frames):
the entry points are declared, exported and bound and the ABI version stays 4; the frame count is host arithmetic that agrees
with the oracle's; every refusal the Python call makes happens on the host -- with host tensors, on a machine without a device,
a refusal that touched one would be another error --; ``inspect.signature(repet.separate)`` is what it was."""
import ctypes as C
import inspect

import numpy as np
import pytest

import repet
from oracle import repet_oracle as orc
from repet import _native
from test_abi import declared_functions

NEW = ["repet_ctx_request_frames", "repet_ctx_clear_requests", "repet_result_frame_count", "repet_ctx_last_spectrum_form"]
FS = 8000


def test_new_names_are_declared_exported_and_bound():
    lib = _native.lib()
    declared = declared_functions()
    for name in NEW:
        assert name in declared, f"{name} is not declared in repet_hip.h"
        assert name in _native.EXPORTED_SYMBOLS and name in _native._SIGNATURES
        assert getattr(lib, name).argtypes == _native._SIGNATURES[name][1]
    P = C.c_void_p
    assert _native._SIGNATURES[NEW[0]] == (C.c_int, [P, C.c_int, P, C.c_int32, P, P, P])
    assert _native._SIGNATURES[NEW[2]] == (C.c_int64, [C.c_int, C.POINTER(_native.Params), C.c_int64])
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4                      # additions: the version stays
    assert _native.MAX_BANDS == 128


def test_null_arguments_are_refused_with_a_message():
    lib = _native.lib()
    v = C.c_int32(7)
    strides = (C.c_int64 * 4)(1, 1, 1, 1)
    assert lib.repet_ctx_request_frames(None, 0, None, 0, None, strides, None) == _native.ERR_BAD_ARG and lib.repet_last_error()
    assert lib.repet_ctx_clear_requests(None) == _native.ERR_BAD_ARG and lib.repet_last_error()
    assert lib.repet_ctx_last_spectrum_form(None, C.byref(v)) == _native.ERR_BAD_ARG and lib.repet_last_error()
    assert v.value == 7
    assert lib.repet_result_frame_count(_native.ALGO_IDS["sim"], None, 1000) == -1


@pytest.mark.parametrize("fs", (8000, 44100, 192000))
def test_frame_count_is_the_oracles_without_a_device(fs):
    w, _, h = orc.stft_geometry(fs)
    for n in (0, 1, h - 1, h, w - 1, w, w + 1, 3 * w + 5, int(4.3 * fs), 12 * fs):
        for algo in ("original", "adaptive", "sim"):
            assert repet.frame_count(algo, n, fs) == orc.centred_frame_count(n, w, h) == -(-n // h) + 1
        if n >= w:
            assert repet.frame_count("simonline", n, fs) == orc.online_frame_count(n, w, h)
    with pytest.raises(ValueError):
        repet.frame_count("extended", 12 * fs, fs)
    with pytest.raises(ValueError):
        repet.frame_count("median", 12 * fs, fs)
    with pytest.raises(ValueError):
        repet.frame_count("sim", -1, fs)


def test_the_published_signature_of_separate_is_unchanged():
    names = list(inspect.signature(repet.separate).parameters)
    assert names == ["algo", "audio_signal", "sampling_frequency", "out", "which", "background_gain", "levels", "dtype", "silent_frames",
                     "background_band_gains", "band_edges"]
    for word in ("frames", "frame_bands", "frames_out", "repet.frame_count"):
        assert word in repet.separate.__doc__
    p = inspect.signature(_native.Context.request_frames).parameters
    assert list(p) == ["self", "algo", "params", "which", "out", "bands", "stream"]
    assert isinstance(inspect.getattr_static(_native.Context, "last_spectrum_form"), property)
    assert callable(_native.Context.clear_requests)


def test_every_refusal_happens_on_the_host():
    torch = pytest.importorskip("torch")
    n = 4 * FS
    x = torch.zeros(n, 2, dtype=torch.float64)                       # a HOST tensor: a call that got past the checks is a TypeError
    batch = torch.zeros(3, n, 2, dtype=torch.float64)
    f = repet.derive_params(FS).window_length // 2 + 1
    t = repet.frame_count("sim", n, FS)
    edges = repet.band_edges(FS, 8)

    def refused(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            repet.separate(*args, **kw)

    refused("frames is", "sim", x, FS, frames="median")
    refused("frames is", "sim", x, FS, frames=1)
    refused("go with frames", "sim", x, FS, frame_bands=edges)
    refused("go with frames", "sim", x, FS, frames_out=torch.zeros(t, 2, f))
    refused("extended", "extended", x, FS, frames="background")
    # edges, by the live checks: integers, ascending, inside [0, F], at most REPET_MAX_BANDS bands
    refused("bands", "sim", x, FS, frames="background", frame_bands=[0.0, 4.5])
    refused("bands", "sim", x, FS, frames="background", frame_bands=[3])
    refused("band edges", "sim", x, FS, frames="background", frame_bands=[0, 9, 5])
    refused("band edges", "sim", x, FS, frames="background", frame_bands=[-1, 5])
    refused("band edges", "sim", x, FS, frames="background", frame_bands=[0, f + 1])
    refused("at most 128", "sim", x, FS, frames="background", frame_bands=list(range(130)))
    # the destination: shape, dtype, device, density
    refused("shape", "sim", x, FS, frames="background", frames_out=torch.zeros(t + 1, 2, f))
    refused("shape", "sim", batch, FS, frames="background", frames_out=torch.zeros(t, 2, f))
    refused("shape", "simonline", x, FS, frames="background", frames_out=torch.zeros(t, 2, f))     # the online grid is another
    refused("float32", "sim", x, FS, frames="background", frames_out=torch.zeros(t, 2, f, dtype=torch.float64))
    refused("float64", "sim", x, FS, frames="background", frame_bands=edges, frames_out=torch.zeros(t, 2, 8))
    refused("dense", "sim", x, FS, frames="background", frame_bands=edges,
            frames_out=torch.zeros(t, 8, 2, dtype=torch.float64).transpose(1, 2))
    refused("tensor", "sim", x, FS, frames="background", frames_out=np.zeros((t, 2, f), dtype=np.float32))
    refused("must be a tensor on", "sim", x, FS, frames="background", frames_out=torch.zeros(t, 2, f, device="meta"))
    # and a request that passes every check reaches the call itself, which takes device tensors only
    with pytest.raises(TypeError):
        repet.separate("sim", x, FS, frames="background", frame_bands=edges, frames_out=torch.zeros(t, 2, 8, dtype=torch.float64))
