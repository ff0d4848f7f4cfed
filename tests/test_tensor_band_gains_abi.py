"""CPU tier of the tensor calls' band gains (a share of the background kept band by band in the foreground of
``repet.separate`` and of a ``Context``): the three entry points are declared, exported, bound and listed together, the ABI version
stays 4, each refuses a null context with a message, and the Python layer rejects bad gains, bad edges, a wrong size or another
``which`` with ValueError before it touches the library."""
import ctypes as C
import inspect

import numpy as np
import pytest

import repet
from repet import _native
from test_abi import declared_functions
from test_online_foreground_abi import bare

NEW = ["repet_ctx_set_background_band_gains", "repet_ctx_background_band_gains", "repet_set_run_background_band_gains"]
F = 257


def test_new_names_are_declared_exported_and_bound():
    lib = _native.lib()
    declared = declared_functions()
    for name in NEW:
        assert name in declared, f"{name} is not declared in repet_hip.h"
        assert name in _native.EXPORTED_SYMBOLS and name in _native._SIGNATURES
        assert getattr(lib, name).argtypes == _native._SIGNATURES[name][1]
    assert [len(_native._SIGNATURES[name][1]) for name in NEW] == [6, 4, 6]
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4


def test_a_null_context_is_refused_with_a_message():
    lib = _native.lib()
    gains = (C.c_float * 2)(0.5, 0.25)
    edges = (C.c_int32 * 3)(0, 4, 9)
    out = (C.c_float * F)(*([7.0] * F))
    for call in (lambda: lib.repet_ctx_set_background_band_gains(None, 512, edges, 2, gains, 1),
                 lambda: lib.repet_ctx_set_background_band_gains(None, 512, None, 0, None, 0),
                 lambda: lib.repet_ctx_background_band_gains(None, 0, out, F)):
        assert call() == _native.ERR_BAD_ARG
        assert lib.repet_last_error()
    assert list(out) == [7.0] * F


class FakeTensor:
    """Enough of a tensor for the checks that come before the library: a shape."""
    def __init__(self, *shape):
        self.shape = shape


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan"), float("inf")])
def test_python_rejects_bad_arguments_before_the_library_is_touched(bad, monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    monkeypatch.setattr(_native, "is_device_tensor", lambda x: (_ for _ in ()).throw(AssertionError("the tensor was looked at")))
    x, batch = FakeTensor(4000, 2), FakeTensor(3, 4000, 2)
    fs = 8000                                                                      # W = 512, F = 257
    for kw in (dict(background_band_gains=[0.5, bad], band_edges=[0, 4, 9]),
               dict(background_band_gains=np.full(F, bad)),
               dict(background_band_gains=[[0.5, 0.5], [0.5, bad], [0.0, 0.0]], band_edges=[0, 4, 9])):
        with pytest.raises(ValueError, match="band gains"):
            repet.separate("sim", batch, fs, which="foreground", **kw)
    ctx = bare(_native.Context)
    try:
        for call in (lambda: ctx.set_background_band_gains([0.5, bad], [0, 4, 9], window_length=512),
                     lambda: ctx.set_background_band_gains(np.full(F, bad), window_length=512)):
            with pytest.raises(ValueError, match="band gains"):
                call()
        for kw in (dict(gains=[0.5, 0.5], edges=[4, 0, 9], window_length=512),      # edges that descend
                   dict(gains=[0.5, 0.5], edges=[0, 4, F + 1], window_length=512),  # an edge past the last bin
                   dict(gains=np.zeros(F), window_length=1024),                     # per bin, for another window
                   dict(gains=np.zeros(F)),                                         # no window length
                   dict(gains=np.zeros(F), window_length=500),
                   dict(gains=np.zeros((1, 1, F)), window_length=512)):
            with pytest.raises(ValueError):
                ctx.set_background_band_gains(**kw)
        assert ctx.background_band_gains() is None
    finally:
        ctx._h = None                          # (its __del__ must find nothing to close)
    for kw in (dict(background_band_gains=[0.5], band_edges=[0, 4, 9]),            # one gain for two bands
               dict(background_band_gains=np.zeros(F - 1)),                        # per bin, one short
               dict(background_band_gains=np.zeros((2, F))),                       # rows without a batch
               dict(background_band_gains=[0.5, 0.5], band_edges=[4, 0, 9]),
               dict(background_band_gains=[0.5, 0.5], band_edges=[0, 4, F + 1]),
               dict(band_edges=[0, 4, 9])):                                        # edges without gains
        with pytest.raises(ValueError):
            repet.separate("sim", x, fs, which="foreground", **kw)
    with pytest.raises(ValueError, match="band gains"):
        repet.separate("sim", batch, fs, which="both", background_band_gains=np.zeros((2, F)))      # two rows, three clips
    for which in ("background", "mixture"):
        with pytest.raises(ValueError, match="which"):
            repet.separate("sim", x, fs, which=which, background_band_gains=np.zeros(F))


def test_host_arrays_are_not_taken():
    with pytest.raises(TypeError):
        repet.separate("sim", np.zeros((4000, 2)), 8000, which="foreground", background_band_gains=np.zeros(F))


def test_signatures():
    p = inspect.signature(repet.separate).parameters
    assert list(p)[-2:] == ["background_band_gains", "band_edges"]
    assert p["background_band_gains"].default is None and p["band_edges"].default is None
    p = inspect.signature(_native.Context.set_background_band_gains).parameters
    assert list(p) == ["self", "gains", "edges", "window_length"] and p["edges"].default is None
    p = inspect.signature(_native.Context.background_band_gains).parameters
    assert list(p) == ["self", "clip"] and p["clip"].default == 0
    assert list(inspect.signature(_native.Context.clear_background_band_gains).parameters) == ["self"]
