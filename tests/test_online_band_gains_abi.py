"""CPU tier of the band gains (a share of the background kept band by band in the foreground of the live handles): the two entry
points are declared, exported, bound and listed together, the ABI version stays 4, each refuses a null handle with a message,
and the Python layer rejects bad gains, bad edges, a wrong size or a bad slot with ValueError before it touches the library."""
import ctypes as C
import inspect

import numpy as np
import pytest

from repet import _native
from test_abi import declared_functions
from test_online_foreground_abi import bare

NEW = ["repet_online_set_background_band_gains", "repet_online_background_band_gains"]
F = 257


def test_new_names_are_declared_exported_and_bound():
    lib = _native.lib()
    declared = declared_functions()
    for name in NEW:
        assert name in declared, f"{name} is not declared in repet_hip.h"
        assert name in _native.EXPORTED_SYMBOLS and name in _native._SIGNATURES
        assert getattr(lib, name).argtypes == _native._SIGNATURES[name][1]
    assert len(_native._SIGNATURES[NEW[0]][1]) == 7 and len(_native._SIGNATURES[NEW[1]][1]) == 4
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4


def test_null_handles_are_refused_with_a_message():
    lib = _native.lib()
    gains = (C.c_float * 2)(0.5, 0.25)
    edges = (C.c_int32 * 3)(0, 4, 9)
    slots = (C.c_int32 * 2)(0, 1)
    out = (C.c_float * F)(*([7.0] * F))
    for call in (lambda: lib.repet_online_set_background_band_gains(None, slots, 2, edges, 2, gains, 1),
                 lambda: lib.repet_online_set_background_band_gains(None, None, 0, edges, 2, gains, 1),
                 lambda: lib.repet_online_background_band_gains(None, 0, out, F)):
        assert call() == _native.ERR_BAD_ARG
        assert lib.repet_last_error()
    assert list(out) == [7.0] * F


def test_gain_rows_of_the_python_layer():
    edges, g = _native.band_gain_rows([0.25, 1.0], [0, 4, 9], F)
    assert edges.dtype == np.int32 and edges.tolist() == [0, 4, 9] and g.dtype == np.float32 and g.tolist() == [[0.25, 1.0]]
    edges, g = _native.band_gain_rows(np.full(F, 0.5), None, F)
    assert edges is None and g.shape == (1, F)
    edges, g = _native.band_gain_rows([[0.0, 1.0], [0.5, 0.5], [1.0, 0.0]], [3, 3, F], F, 3)
    assert g.shape == (3, 2) and g.flags["C_CONTIGUOUS"]
    assert _native.band_gain_rows(np.zeros(F), range(F + 1), F)[1].shape == (1, F)          # one band per bin: the most
    assert _native.band_gain_rows([10 ** (-12 / 20)], [0, F], F)[1][0, 0] == np.float32(10 ** (-12 / 20))
    for bad in ([-0.1, 0.5], [0.5, 1.5], [float("nan"), 0.0], [float("inf"), 0.0], ["loud", 0.0]):
        with pytest.raises(ValueError, match="band gains"):
            _native.band_gain_rows(bad, [0, 4, 9], F)
    for gains, edges, count in (([0.5], [0, 4, 9], None),                  # one gain for two bands
                                ([0.5, 0.5, 0.5], [0, 4, 9], None),
                                (np.zeros(F - 1), None, None),             # per bin, one short
                                (np.zeros((2, 2)), [0, 4, 9], 3),          # two rows for three slots
                                (np.zeros((2, 2)), [0, 4, 9], None),       # rows where there are no slots to name
                                (np.zeros((1, 1, 2)), [0, 4, 9], None)):
        with pytest.raises(ValueError, match="band gains"):
            _native.band_gain_rows(gains, edges, F, count)
    for edges in ([4, 0, 9], [-1, 4, 9], [0, 4, F + 1], [0.0, 4.0, 9.0], [4], "low", list(range(F + 2))):
        with pytest.raises(ValueError):
            _native.band_gain_rows(np.zeros(max(len(edges) - 1, 1)), edges, F)


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan"), float("inf")])
def test_python_methods_reject_bad_arguments_before_the_library_is_touched(bad, monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    streams, single = bare(_native.OnlineStreams), bare(_native.OnlineSeparator)
    streams._streams = 3
    streams._bins = single._bins = F
    try:
        for call in (lambda: streams.set_background_band_gains([0.5, bad], [0, 4, 9]),
                     lambda: streams.set_background_band_gains([0.5, bad], [0, 4, 9], slots=[0, 2]),
                     lambda: streams.set_background_band_gains([[0.5, 0.5], [0.5, bad]], [0, 4, 9], slots=[0, 2]),
                     lambda: streams.set_background_band_gains(np.full(F, bad)),
                     lambda: single.set_background_band_gains([0.5, bad], [0, 4, 9]),
                     lambda: single.set_background_band_gains(np.full(F, bad))):
            with pytest.raises(ValueError, match="band gains"):
                call()
        with pytest.raises(ValueError):
            streams.set_background_band_gains([0.5, 0.5], [0, 4, 9], slots=[3])             # a slot out of range
        with pytest.raises(ValueError):
            streams.clear_background_band_gains(slots=[-1])
        with pytest.raises(ValueError):
            streams.background_band_gains(3)
        with pytest.raises(ValueError):
            streams.set_background_band_gains(np.zeros((3, 2)), [0, 4, 9], slots=[0, 1])    # three rows for two slots
        with pytest.raises(ValueError):
            streams.set_background_band_gains([0.5, 0.5], [4, 0, 9])                        # edges that descend
        with pytest.raises(ValueError):
            single.set_background_band_gains([0.5, 0.5], [0, 4, F + 1])                     # an edge past the last bin
    finally:
        streams._h = single._h = None          # (their __del__ must find nothing to close)


def test_signatures():
    p = inspect.signature(_native.OnlineStreams.set_background_band_gains).parameters
    assert list(p) == ["self", "gains", "edges", "slots"] and p["edges"].default is None and p["slots"].default is None
    assert list(inspect.signature(_native.OnlineStreams.background_band_gains).parameters) == ["self", "slot"]
    assert inspect.signature(_native.OnlineStreams.clear_background_band_gains).parameters["slots"].default is None
    assert list(inspect.signature(_native.OnlineSeparator.set_background_band_gains).parameters) == ["self", "gains", "edges"]
    assert list(inspect.signature(_native.OnlineSeparator.background_band_gains).parameters) == ["self"]
    assert list(inspect.signature(_native.OnlineSeparator.clear_background_band_gains).parameters) == ["self"]
