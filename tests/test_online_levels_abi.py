"""CPU tier of the level records (what a live handle or a tensor call emitted, reduced on the device): the three entry points
are declared, exported, bound and listed, the ABI version stays 4, each refuses a null handle or context with a message and
leaves the destination alone, the field names of the header and of ``repet.LEVELS`` agree, ``repet.separate(..., levels=True)``
still takes device tensors only, and the NumPy reference the GPU tier measures against is right on hand-made cases."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import repet
from repet import _native
from levels_reference import check, levels
from test_abi import HEADER, declared_functions

NEW = ["repet_online_last_levels", "repet_online_last_levels_device", "repet_ctx_result_levels_device"]


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
    out = np.full(16, 7.0)
    n = C.c_int64(5)
    for call in (lambda: lib.repet_online_last_levels(None, _native.ptr(out), out.size, C.byref(n)),
                 lambda: lib.repet_online_last_levels(None, None, 0, C.byref(n)),
                 lambda: lib.repet_online_last_levels_device(None, _native.ptr(out), None),
                 lambda: lib.repet_ctx_result_levels_device(None, _native.ptr(out), None)):
        assert call() == _native.ERR_BAD_ARG
        assert lib.repet_last_error()
    assert (out == 7.0).all() and n.value == 5


def header_defines():
    text = open(HEADER).read()
    return {k: int(v) for k, v in re.findall(r"^#define (REPET_LEVEL_[A-Z_]+) (\d+)", text, flags=re.M)}


def test_field_names_of_the_header_and_of_the_package():
    d = header_defines()
    assert d["REPET_LEVEL_FIELDS"] == 8 == len(repet.LEVELS) == _native.LEVEL_FIELDS
    order = ["REPET_LEVEL_MIX_ENERGY", "REPET_LEVEL_BG_ENERGY", "REPET_LEVEL_FG_ENERGY", "REPET_LEVEL_MIX_PEAK",
             "REPET_LEVEL_BG_PEAK", "REPET_LEVEL_FG_PEAK", "REPET_LEVEL_LIVE", "REPET_LEVEL_NONFINITE"]
    assert [d[name] for name in order] == list(range(8))
    assert repet.LEVELS == ("mixture_energy", "background_energy", "foreground_energy", "mixture_peak", "background_peak",
                            "foreground_peak", "live_samples", "nonfinite_samples")
    assert isinstance(repet.LEVELS, tuple) and len(set(repet.LEVELS)) == 8
    assert d["REPET_LEVEL_CHUNK"] == _native.LEVEL_CHUNK > 0


def test_levels_is_an_optional_argument_and_separate_still_takes_device_tensors_only(monkeypatch):
    assert inspect.signature(repet.separate).parameters["levels"].default is False
    assert inspect.signature(_native.OnlineStreams.last_levels).parameters["out"].default is None
    assert list(inspect.signature(_native.OnlineSeparator.last_levels).parameters) == ["self"]
    assert list(inspect.signature(_native.Context.result_levels).parameters) == ["self", "out", "stream"]
    monkeypatch.setattr(_native, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    with pytest.raises(TypeError):
        repet.separate("sim", np.zeros((100, 2)), 8000, levels=True)
    with pytest.raises(TypeError):
        repet.separate("sim", np.zeros((100, 2)), 8000, which="both", background_gain=0.25, levels=True)


# ---- the reference itself, on cases small enough to do by hand ---------------------------------------------------------------
def test_reference_idle_slot_and_a_slot_that_goes_live_mid_emission():
    mix = np.zeros((3, 4, 2))
    mix[0] = [[1, -2], [3, 4], [-5, 6], [7, -8]]
    mix[1] = np.nan                                  # an idle slot: whatever its share of the chunk held
    mix[2] = [[1, 1], [2, 2], [3, -3], [0.5, 4]]
    bg = 0.5 * mix
    bg[1] = np.inf
    fg = mix - bg
    live = np.array([[True] * 4, [False] * 4, [False, False, True, True]])
    got = levels(mix, bg, fg, live)
    assert got.shape == (3, 2, 8)
    assert got[0, 0].tolist() == [1 + 9 + 25 + 49, 84 / 4, 84 / 4, 7, 3.5, 3.5, 4, 0]
    assert got[0, 1].tolist() == [4 + 16 + 36 + 64, 30, 30, 8, 4, 4, 4, 0]
    assert (got[1] == 0).all()
    assert got[2, 0].tolist() == [9.25, 9.25 / 4, 9.25 / 4, 3, 1.5, 1.5, 2, 0]
    assert got[2, 1].tolist() == [25, 6.25, 6.25, 4, 2, 2, 2, 0]


def test_reference_nan_and_inf_samples():
    mix = np.array([[[1.0, 2.0], [np.nan, -np.inf], [-3.0, 0.25]]])
    bg = np.array([[[0.5, 1.0], [np.nan, np.nan], [1.0, 0.25]]])
    fg = mix - bg
    got = levels(mix, bg, fg)
    assert np.isnan(got[0, 0, 0]) and np.isnan(got[0, 0, 1]) and np.isnan(got[0, 0, 2])
    assert got[0, 0, 3:].tolist() == [3, 1, 4, 3, 1]                  # peaks skip NaN; one sample of three is not finite
    assert got[0, 1, 0] == np.inf and np.isnan(got[0, 1, 1]) and np.isnan(got[0, 1, 2])
    assert got[0, 1, 3:].tolist() == [np.inf, 1, 1, 3, 1]             # an infinite sample is the peak
    not_live = levels(mix, bg, fg, np.array([[True, False, True]]))     # the bad sample outside the slot's life: never shows
    assert np.isfinite(not_live).all() and not_live[0, :, 6].tolist() == [2, 2] and not_live[0, :, 7].tolist() == [0, 0]


def test_reference_empty_emission():
    got = levels(np.zeros((5, 0, 3)), np.zeros((5, 0, 3)), np.zeros((5, 0, 3)))
    assert got.shape == (5, 3, 8) and got.dtype == np.float64 and (got == 0).all()


def test_the_comparison_holds_energies_to_the_derived_bound_and_the_rest_to_the_bit():
    rs = np.random.RandomState(1)
    mix = rs.standard_normal((2, 1000, 2))
    bg = 0.3 * mix
    want = levels(mix, bg, mix - bg)
    assert check(want.copy(), want) == 0.0
    near = want.copy()
    near[0, 0, 0] *= 1 + 2000 * 2.0 ** -53                            # inside 4 n 2**-53 with n = 1000
    assert 0.4 < check(near, want) <= 1.0
    for f, factor in ((0, 1 + 5000 * 2.0 ** -53), (3, 1 + 2.0 ** -52), (6, 1 + 1e-3)):
        off = want.copy()
        off[1, 1, f] *= factor
        with pytest.raises(AssertionError):
            check(off, want)
