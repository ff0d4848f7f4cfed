"""tests/result_frames_reference.py against the oracle (CPU): the statement the GPU test of ``separate(..., frames=...)`` compares
with is the oracle's own computation, looked at in the time-frequency plane.

For ``original``, ``adaptive`` and ``sim`` the statement's masks, resynthesised with ``orc.resynthesize``, are the oracle's
background BIT FOR BIT, channel 0's mask is the oracle's ``mask_c0`` trace, and ``bg`` is exactly ``mask * mix``. The quotient
``bg / mix`` cannot give the mask back to the bit -- a division does not undo a rounded product -- so it is held to one rounding of
the mask (2**-53 relative, the mask being at most 1) and its resynthesis to the oracle's background within the same rounding of
every term. ``simonline`` is ``frames_reference.frames_from``, whose samples are the oracle's bit for bit."""
import functools

import numpy as np
import pytest

from oracle import repet_oracle as orc
from repet_synth import synth
from result_frames_reference import ALGOS, frame_count, resynthesized, statement

FS = 8000


@functools.lru_cache(maxsize=None)
def case(algo):
    x = synth(14 if algo == "simonline" else 6, FS, 2, 9)
    trace = orc.Trace()
    with np.errstate(invalid="ignore", divide="ignore"):
        want = getattr(orc, algo)(x, FS, trace=trace)
    return x, want, trace, statement(algo, x, FS)


@pytest.mark.parametrize("algo", ("original", "adaptive", "sim"))
def test_masks_resynthesise_to_the_oracles_background(algo):
    x, want, trace, st = case(algo)
    assert np.array_equal(resynthesized(st, x, FS), want)
    assert np.array_equal(trace.items["mask_c0"], st["masks"][0])
    masks = np.transpose(st["masks"], (2, 0, 1))
    assert np.array_equal(st["bg"], masks * st["mix"]) and np.array_equal(st["fg"], st["mix"] - st["bg"])
    assert (st["mix"] > 0).all()
    ratio = st["bg"] / st["mix"]
    assert np.max(np.abs(ratio - masks)) <= 2.0 ** -53 and masks.max() <= 1.0
    _, window, h = orc.stft_geometry(FS)
    again = np.stack([orc.resynthesize(np.ascontiguousarray(ratio[:, c].T), st["spec"][:, :, c], window, h, len(x)) for c in range(2)], axis=1)
    assert np.max(np.abs(again - want)) <= 2.0 ** -50 * np.max(np.abs(x))
    cut = st["cutoff"]
    assert cut >= 1 and np.array_equal(st["bg"][..., 1:cut + 1], st["mix"][..., 1:cut + 1])


def test_simonline_is_the_live_statement():
    x, want, trace, st = case("simonline")
    assert np.array_equal(st["samples"], want, equal_nan=True)
    warm = st["warm"]
    assert warm == trace.items["buffer_frames"] - 1
    assert not st["bg"][:warm].any() and np.array_equal(st["fg"][:warm], st["mix"][:warm])
    lists = trace.items["similarity_indices"]
    assert len(st["lists"]) == warm + len(lists)
    for j, ix in enumerate(lists):
        assert np.array_equal(st["lists"][warm + j], np.sort(ix))
    assert all(len(ix) == 0 for ix in st["lists"][:warm])


@pytest.mark.parametrize("algo", ALGOS)
def test_shapes_and_decisions(algo):
    x, _, trace, st = case(algo)
    t = frame_count(algo, len(x), FS)
    w = orc.window_length_for(FS)
    assert st["mix"].shape == st["bg"].shape == st["fg"].shape == (t, 2, w // 2 + 1)
    if algo == "original":
        assert st["period"] == trace.items["repeating_period"]
    if algo == "adaptive":
        assert np.array_equal(st["periods"], trace.items["repeating_periods"])
    if algo == "sim":
        s = trace.items["similarity_matrix"]
        for j, ix in enumerate(trace.items["similarity_indices"]):
            assert np.array_equal(st["lists"][j], np.sort(ix)) and np.array_equal(st["similarities"][j], s[j, np.sort(ix)])
            assert (np.diff(st["lists"][j]) > 0).all()
