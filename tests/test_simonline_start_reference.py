"""The float64 statement of ``start_frames`` (tests/simonline_start_reference.py) against the oracle it is built from: with
M = B it IS the oracle, a young frame j is the oracle's first processed frame when its buffer has j + 1 frames, and outside the
young frames nothing differs. 8 kHz stereo: W = 512, H = 256, B = 312, similarity_distance2 = 31. No GPU."""
import functools

import numpy as np
import pytest

from oracle import repet_oracle as orc
from repet_synth import synth
from simonline_start_reference import simonline_from

FS, CH = 8000, 2
W, H, B = 512, 256, 312
N = (B + 20) * H + 77
M_YOUNG = 1                      # every frame from the first on: all the anchors below come from one run


@functools.lru_cache(maxsize=None)
def signal():
    x = synth(N / FS + 0.01, FS, CH, 21)[:N]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle_run():
    want = orc.simonline(np.array(signal()), FS)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def young_run():
    trace = orc.Trace()
    got = simonline_from(np.array(signal()), FS, M_YOUNG, trace=trace)
    got.setflags(write=False)
    return got, trace.items


def test_geometry():
    w, _, h = orc.stft_geometry(FS)
    assert (w, h, round(orc.Params().buffer_length * FS / h), int(round(orc.Params().similarity_distance * FS / h))) == (W, H, B, 31)


def test_start_at_the_buffer_length_is_the_oracle():
    trace, otrace = orc.Trace(), orc.Trace()
    got = simonline_from(np.array(signal()), FS, B, trace=trace)
    want = orc.simonline(np.array(signal()), FS, trace=otrace)
    assert np.array_equal(got, want)
    assert len(trace.items["similarity_indices"]) == len(otrace.items["similarity_indices"])
    for a, b in zip(trace.items["similarity_indices"], otrace.items["similarity_indices"]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("j", [0, 31, 32, 40, 150, 310])
def test_young_frame_is_the_oracles_first_frame_on_a_buffer_of_its_age(j):
    x = np.array(signal())
    _, items = young_run()
    otrace = orc.Trace()
    want = orc.simonline(x[: j * H + W], FS, orc.Params(buffer_length=(j + 1) * H / FS), trace=otrace)
    assert otrace.items["buffer_frames"] == j + 1
    assert np.array_equal(items["similarity_indices"][j - (M_YOUNG - 1)], otrace.items["similarity_indices"][0])
    if j <= 31:                                              # nothing but the frame itself lies within the distance
        assert list(items["similarity_indices"][j]) == [j]
    _, window, _ = orc.stft_geometry(FS)
    added = items["contributions"][j - (M_YOUNG - 1)] / sum(window[0:W:H])
    assert np.array_equal(added, want[j * H: j * H + W])     # the oracle's only overlap-add term there


@pytest.mark.parametrize("m", [1, 33, 200])
def test_output_ranges(m):
    x = np.array(signal())
    got = young_run()[0] if m == M_YOUNG else simonline_from(x, FS, m)
    want = oracle_run()
    assert got.shape == want.shape
    assert not got[: (m - 1) * H].any()                      # warm-up: nothing written
    assert got[(m - 1) * H: (m - 1) * H + W].any()
    assert np.array_equal(got[(B - 1) * H + W:], want[(B - 1) * H + W:])


def test_too_short_and_range():
    x = np.array(signal())
    m = 40
    assert simonline_from(x[: (m - 2) * H + W], FS, m).shape == ((m - 2) * H + W, CH)
    with pytest.raises(ValueError, match="shorter"):
        simonline_from(x[: (m - 2) * H + W - 1], FS, m)
    for bad in (0, B + 1):
        with pytest.raises(ValueError, match="start_frames"):
            simonline_from(x, FS, bad)
