"""The float64 statement of ``silent_frames="zero"`` (tests/silence_reference.py) against what it is built from: on a clip
without a silent frame it IS ``simonline_from`` (and, for M = B, the oracle); on the silence layouts it is finite everywhere,
exactly 0 on the samples that only silent frames cover, its silent frames are the all-zero frames, and every list is
``orc.localmaxima`` of the vector with zeros in the silent columns. 8 kHz stereo: W = 512, H = 256, B = 312,
similarity_distance = 31 frames. No GPU."""
import functools

import numpy as np
import pytest

from oracle import repet_oracle as orc
from repet_synth import synth
from simonline_start_reference import simonline_from
from silence_reference import layouts, mute, silent_frames_of, simonline_silence

FS, CH = 8000, 2
W, H, B = 512, 256, 312
N = (B + 20) * H + 77
DIST = 31


@functools.lru_cache(maxsize=None)
def signal():
    x = synth(N / FS + 0.01, FS, CH, 5)[:N].astype(np.float32).astype(np.float64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def run(name):
    x, m = mute(signal(), name, W, H, B)
    trace = orc.Trace()
    got = simonline_silence(x, FS, m, trace=trace)
    got.setflags(write=False)
    return x, m, got, trace.items


def test_geometry_and_the_clip_has_no_silent_frame_of_its_own():
    w, _, h = orc.stft_geometry(FS)
    assert (w, h, round(orc.Params().buffer_length * FS / h), int(round(orc.Params().similarity_distance * FS / h))) == (W, H, B, DIST)
    assert not silent_frames_of(signal(), W, H).any()
    counts = {name: int(silent_frames_of(mute(signal(), name, W, H, B)[0], W, H).sum()) for name in "ABCD"}
    assert counts["A"] == 13 and counts["B"] == 13 + 6 and counts["C"] == 29 and counts["D"] > 2 * DIST + 1, counts


@pytest.mark.parametrize("m", [B, 64])
def test_without_silence_it_is_the_statement_it_was_taken_from(m):
    x = np.array(signal())
    trace, strace = orc.Trace(), orc.Trace()
    got = simonline_silence(x, FS, m, trace=trace)
    want = simonline_from(x, FS, m, trace=strace)
    assert np.array_equal(got, want)
    assert not trace.items["silent"].any()
    assert len(trace.items["similarity_indices"]) == len(strace.items["similarity_indices"])
    for a, b in zip(trace.items["similarity_indices"], strace.items["similarity_indices"]):
        assert np.array_equal(a, b)
    if m == B:
        assert np.array_equal(got, orc.simonline(x, FS))


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_finite_everywhere_and_zero_under_silence(name):
    x, m, got, items = run(name)
    silent = items["silent"]
    assert np.array_equal(silent, silent_frames_of(x, W, H))
    assert np.isfinite(got).all()
    t = len(silent)
    # sample s lies in frames s // H - 1 and s // H: nothing is added where both are silent or not processed
    quiet = np.array([silent[j] or j < m - 1 for j in range(t)])
    covered = 0
    for s0 in range(0, N, H):
        k = s0 // H
        if all(quiet[j] for j in (k - 1, k) if 0 <= j < t):
            assert not got[s0:s0 + H].any(), (name, k)
            covered += 1
        elif not quiet[min(k, t - 1)] and k >= 1 and not quiet[k - 1]:
            assert got[s0:s0 + H].any(), (name, k)
    assert covered > 0
    # the frames around a mute ring into its first and last hop
    first = int(np.flatnonzero(silent & (np.arange(t) >= m))[0]) if (silent & (np.arange(t) >= m)).any() else None
    if first is not None and not quiet[first - 1]:
        assert got[first * H:(first + 1) * H].any()


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_lists_are_localmaxima_on_the_zero_substituted_vector(name):
    """Outside R2's edge case (similarity_distance >= 1 frame, rows of at least two columns: every row here) the rule IS the
    reference's peak picking on the vector with zeros in the silent columns, and a silent frame is in nobody's list."""
    x, m, _, items = run(name)
    silent = items["silent"]
    for r, (vec, got) in enumerate(zip(items["similarity_vectors"], items["similarity_indices"])):
        j = m - 1 + r
        if silent[j]:
            assert len(got) == 0
            continue
        nb = min(B, j + 1)
        in_col = j - np.mod(j - np.arange(nb), nb)
        # (the row of a frame with a NaN sample is NaN throughout: 0 x NaN, as in NumPy's product)
        assert nb >= 2 and (np.isnan(vec).all() or np.array_equal(vec[silent[in_col]], np.zeros(int(silent[in_col].sum()))))
        assert np.array_equal(got, in_col[orc.localmaxima(vec, 0, DIST, 100)[1]])
        assert not silent[got].any()
        # a silent row decided by the same rule would be empty as well: zero is never strictly above its neighbours
    zero_row = np.zeros(B)
    assert len(orc.localmaxima(zero_row, 0, DIST, 100)[1]) == 0


def test_a_nan_sample_keeps_the_references_behaviour():
    x, m, got, items = run("E")
    xa, _, want_a, items_a = run("A")
    at = layouts(W, H, B)["E"][2]
    frames = [at // H - 1, at // H]
    assert not items["silent"][frames].any() and np.array_equal(items["silent"], items_a["silent"])
    for j in frames:                                            # a NaN frame: its own list is empty, as in the reference
        assert len(items["similarity_indices"][j - (m - 1)]) == 0
    nan = np.isnan(got)
    assert nan[frames[0] * H: frames[1] * H + W].all() and not nan[: frames[0] * H].any() and not nan[frames[1] * H + W:].any()
    # the reference rule on the same clip: NaN there too, and on the silent frames besides
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = orc.simonline(np.array(x), FS)
    assert np.isnan(ref)[nan].all() and np.isnan(ref).sum() > nan.sum()
    assert np.array_equal(got[: frames[0] * H - 32 * H], want_a[: frames[0] * H - 32 * H])


def test_one_channel_of_silence_is_not_silence():
    x, m, _, items = run("A")
    for j in (B + 9, B + 10, B + 11):
        assert not x[j * H: j * H + W, 0].any() and x[j * H: j * H + W, 1].any()
        assert not items["silent"][j] and len(items["similarity_indices"][j - (m - 1)]) > 0
