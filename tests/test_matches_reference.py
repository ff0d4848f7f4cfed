"""The float64 statement of ``last_matches`` (tests/matches_reference.py) against the oracle it is built from. No GPU.

* With ``start_frames = B`` the lists are ``orc.simonline``'s own trace, entry for entry, and the similarities are the entries of
  the similarity vector the oracle's loop picks its peaks from, within the rounding of a float64 dot product of F terms.
* Ages are distinct and ascending, ``0 <= age <= min(B - 1, j)``, ``count <= K``, the padding is ``-1`` / ``0``.
* On the signals the GPU tests use (tests/test_gpu_online_matches.py) the counts run from 1 to 6 under a capacity of 10 and the
  frame itself is in every list: padding, ordering and "fewer than K" are all exercised there.
"""
import functools

import numpy as np
import pytest

from oracle import repet_oracle as orc
from matches_reference import capacity, geometry, lists_from, matches_from, unit_spectra
from repet_synth import synth


@functools.lru_cache(maxsize=None)
def signal(seed, fs, ch):
    """signal(seed, n, fs, ch) of tests/test_gpu_online_start.py at the length the GPU tests use."""
    w, h, b, _ = geometry(fs)
    n = (b + 20) * h + 77
    x = synth(n / fs + 0.01, fs, ch, seed)[:n].astype(np.float32).astype(np.float64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def statement(seed, fs, ch, m):
    out = matches_from(np.array(signal(seed, fs, ch)), fs, m)
    for a in out:
        a.setflags(write=False)
    return out


def test_with_a_full_buffer_the_lists_are_the_oracles():
    fs, ch = 8000, 2
    w, h, b, dist = geometry(fs)
    assert (w, h, b, dist) == (512, 256, 312, 31) and capacity(fs) == 10
    x = np.array(signal(31, fs, ch))
    count, age, similarity = statement(31, fs, ch, b)
    otrace = orc.Trace()
    orc.simonline(x, fs, trace=otrace)
    want = otrace.items["similarity_indices"]
    assert len(want) == len(count) - (b - 1) and not count[:b - 1].any()
    unit = unit_spectra(x, fs)
    for r, ix in enumerate(want):
        j = b - 1 + r
        ix = np.sort(np.asarray(ix, dtype=np.int64))[::-1]
        assert count[j] == len(ix)
        assert np.array_equal(j - age[j, :count[j]], ix)
        # the oracle's similarity vector of frame j (orc.simonline's loop), at the entries it picked
        cols = np.arange(b)
        in_col = j - np.mod(j - cols, b)
        simvec = unit[in_col] @ unit[j]
        # (two float64 dot products of the same F non-negative terms, summed in whatever order the BLAS call of that
        # shape takes: each within F * 2**-53 of the exact sum, which is at most 1)
        assert np.abs(similarity[j, :count[j]] - simvec[np.mod(ix, b)]).max() <= 2 * unit.shape[1] * 2.0 ** -53
    assert lists_from(x, fs, b)[b - 1:] and all(len(l) == 0 for l in lists_from(x, fs, b)[:b - 1])


@pytest.mark.parametrize("seed,fs,ch,m", [(31, 8000, 2, 33), (31, 8000, 2, 1), (32, 16000, 1, 64)])
def test_rows_are_well_formed_and_exercise_the_padding(seed, fs, ch, m):
    w, h, b, dist = geometry(fs)
    k = capacity(fs)
    assert k == 10
    count, age, similarity = statement(seed, fs, ch, m)
    assert count.dtype == np.int32 and age.dtype == np.int32 and age.shape == similarity.shape == (len(count), k)
    assert not count[:m - 1].any()
    live = count[m - 1:]
    assert live.min() == (2 if fs == 16000 else 1) and live.max() == 6 < k, (live.min(), live.max())
    for j in range(len(count)):
        n = count[j]
        assert 0 <= n <= k
        assert (age[j, n:] == -1).all() and (similarity[j, n:] == 0).all()
        if j < m - 1:
            continue
        a = age[j, :n]
        assert a[0] == 0                                          # the frame itself is in its own list
        assert (np.diff(a) > 0).all()                             # distinct, ascending
        assert a[-1] <= min(b - 1, j)
        assert similarity[j, 0] == pytest.approx(1.0, abs=1e-12) and (similarity[j, :n] > 0).all()
