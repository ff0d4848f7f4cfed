"""Float64 NumPy statement of what a live handle's ``last_matches`` hands out (include/repet_hip.h: repet_online_last_matches).

``matches_from(x, fs, start_frames)`` runs the float64 model of a live stream that exists,
``simonline_start_reference.simonline_from`` with a trace, and reads the similar-frame list of every processed frame from it.
The trace's ``similarity_indices`` are the stream's own frame numbers, so for frame ``j`` and list entry ``i``

* ``age = j - i`` (0: the frame itself), sorted ascending -- the order inside the reference's list is by similarity and is
  not part of what is compared;
* ``similarity = unit[i] @ unit[j]``, the product the model's own loop forms (``unit``: the channel-mean magnitude spectra,
  each divided by its norm, repet.py:855-858), in float64;
* ``count = len(list)``.

Frames below ``start_frames - 1`` are warm-up frames and have no list: count 0. Rows are padded to
``capacity(fs, p) = min(similarity_number, ceil(buffer_frames / (similarity_distance_frames + 1)))`` entries with age -1 and
similarity 0: peaks lie more than ``similarity_distance_frames`` apart (repet.py:1315-1329), so no list is longer.
"""
import numpy as np

from oracle import repet_oracle as orc
from simonline_start_reference import simonline_from


def geometry(fs, p=None):
    """(W, H, B, similarity_distance_frames) as the model derives them."""
    p = p or orc.Params()
    w, _, h = orc.stft_geometry(fs)
    return w, h, round((p.buffer_length * fs) / h), int(round(p.similarity_distance * fs / h))


def capacity(fs, p=None):
    p = p or orc.Params()
    _, _, b, dist = geometry(fs, p)
    return min(int(p.similarity_number), -(-b // (dist + 1)))


def unit_spectra(x, fs):
    """(T, F): the rows the model's similarities are products of -- the lines of ``simonline_from``."""
    n, ch = np.shape(x)
    w, window, h = orc.stft_geometry(fs)
    f = int(w / 2 + 1)
    t = orc.online_frame_count(n, w, h)
    padded = np.zeros(((t - 1) * h + w, ch))
    padded[:n] = x
    frames = np.stack([np.lib.stride_tricks.sliding_window_view(padded[:, c], w)[::h][:t] * window
                       for c in range(ch)], axis=0)
    mag = np.abs(np.fft.fft(frames, axis=2)[:, :, :f])
    mean_mag = np.mean(np.moveaxis(mag, 0, 2), axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return mean_mag / np.sqrt(np.sum(np.power(mean_mag, 2), axis=1))[:, np.newaxis]


def lists_from(x, fs, start_frames, p=None):
    """The model's list of every frame of the stream, as arrays of own frame numbers; empty for the warm-up frames."""
    p = p or orc.Params()
    trace = orc.Trace()
    with np.errstate(invalid="ignore", divide="ignore"):
        simonline_from(np.asarray(x, dtype=np.float64), fs, start_frames, p, trace)
    lists = [np.asarray(ix, dtype=np.int64) for ix in trace.items["similarity_indices"]]
    return [np.zeros(0, dtype=np.int64)] * (int(start_frames) - 1) + lists


def matches_from(x, fs, start_frames, p=None):
    """(count (T,) int32, age (T, K) int32, similarity (T, K) float64) of every frame of the stream ``x`` (N, C)."""
    p = p or orc.Params()
    x = np.asarray(x, dtype=np.float64)
    lists = lists_from(x, fs, start_frames, p)
    unit = unit_spectra(x, fs)
    assert len(lists) == len(unit)
    k = capacity(fs, p)
    count = np.zeros(len(lists), dtype=np.int32)
    age = np.full((len(lists), k), -1, dtype=np.int32)
    similarity = np.zeros((len(lists), k), dtype=np.float64)
    for j, ix in enumerate(lists):
        ix = np.sort(ix)[::-1]                                    # ascending age
        count[j] = len(ix)
        age[j, :len(ix)] = j - ix
        similarity[j, :len(ix)] = unit[ix] @ unit[j]
    return count, age, similarity
