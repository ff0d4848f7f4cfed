"""Float64 NumPy statement of online REPET-SIM under ``silent_frames="zero"`` (include/repet_hip.h:
REPET_FLAG_SILENT_FRAMES_ZERO).

``simonline_silence(x, fs, start_frames)`` is the loop of ``simonline_start_reference.simonline_from`` -- same functions, same
order of operations -- with three changes:

* ``silent = norm == 0``: the frames whose channel-mean magnitude row has the norm 0 (here the float64 norm: for the exact zeros
  the tests place, the engine's float32 norm is 0 exactly where this one is);
* ``unit[silent] = 0``: their unit rows are zeros instead of 0 / 0, so every similarity with a silent member is 0;
* a silent frame ``j`` appends an empty list and adds nothing to the overlap-add.

Every other frame is decided by ``orc.localmaxima`` on its similarity vector as it then is, zeros in the silent columns. On a
clip without a silent frame every line reduces to ``simonline_from``'s and the result is ``np.array_equal`` to it
(tests/test_silence_reference.py).

trace: as ``simonline_from``'s, plus ``silent`` (the boolean mask over all T frames) and ``similarity_vectors`` (the vector
every processed frame was decided on; empty for a silent one).
"""
import numpy as np

from oracle import repet_oracle as orc


def simonline_silence(x, fs, start_frames, p=None, trace=None):
    p = p or orc.Params()
    n, ch = np.shape(x)
    w, window, h = orc.stft_geometry(fs)
    f = int(w / 2 + 1)
    t = orc.online_frame_count(n, w, h)
    b = round((p.buffer_length * fs) / h)
    m_start = int(start_frames)
    if not 1 <= m_start <= b:
        raise ValueError("start_frames must lie in [1, buffer_frames]")
    if n < (m_start - 2) * h + w:
        raise ValueError("operands could not be broadcast together: signal shorter than the buffer")
    total = (t - 1) * h + w
    padded = np.zeros((total, ch))
    padded[:n] = x
    dist = int(round(p.similarity_distance * fs / h))
    cut = orc.cutoff_bins(p, fs, w)

    frames = np.stack([np.lib.stride_tricks.sliding_window_view(padded[:, c], w)[::h][:t] * window
                       for c in range(ch)], axis=0)           # (C, T, W)
    spec = np.fft.fft(frames, axis=2)                         # (C, T, W)
    mag = np.abs(spec[:, :, :f])                              # (C, T, F)
    mean_mag = np.mean(np.moveaxis(mag, 0, 2), axis=2)        # (T, F)
    norm = np.sqrt(np.sum(np.power(mean_mag, 2), axis=1))
    silent = norm == 0                                        # (a NaN sample: the norm is NaN, the frame is not silent)
    with np.errstate(invalid="ignore"):
        unit = mean_mag / norm[:, np.newaxis]
    unit[silent] = 0

    out = np.zeros((total, ch))
    all_idx = []
    contributions = []
    vectors = []
    for j in range(m_start - 1, t):
        if silent[j]:
            all_idx.append(np.zeros(0, dtype=int))
            contributions.append(np.zeros((w, ch)))
            vectors.append(np.zeros(0))
            continue
        nb = min(b, j + 1)                                    # columns the buffer holds at frame j
        cols = np.arange(nb)
        in_col = j - np.mod(j - cols, nb)                     # frame held by each of them (young frame: 0 .. j)
        simvec = unit[in_col] @ unit[j]
        _, peaks = orc.localmaxima(simvec, p.similarity_threshold, dist, p.similarity_number)
        similar = in_col[peaks]
        all_idx.append(similar)
        vectors.append(simvec)
        added = np.empty((w, ch))
        for c in range(ch):
            cur = mag[c, j]
            model = np.median(mag[c, similar], axis=0) if len(similar) else np.full(f, np.nan)
            m = (np.minimum(model, cur) + orc.EPS) / (cur + orc.EPS)
            m[1:cut + 1] = 1
            full = np.concatenate((m, m[-2:0:-1]))
            added[:, c] = np.real(np.fft.ifft(full * spec[c, j]))
            out[j * h:j * h + w, c] += added[:, c]
        contributions.append(added)
    if trace is not None:
        trace.put("similarity_indices", all_idx)
        trace.put("contributions", contributions)
        trace.put("buffer_frames", b)
        trace.put("start_frames", m_start)
        trace.put("silent", silent)
        trace.put("similarity_vectors", vectors)
    return out[0:n] / sum(window[0:w:h])


# ---- the silence layouts of the tests (8 kHz: W 512, H 256, B 312; frame j covers samples [j H, j H + W)) ---------------
# name -> (runs of zeros in every channel, runs in channel 0 only, a NaN sample or None, start_frames), runs as (first, length)
def layouts(w, h, b):
    a = [(40 * h + 13, 5 * w), ((b + 4) * h + 7, 3 * w), ((b + 14) * h, w)]
    one = [((b + 9) * h, 2 * w)]
    return {
        "A": (a, one, None, b),                                  # inside the first buffer, off the hop grid, exactly one frame
        "B": (a + [(100 * h + 5, 4 * w)], one, None, 64),        # silent rows among young rows
        "C": ([(0, 30 * h + 5)], [], None, 64),                  # a call that begins muted
        "D": ([((b - 150) * h + 3, 80 * h + w)], [], None, b),   # longer than 2 d + 1 frames: silent columns with silent neighbours only
        "E": (a, one, (b + 17) * h + 9, b),                      # a NaN sample: its frames stay the reference's
    }


def mute(x, name, w, h, b):
    """x (N, C) with layout `name` applied (a copy), and the layout's start_frames."""
    every, first, nan_at, m = layouts(w, h, b)[name]
    y = np.array(x, dtype=float)
    for at, n in every:
        y[at:at + n] = 0
    for at, n in first:
        y[at:at + n, 0] = 0
    if nan_at is not None:
        y[nan_at, 0] = np.nan
    return y, m


def silent_frames_of(x, w, h):
    """The frames of x (N, C), zero-padded to whole frames, that hold nothing but zeros."""
    n = x.shape[0]
    t = orc.online_frame_count(n, w, h)
    padded = np.zeros(((t - 1) * h + w, x.shape[1]))
    padded[:n] = x
    return np.array([not padded[j * h:j * h + w].any() for j in range(t)])
