"""Float64 NumPy statement of online REPET-SIM that starts separating before its buffer is full (``start_frames``, see
include/repet_hip.h: repet_online_set_start_frames).

``simonline_from(x, fs, start_frames)`` follows the loop of ``oracle.repet_oracle.simonline`` -- same functions, same order of
operations -- from frame ``M - 1`` instead of frame ``B - 1``, and gives frame ``j`` a buffer of ``nb = min(B, j + 1)`` columns:
the stream's own frames ``0 .. j`` while the buffer is still filling (the circular position of a frame is its number while
``j < B``), the oracle's ``B`` columns afterwards. The peak picking sees exactly those ``nb`` similarities; the columns past
``j`` do not exist. With ``M = B`` every line reduces to the oracle's, and the result is ``np.array_equal`` to it
(tests/test_simonline_start_reference.py).

trace (an ``oracle.repet_oracle.Trace``): ``similarity_indices`` -- the list of every processed frame, the first for frame
``M - 1``; ``contributions`` -- what each processed frame adds to the overlap-add, (W, C) before the division by the window
sum; ``buffer_frames`` and ``start_frames``.
"""
import numpy as np

from oracle import repet_oracle as orc


def simonline_from(x, fs, start_frames, p=None, trace=None):
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
        # the oracle's rule with start_frames in place of the buffer length
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
    unit = mean_mag / np.sqrt(np.sum(np.power(mean_mag, 2), axis=1))[:, np.newaxis]

    out = np.zeros((total, ch))
    all_idx = []
    contributions = []
    for j in range(m_start - 1, t):
        nb = min(b, j + 1)                                    # columns the buffer holds at frame j
        cols = np.arange(nb)
        in_col = j - np.mod(j - cols, nb)                     # frame held by each of them (young frame: 0 .. j)
        simvec = unit[in_col] @ unit[j]
        _, peaks = orc.localmaxima(simvec, p.similarity_threshold, dist, p.similarity_number)
        similar = in_col[peaks]
        all_idx.append(similar)
        added = np.empty((w, ch))
        for c in range(ch):
            cur = mag[c, j]
            model = np.median(mag[c, similar], axis=0) if len(similar) else np.full(f, np.nan)
            m = (np.minimum(model, cur) + orc.EPS) / (cur + orc.EPS)
            m[1:cut + 1] = 1
            full = np.concatenate((m, m[-2:0:-1]))
            added[:, c] = np.real(np.fft.ifft(full * spec[c, j]))
            out[j * h:j * h + w, c] += added[:, c]
        if trace is not None:
            contributions.append(added)
    if trace is not None:
        trace.put("similarity_indices", all_idx)
        trace.put("contributions", contributions)
        trace.put("buffer_frames", b)
        trace.put("start_frames", m_start)
    return out[0:n] / sum(window[0:w:h])
