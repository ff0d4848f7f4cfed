"""Float64 NumPy statement of what a live handle's ``last_frames`` hands out (include/repet_hip.h: repet_online_last_frames).

``frames_from(x, fs, start_frames)`` is the loop of ``simonline_start_reference.simonline_from`` -- same functions, same order of
operations, so its samples are that function's bit for bit (and the oracle's for ``start_frames = B``) -- which also returns,
for every frame ``j`` of the stream, channel ``c`` and bin ``f`` in ``[0, F)``, the reference's own quantities
(repet.py:834-898):

* ``mix = |audio_stft[f, j]|``
* ``bg = mask[f] * mix``, the mask with the high-pass rule ``mask[1:cutoff_bins + 1] = 1`` applied
* ``fg = mix - bg``

as ``(T, C, F)`` arrays. Frames below ``start_frames - 1`` are warm-up frames: nothing is removed there, ``bg = 0`` and
``fg = mix``.

``band_energies(m, edges)`` sums the squares of the last axis over ``[edges[k], edges[k + 1])`` in float64.
"""
import numpy as np

from oracle import repet_oracle as orc


def frames_from(x, fs, start_frames, p=None):
    """(samples (N, C), mix, bg, fg (T, C, F)) of online REPET-SIM that separates from its frame ``start_frames - 1`` on."""
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
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = mean_mag / np.sqrt(np.sum(np.power(mean_mag, 2), axis=1))[:, np.newaxis]

    mix = np.ascontiguousarray(np.moveaxis(mag, 0, 1))        # (T, C, F)
    bg = np.zeros_like(mix)
    out = np.zeros((total, ch))
    for j in range(m_start - 1, t):
        nb = min(b, j + 1)
        cols = np.arange(nb)
        in_col = j - np.mod(j - cols, nb)
        simvec = unit[in_col] @ unit[j]
        _, peaks = orc.localmaxima(simvec, p.similarity_threshold, dist, p.similarity_number)
        similar = in_col[peaks]
        for c in range(ch):
            cur = mag[c, j]
            model = np.median(mag[c, similar], axis=0) if len(similar) else np.full(f, np.nan)
            m = (np.minimum(model, cur) + orc.EPS) / (cur + orc.EPS)
            m[1:cut + 1] = 1
            bg[j, c] = m * cur
            full = np.concatenate((m, m[-2:0:-1]))
            out[j * h:j * h + w, c] += np.real(np.fft.ifft(full * spec[c, j]))
    fg = mix - bg
    return out[0:n] / sum(window[0:w:h]), mix, bg, fg


def band_energies(m, edges):
    """Float64 sums of squares of ``m``'s last axis over the bins ``[edges[k], edges[k + 1])``: shape ``m.shape[:-1] + (n_bands,)``."""
    m = np.asarray(m, dtype=np.float64)
    edges = [int(e) for e in edges]
    out = np.zeros(m.shape[:-1] + (len(edges) - 1,), dtype=np.float64)
    for k in range(len(edges) - 1):
        out[..., k] = np.sum(np.square(m[..., edges[k]:edges[k + 1]]), axis=-1)
    return out
