"""Float64 NumPy statement of the SHAPED background of a live handle with band gains (include/repet_hip.h:
repet_online_set_background_band_gains).

``band_gains_from(x, fs, start_frames, factors)`` is the loop of ``frames_reference.frames_from`` -- same functions, same order of
operations, so its plain background is that function's samples bit for bit -- which additionally takes one factor table per
frame, ``factors`` of shape ``(T, F)`` (``a = 1 - g``), and accumulates ``ifft(full(a_j) * full(mask) * spec)`` into a second
signal: bin ``N - k`` takes bin ``k``'s factor. It returns ``(bg, shaped_bg)``, both ``(N, C)``. Frames below ``start_frames - 1``
are warm-up frames: nothing is removed there and both signals are zero.

``masks_of(x, fs, start_frames)`` is the part of the loop that does not depend on the factors (the spectra and the full-length
masks of every frame); ``shaped_from(state, factors)`` is the part that does. A test that shapes one signal with several tables
computes the first once; ``band_gains_from`` is the two in a row.

``factor(g)`` is the library's ``a``: ``float32(1 - float64(float32(g)))`` as float64."""
import numpy as np

from oracle import repet_oracle as orc


def factor(g):
    return np.float32(1.0 - np.float32(g).astype(np.float64)).astype(np.float64)


def frame_count(n, fs):
    w, _, h = orc.stft_geometry(fs)
    return orc.online_frame_count(n, w, h)


def masks_of(x, fs, start_frames, p=None):
    """What the accumulation needs of ``frames_from``'s loop: a dict with the spectra (C, T, W), the full-length masks (C, T, W;
    zero rows for the warm-up frames) and the geometry."""
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

    masks = np.zeros((ch, t, w))
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
            masks[c, j] = np.concatenate((m, m[-2:0:-1]))
    return {"spec": spec, "masks": masks, "n": n, "ch": ch, "w": w, "h": h, "f": f, "t": t, "first": m_start - 1,
            "total": total, "cola": sum(window[0:w:h])}


def shaped_from(state, factors):
    """(bg, shaped_bg), both (N, C), of the frames of ``state`` under ``factors`` (T, F)."""
    t, f, w, h, ch = state["t"], state["f"], state["w"], state["h"], state["ch"]
    factors = np.asarray(factors, dtype=np.float64)
    if factors.shape != (t, f):
        raise ValueError(f"factors of shape {factors.shape}: one table ({f},) per frame, {t} of them")
    spec, masks = state["spec"], state["masks"]
    out = np.zeros((state["total"], ch))
    shaped = np.zeros((state["total"], ch))
    for j in range(state["first"], t):
        a = factors[j]
        full_a = np.concatenate((a, a[-2:0:-1]))
        for c in range(ch):
            full = masks[c, j]
            out[j * h:j * h + w, c] += np.real(np.fft.ifft(full * spec[c, j]))
            shaped[j * h:j * h + w, c] += np.real(np.fft.ifft(full_a * full * spec[c, j]))
    n = state["n"]
    return out[0:n] / state["cola"], shaped[0:n] / state["cola"]


def band_gains_from(x, fs, start_frames, factors, p=None):
    """(bg, shaped_bg) of online REPET-SIM that separates from its frame ``start_frames - 1`` on, frame j shaped with
    ``factors[j]``."""
    return shaped_from(masks_of(x, fs, start_frames, p), factors)


def table(f, edges, gains):
    """The per-bin gains ``g`` (F,) a set with these ``edges`` and ``gains`` leaves (``edges`` None: ``gains`` is per bin)."""
    g = np.zeros(f, dtype=np.float32)
    if edges is None:
        g[:] = np.asarray(gains, dtype=np.float32)
        return g
    for k in range(len(edges) - 1):
        g[int(edges[k]):int(edges[k + 1])] = np.float32(gains[k])
    return g
