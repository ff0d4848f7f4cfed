"""Float64 NumPy statement of the spectra a tensor call hands out (``repet.separate(..., frames=...)``; include/repet_hip.h:
repet_ctx_request_frames).

``statement(algo, x, fs)`` follows the oracle's own function for ``algo`` -- the same functions in the same order
(``orc.spectrogram_channels``, then ``orc.mask`` / ``orc.adaptivemask`` / ``orc.simmask`` behind the decisions that feed them, the
soft mask inside them, the high-pass rule ``mask[1:cutoff + 1] = 1``) -- and returns, for every frame ``j``, channel ``c`` and bin
``f`` in ``[0, F)``, as ``(T, C, F)`` arrays:

* ``mix = |audio_stft[f, j]|``
* ``bg = mask * mix``
* ``fg = mix - bg``

together with the masks themselves ``(C, F, T)``, the spectra ``(W, T, C)`` and what the variant decided: ``period`` (original),
``periods`` (adaptive, one per frame) or ``lists`` (sim, simonline: per frame the similar frames as ASCENDING frame numbers, and
``similarities``, their float64 cosine similarities in the same order). tests/test_result_frames_reference.py ties it to the
oracle: resynthesising the masks gives the oracle's samples bit for bit.

``simonline`` is ``frames_reference.frames_from`` (the live handles' statement: the same loop), with ``start_frames`` the frame
count from which on it separates (None: buffer_frames, the reference); frames below ``start_frames - 1`` are warm-up frames with
``bg = 0`` and ``fg = mix`` and an empty list.
"""
import numpy as np

from frames_reference import frames_from
from matches_reference import lists_from, unit_spectra
from oracle import repet_oracle as orc

ALGOS = ("original", "adaptive", "sim", "simonline")


def frame_count(algo, n, fs):
    w, _, h = orc.stft_geometry(fs)
    return orc.online_frame_count(n, w, h) if algo == "simonline" else orc.centred_frame_count(n, w, h)


def _sorted_lists(lists, unit_rows):
    """Ascending frame numbers per frame, and unit[i] @ unit[j] for them."""
    out, sims = [], []
    for j, ix in enumerate(lists):
        ix = np.sort(np.asarray(ix, dtype=np.int64))
        out.append(ix)
        sims.append(unit_rows[ix] @ unit_rows[j] if len(ix) else np.zeros(0))
    return out, sims


def statement(algo, x, fs, start_frames=None, p=None):
    p = p or orc.Params()
    x = np.asarray(x, dtype=np.float64)
    n, ch = x.shape
    w, window, h = orc.stft_geometry(fs)
    cut = orc.cutoff_bins(p, fs, w)
    if algo == "simonline":
        b = round((p.buffer_length * fs) / h)
        m = b if start_frames is None else int(start_frames)
        with np.errstate(invalid="ignore", divide="ignore"):
            samples, mix, bg, fg = frames_from(x, fs, m, p)
        lists, sims = _sorted_lists(lists_from(x, fs, m, p), unit_spectra(x, fs))
        return {"mix": mix, "bg": bg, "fg": fg, "samples": samples, "lists": lists, "similarities": sims, "warm": m - 1,
                "cutoff": cut}
    spec, mag = orc.spectrogram_channels(x, window, h)
    out = {"cutoff": cut, "warm": 0}
    if algo == "original":
        beat = orc.beatspectrum(np.power(np.mean(mag, axis=2), 2))
        period = orc.periods(beat, orc.period_range_frames(p, fs, h))
        out["period"] = int(period)
        mask_fn = lambda v: orc.mask(v, period)
    elif algo == "adaptive":
        seg_len = int(round(p.segment_length * fs / h))
        seg_step = int(round(p.segment_step * fs / h))
        bsg = orc.beatspectrogram(np.power(np.mean(mag, axis=2), 2), seg_len, seg_step)
        per = orc.periods(bsg, orc.period_range_frames(p, fs, h))
        out["periods"] = np.asarray(per, dtype=np.int64)
        mask_fn = lambda v: orc.adaptivemask(v, per, p.filter_order)
    elif algo == "sim":
        mean_mag = np.mean(mag, axis=2)
        s = orc.selfsimilaritymatrix(mean_mag)
        dist = int(round(p.similarity_distance * fs / h))
        idx = orc.indices(s, p.similarity_threshold, dist, p.similarity_number)
        out["lists"] = [np.sort(np.asarray(ix, dtype=np.int64)) for ix in idx]
        out["similarities"] = [s[j, ix] for j, ix in enumerate(out["lists"])]
        mask_fn = lambda v: orc.simmask(v, idx)
    else:
        raise ValueError(f"no single frame grid for {algo!r}")
    masks = []
    for c in range(ch):
        m = mask_fn(mag[:, :, c])
        m[1:cut + 1, :] = 1                                    # repet.py:185
        masks.append(m)
    masks = np.stack(masks)                                    # (C, F, T)
    mix = np.ascontiguousarray(np.transpose(mag, (1, 2, 0)))   # (T, C, F)
    bg = np.ascontiguousarray(np.transpose(masks, (2, 0, 1))) * mix
    out.update({"mix": mix, "bg": bg, "fg": mix - bg, "masks": masks, "spec": spec})
    return out


def resynthesized(st, x, fs):
    """The samples the statement's masks give back through the oracle's own inverse: (N, C)."""
    n, ch = np.shape(x)
    _, window, h = orc.stft_geometry(fs)
    return np.stack([orc.resynthesize(st["masks"][c], st["spec"][:, :, c], window, h, n) for c in range(ch)], axis=1)
