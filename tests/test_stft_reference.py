"""The float64 references of tests/stft_reference.py, pinned to the oracle where it has the same operation: the yardstick of
tests/test_gpu_stft_stages.py is tested here, without a GPU."""
import numpy as np
import pytest

from oracle import repet_oracle as orc

import stft_reference as ref
from repet_synth import synth


def _half(spec_full, w):
    """(W, T) complex of the oracle -> (T, F)."""
    return np.ascontiguousarray(spec_full[:w // 2 + 1].T)


@pytest.mark.parametrize("fs,n", [(8000, 4000), (8000, 4001), (8000, 129), (44100, 9001)])
def test_unmasked_inverse_is_the_oracle_istft(fs, n):
    x = synth(2.0, fs, 1, 5)[:n, 0]
    w, window, h = orc.stft_geometry(fs)
    spec = orc.stft(x, window, h)
    want = orc.istft(spec, window, h)
    got = ref.inverse_piece(_half(spec, w)[None], w, w - h, len(want), 1.0 / sum(window[0:w:h]))
    assert got.shape == (len(want), 1)
    assert np.max(np.abs(got[:, 0] - want)) < 1e-12
    # trim and n_out are a plain slice of the padded overlap-add [w - h | clip | w - h]; hop T, the last frame's tail, ends it
    padded = np.concatenate((np.full(w - h, np.nan), want, np.full(w - h, np.nan)))
    assert len(padded) == (spec.shape[1] + 1) * h
    for trim, n_out in ((0, 7), (1, h), (h - 1, h + 1), (w - h + 5, len(want) - 5), (3 * h + 1, 2 * h), (len(padded) - 3, 10)):
        part = ref.inverse_piece(_half(spec, w)[None], w, trim, n_out, 1.0 / sum(window[0:w:h]))[:, 0]
        assert len(part) == max(min(n_out, len(padded) - trim), 0)
        ends = np.isnan(padded[trim:trim + n_out])
        assert np.max(np.abs(part - padded[trim:trim + n_out])[~ends], initial=0) < 1e-12


def test_masked_inverse_is_the_oracle_resynthesis():
    fs = 8000
    x = synth(3.0, fs, 2, 7)
    n = len(x)
    w, window, h = orc.stft_geometry(fs)
    spec, mag = orc.spectrogram_channels(x, window, h)
    rng = np.random.default_rng(3)
    mask = rng.random(mag.shape[:2])
    mask[rng.random(mask.shape) < 0.2] = 0
    mask[rng.random(mask.shape) < 0.2] = 1
    Y = np.stack([_half(spec[:, :, c], w) for c in range(2)])
    got = ref.inverse_piece(Y, w, w - h, n, 1.0 / sum(window[0:w:h]), mask=np.broadcast_to(mask.T, Y.shape))
    for c in range(2):
        want = orc.resynthesize(mask, spec[:, :, c], window, h, n)
        assert np.max(np.abs(got[:, c] - want)) < 1e-12


def _period_model(v, period):
    """Medians over the repetitions of every position of the period, v (F, T) -> (period, F): the W of repet.py:1386-1440,
    a NaN-padded restatement (the last, partial repetition does not count where it has no frame)."""
    f, t = v.shape
    s = int(np.ceil(t / period))
    padded = np.full((f, s * period), np.nan)
    padded[:, :t] = v
    return np.nanmedian(padded.reshape(f, s, period), axis=1).T


def test_model_mask_is_the_oracle_period_mask():
    fs = 8000
    x = synth(4.0, fs, 1, 2)
    w, window, h = orc.stft_geometry(fs)
    _, mag = orc.spectrogram_channels(x, window, h)
    v = mag[:, :, 0]
    for period, cut in ((1, 0), (2, 3), (37, 3), (v.shape[1] + 5, 0)):
        want = orc.mask(v, min(period, v.shape[1])) if period <= v.shape[1] else np.ones_like(v)
        want = want.copy()
        want[1:cut + 1, :] = 1
        if period > v.shape[1]:
            model = v.T                                  # every frame is its own only repetition: min(v, v) / v = 1
            model = np.concatenate((model, np.zeros((period - v.shape[1], v.shape[0]))))
        else:
            model = _period_model(v, period)
        got = ref.model_mask(v.T, model, period, cut)
        assert np.max(np.abs(got - want.T)) < 1e-15


def test_weighted_segments_sum_to_the_oracle_extended_range():
    """Segments shorter than twice their step (several later segments fade one sample: `later` > 1)."""
    fs = 8000
    p = orc.Params(segment_length=2, segment_step=0.5, period_range=(0.1, 0.6))
    x = synth(7.0, fs, 2, 13)
    n = len(x)
    w, window, h = orc.stft_geometry(fs)
    segs, overlap = orc.extended_plan(n, fs, p)
    step = segs[1][0]
    assert len(segs) >= 5 and step < overlap and all(length == segs[0][1] for _, length in segs)
    cut = orc.cutoff_bins(p, fs, w)
    prange = orc.period_range_frames(p, fs, h)
    pieces = []
    for j, (start, length) in enumerate(segs):
        spec, mag = orc.spectrogram_channels(x[start:start + length], window, h)
        period = orc.periods(orc.beatspectrum(np.power(np.mean(mag, axis=2), 2)), prange)
        masks = []
        for c in range(2):
            m = orc.mask(mag[:, :, c], period)
            m[1:cut + 1, :] = 1
            masks.append(m.T)
        Y = np.stack([_half(spec[:, :, c], w) for c in range(2)])
        y = ref.inverse_piece(Y, w, w - h, length, 1.0 / sum(window[0:w:h]), mask=np.stack(masks))
        wts = ref.fade_weights(length, j, len(segs), step, overlap)
        assert np.array_equal(wts, orc.segment_weights(j, segs, overlap))
        pieces.append((start, y, wts))
    for first, count in ((0, len(segs)), (2, 3)):
        got = ref.inverse(np.zeros((n, 2)), pieces[first:first + count], mode=1)
        want = orc.extended_range(x, fs, first, count, p)
        assert np.max(np.abs(got - want)) < 1e-12
    assert np.max(np.abs(ref.inverse(np.zeros((n, 2)), pieces, mode=1) - orc.extended(x, fs, p))) < 1e-12


def test_single_fade_is_the_rising_half_of_the_triangle():
    import scipy.signal
    for n_out, fade in ((100, 10), (7, 10), (50, 0), (64, 64)):
        w = ref.single_fade_weights(n_out, fade)
        tri = scipy.signal.windows.triang(2 * fade) if fade else np.ones(0)
        k = min(n_out, fade)
        assert np.allclose(w[:k], tri[:k], rtol=0, atol=1e-15) and np.all(w[k:] == 1)


@pytest.mark.parametrize("centred", [True, False])
def test_forward_reference_against_definitions(centred):
    w, h = 64, 32
    window = np.hamming(w)
    rng = np.random.default_rng(5)
    from repet import _native
    lib = _native.lib()
    for n in (1, h - 1, h, h + 1, w - 1, w, w + 1, 97, 331):
        x = rng.standard_normal(n).astype(np.float32)
        got = ref.stft_half(x, window, h, centred)
        t = lib.repet_frame_count(n, w, h, int(centred))
        assert got.shape == (max(t, 0), w // 2 + 1) and ref.frame_count(n, w, h, centred) == max(t, 0)
        # frame by frame from the definition: sample i of frame t is x[t h + i - pad], zero outside the clip
        pad = w // 2 if centred else 0
        w32 = window.astype(np.float32).astype(np.float64)
        for fr in range(got.shape[0]):
            idx = fr * h + np.arange(w) - pad
            frame = np.where((idx >= 0) & (idx < n), x.astype(np.float64)[np.clip(idx, 0, n - 1)], 0.0) * w32
            assert np.max(np.abs(got[fr] - np.fft.rfft(frame))) < 1e-12
    if centred:
        x = rng.standard_normal(500).astype(np.float32)
        assert np.array_equal(ref.stft_half(x, window, h), orc.stft(x.astype(np.float64), window.astype(np.float32).astype(np.float64), h)[:w // 2 + 1].T)


def test_forward_side_products_and_batch_geometry():
    w, h = 64, 32
    window = np.hamming(w)
    rng = np.random.default_rng(6)
    audio = rng.standard_normal((700, 3)).astype(np.float32)
    audio[200:200 + 3 * w] = 0                                        # a silent stretch: whole silent frames
    r = ref.forward(audio, window, h, True, sample_offset=50, n_samples=300, n_batch=2, batch_sample_stride=310)
    assert r["X"].shape == (2, 3, ref.frame_count(300, w, h, True), w // 2 + 1)
    for b in range(2):
        clip = audio[50 + 310 * b:][:300]
        for c in range(3):
            assert np.array_equal(r["X"][b, c], ref.stft_half(clip[:, c], window, h))
    assert np.array_equal(r["V"], np.abs(r["X"])) and np.array_equal(r["Vm"], r["V"].mean(axis=1)) and np.array_equal(r["P"], r["Vm"] ** 2)
    silent = ~np.any(r["Vm"] > 0, axis=2)
    assert silent.any() and np.all(np.isnan(r["Vn"][silent])) and np.all(r["V"].transpose(0, 2, 1, 3)[silent] == 0)
    assert np.allclose(np.sum(r["Vn"][~silent] ** 2, axis=-1), 1.0, rtol=0, atol=1e-12)


def test_plane_decode_inverts_the_split():
    rng = np.random.default_rng(7)
    fs = 96
    rows = (rng.random((5, 11, fs)) ** 4).astype(np.float32)
    rows[0, 0] = 0
    rows[1, 2, 5] = 2.0 ** -30
    # the unit rows: fixed scale 2^7
    planes = ref.split_planes(rows, 128.0)
    assert planes.dtype == np.float16 and planes.shape == (5, 11, 2 * fs)
    e = 37                                                        # component e: hi at 64 (e >> 5) + (e & 31), lo 32 further
    v = np.float32(rows[2, 3, e] * np.float32(128))
    assert planes[2, 3, 64 * (e >> 5) + (e & 31)] == np.float16(v)
    assert planes[2, 3, 64 * (e >> 5) + (e & 31) + 32] == np.float16(v - np.float32(np.float16(v)))
    back = ref.decode_planes(planes, 1.0 / 128)
    assert np.all(np.abs(back - rows) <= 2.0 ** -21 * np.abs(rows) + 2.0 ** -24 / 128)
    # the power rows: every row by its own power of two
    scale = np.array([[ref.row_scale(float(r.max())) for r in plane] for plane in rows], dtype=np.float32)
    assert scale[0, 0] == 1 and np.all(np.log2(scale) == np.round(np.log2(scale)))
    top = rows.max(axis=-1) * scale
    assert np.all((top[rows.max(axis=-1) > 0] >= 2 ** 13) & (top[rows.max(axis=-1) > 0] < 2 ** 14))
    planes = ref.split_planes(rows, scale)
    back = ref.decode_planes(planes, 1.0 / scale)
    assert np.all(np.abs(back - rows) <= 2.0 ** -21 * np.abs(rows) + 2.0 ** -24 / scale[..., None])
