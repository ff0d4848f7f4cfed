"""Float64 references of the chain rows -> banded Gram -> windowed diagonal sums -> argmax -> per-frame periods, written from
the formulas in the comments of gram.hip / gram_f16.hip and from oracle/repet_oracle.py, not from the kernels.
tests/test_gram_reference.py pins the chain to the oracle on the CPU; tests/test_gpu_gram_band_stages.py holds the HIP
kernels against it. The full similarity matrix, its segment records and the unit rows (tests/test_gpu_gram_full_stages.py) are
the same statements without the band."""
import numpy as np

from stft_reference import decode_planes, row_scale, split_planes  # noqa: F401  (re-exported: one restatement of the split)

U = 2.0 ** -24            # unit roundoff of fp32
UNIT_SCALE = 128.0        # the fixed scale of the unit rows' planes (2^7)


def pad_bins(rows, fs):
    """(..., F) -> (..., FS) float64 with zero pad bins."""
    rows = np.asarray(rows, dtype=np.float64)
    out = np.zeros(rows.shape[:-1] + (fs,))
    out[..., :rows.shape[-1]] = rows
    return out


def band_of_gram(gram, n_lags, lookback=False):
    """The band of a (T, T) matrix g[i][j]: forward band[t][l] = g[t][t + l], look-back band[j][l] = g[j - l][j]; NaN marks
    the cells outside the matrix (t + l >= T, j - l < 0)."""
    t = gram.shape[0]
    band = np.full((t, n_lags), np.nan)
    for l in range(min(n_lags, t)):
        d = np.diagonal(gram, l)
        if lookback:
            band[l:, l] = d
        else:
            band[:t - l, l] = d
    return band


def band64(rows, n_lags, lookback=False):
    """band[t][l] = row t . row t + l in float64 (look-back: row j . row j - l); rows (T, F)."""
    r = np.asarray(rows, dtype=np.float64)
    return band_of_gram(r @ r.T, n_lags, lookback)


def band_abs64(rows, n_lags, lookback=False):
    """sum_k |a_k b_k| of every band entry: the scale of the fp32 kernel's accumulation bound."""
    r = np.abs(np.asarray(rows, dtype=np.float64))
    return band_of_gram(r @ r.T, n_lags, lookback)


def plane_halves(planes):
    """(hi, lo) of planes (..., 2 FS) [kb][hi 32 | lo 32] as float64 (..., FS) each."""
    planes = np.asarray(planes)
    fs = planes.shape[-1] // 2
    blocks = planes.reshape(planes.shape[:-1] + (fs // 32, 2, 32)).astype(np.float64)
    shape = planes.shape[:-1] + (fs,)
    return blocks[..., 0, :].reshape(shape), blocks[..., 1, :].reshape(shape)


def three_product_band(planes, inv, n_lags, lookback=False):
    """What the f16-split kernel is asked to compute, exactly: sum (hi hi' + hi lo' + lo hi') inv_i inv_j in float64 from the
    planes (T, 2 FS) it read (inv: one value per row, or the scalar 1 / 128 of the unit rows). Returns (band, sum of the
    |products|) -- the second is the scale of the accumulation bound."""
    hi, lo = plane_halves(planes)
    inv = np.broadcast_to(np.asarray(inv, dtype=np.float64), hi.shape[:1])
    outer = inv[:, None] * inv[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        g = (hi @ hi.T + hi @ lo.T + lo @ hi.T) * outer
        ah, al = np.abs(hi), np.abs(lo)
        s = (ah @ ah.T + ah @ al.T + al @ ah.T) * outer
    return band_of_gram(g, n_lags, lookback), band_of_gram(s, n_lags, lookback)


def split_error(rows, scale):
    """Bound of |decoded planes - rows| per component: 2^-21 |v| + 2^-24 / scale (hi = f16(v s), lo = f16(v s - hi)); a zero
    splits into zeros. rows (T, FS), scale per row or scalar."""
    r = np.abs(np.asarray(rows, dtype=np.float64))
    sc = np.broadcast_to(np.asarray(scale, dtype=np.float64), r.shape[:1])[:, None]
    return np.where(r == 0, 0.0, 2.0 ** -21 * r + 2.0 ** -24 / sc)


def split_band_bound(rows, scale, n_lags, lookback=False):
    """|three-product band - float64 band| at most: with a' = a + da, |da| <= split_error, sum a' b' - sum a b is bounded by
    sum (|a| db + |b| da + da db); the dropped lo lo' is at most 2^-22 of each |a' b'| (|lo| <= 2^-11 |hi|)."""
    a = np.abs(np.asarray(rows, dtype=np.float64))
    d = split_error(rows, scale)
    ad = a @ d.T
    g = ad + ad.T + d @ d.T + 2.0 ** -22 * ((a + d) @ (a + d).T)
    return band_of_gram(g, n_lags, lookback)


# ---- the full matrix (tests/test_gpu_gram_full_stages.py): the same statements without the band ------------------------------
def full64(rows):
    """S[i][j] = row i . row j in float64; rows (T, F)."""
    r = np.asarray(rows, dtype=np.float64)
    return r @ r.T


def full_abs64(rows):
    """sum_k |a_k b_k| of every entry: the scale of the fp32 kernel's accumulation bound."""
    r = np.abs(np.asarray(rows, dtype=np.float64))
    return r @ r.T


def three_product_full(planes, inv):
    """three_product_band for every pair of rows: (sum (hi hi' + hi lo' + lo hi') inv_i inv_j, the same sum of |products|), both
    (T, T) float64, from the planes (T, 2 FS) the kernel read."""
    hi, lo = plane_halves(planes)
    inv = np.broadcast_to(np.asarray(inv, dtype=np.float64), hi.shape[:1])
    outer = inv[:, None] * inv[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        hl = hi @ lo.T
        g = (hi @ hi.T + hl + hl.T) * outer
        ah, al = np.abs(hi), np.abs(lo)
        ahl = ah @ al.T
        s = (ah @ ah.T + ahl + ahl.T) * outer
    return g, s


def split_full_bound(rows, scale):
    """split_band_bound for every pair of rows: |three-product matrix - float64 matrix| at most sum (|a| db + |b| da + da db) with
    da, db the split bound, + the dropped lo lo' <= 2^-22 of each |a' b'|."""
    a = np.abs(np.asarray(rows, dtype=np.float64))
    d = split_error(rows, scale)
    ad = a @ d.T
    return ad + ad.T + d @ d.T + 2.0 ** -22 * ((a + d) @ (a + d).T)


def segment_records(s, t):
    """The segment records of the rows of s[:t, :t] (peaks.h): for every aligned run of 32 columns (the last one ragged) the
    largest value with NaN counted as +inf, the largest of the run's OTHER elements (-inf for a run with one live column) and the
    offset of the largest inside the run, the lowest among equals. Returns (top, second, at), each (t, ceil(t / 32)), the values in
    the dtype of s."""
    s = np.asarray(s)[:t, :t]
    n_seg = -(-t // 32)
    padded = np.full((t, n_seg * 32), -np.inf, dtype=s.dtype)
    padded[:, :t] = np.where(np.isnan(s), np.inf, s)
    runs = padded.reshape(t, n_seg, 32)
    at = np.argmax(runs, axis=2)                                  # (the lowest index among equals)
    top = np.take_along_axis(runs, at[:, :, None], axis=2)[:, :, 0]
    others = runs.copy()
    np.put_along_axis(others, at[:, :, None], -np.inf, axis=2)
    return top, others.max(axis=2), at.astype(np.int32)


def unit_rows64(rows):
    """row / ||row|| in float64 (repet.py:1220 for a frame-major matrix); a zero row gives NaN."""
    r = np.asarray(rows, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return r / np.sqrt(np.sum(r * r, axis=-1, keepdims=True))


def window_sums64(band, n_lags, n_freq, start0, step, length, n_windows):
    """beat[w][l] = sum of band[t][l] over the t with t and t + l inside window w = [start0 + w step, + length) and inside
    [0, T), divided by (length - l) n_freq (the unbiased autocorrelation, averaged over the bins); 0 for l >= length. band
    (T, >= n_lags). Returns (beat (n_windows, n_lags), the same sums of |band|, the number of rows added (n_windows, n_lags))."""
    band = np.asarray(band, dtype=np.float64)
    t = band.shape[0]
    beat = np.zeros((n_windows, n_lags))
    mag = np.zeros((n_windows, n_lags))
    count = np.zeros((n_windows, n_lags), dtype=np.int64)
    for w in range(n_windows):
        a = start0 + w * step
        first = max(a, 0)
        for l in range(min(n_lags, length)):
            last = min(a + length - 1 - l, t - 1 - l)
            if last >= first:
                col = band[first:last + 1, l]
                beat[w, l] = col.sum() / ((length - l) * n_freq)
                mag[w, l] = np.abs(col).sum() / ((length - l) * n_freq)
                count[w, l] = last + 1 - first
    return beat, mag, count


def periods_rule(beat_rows, lo, hi, n_lags_for_clamp):
    """period = lo + 1 + (first arg-max of beat[lo:h]), h = min(hi, n_lags_for_clamp // 3); a value in that range that is not
    finite gives lo + 1: the reference's autocorrelation goes through an FFT over time, so one such frame makes every lag NaN
    and np.argmax returns 0. beat_rows (n, >= h)."""
    rows = np.atleast_2d(np.asarray(beat_rows, dtype=np.float64))
    h = min(hi, n_lags_for_clamp // 3)
    assert h > lo
    cut = rows[:, lo:h]
    out = np.argmax(cut, axis=1) + 1 + lo
    out[~np.all(np.isfinite(cut), axis=1)] = lo + 1
    return out


def expand_periods(win_periods, step, t, lo):
    """Per-frame periods of `adaptive`: frames [i, min(i + step - 1, T)) and frame i of window i / step copy its period; frame
    i + step - 1 keeps the all-zero column of the reference's beat spectrogram, whose arg-max is 0: lo + 1."""
    out = np.full(t, lo + 1, dtype=np.int64)
    for w, i in enumerate(range(0, t, step)):
        out[i] = win_periods[w]
        out[i:min(i + step - 1, t)] = win_periods[w]
    return out


def beat_spectrogram(power_rows, seg_len, seg_step):
    """The chain for `adaptive`: (window beat rows (n_windows, seg_len), the (seg_len, T) beat spectrogram with the hole)."""
    rows = np.asarray(power_rows, dtype=np.float64)
    t, f = rows.shape
    n_win = -(-t // seg_step)
    band = band64(rows, seg_len)                      # (the sums below never reach a cell outside the matrix)
    win, _, _ = window_sums64(band, seg_len, f, -(seg_len // 2), seg_step, seg_len, n_win)
    out = np.zeros((seg_len, t))
    for w, i in enumerate(range(0, t, seg_step)):
        out[:, i] = win[w]
        out[:, i:min(i + seg_step - 1, t)] = win[w][:, None]
    return win, out
