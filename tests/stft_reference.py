"""Float64 references of what launch_stft and launch_istft_ola compute, written from the definitions (the oracle's STFT,
np.fft, the reference's soft mask and cross-fade), not from the kernels. tests/test_stft_reference.py pins them to the
oracle on the CPU; tests/test_gpu_stft_stages.py holds the HIP kernels against them."""
import numpy as np

from oracle import repet_oracle as orc

EPS = np.finfo(float).eps


def frame_count(n, w, h, centred):
    """Frames of a clip of n samples: the centred form of repet.py:1018-1028, the plain one of repet.py:781."""
    if centred:
        return orc.centred_frame_count(n, w, h)
    return max(int(np.ceil((n - w) / h)) + 1, 0)          # (no frame until W - H + 1 samples are there)


def stft_half(x, window, h, centred=True):
    """(T, F) complex128 half spectrum of one channel. x and window are taken as the fp32 values the kernels see."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    window = np.asarray(window, dtype=np.float32).astype(np.float64)
    w = len(window)
    f = w // 2 + 1
    if centred:
        return np.ascontiguousarray(orc.stft(x, window, h)[:f].T)
    t = frame_count(len(x), w, h, False)
    if t == 0:
        return np.zeros((0, f), dtype=complex)
    padded = np.zeros((t - 1) * h + w)
    padded[:len(x)] = x
    frames = np.lib.stride_tricks.sliding_window_view(padded, w)[::h][:t] * window
    return np.fft.fft(frames, axis=1)[:, :f]


def forward(audio, window, h, centred=True, sample_offset=0, n_samples=None, n_batch=1, batch_sample_stride=0):
    """What the forward launcher is asked for: X (B, C, T, F) complex128, V = |X|, Vm = mean over channels (B, T, F),
    Vn = Vm / ||Vm|| per frame (0 / 0 = NaN for a silent frame, repet.py:1220), P = Vm^2."""
    audio = np.asarray(audio, dtype=np.float32)
    if audio.ndim == 1:
        audio = audio[:, None]
    n = audio.shape[0] - sample_offset if n_samples is None else n_samples
    X = []
    for b in range(n_batch):
        clip = audio[sample_offset + b * batch_sample_stride:][:n]
        assert clip.shape[0] == n
        X.append([stft_half(clip[:, c], window, h, centred) for c in range(audio.shape[1])])
    X = np.array(X)
    V = np.abs(X)
    Vm = V.mean(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        Vn = Vm / np.sqrt(np.sum(Vm * Vm, axis=2, keepdims=True))
    return {"X": X, "V": V, "Vm": Vm, "Vn": Vn, "P": Vm * Vm}


# ---- the f16 hi / lo planes: [row][FS / 32][hi 32 | lo 32] ---------------------------------------------------------------
def split_planes(rows, scale):
    """NumPy restatement of the split: v = x * scale (fp32), hi = f16(v), lo = f16(v - hi). rows (..., FS) with FS a multiple
    of 32, scale a scalar or one value per row (...,). Returns float16 (..., 2 FS)."""
    rows = np.asarray(rows, dtype=np.float32)
    scale = np.asarray(scale, dtype=np.float32)
    v = rows * (scale[..., None] if scale.ndim else scale)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    shape = rows.shape[:-1] + (rows.shape[-1] // 32, 32)
    return np.concatenate((hi.reshape(shape), lo.reshape(shape)), axis=-1).reshape(rows.shape[:-1] + (2 * rows.shape[-1],))


def decode_planes(planes, inv_scale):
    """(hi + lo) * inv_scale in float64: inv_scale = 1 / 128 for the unit rows (Vh), Ph_inv[row] for the power rows (Ph)."""
    planes = np.asarray(planes)
    fs = planes.shape[-1] // 2
    blocks = planes.reshape(planes.shape[:-1] + (fs // 32, 2, 32)).astype(np.float64)
    inv = np.asarray(inv_scale, dtype=np.float64)
    return (blocks[..., 0, :] + blocks[..., 1, :]).reshape(planes.shape[:-1] + (fs,)) * (inv[..., None] if inv.ndim else inv)


def row_scale(m):
    """The power of two that brings a row's largest value m into [2^13, 2^14); 1 for a row without a positive finite one."""
    if not (m > 0 and np.isfinite(m)):
        return 1.0
    return float(np.ldexp(1.0, 14 - np.frexp(m)[1]))


# ---- inverse -------------------------------------------------------------------------------------------------------------
def model_mask(mag, model, period, cutoff):
    """soft_mask(|Y|, model[t mod period]) of one channel, (T, F), bins 1 .. cutoff forced to 1 (repet.py:185)."""
    t = mag.shape[0]
    m = orc.soft_mask(mag, np.asarray(model, dtype=np.float64)[np.arange(t) % period])
    m[:, 1:cutoff + 1] = 1
    return m


def overlap_add(Y, w):
    """irfft of every frame of Y (T, F), overlap-added at hop N = w / 2: (T + 1) N padded samples."""
    t = Y.shape[0]
    n = w // 2
    frames = np.fft.irfft(Y, n=w, axis=1)
    y = np.zeros((t + 1) * n)
    rows = y.reshape(t + 1, n)
    rows[:t] += frames[:, :n]
    rows[1:] += frames[:, n:]
    return y


def inverse_piece(Y, w, trim, n_out, scale=1.0, mask=None):
    """One clip: Y (C, T, F) -> (n_written, C) float64, the samples [trim, trim + n_out) of the padded overlap-add times
    scale, as far as they exist (hop T, the last frame's tail, is the last)."""
    Y = np.asarray(Y, dtype=np.complex128)
    if mask is not None:
        Y = Y * np.asarray(mask, dtype=np.float64)
    cols = [overlap_add(Y[c], w)[trim:trim + n_out] * scale for c in range(Y.shape[0])]
    return np.stack(cols, axis=1)


def fade_weights(n_out, j, total, step, overlap):
    """Weight of every sample of segment j of `total` equal segments `step` apart (orc.segment_weights)."""
    segs = [(q * step, n_out) for q in range(total)]
    return orc.segment_weights(j, segs, overlap) if overlap > 0 else np.ones(n_out)


def single_fade_weights(n_out, fade_in):
    """A single segment outside a batch: only its own rise over fade_in samples (no later segment)."""
    w = np.ones(n_out)
    if fade_in > 0:
        k = min(fade_in, n_out)
        w[:k] = (2 * np.arange(k) + 1) / (2 * fade_in)
    return w


def inverse(out, pieces, mode=0):
    """Place pieces [(offset, (n, C) samples, weights or None)] into a float64 copy of `out`: mode 0 / 2 store, 1 adds."""
    res = np.array(out, dtype=np.float64, copy=True)
    if res.ndim == 1:
        res = res[:, None]
    for offset, y, wts in pieces:
        y = y if wts is None else y * wts[:len(y), None]
        if mode == 1:
            res[offset:offset + len(y)] += y
        else:
            res[offset:offset + len(y)] = y
    return res
