"""The float64 statement of ``last_frames`` (tests/frames_reference.py) against the oracle it is built from, and
``repet.band_edges``. No GPU.

* With ``start_frames = B`` the statement's samples ARE ``orc.simonline``'s (``np.array_equal``): the loop that forms ``bg`` is
  the oracle's, and the mask that weighted its spectra is the mask ``bg`` was made with.
* Read back from the returned arrays alone, the mask is ``bg / mix``: two more roundings per bin (the product that formed
  ``bg``, the division), so the overlap-add of the ``ifft`` of the ``(bg / mix)``-weighted spectra is the oracle's within
  ``(2 + log2(W)) * 2**-53`` of the overlap-added mean magnitude of the weighted spectra: two roundings of relative size
  ``2**-53`` on every weight, and pocketfft's own error on an input that differs by that much, about ``2**-53`` per butterfly
  stage. Bit equality is not attainable there: ``(m * v) / v != m`` for most ``m``.
* ``bg + fg == mix`` within one float64 rounding of ``mix``.
"""
import functools

import numpy as np
import pytest

import repet
from oracle import repet_oracle as orc
from frames_reference import band_energies, frames_from
from helpers import golden_input

CASES = ["small_mono", "small_stereo"]


@functools.lru_cache(maxsize=None)
def statement(case):
    x, fs = golden_input(case)
    _, _, h = orc.stft_geometry(fs)
    b = round(orc.Params().buffer_length * fs / h)
    out = frames_from(np.array(x), fs, b)
    for a in out:
        a.setflags(write=False)
    return out, b


@pytest.mark.parametrize("case", CASES)
def test_samples_are_the_oracles(case):
    x, fs = golden_input(case)
    (samples, mix, bg, fg), b = statement(case)
    want = orc.simonline(np.array(x), fs)
    assert np.array_equal(samples, want)
    assert mix.shape == bg.shape == fg.shape and mix.shape[1:] == (x.shape[1], orc.stft_geometry(fs)[0] // 2 + 1)
    assert not bg[:b - 1].any() and np.array_equal(fg[:b - 1], mix[:b - 1])       # warm-up: nothing removed
    assert bg[b - 1:].any() and fg[b - 1:].any()
    cut = orc.cutoff_bins(orc.Params(), fs, orc.stft_geometry(fs)[0])
    assert cut >= 1 and np.array_equal(bg[b - 1:, :, 1:cut + 1], mix[b - 1:, :, 1:cut + 1])   # the high-pass rule


@pytest.mark.parametrize("case", CASES)
def test_weighted_spectra_overlap_add_to_the_oracle(case):
    x, fs = golden_input(case)
    x = np.array(x)
    (_, mix, bg, _), b = statement(case)
    want = orc.simonline(x, fs)
    w, window, h = orc.stft_geometry(fs)
    n, ch = x.shape
    t = mix.shape[0]
    padded = np.zeros(((t - 1) * h + w, ch))
    padded[:n] = x
    got, scale = np.zeros_like(padded), np.zeros_like(padded)
    for j in range(b - 1, t):
        for c in range(ch):
            spec = np.fft.fft(padded[j * h:j * h + w, c] * window)
            with np.errstate(invalid="ignore", divide="ignore"):
                m = bg[j, c] / mix[j, c]
            assert np.isfinite(m).all()                                   # (no silent bin in these fixtures)
            full = np.concatenate((m, m[-2:0:-1]))
            got[j * h:j * h + w, c] += np.real(np.fft.ifft(full * spec))
            scale[j * h:j * h + w, c] += np.mean(np.abs(full * spec))
    cola = sum(window[0:w:h])
    got, scale = got[:n] / cola, scale[:n] / cola
    bound = (2 + np.log2(w)) * 2.0 ** -53 * scale
    err = np.abs(got - want)
    print(f"{case}: largest error {err.max():.3e}, largest ratio to its bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.array_equal(got[:(b - 1) * h], want[:(b - 1) * h])             # zeros before the first processed frame
    assert (err <= bound).all()


@pytest.mark.parametrize("case", CASES)
def test_background_plus_foreground_is_the_mixture(case):
    (_, mix, bg, fg), _ = statement(case)
    assert (np.abs((bg + fg) - mix) <= np.spacing(mix)).all()
    assert (bg >= 0).all() and (bg <= mix * (1 + 2.0 ** -52)).all()


def test_band_energies_by_hand():
    m = np.array([[1.0, 2.0, 3.0, 4.0, 5.0], [0.5, 0.0, np.nan, 1.0, 2.0]])
    got = band_energies(m, [0, 2, 2, 3, 5])
    assert got.dtype == np.float64 and got.shape == (2, 4)
    assert got[0].tolist() == [5.0, 0.0, 9.0, 41.0]
    assert got[1, :2].tolist() == [0.25, 0.0] and np.isnan(got[1, 2]) and got[1, 3] == 5.0
    assert band_energies(np.zeros((3, 0, 2, 7)), [0, 7]).shape == (3, 0, 2, 1)


@pytest.mark.parametrize("fs", [8000, 16000, 44100, 48000])
def test_band_edges_defaults_cover_every_bin(fs):
    w = orc.stft_geometry(fs)[0]
    f = w // 2 + 1
    for n in (1, 2, 24, 32, 40, 128):
        e = repet.band_edges(fs, n)
        assert len(e) == n + 1 and all(isinstance(v, int) for v in e)
        assert e[0] == 0 and e[-1] == f
        assert all(a <= b for a, b in zip(e, e[1:]))
    e = repet.band_edges(fs, 32)
    widths = np.diff(e)
    assert widths[-1] > widths[0] and widths.sum() == f                      # mel: wider towards the top, no bin lost


def test_band_edges_range_and_refusals():
    fs = 44100
    w = orc.stft_geometry(fs)[0]
    e = repet.band_edges(fs, 24, f_min=100.0, f_max=8000.0)
    assert e[0] == round(100.0 * w / fs) and e[-1] == round(8000.0 * w / fs) + 1
    assert all(a <= b for a, b in zip(e, e[1:])) and len(e) == 25
    # equally spaced on the mel scale, to the rounding to bins
    mel = lambda hz: 2595.0 * np.log10(1.0 + hz / 700.0)
    steps = np.diff(mel(np.array(e) * fs / w))
    assert np.max(np.abs(steps - steps.mean())) <= 2 * (mel(200.0 + fs / w) - mel(200.0))
    assert repet.band_edges(8000, 1, f_min=0.0, f_max=0.0) == [0, 1]
    for bad in (dict(number_bands=0), dict(number_bands=4, f_min=-1.0), dict(number_bands=4, f_max=fs), dict(number_bands=4, f_min=9.0, f_max=3.0)):
        with pytest.raises(ValueError):
            repet.band_edges(fs, **bad)
