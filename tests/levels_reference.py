"""NumPy reference of the level record (``repet.LEVELS``, REPET_LEVEL_* of include/repet_hip.h), for the tests: what the device
reduction must return for given float64 signals. Not the code under test and never derived from it."""
import numpy as np

FIELDS = 8
MIX_ENERGY, BG_ENERGY, FG_ENERGY, MIX_PEAK, BG_PEAK, FG_PEAK, LIVE, NONFINITE = range(FIELDS)


def levels(mix, bg, fg, live=None):
    """The record ``(S, C, 8)`` of an emission: ``mix``, ``bg``, ``fg`` float64 ``(S, n, C)``, ``live`` a boolean ``(S, n)``
    (None: every sample is live). A sample that is not live adds zero to every field, whatever the signals hold there, and is
    not counted. Energies are plain sums (NaN and inf propagate), peaks skip NaN (``fmax``), are inf for an infinite sample and
    0 with nothing live; field 7 counts the live samples whose mixture is NaN or infinite."""
    mix, bg, fg = (np.asarray(a, dtype=np.float64) for a in (mix, bg, fg))
    assert mix.ndim == 3 and mix.shape == bg.shape == fg.shape
    S, n, C = mix.shape
    live = np.ones((S, n), dtype=bool) if live is None else np.asarray(live, dtype=bool)
    assert live.shape == (S, n)
    on = np.broadcast_to(live[:, :, None], mix.shape)
    out = np.zeros((S, C, FIELDS), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, a in enumerate((mix, bg, fg)):
            a = np.where(on, a, 0.0)
            out[:, :, MIX_ENERGY + k] = np.sum(a * a, axis=1)
            out[:, :, MIX_PEAK + k] = np.fmax.reduce(np.abs(a), axis=1, initial=0.0)
    out[:, :, LIVE] = np.sum(on, axis=1)
    out[:, :, NONFINITE] = np.sum(on & ~np.isfinite(mix), axis=1)
    return out


def check(got, want, label=""):
    """``got`` against the reference record ``want``: peaks and the two counts identical; energies within ``4 * n * 2**-53 *
    E_want`` with ``n`` the live samples of that stream and channel (each side squares with one rounding and sums ``n``
    non-negative terms in some order: at most about ``n * 2**-53`` relative per side, ``2 n * 2**-53`` between them to first
    order; the factor 4 covers the second-order terms and an fma on one side), a NaN or infinite energy identical. Returns the
    largest observed ratio of an energy's error to its bound."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(got[..., MIX_PEAK:], want[..., MIX_PEAK:], equal_nan=True), \
        f"{label}: peaks or counts differ\n{got[..., MIX_PEAK:]}\n{want[..., MIX_PEAK:]}"
    worst = 0.0
    for f in (MIX_ENERGY, BG_ENERGY, FG_ENERGY):
        g, w, n = got[..., f], want[..., f], want[..., LIVE]
        finite = np.isfinite(w)
        assert np.array_equal(g[~finite], w[~finite], equal_nan=True), f"{label}: field {f}: {g[~finite]} against {w[~finite]}"
        bound = 4.0 * n[finite] * 2.0 ** -53 * w[finite]
        err = np.abs(g[finite] - w[finite])
        assert (err <= bound).all(), f"{label}: field {f} off by up to {err.max():.3e}, bound {bound[np.argmax(err - bound)]:.3e}"
        if np.any(bound > 0):
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    return worst
