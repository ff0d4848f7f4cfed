"""The float64 chain of tests/gram_reference.py -- band -> windowed diagonal sums -> periods -- pinned to the oracle's beat
spectrum, beat spectrogram and periods: the yardstick of tests/test_gpu_gram_band_stages.py is tested here, without a GPU."""
import numpy as np
import pytest

from oracle import repet_oracle as orc

import gram_reference as ref


def power(f, t, seed):
    """A random power spectrogram (F, T) with a slow repetition in it, so that the arg-max is not a coin toss."""
    rs = np.random.RandomState(seed)
    base = rs.rand(f, 7) ** 2
    return base[:, np.arange(t) % 7] + 0.3 * rs.rand(f, t)


@pytest.mark.parametrize("f,t", [(5, 1), (17, 40), (33, 129), (9, 300)])
def test_band_and_window_sums_are_the_oracle_beat_spectrum(f, t):
    p = power(f, t, f + t)
    band = ref.band64(p.T, t)
    beat, _, count = ref.window_sums64(band, t, f, 0, 0, t, 1)
    want = orc.beatspectrum(p)
    assert np.max(np.abs(beat[0] - want)) <= 1e-12 * np.max(np.abs(want))
    assert np.array_equal(count[0], t - np.arange(t))
    # the look-back layout holds the same numbers: band[j][l] of it is band[j - l][l] of the forward one
    back = ref.band64(p.T, t, lookback=True)
    for l in sorted({0, min(1, t - 1), t // 2, t - 1}):
        assert np.array_equal(back[l:, l], band[:t - l, l]) and np.all(np.isnan(back[:l, l])) and np.all(np.isnan(band[t - l:, l]))
    if t >= 30:
        pr = [2, t]
        assert ref.periods_rule(beat, pr[0], pr[1], t)[0] == orc.periods(want, pr)
        assert ref.periods_rule(want[None], pr[0], pr[1], t)[0] == orc.periods(want, pr)


@pytest.mark.parametrize("f,t,seg_len,seg_step", [(9, 100, 30, 7), (9, 100, 31, 1), (5, 61, 40, 61), (5, 61, 40, 200), (4, 50, 90, 9),
                                                  (3, 300, 270, 40)])
def test_chain_is_the_oracle_beat_spectrogram_hole_included(f, t, seg_len, seg_step):
    p = power(f, t, seg_len + seg_step)
    win, got = ref.beat_spectrogram(p.T, seg_len, seg_step)
    want = orc.beatspectrogram(p, seg_len, seg_step)
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    if seg_step > 1 and seg_step - 1 < t:
        assert np.all(got[:, seg_step - 1] == 0)
    lo, hi = 2, seg_len
    want_periods = orc.periods(want, [lo, hi])
    frames = ref.expand_periods(ref.periods_rule(win, lo, hi, seg_len), seg_step, t, lo)
    assert np.array_equal(frames, want_periods)
    assert np.array_equal(ref.periods_rule(want.T, lo, hi, seg_len), want_periods)


def test_period_rule_on_ties_clamp_and_values_that_are_not_finite():
    beat = np.zeros((4, 300))
    beat[0, [70, 134, 198]] = 5.0                            # exact ties: the first wins
    beat[1, 99] = 1.0                                        # n_lags // 3 = 100 clamps hi = 250
    beat[1, 100] = 9.0
    beat[2, 50] = np.inf                                     # np.argmax would point at it; the reference's whole row is NaN
    beat[3, 10] = np.nan
    beat[3, 40] = 3.0
    got = ref.periods_rule(beat, 8, 250, 300)
    assert list(got) == [71, 100, 9, 9]
    for row, g in zip(beat[:2], got[:2]):
        assert g == orc.periods(row, [8, 250])
    assert orc.periods(np.full(300, np.nan), [8, 250]) == 9   # the all-NaN row the reference would hold


def test_three_product_band_against_the_split_it_restates():
    rs = np.random.RandomState(3)
    rows = (rs.rand(40, 64) * np.exp2(rs.randint(-40, 41, size=(40, 1)))).astype(np.float32)
    rows[7] = 0
    scale = np.array([ref.row_scale(float(m)) for m in rows.max(axis=1)], dtype=np.float32)
    planes = ref.split_planes(rows, scale)
    inv = 1.0 / scale.astype(np.float64)
    assert np.all(np.abs(ref.decode_planes(planes, inv) - rows) <= ref.split_error(rows, scale))
    band, mag = ref.three_product_band(planes, inv, 40)
    want = ref.band64(rows, 40)
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(band), ~ok)
    assert np.all(np.abs(band - want)[ok] <= ref.split_band_bound(rows, scale, 40)[ok])
    assert np.all(band[7][ok[7]] == 0) and np.all(mag[ok] >= np.abs(band[ok]))


# ---- the full matrix: the yardstick of tests/test_gpu_gram_full_stages.py ---------------------------------------------------
def test_three_product_full_holds_the_band_it_contains():
    rs = np.random.RandomState(4)
    rows = rs.rand(70, 64).astype(np.float32) ** 2
    rows[3] = 0
    rows[9, 5] = 1.0
    planes = ref.split_planes(rows, np.full(70, ref.UNIT_SCALE, dtype=np.float32))
    inv = 1.0 / ref.UNIT_SCALE
    g, s = ref.three_product_full(planes, inv)
    eps = 2.0 ** -52                                          # (the two add the same float64 products in another order)
    for n_lags in (1, 33, 70):
        for lookback in (False, True):
            band, mag = ref.three_product_band(planes, inv, n_lags, lookback)
            ok = ~np.isnan(band)
            assert np.array_equal(np.isnan(ref.band_of_gram(g, n_lags, lookback)), ~ok) and np.sum(ok) == sum(70 - l for l in range(n_lags))
            assert np.all(np.abs(ref.band_of_gram(g, n_lags, lookback) - band)[ok] <= 3 * 64 * eps * mag[ok])
            assert np.all(np.abs(ref.band_of_gram(s, n_lags, lookback) - mag)[ok] <= 3 * 64 * eps * mag[ok])
    want = ref.full64(rows)
    assert np.all(np.abs(g - want) <= ref.split_full_bound(rows, ref.UNIT_SCALE))
    assert np.array_equal(ref.band_of_gram(ref.split_full_bound(rows, ref.UNIT_SCALE), 33)[:37, :33],
                          ref.split_band_bound(rows, ref.UNIT_SCALE, 33)[:37, :33])
    assert np.all(g[3] == 0) and np.all(s >= np.abs(g)) and np.array_equal(ref.full_abs64(rows), want)   # (rows >= 0)


def test_segment_records_on_a_matrix_written_by_hand():
    """Three runs, the last ragged (70 = 32 + 32 + 6): ties inside a run and across a border, a NaN, a run of one live column."""
    t = 70
    s = np.full((t, t + 2), 0.25, dtype=np.float32)          # (a pitched image: the columns from t on are not the matrix's)
    s[:, t:] = 9.0
    s[0, [5, 9]] = 0.5                                        # a tie inside run 0: the lower index, second = top
    s[1, [31, 32]] = 0.75                                     # a tie across the border 31 | 32: one in each run
    s[2, 40] = np.nan                                         # NaN counts as +inf
    s[2, 41] = 0.5
    s[3, 64:70] = [0.1, 0.3, 0.3, 0.2, 0.1, 0.0]              # the ragged run
    s[4, 33] = np.inf
    s[4, 35] = np.nan                                         # +inf and NaN tie: the lower index
    s[5, 3] = -np.inf
    top, second, at = ref.segment_records(s, t)
    assert top.shape == second.shape == at.shape == (t, 3) and top.dtype == np.float32 and at.dtype == np.int32
    assert (top[0, 0], second[0, 0], at[0, 0]) == (0.5, 0.5, 5)
    assert (top[1, 0], second[1, 0], at[1, 0]) == (0.75, 0.25, 31) and (top[1, 1], second[1, 1], at[1, 1]) == (0.75, 0.25, 0)
    assert (top[2, 1], second[2, 1], at[2, 1]) == (np.inf, 0.5, 8)
    assert (top[3, 2], at[3, 2]) == (np.float32(0.3), 1) and second[3, 2] == np.float32(0.3)
    assert (top[4, 1], second[4, 1], at[4, 1]) == (np.inf, np.inf, 1)
    assert (top[5, 0], second[5, 0], at[5, 0]) == (0.25, 0.25, 0)
    assert np.all(top[6:] == 0.25) and np.all(second[6:] == 0.25) and np.all(at[6:] == 0)      # a plateau: the first column
    # a run with one live column: second = -inf
    top, second, at = ref.segment_records(s, 33)
    assert top.shape == (33, 2) and np.all(second[:, 1] == -np.inf) and np.all(at[:, 1] == 0)
    assert (top[1, 1], top[0, 1]) == (0.75, 0.25)
    top, second, at = ref.segment_records(np.array([[np.nan]], dtype=np.float32), 1)
    assert (top[0, 0], second[0, 0], at[0, 0]) == (np.inf, -np.inf, 0)


@pytest.mark.parametrize("f,t", [(5, 1), (17, 40), (33, 129)])
def test_full64_of_unit_rows_is_the_oracle_similarity_matrix(f, t):
    v = np.random.RandomState(f + t).rand(f, t) + 0.01             # (F, T) as the oracle takes it
    unit = ref.unit_rows64(v.T)
    want = orc.selfsimilaritymatrix(v)
    assert np.max(np.abs(ref.full64(unit) - want)) <= 1e-14
    assert np.max(np.abs(np.sum(unit * unit, axis=1) - 1)) <= 1e-14
    assert np.all(np.isnan(ref.unit_rows64(np.zeros((2, f)))))
