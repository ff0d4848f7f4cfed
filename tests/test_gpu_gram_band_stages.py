"""The banded Gram, the windowed diagonal sums, the period arg-max and the expansion to frames, entry by entry: the production
code (exec_gram_band, the second half of run_gram_band, through repet._gram_band_stage; run_band_window_sum -> launch_periods
-> launch_expand_periods through repet._band_periods_stage) against the float64 references of tests/gram_reference.py, in
every form the pipelines run the band in -- exact fp32, f16-split with row-scaled planes, f16-split unit rows, the same in the
look-back layout, and batches of each -- at the shapes where the kernels change path: T around the 128-row tile and past the
8-tile super-block of the tile list (1030 = nine tile rows), FS / 32 = 1 and 2 (their own prologue in the DMA pipeline),
n_lags at the steps of gram_band_diagonals (2 and 130), batches of nine so that the rotation of the tile list wraps.

Bounds (all derived, none fitted to the kernels; u = 2^-24, `terms` are the summed products):
  split, form f16_rows     |decoded planes - row| <= 2^-21 |v| + 2^-24 / scale: hi = f16(v s) leaves a remainder of at most
                           2^-11 |v s| that lo = f16(.) holds to 2^-11 of itself (2^-22 |v s|) or, where lo is subnormal, to
                           2^-25 absolute; the bound tests/test_gpu_stft_stages.py states for Ph. row_inv = 1 / row_scale(max
                           |row|) bit for bit (powers of two), pad rows: zeros, inverse 1.
  kernel vs its own        the exact three-product band sum (hi hi' + hi lo' + lo hi') inv_i inv_j of the planes the kernel read,
  arithmetic (f16 forms)   in float64: the f16 MFMA multiplies exactly and adds in fp32, so an entry is a sum of n = 3 FS terms
                           with one rounding per addition: |error| <= n u sum |terms|. The scales are powers of two: exact.
  kernel vs float64        f16 forms: the accumulation above + the split of both operands, sum (|a| db + |b| da + da db) with
                           da, db the split bound + the dropped lo lo' <= 2^-22 of each |product| (|lo| <= 2^-11 |hi|).
                           fp32 form: a dot product of FS terms in fp32: FS u sum |terms|.
  window sums              beat[w][l] adds n_rows band entries in fp32 and divides once by (len - l) F (an integer below 2^24:
                           exact as a float): n_rows roundings, |error| <= n_rows u sum |band| / ((len - l) F) against the
                           float64 sum of the same fp32 band.
  layout, guards, batches, special rows, periods, expansion: exact.
The largest error met per check is collected in PARITY and printed (and written to $REPET_GRAM_STAGE_PARITY_OUT) by the last
test of the module: profiles/gram_band_stage_parity.txt is that output from an MI355X (documentation; the asserts use the bounds)."""
import os

import numpy as np
import pytest

import repet
import gram_reference as ref
from oracle import repet_oracle as orc

pytestmark = pytest.mark.gpu

U = ref.U
F16_FORMS = ("f16_rows", "f16_unit", "f16_unit_lookback")
PARITY = {}          # (stage, form, check) -> (error / bar, error, bar, shape)
# (T, F, n_lags): every T of {1, 127, 128, 129, 257, 300, 1030}, F of {17, 33, 129, 513, 1025} and n_lags of {1, 2, 64, 128,
# 129, 130, 257, min(T, 431)} at least once
SHAPES = [(1, 17, 1), (127, 33, 64), (127, 17, 127), (128, 17, 128), (128, 129, 2), (129, 129, 129), (129, 33, 2), (257, 33, 130),
          (257, 513, 257), (300, 1025, 300), (300, 129, 1), (1030, 129, 431), (1030, 1025, 128), (1030, 17, 257), (1030, 33, 130)]


def note(stage, form, check, err, bar, shape):
    """Keep the largest error / bar of a check (arrays: the worst entry)."""
    err, bar = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64))
    if err.size == 0:
        return
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    k = int(np.argmax(ratio))
    key = (stage, form, check)
    if key not in PARITY or ratio.flat[k] > PARITY[key][0]:
        PARITY[key] = (float(ratio.flat[k]), float(err.flat[k]), float(bar.flat[k]), shape)


def power_rows(b, t, f, seed):
    """Non-negative rows whose levels span 2^-40 .. 2^+40 inside one matrix; every clip its own matrix."""
    rs = np.random.RandomState(seed)
    return (rs.rand(b, t, f) * np.exp2(rs.randint(-40, 41, size=(b, t, 1)))).astype(np.float32)


def unit_rows(b, t, f, seed):
    rs = np.random.RandomState(seed)
    v = rs.rand(b, t, f) ** 2
    return (v / np.sqrt(np.sum(v * v, axis=2, keepdims=True))).astype(np.float32)


def rows_for(form, b, t, f, seed):
    return unit_rows(b, t, f, seed) if form in ("f16_unit", "f16_unit_lookback") else power_rows(b, t, f, seed)


def fill_word(prefill):
    return np.frombuffer(bytes([prefill]) * 4, dtype=np.uint32)[0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pairs_row(t, n_lags, r, lookback):
    """The band cells (T, n_lags) whose entry pairs row r: forward (t, l) with t == r or t + l == r, look-back (j, l) with j == r
    or j - l == r."""
    rows, lags = np.arange(t)[:, None], np.arange(n_lags)[None, :]
    other = rows - lags if lookback else rows + lags
    return (rows == r) | (other == r)


@np.errstate(all="ignore")                  # (NaN marks the cells outside the matrix)
def check_band(form, rows, n_lags, stride=None, prefill=0xFF, special=(), tag=""):
    """Run one form on rows (B, T, F) and hold every clip to the bounds of the module's docstring. special: rows whose entries are
    expected not to be finite (they hold a NaN or an inf). Returns the stage's result."""
    rows = np.asarray(rows, dtype=np.float32)
    b, t, f = rows.shape
    r = repet._gram_band_stage(rows, n_lags, clip_stride=stride, form=form, prefill=prefill)
    tpad, fs, lp = r["Tpad"], r["FS"], r["LP"]
    stride = tpad if stride is None else stride
    shape = "T=%d F=%d lags=%d B=%d stride=%d %s" % (t, f, n_lags, b, stride, tag)
    lookback = form == "f16_unit_lookback"
    assert tpad == -(-t // 128) * 128 and fs == -(-f // 32) * 32 and lp == -(-n_lags // 64) * 64
    assert r["form"] == form and r["band_on_f16"] == (form in F16_FORMS) and r["band_lookback"] == lookback, r["form"]
    assert r["kernel"] == ("gram_f16_kernel<true>" if form in F16_FORMS else "gram_kernel<GRAM_BAND>")
    band = r["band"]
    assert band.shape == (b, stride, lp)
    fill = fill_word(prefill)
    for clip in range(b):
        a = ref.pad_bins(rows[clip], fs)
        clean = a.copy()
        clean[list(special)] = 0                                    # (the bounds of the other entries do not see those rows)
        want = ref.band64(clean, n_lags, lookback)
        inside = ~np.isnan(want)                                    # t + l < T (look-back: j - l >= 0)
        got = band[clip, :t, :n_lags]
        # guards: the cells outside the matrix, the lags from n_lags on and the rows from T to the stride keep the prefill
        assert np.all(bits(got)[~inside] == fill), shape
        assert np.all(bits(band[clip, :t, n_lags:]) == fill) and np.all(bits(band[clip, t:]) == fill), shape
        bad = np.zeros_like(inside)
        for s in special:
            bad |= pairs_row(t, n_lags, s, lookback)
        assert not np.any(np.isfinite(got[inside & bad])), shape
        ok = inside & ~bad
        assert np.all(np.isfinite(got[ok])), shape
        got64 = got.astype(np.float64)
        if form in F16_FORMS:
            planes = r["planes"][clip]
            if form == "f16_rows":
                inv = r["inv"][clip]
                scale = np.array([ref.row_scale(float(m)) for m in np.fmax.reduce(rows[clip], axis=1)] + [1.0] * (tpad - t))   # (fmaxf drops a NaN)
                assert np.array_equal(bits(inv), bits((1.0 / scale).astype(np.float32))), shape
            else:
                inv, scale = np.float32(1.0 / ref.UNIT_SCALE), ref.UNIT_SCALE
            inv64 = np.asarray(inv, dtype=np.float64)
            keep = np.array([k for k in range(t) if k not in special], dtype=int)
            dec = ref.decode_planes(planes, inv64)
            sc_rows = np.broadcast_to(np.asarray(scale, dtype=np.float64), (tpad,))[:t]
            split_bar = 2.0 ** -21 * np.abs(a) + 2.0 ** -24 / sc_rows[:, None]
            assert np.all(np.abs(dec[:t] - a)[keep] <= split_bar[keep]), shape
            note("split", form, "decode", np.abs(dec[:t] - a)[keep], split_bar[keep], shape)
            assert np.all(planes[t:].view(np.uint16) == 0), shape          # pad rows decode to zero
            planes_clean = planes[:t].copy()
            planes_clean[list(special)] = 0
            own, mag = ref.three_product_band(planes_clean, inv64[:t] if inv64.ndim else inv64, n_lags, lookback)
            own_bar = 3 * fs * U * mag
            assert np.all(np.abs(got64 - own)[ok] <= own_bar[ok]), (shape, float(np.max((np.abs(got64 - own) / own_bar)[ok & (own_bar > 0)], initial=0)))
            note("band", form, "vs own arithmetic", np.abs(got64 - own)[ok], own_bar[ok], shape)
            bar = own_bar + ref.split_band_bound(clean, sc_rows, n_lags, lookback)
        else:
            bar = fs * U * ref.band_abs64(clean, n_lags, lookback)
        assert np.all(np.abs(got64 - want)[ok] <= bar[ok]), shape
        note("band", form, "vs float64", np.abs(got64 - want)[ok], bar[ok], shape)
    return r


# ---- the banded Gram -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("f32",) + F16_FORMS)
def test_band_entry_by_entry_at_the_seams(form):
    for k, (t, f, n_lags) in enumerate(SHAPES):
        check_band(form, rows_for(form, 1, t, f, 100 + k), n_lags, prefill=(0xFF, 0xA5)[k & 1])


def test_lookback_holds_the_forward_band_bit_for_bit():
    for k, (t, f, n_lags) in enumerate(SHAPES):
        rows = unit_rows(1, t, f, 200 + k)
        fwd = repet._gram_band_stage(rows, n_lags, form="f16_unit")["band"][0]
        back = repet._gram_band_stage(rows, n_lags, form="f16_unit_lookback")["band"][0]
        for l in range(min(n_lags, t)):
            assert np.array_equal(bits(back[l:t, l]), bits(fwd[:t - l, l])), (t, f, n_lags, l)


@pytest.mark.parametrize("form", ("f32",) + F16_FORMS)
def test_a_clip_of_a_batch_is_the_clip_alone(form):
    """B = 9: clip 8 takes the tile list rotated all the way round; (300, 130) is a list of six tiles and two fillers, (1030, 257)
    one of 24 in three groups. Strides: the padded clip, and more (the online handle's windows) where the form takes it."""
    for t, f, n_lags, batches in ((300, 33, 130, (2, 8, 9)), (1030, 17, 257, (9,))):
        rows = rows_for(form, 9, t, f, 7)
        tpad = -(-t // 128) * 128
        alone = [repet._gram_band_stage(rows[k], n_lags, form=form, prefill=0xFF)["band"][0, :t] for k in range(9)]
        for b in batches:
            for stride in (tpad, tpad + 3):
                if form == "f16_rows" and stride != tpad:
                    with pytest.raises(ValueError, match="packed clip by clip"):        # (REPET_ERR_BAD_ARG)
                        repet._gram_band_stage(rows[:b], n_lags, clip_stride=stride, form=form)
                    continue
                r = check_band(form, rows[:b], n_lags, stride=stride, tag="batch") if t == 300 else \
                    repet._gram_band_stage(rows[:b], n_lags, clip_stride=stride, form=form, prefill=0xFF)
                for k in range(b):
                    assert np.array_equal(bits(r["band"][k, :t]), bits(alone[k])), (form, t, b, stride, k)
                assert np.all(bits(r["band"][:, t:]) == fill_word(0xFF))


@pytest.mark.parametrize("form", ("f32",) + F16_FORMS)
def test_zero_nan_and_infinite_rows(form):
    t, f, n_lags = 300, 33, 130
    rows = rows_for(form, 1, t, f, 11)
    rows[0, 5] = 0
    rows[0, 150] = 0
    r = check_band(form, rows, n_lags, tag="zero rows")
    lookback = form == "f16_unit_lookback"
    inside = ~np.isnan(ref.band64(rows[0], n_lags, lookback))
    zero = (pairs_row(t, n_lags, 5, lookback) | pairs_row(t, n_lags, 150, lookback)) & inside
    assert np.all(bits(r["band"][0, :t, :n_lags])[zero] == 0)                 # exact zeros, +0
    rows = rows_for(form, 1, t, f, 12)
    rows[0, 40, 7] = np.nan
    rows[0, 131, 20] = np.inf
    check_band(form, rows, n_lags, special=(40, 131), tag="NaN, inf")


def f16_enabled():
    return not os.environ.get("REPET_GRAM", "").startswith("f3")


def tile_count(t, n_lags):
    nb = -(-t // 128)
    ndiag = min((n_lags + 126) // 128 + 1, nb)
    return -(-sum(nb - d for d in range(ndiag)) // 8) * 8


def test_form_zero_is_the_choice_of_run_gram_band():
    """band_rows_on_f16's stated rule: the f16-split kernel with row-scaled planes from 512 tiles (list length x clips) on, for
    one clip or clips packed at round_up(T, 128) rows; always with planes the STFT has written; unit rows on the f16-split kernel
    (REPET_GRAM=f32: nowhere). Asked of the choice itself, so the large shapes cost nothing."""
    unit_form = lambda lookback: ("f16_unit_lookback" if lookback else "f16_unit") if f16_enabled() else "f32"
    for t, f, n_lags in SHAPES:
        assert tile_count(t, n_lags) * 9 < 512
        r = repet._gram_band_stage(power_rows(1, t, f, 5), n_lags, form="auto")
        assert r["form"] == "f32" and r["kernel"] == "gram_kernel<GRAM_BAND>" and not r["band_on_f16"] and r["n_tiles"] == tile_count(t, n_lags)
    for lookback in (False, True):
        rows = unit_rows(2, 257, 33, 6)
        r = repet._gram_band_stage(rows, 130, form="auto", unit_rows=True, lookback=lookback)
        assert r["form"] == unit_form(lookback) and r["band_lookback"] == (lookback and f16_enabled())
        want = repet._gram_band_stage(rows, 130, form=unit_form(lookback))
        assert np.array_equal(bits(r["band"]), bits(want["band"]))
    # power rows at run time ignore the look-back request
    assert repet._gram_band_stage(power_rows(1, 129, 17, 1), 64, form="auto", lookback=True)["band_lookback"] is False
    for b, t, n_lags, extra in ((1, 7753, 431, 0), (1, 20000, 431, 0), (1, 13000, 431, 0), (1, 13200, 431, 0), (40, 1030, 431, 0),
                                (40, 1030, 431, 128), (7, 1030, 431, 0), (64, 900, 300, 0), (63, 900, 300, 0), (1, 60000, 1, 0)):
        tpad = -(-t // 128) * 128
        q = repet._gram_band_stage((b, t, 1025), n_lags, clip_stride=tpad + extra, form="auto", choice_only=True)
        assert q["n_tiles"] == tile_count(t, n_lags)
        on = f16_enabled() and q["n_tiles"] * b >= 512 and (b == 1 or extra == 0)
        assert q["form"] == ("f16_rows" if on else "f32"), (b, t, n_lags, extra, q)
        ready = repet._gram_band_stage((b, t, 1025), n_lags, clip_stride=tpad + extra, form="auto", planes_ready=True, choice_only=True)
        assert ready["form"] == "f16_rows"
        unit = repet._gram_band_stage((b, t, 1025), n_lags, clip_stride=tpad + extra, form="auto", unit_rows=True, lookback=True,
                                      planes_ready=True, choice_only=True)
        assert unit["form"] == unit_form(True)


# ---- windowed diagonal sums ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sum_band():
    return np.random.RandomState(21).standard_normal((3, 700, 448)).astype(np.float32)


@pytest.mark.parametrize("length", (1, 63, 64, 65, 255, 256, 257, 430, 600))
def test_window_sums(sum_band, length):
    """T = 700, 431 lags: windows that start before frame 0 (adaptive's -ceil((len - 1) / 2)) and run past T, lengths at the
    quarter-chunk (64), 16-row unroll and chunk (256) seams; lags from `len` on are zero. A window's beat row is the same bits
    alone, among seven windows and in a batch."""
    t, lp, n_lags, n_freq, step = 700, 448, 431, 1025, 109
    start0 = -(length // 2)
    args = dict(lo=1, hi=100, n_lags_for_clamp=300, n_lags=n_lags, prefill=0xFF)
    beat7, _, _ = repet._band_periods_stage(sum_band, n_freq, start0, step, length, 7, **args)
    assert start0 < 0 or length == 1
    assert start0 + 6 * step + length > t or length < 100
    for b in range(3):
        want, mag, count = ref.window_sums64(sum_band[b], n_lags, n_freq, start0, step, length, 7)
        got = beat7[b, :, :n_lags].astype(np.float64)
        bar = count * U * mag
        assert np.all(np.abs(got - want) <= bar), (length, b, float(np.max(np.abs(got - want)[bar > 0] / bar[bar > 0], initial=0)))
        note("window sum", "-", "vs float64", np.abs(got - want), bar, "T=%d len=%d start0=%d step=%d windows=7 B=3" % (t, length, start0, step))
        assert np.all(bits(beat7[b, :, min(length, n_lags):n_lags]) == 0)                # n_lags > len: zeros
        assert np.all(bits(beat7[b, :, n_lags:]) == fill_word(0xFF))
    beat_one, _, _ = repet._band_periods_stage(sum_band[0], n_freq, start0, step, length, 7, **args)
    assert np.array_equal(bits(beat_one[0]), bits(beat7[0]))
    for w in (0, 3, 6):
        for b in (0, 2):
            alone, _, _ = repet._band_periods_stage(sum_band[b], n_freq, start0 + w * step, step, length, 1, **args)
            assert np.array_equal(bits(alone[0, 0]), bits(beat7[b, w])), (length, w, b)


# ---- periods ---------------------------------------------------------------------------------------------------------------
def test_periods_exact_on_crafted_rows():
    rs = np.random.RandomState(31)
    n = 640
    cases = []                                                    # (row, lo, hi)
    for lo, hi in ((8, 200), (1, 213), (0, 64), (5, 69), (3, 40), (10, 11), (17, 500)):
        h = min(hi, n // 3)
        for at in {lo, h - 1, min(lo + 63, h - 1), min(lo + 64, h - 1), (lo + h) // 2}:
            row = rs.rand(n).astype(np.float32)
            row[at] = 2.0
            row[h:] = 3.0                                         # larger, but outside the range (hi clamped by n_lags / 3 too)
            row[:lo] = 3.0
            cases.append((row, lo, hi))
        for gap in (1, 31, 32, 63, 64, 65, 128):                  # exact ties: the first wins, in a lane (64, 128) and across lanes
            for first in (lo, lo + 1, lo + 37):
                if first + gap < h:
                    row = rs.rand(n).astype(np.float32)
                    row[[first, first + gap]] = 2.0
                    if first + 2 * gap < h:
                        row[first + 2 * gap] = 2.0
                    cases.append((row, lo, hi))
        flat = np.full(n, 0.25, dtype=np.float32)                 # a plateau: lag lo
        cases.append((flat, lo, hi))
        for value in (np.nan, np.inf, -np.inf):                   # not finite inside [lo, h): lo + 1, wherever the maximum is
            for at in {lo, h - 1, (lo + h) // 2}:
                row = rs.rand(n).astype(np.float32)
                row[min(lo + 2, h - 1)] = 2.0
                row[at] = value
                cases.append((row, lo, hi))
        row = rs.rand(n).astype(np.float32)                       # not finite outside the range: ignored
        row[:lo] = np.nan
        row[h:] = np.inf
        cases.append((row, lo, hi))
    for row, lo, hi in cases:
        want = ref.periods_rule(row[None], lo, hi, n)[0]
        assert repet._periods(row, [lo, hi]) == want, (lo, hi, np.flatnonzero(row[lo:min(hi, n // 3)] >= 2.0), want)
        if np.all(np.isfinite(row[lo:min(hi, n // 3)])):
            assert want == orc.periods(row.astype(np.float64), [lo, hi])
        else:
            assert want == orc.periods(np.full(n, np.nan), [lo, hi]) == lo + 1
    # many rows at once, each with its own answer
    rows = np.stack([c[0] for c in cases if (c[1], c[2]) == (8, 200)])
    assert np.array_equal(repet._periods(rows.T, [8, 200]), ref.periods_rule(rows, 8, 200, n))


def two_tempo_power(f, t, seed):
    """Period 5 in the first half, 9 in the second, far above the noise: one clear maximum among the lags 3 .. 9."""
    rs = np.random.RandomState(seed)
    a, b = rs.rand(f, 5) + 0.1, rs.rand(f, 9) + 0.1
    a[:, 0] += 4
    b[:, 0] += 4
    frames = np.arange(t)
    p = np.where(frames[None, :] < t // 2, a[:, frames % 5], b[:, frames % 9]) + 0.05 * rs.rand(f, t)
    return p.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("t,seg_len,step", [(100, 40, 7), (100, 40, 1), (61, 40, 150), (300, 270, 40), (130, 41, 10)])
def test_chain_to_frame_periods_is_the_oracle(t, seg_len, step):
    """fp32 band -> window sums -> periods -> expansion against orc.beatspectrogram / orc.periods, the hole column lo + 1
    included: T not a multiple of the step, step = 1, step > T, a window of two chunks (270 rows)."""
    f = 20
    p = two_tempo_power(f, t, t + step)
    lo, hi = 3, 10                                                         # lags 3 .. 9: 5 and 9, not 10 = 2 x 5
    n_win = -(-t // step)
    band = repet._gram_band_stage(p.T, seg_len, form="f32", prefill=0)["band"][0, :t]
    beat, win, frames = repet._band_periods_stage(band, f, -(seg_len // 2), step, seg_len, n_win, lo, hi, seg_len, n_lags=seg_len, t_expand=t,
                                                  prefill=0xFF)
    want = orc.beatspectrogram(p, seg_len, step)
    want_win, want_full = ref.beat_spectrogram(p.T, seg_len, step)
    assert np.max(np.abs(beat[0, :, :seg_len] - want_win)) <= 2e-5 * np.max(np.abs(want_win))
    top = np.sort(want_win[:, lo:min(hi, seg_len // 3)], axis=1)
    assert np.all(top[:, -1] - top[:, -2] > 1e-3 * top[:, -1])            # (the arg-max of this input is no near-tie)
    assert np.array_equal(win[0], ref.periods_rule(want_win, lo, hi, seg_len))
    assert np.array_equal(frames, orc.periods(want, [lo, hi]))
    assert np.array_equal(frames, ref.expand_periods(win[0], step, t, lo))
    if 1 < step <= t:
        assert frames[step - 1] == lo + 1
    assert len(set(frames.tolist())) >= (2 if step <= t else 1)


def test_zz_report_the_largest_errors():
    """Last in the module: the table of (stage, form, check, max error, bar, shape), as profiles/stft_stage_parity.txt has it."""
    lines = ["%-10s %-17s %-18s err %.3e  bar %.3e  (%.2f of the bar)  %s" % (stage, form, check, err, bar, ratio, shape)
             for (stage, form, check), (ratio, err, bar, shape) in sorted(PARITY.items())]
    print("\n".join(lines))
    path = os.environ.get("REPET_GRAM_STAGE_PARITY_OUT")
    if path and lines:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
