"""The full similarity matrix of `sim`, entry by entry, records included: the production code (exec_gram_full, the second half of
run_gram_full, through repet._gram_full_stage) against the float64 references of tests/gram_reference.py, in the three forms the
pipeline can run it in -- exact fp32 (gram_kernel<GRAM_FULL>), f16-split with 128 x 128 tiles (gram_f16_kernel<false>), f16-split
with 256 x 256 tiles (gram_f16_big_pipe_kernel) -- at the shapes where the kernels change path: T around the 64-column patch, the
128- and the 256-row tile, T mod 4 = 1, 2, 3 (the float4 stores of the 256 kernel split per element), T mod 32 = 1 (a segment with
one live column), nine tile rows (the tile list's super-block wraps: T = 1030 for 128, 2049 for 256), FS / 32 = 1, 2, 3 (each its
own way through the K pipeline's prologue), and the production K (F = 1025).

Bounds (all derived, none fitted to the kernels; u = 2^-24, `terms` are the summed products):
  split                    |decoded planes - v| <= 2^-21 |v| + 2^-24 / 128: hi = f16(128 v) leaves a remainder of at most 2^-11
                           |128 v| that lo = f16(.) holds to 2^-11 of itself or, where lo is subnormal, to 2^-25 absolute; pad
                           rows [T, round_up(T, 128)) decode to zero. (tests/test_gpu_gram_band_stages.py states the same.)
  kernel vs its own        the exact sum (hi hi' + hi lo' + lo hi') / 2^14 of the planes the kernel read, in float64: the f16
  arithmetic (f16 forms)   MFMA multiplies exactly and adds in fp32, so an entry is a sum of n = 3 FS terms with one rounding per
                           addition: |error| <= 3 FS u sum |terms|. The 2^-14 unscale is exact.
  kernel vs float64        f16 forms: the accumulation above + the split of both operands, sum (|a| db + |b| da + da db) with da,
                           db the split bound + the dropped lo lo' <= 2^-22 of each |product| (|lo| <= 2^-11 |hi|).
                           fp32 form: a dot product of FS terms in fp32: FS u sum |terms|.
  unit rows (normalise)    unit_rows_kernel adds the F squares in fp32 -- a thread its ceil(F / 256) squares in turn (the first
                           to 0, exactly), six shuffle steps, three additions of the four waves' sums -- so a square goes
                           through at most n = ceil(F / 256) + 9 roundings, its own product's included (none if the compiler
                           fuses it). All terms are positive: the sum is the exact one times (1 + t), |t| <= g = n u / (1 - n u).
                           sqrtf and the division are correctly rounded (no fast-math in the build): one factor (1 +- u) each. So
                           out / (v / ||v||) lies within (1 - g)^-1/2 (1 + u) / (1 - u) of 1 on either side; 2^-149 absolute for a
                           quotient that is subnormal (the test's squares are far above the underflow threshold). A zero row
                           gives 0 / 0 = NaN in its F bins and 0 in the pad bins.
  layout, guard columns, symmetry, records, the pick, bit-identity between the forms: exact.
The only cells excused from the numeric bounds pair a row that deliberately holds a NaN or an inf: they must be non-finite.
The largest error met per check is collected in PARITY and printed (and written to $REPET_GRAM_FULL_PARITY_OUT) by the last test
of the module: profiles/gram_full_stage_parity.txt is that output from an MI355X (documentation; the asserts use the bounds)."""
import ctypes
import os

import numpy as np
import pytest

import repet
from repet import _native
import gram_reference as ref

pytestmark = pytest.mark.gpu

U = ref.U
KERNELS = {"f32": "gram_kernel<GRAM_FULL>", "f16_128": "gram_f16_kernel<false>", "f16_256": "gram_f16_big_pipe_kernel"}
TILE = {"f32": 128, "f16_128": 128, "f16_256": 256}
PARITY = {}          # (stage, form, check) -> (error / bar, error, bar, shape)
# every T of {1, 63, 64, 65, 127, 128, 129, 255, 257, 1030} and every F of {17, 33, 65, 129} (FS / 32 = 1, 2, 3, 5) at least once
SEAMS_128 = [(1, 17), (63, 33), (64, 65), (65, 129), (127, 17), (128, 33), (129, 65), (255, 129), (257, 17), (257, 65), (1030, 33),
             (1030, 129)]
# every T of {1, 63, 64, 65, 191, 193, 255, 256, 257, 300, 513, 514, 515} and every F of {17, 33, 65} at least once
SEAMS_256 = [(1, 33), (63, 17), (64, 33), (65, 65), (191, 17), (193, 33), (255, 65), (256, 17), (257, 33), (300, 65), (513, 17),
             (514, 33), (515, 65), (65, 17), (257, 65), (513, 33)]


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


def unit_rows(t, f, seed):
    rs = np.random.RandomState(seed)
    v = rs.rand(t, f) ** 2
    return (v / np.sqrt(np.sum(v * v, axis=1, keepdims=True))).astype(np.float32)


def raw_rows(t, f, seed):
    """Magnitudes for `normalise`: rows of rand^2 at levels 1 .. 100."""
    rs = np.random.RandomState(seed)
    return (rs.rand(t, f) ** 2 * rs.uniform(1, 100, size=(t, 1))).astype(np.float32)


def stress(rows):
    """Rows that stress the split: a one-hot row (hi = 128, lo = 0 and zeros) and a row whose components span 2^-40 .. 1 (hi or lo
    f16-subnormal or zero)."""
    t, f = rows.shape
    rows = rows.copy()
    rows[t // 2] = 0
    rows[t // 2, f // 2] = 1.0
    if t > 1:
        rows[t - 1] = np.exp2(-40.0 * np.arange(f)[::-1] / (f - 1))
    return rows


def fill_word(prefill):
    return np.frombuffer(bytes([prefill]) * 4, dtype=np.uint32)[0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def f16_enabled():
    return not os.environ.get("REPET_GRAM", "").startswith("f3")


def picked(t):
    """run_gram_full's rule for unit rows: fp32 under REPET_GRAM=f32, else the 256 x 256 kernel from 2 048 frames on (unless
    REPET_GRAM_TILE=128), else the 128 x 128 one."""
    if not f16_enabled():
        return "f32"
    return "f16_256" if t >= 2048 and not os.environ.get("REPET_GRAM_TILE", "").startswith("1") else "f16_128"


def source(form, records):
    """Where the records come from: the epilogue of the 256 x 256 kernel for records = 1 (unless REPET_GRAM_SEGMENTS=0), the pass."""
    if not records:
        return None
    return "epilogue" if records == 1 and form == "f16_256" and not os.environ.get("REPET_GRAM_SEGMENTS", "").startswith("0") else "pass"


def tile_count(t, edge):
    nb = -(-t // edge)
    return -(-(nb * (nb + 1) // 2) // 8) * 8


def check_unit_rows(raw, vn, fs, zero_rows, shape):
    """launch_unit_rows against float64, by the bound the module's docstring derives."""
    t, f = raw.shape
    want = ref.unit_rows64(raw)
    n = -(-f // 256) + 9
    g = n * U / (1 - n * U)
    rel = (1 - g) ** -0.5 * (1 + U) / (1 - U) - 1
    live = np.array([k for k in range(t) if k not in zero_rows], dtype=int)
    err, bar = np.abs(vn[:t, :f].astype(np.float64) - want)[live], (rel * np.abs(want) + 2.0 ** -149)[live]
    assert np.all(err <= bar), (shape, float(np.max(err / bar)))
    note("unit rows", "-", "vs float64", err, bar, shape)
    assert np.all(bits(vn[:t, f:]) == 0) and np.all(bits(vn[t:]) == 0), shape           # pad bins and pad rows: +0
    for z in zero_rows:
        assert np.all(np.isnan(vn[z, :f])), shape


@np.errstate(all="ignore")
def check_full(form, rows, records=1, prefill=0xFF, special=(), normalise=False, tag=""):
    """Run one form on rows (T, F) and hold every cell of what comes back to the module's docstring. special: rows whose entries
    are expected not to be finite (given with a NaN or an inf; under normalise: zero rows). Returns the stage's result."""
    rows = np.asarray(rows, dtype=np.float32)
    t, f = rows.shape
    r = repet._gram_full_stage(rows, form=form, records=records, normalise=normalise, prefill=prefill)
    ran = picked(t) if form == "auto" else form
    edge = TILE[ran]
    tpad, fs, ts = -(-t // 128) * 128, -(-f // 32) * 32, -(-t // 64) * 64
    shape = "T=%d F=%d %s" % (t, f, tag)
    assert (r["Tpad"], r["FS"], r["TS"], r["seg_pitch"]) == (tpad, fs, ts, -(-(ts // 32) // 4) * 4), shape
    assert (r["form"], r["kernel"], r["tile"], r["n_tiles"], r["records"]) == (ran, KERNELS[ran], edge, tile_count(t, edge), source(ran, records)), (shape, r["form"])
    would = repet._gram_full_stage((t, f), form=form, records=records, choice_only=True)        # nothing runs: the same report
    assert all(would[k] == r[k] for k in would), shape
    s = r["S"]
    assert s.shape == (t, ts)
    fill = fill_word(prefill)
    assert np.all(bits(s[:, t:]) == fill), shape                      # the guard columns [T, TS) of every row keep the prefill
    got = s[:, :t]
    if normalise:
        check_unit_rows(rows, r["Vn"], fs, special, shape)
        a = r["Vn"][:t].astype(np.float64)                            # the rows the Gram kernel read
    else:
        a = ref.pad_bins(rows, fs)
    special = sorted(special)
    keep = np.array([k for k in range(t) if k not in special], dtype=int)
    bad = np.zeros((t, t), dtype=bool)
    bad[special, :] = True
    bad[:, special] = True
    ok = ~bad
    assert not np.any(np.isfinite(got[bad])), shape
    assert np.all(np.isfinite(got[ok])), shape
    if ran == "f32":        # (every cell is computed where it lies: a NaN's payload is not part of the claim)
        assert np.array_equal(bits(got)[ok], bits(got.T)[ok]) and np.array_equal(got, got.T, equal_nan=True), shape
    else:                   # both sides of the diagonal are copies of ONE computed value
        assert np.array_equal(bits(got), bits(got.T)), shape
    clean = a.copy()
    clean[special] = 0                                                 # (the bounds of the other entries do not see those rows)
    want = ref.full64(clean)
    got64 = got.astype(np.float64)
    if ran != "f32":
        planes = r["planes"]
        assert planes.shape == (-(-t // edge) * edge, 2 * fs), shape
        inv = 1.0 / ref.UNIT_SCALE
        dec = ref.decode_planes(planes[:t], inv)
        split_bar = 2.0 ** -21 * np.abs(a) + 2.0 ** -24 / ref.UNIT_SCALE
        assert np.all(np.abs(dec - a)[keep] <= split_bar[keep]), shape
        note("split", ran, "decode", np.abs(dec - a)[keep], split_bar[keep], shape)
        assert np.all(planes[t:tpad].view(np.uint16) == 0), shape     # pad rows decode to zero
        stale = planes[tpad:]                                          # 256 x 256 tiles: read by the last tile row, never written
        assert np.all(stale.view(np.uint8) == prefill), shape
        if stale.size:
            assert prefill == 0xFF and np.all(np.isnan(stale)), shape  # the kernel's operands there really were NaN
        planes_clean = planes[:t].copy()
        planes_clean[special] = 0
        own, mag = ref.three_product_full(planes_clean, inv)
        own_bar = 3 * fs * U * mag
        assert np.all(np.abs(got64 - own)[ok] <= own_bar[ok]), (shape, float(np.max((np.abs(got64 - own) / own_bar)[ok & (own_bar > 0)], initial=0)))
        note("full", ran, "vs own arithmetic", np.abs(got64 - own)[ok], own_bar[ok], shape)
        bar = own_bar + ref.split_full_bound(clean, ref.UNIT_SCALE)
    else:
        bar = fs * U * ref.full_abs64(clean)
    assert np.all(np.abs(got64 - want)[ok] <= bar[ok]), (shape, float(np.max((np.abs(got64 - want) / bar)[ok & (bar > 0)], initial=0)))
    note("full", ran, "vs float64", np.abs(got64 - want)[ok], bar[ok], shape)
    if records:
        check_records(r, t, fill, not special, shape)
    return r


def check_records(r, t, fill, all_finite, shape):
    """top, second and at are exactly segment_records of the S the same call returned, over ceil(T / 32) runs."""
    n_seg = -(-t // 32)
    top, second, at = ref.segment_records(r["S"], t)
    assert np.array_equal(bits(r["top"][:, :n_seg]), bits(top)), (shape, r["records"])
    assert np.array_equal(bits(r["second"][:, :n_seg]), bits(second)), (shape, r["records"])
    assert np.array_equal(r["at"][:, :n_seg], at), (shape, r["records"])
    if t % 32 == 1:
        assert np.all(r["second"][:, n_seg - 1] == -np.inf), shape    # a run with one live column
    if all_finite:                                                     # every record is finite or -inf
        assert np.all(np.isfinite(r["top"][:, :n_seg])), shape
        assert np.all(np.isfinite(r["second"][:, :n_seg]) | (r["second"][:, :n_seg] == -np.inf)), shape
    # the rest of the pitch: untouched by the pass; the epilogue writes both runs of a 64-column patch: an empty run's record there
    for key, empty in (("top", -np.inf), ("second", -np.inf), ("at", 0)):
        tail = r[key][:, n_seg:]
        untouched = bits(tail) == fill
        assert np.all(untouched | (tail == empty) if r["records"] == "epilogue" else untouched), (shape, key)


def prefill_for(k, form, t):
    """0xFF and 0xA5 in turn; 0xFF (f16 NaNs) wherever the 256 x 256 kernel reads plane rows nobody wrote."""
    return 0xFF if form == "f16_256" and -(-t // 256) * 256 != -(-t // 128) * 128 else (0xFF, 0xA5)[k & 1]


# ---- entry by entry at the seams -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("f32", "f16_128"))
@pytest.mark.parametrize("k", range(len(SEAMS_128)))
def test_entry_by_entry_at_the_tile_seams(form, k):
    """The 128 x 128 kernels: T at 64 (a wave's block), 128 (the tile), nine tile rows; FS / 32 = 1, 2, 3, 5."""
    t, f = SEAMS_128[k]
    if k % 3 == 2:
        check_full(form, raw_rows(t, f, 300 + k), records=1 + (k & 1), prefill=prefill_for(k, form, t), normalise=True, tag="normalise")
    else:
        rows = unit_rows(t, f, 300 + k)
        check_full(form, stress(rows) if k & 1 else rows, records=1 + (k & 1), prefill=prefill_for(k, form, t), tag="stress" if k & 1 else "")


@pytest.mark.parametrize("k", range(len(SEAMS_256)))
def test_entry_by_entry_at_the_patch_seams_of_the_256_kernel(k):
    """gram_f16_big_pipe_kernel below its production sizes: T mod 4 = 1, 2, 3 (513, 514, 515), T mod 32 = 1 (65, 193, 257, 513), T
    mod 64 = 63, 0, 1, one row into a new 256 tile (257, 513); FS / 32 = 1, 2, 3. The records from the epilogue and from the pass
    over S, on the same S."""
    t, f = SEAMS_256[k]
    prefill = prefill_for(k, "f16_256", t)
    if k % 3 == 2:
        rows, kw = raw_rows(t, f, 400 + k), dict(normalise=True, tag="normalise")
    else:
        rows = unit_rows(t, f, 400 + k)
        rows, kw = (stress(rows), dict(tag="stress")) if k & 1 else (rows, {})
    a = check_full("f16_256", rows, records=1, prefill=prefill, **kw)
    b = check_full("f16_256", rows, records=2, prefill=prefill, **kw)
    assert (a["records"], b["records"]) == (source("f16_256", 1), "pass")
    n_seg = -(-t // 32)
    assert np.array_equal(bits(a["S"]), bits(b["S"]))
    for key in ("top", "second", "at"):
        assert np.array_equal(bits(a[key][:, :n_seg]), bits(b[key][:, :n_seg])), (t, f, key)


@pytest.mark.parametrize("t,f", [(2047, 33), (2048, 33), (2049, 33), (2305, 33), (2048, 1025)])
def test_production_sizes_as_run_gram_full_picks(t, f):
    """Form 0 around the 2 048-frame threshold: 2047 on the 128 x 128 kernel with the pass over S, 2048 on the 256 x 256 kernel with
    the epilogue's records, 2049 = nine tile rows (the big list wraps; the last tile row holds one real row), 2305 = ten with a
    ragged edge; F = 1025 is the production K (FS / 32 = 33). The two sources of the records agree bit for bit."""
    rows = unit_rows(t, f, t + f)
    a = check_full("auto", rows, records=1, prefill=0xFF)
    if f16_enabled() and not os.environ.get("REPET_GRAM_TILE") and not os.environ.get("REPET_GRAM_SEGMENTS"):
        assert (a["form"], a["records"]) == (("f16_128", "pass") if t == 2047 else ("f16_256", "epilogue"))
    if f > 64:
        return                                                         # (one pass of the float64 references at the production K)
    b = check_full("auto", rows, records=2, prefill=0xFF)
    assert b["records"] == "pass"
    n_seg = -(-t // 32)
    assert np.array_equal(bits(a["S"]), bits(b["S"]))
    for key in ("top", "second", "at"):
        assert np.array_equal(bits(a[key][:, :n_seg]), bits(b[key][:, :n_seg])), (t, key)


# ---- the claims of the file headers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", (300, 513, 2049))
def test_the_256_kernel_is_bit_identical_to_the_128_kernel(t):
    """gram_f16_big.hip: "the matrix is bit-identical to that kernel's"."""
    rows = stress(unit_rows(t, 33, 500 + t))
    small = repet._gram_full_stage(rows, form="f16_128", prefill=0xA5)
    big = repet._gram_full_stage(rows, form="f16_256", prefill=0xFF)
    assert (small["kernel"], big["kernel"]) == (KERNELS["f16_128"], KERNELS["f16_256"])
    assert np.array_equal(bits(small["S"][:, :t]), bits(big["S"][:, :t]))
    assert np.array_equal(small["planes"][:small["Tpad"]].view(np.uint16), big["planes"][:big["Tpad"]].view(np.uint16))


def test_the_band_kernel_holds_the_full_matrix_bit_for_bit():
    """gram_f16.hip: "same products in the same order as every other f16-split kernel": band[t][l] of the banded form is S[t][t + l]."""
    t, n_lags = 300, 130
    rows = stress(unit_rows(t, 33, 77))
    band = repet._gram_band_stage(rows, n_lags, form="f16_unit")["band"][0]
    for form in ("f16_128", "f16_256"):
        s = repet._gram_full_stage(rows, form=form, prefill=0xFF)["S"]
        for l in range(n_lags):
            assert np.array_equal(bits(np.diagonal(s[:, :t], l)), bits(band[:t - l, l])), (form, l)


# ---- records ---------------------------------------------------------------------------------------------------------------
def tied_rows(t, f, seed):
    """Identical frames placed so that exact ties fall inside a run (40 .. 43), across a run border (31 | 32) and across a patch
    and a tile border (63 | 64, 255 | 256); the last frame is one of them too. A row of the group is as similar to every other as
    to itself, so the ties are the maxima of their runs."""
    rows = unit_rows(t, f, seed)
    group = [31, 32, 40, 41, 42, 43, 63, 64, 255, 256, t - 1]
    rows[group] = rows[40]
    return rows, group


@pytest.mark.parametrize("t,form", [(300, "f32"), (300, "f16_128"), (300, "f16_256"), (2049, "auto")])
def test_records_with_exact_ties(t, form):
    rows, group = tied_rows(t, 33, 600 + t)
    last = ((t - 1) // 32, (t - 1) % 32)
    for records in (1, 2):
        r = check_full(form, rows, records=records, prefill=0xFF, tag="ties")
        top, second, at = r["top"], r["second"], r["at"]
        for g in group:                                                # the ties really occurred, and the lowest index won
            v = r["S"][g, g]
            assert np.all(r["S"][g, group] == v)
            assert (top[g, 1], second[g, 1], at[g, 1]) == (v, v, 0)                                  # 32, 40 .. 43, 63: inside a run
            assert (top[g, 0], at[g, 0]) == (v, 31) and second[g, 0] < v                             # 31 | 32: across a run border
            assert (top[g, 2], at[g, 2]) == (v, 0) and (top[g, 7], at[g, 7]) == (v, 31) and (top[g, 8], at[g, 8]) == (v, 0)   # 63 | 64, 255 | 256
            assert (top[g, last[0]], at[g, last[0]]) == (v, last[1])
        if t % 32 == 1:
            assert np.all(second[:, last[0]] == -np.inf)


@pytest.mark.parametrize("t,form", [(300, "f32"), (300, "f16_128"), (2049, "auto")])
def test_zero_nan_and_infinite_rows(t, form):
    """Rows that are not finite at row 0, at T - 1 and on each side of a 64 and a 256 border: a zero row under `normalise` (0 / 0),
    rows holding a NaN or +inf given directly. Their rows and columns of S are not finite, every other entry keeps its bound, and
    the records take them as +inf with `at` the first such column of the run."""
    f = 33
    special = (0, 63, 64, 255, 256, t - 1)
    raw = raw_rows(t, f, 700 + t)
    raw[list(special)] = 0
    direct = unit_rows(t, f, 701 + t)
    direct[[0, 64, 255], 7] = np.nan
    direct[[63, 256, t - 1], 20] = np.inf
    for rows, normalise in ((raw, True), (direct, False)):
        r = check_full(form, rows, records=1, prefill=0xFF, special=special, normalise=normalise, tag="special rows")
        top, at = r["top"], r["at"]
        others = np.array([k for k in range(t) if k not in special], dtype=int)
        for col in special:
            run, first = col // 32, min(c for c in special if c // 32 == col // 32) % 32
            assert np.all(top[:, run] == np.inf) and np.all(at[others, run] == first), (t, form, col)
        for row in special:                                            # its own row: every run's first column
            n_seg = -(-t // 32)
            assert np.all(top[row, :n_seg] == np.inf) and np.all(at[row, :n_seg] == 0), (t, form, row)


# ---- the pick and the refusals ---------------------------------------------------------------------------------------------
def test_form_zero_is_the_choice_of_run_gram_full():
    """gram_full_form's rule, asked of the choice itself (nothing runs): unit rows go to the 256 x 256 kernel from 2 048 frames on
    and take their records from its epilogue; below, the 128 x 128 kernel and the pass over S."""
    for t in (1, 300, 2047, 2048, 2049, 4096):
        for records in (0, 1, 2):
            q = repet._gram_full_stage((t, 1025), form="auto", records=records, choice_only=True)
            form = picked(t)
            assert (q["form"], q["records"], q["tile"], q["n_tiles"]) == (form, source(form, records), TILE[form], tile_count(t, TILE[form])), (t, records, q)
            assert (q["Tpad"], q["FS"], q["TS"]) == (-(-t // 128) * 128, 1056, -(-t // 64) * 64)
    if f16_enabled() and not os.environ.get("REPET_GRAM_TILE") and not os.environ.get("REPET_GRAM_SEGMENTS"):
        q = repet._gram_full_stage((2047, 33), form="auto", records=1, choice_only=True)
        assert (q["form"], q["records"], q["n_tiles"]) == ("f16_128", "pass", 136)
        q = repet._gram_full_stage((2048, 33), form="auto", records=1, choice_only=True)
        assert (q["form"], q["records"], q["n_tiles"]) == ("f16_256", "epilogue", 40)
    for form in KERNELS:                                               # a form asked for is the form that runs, at any T
        for t in (1, 4096):
            assert repet._gram_full_stage((t, 17), form=form, choice_only=True)["form"] == form


def test_refusals_and_a_valid_call_afterwards():
    with pytest.raises(ValueError, match="bad size"):                  # REPET_ERR_BAD_ARG
        repet._gram_full_stage((0, 17), choice_only=True)
    with pytest.raises(ValueError, match="bad size"):
        repet._gram_full_stage((5, 0), choice_only=True)
    with pytest.raises(ValueError, match="bad size"):
        repet._gram_full_stage(np.zeros((0, 17), dtype=np.float32))
    with pytest.raises(RuntimeError, match="at most 4096 rows"):       # REPET_ERR_LIMIT: S is T x TS floats
        repet._gram_full_stage((4097, 17), choice_only=True)
    with pytest.raises(RuntimeError, match="at most 8192 bins"):
        repet._gram_full_stage((5, 8193), choice_only=True)
    for form in (-1, 4):
        with pytest.raises(ValueError, match="form: 0 as production picks"):
            repet._gram_full_stage((5, 17), form=form, choice_only=True)
    for records in (-1, 3):
        with pytest.raises(ValueError, match="records: 0 none"):
            repet._gram_full_stage((5, 17), records=records, choice_only=True)
    # null arguments, asked of the entry itself: no geometry; rows, records or planes missing where the call would write them
    fn, ctx = _native.lib().repet_debug_gram_full_stage, _native.default_context(repet._device).handle
    geo, s = (ctypes.c_int64 * 8)(), np.zeros((5, 64), dtype=np.float32)
    rows = unit_rows(5, 17, 1)
    assert fn(ctx, _native.ptr(rows), 5, 17, 1, 0, 0, 0, None, _native.ptr(s), None, None, None, None, None, None, 0) == _native.ERR_BAD_ARG
    assert fn(ctx, None, 5, 17, 1, 0, 0, 0, geo, _native.ptr(s), None, None, None, None, None, None, 0) == _native.ERR_BAD_ARG
    assert fn(ctx, _native.ptr(rows), 5, 17, 1, 1, 0, 0, geo, _native.ptr(s), None, None, None, None, None, None, 0) == _native.ERR_BAD_ARG
    assert fn(ctx, _native.ptr(rows), 5, 17, 2, 0, 0, 0, geo, _native.ptr(s), None, None, None, None, None, None, 0) == _native.ERR_BAD_ARG
    assert fn(ctx, _native.ptr(rows), 5, 17, 1, 0, 1, 0, geo, _native.ptr(s), None, None, None, None, None, None, 0) == _native.ERR_BAD_ARG
    assert fn(ctx, _native.ptr(rows), 5, 17, 1, 0, 0, 0, geo, _native.ptr(s), None, None, None, None, None, None, 0) == 0
    for form in KERNELS:
        check_full(form, unit_rows(65, 17, 2), records=1, prefill=0xFF, tag="after the refusals")


def test_zz_parity_record():
    """Last in the module: the table of (stage, form, check, max error, bar, shape), as profiles/gram_band_stage_parity.txt has it."""
    lines = ["%-10s %-8s %-18s err %.3e  bar %.3e  (%.2f of the bar)  %s" % (stage, form, check, err, bar, ratio, shape)
             for (stage, form, check), (ratio, err, bar, shape) in sorted(PARITY.items())]
    print("\n".join(lines))
    path = os.environ.get("REPET_GRAM_FULL_PARITY_OUT")
    if path and lines:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
