"""The median-mask kernels (csrc/mask.hip, mask_bits.hip, with rank.hip in front of the rank paths) stage by stage, as the
pipelines launch them: the three production launchers through repet._mask_stage (repet_debug_mask_stage: buffers laid out as
make_geo lays them out, a MaskArgs the caller controls, a report of the kernel that ran) against tests/mask_reference.py -- the
kernels' own arithmetic in NumPy, checked against the float64 oracle on the CPU by tests/test_mask_reference.py.

Bars (derived, none fitted; the issue of this module sets them):
  model      (period family, model output) equal bit for bit, NaN positions included.
  mask       exactly 1.0 where the reference says exactly 1 (model >= magnitude, bins 1 .. cutoff; bin 0 is not overridden);
             NaN exactly where the reference is NaN; exactly 0 in warm-up rows; never above 1; elsewhere |got - want| <=
             3 * 2^-23 * want: soft_mask is two fp32 additions and one product at 2^-24 each plus the hardware reciprocal that
             common.h states as 1 ulp = 2^-23 -- 2.5 * 2^-23 to first order, rounded up for the second-order terms.
  X          where mask and X are both asked for, X_out == X_in * mask_out in fp32, bit for bit, both components; X alone: the
             same with the mask plane of a mask-only run on the same input.
  untouched  cells nobody should write hold the prefill byte (X: the caller's value) bit for bit: bins F .. FS - 1, rows outside
             [frame0, frame_end), rows past T, model rows q >= period, with parts = 1 the Nyquist bin (but for warm-up rows, which
             the main kernel zeroes whole) and with parts = 2 everything but it.
  rank paths the bit-sliced and packed-rank masks equal the float kernel's mask on the same input bit for bit; the code words are
             the integers NumPy's sort gives.
Inputs: mask_reference.magnitudes / build_sim (levels 2^-40 .. 2^40 across bins, exact zeros, a constant bin, ties, otherwise at
least 2^-13 apart in a bin: a wrong order statistic is 2^7 bars away). In every case at least a quarter of the compared cells
have a reference mask below 1 and every list length from 0 to the longest occurs (asserted here again).
The largest error / bar per (kernel, check) is collected in PARITY; the last test prints it and writes it to
$REPET_MASK_STAGE_PARITY_OUT: profiles/mask_stage_parity.txt is that output from an MI355X (documentation; the asserts use the bars)."""
import os

import numpy as np
import pytest

import repet
import mask_reference as ref

pytestmark = pytest.mark.gpu

PREFILL = 0xA5
FILL = np.frombuffer(bytes([PREFILL]) * 4, dtype=np.uint32)[0]
PARITY = {}          # (kernel, check) -> (error / bar, error, bar, shape)
KERNELS_SEEN = set()
IDLE = 1 << 60       # kSlotIdle: a slot without a stream


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def note(kernel, check, err, bar, shape):
    err, bar = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64))
    if err.size == 0:
        return
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    k = int(np.argmax(ratio))
    key = (kernel, check)
    if key not in PARITY or ratio.flat[k] > PARITY[key][0]:
        PARITY[key] = (float(ratio.flat[k]), float(err.flat[k]), float(bar.flat[k]), shape)


def same_bits_or_both_nan(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


UNTOUCHED, ZERO, REF = 0, 1, 2


@np.errstate(all="ignore")
def check_mask_plane(got, t, f, want, one, state, kernel, shape):
    """One channel's mask plane (rows, FS) as the kernel left it, against the reference (T, F) where state says REF."""
    assert np.all(bits(got[t:]) == FILL), "a row past T was written: " + shape
    assert np.all(bits(got[:t, f:]) == FILL), "a pad bin was written: " + shape
    g = got[:t, :f]
    assert np.all(bits(g)[state == UNTOUCHED] == FILL), "a cell outside the launch was written: " + shape
    assert np.all(bits(g)[state == ZERO] == 0), "a warm-up cell is not +0: " + shape
    live = state == REF
    nan = np.isnan(want) & live
    assert np.array_equal(np.isnan(g) & live, nan), "NaN positions: " + shape
    exact = one & live & ~nan
    assert np.all(g[exact] == 1.0), "not exactly 1 where the model is not below the magnitude (or in a cutoff bin): " + shape
    rest = live & ~nan & ~one
    assert np.all(g[rest] <= 1.0), "above 1: " + shape
    err, bar = np.abs(g[rest].astype(np.float64) - want[rest]), ref.MASK_BAR * want[rest]
    note(kernel, "mask", err, bar, shape)
    bad = np.argwhere(rest)[err > bar]
    assert len(bad) == 0, "%s: %d cells past the bar, the first at (t, f) = %s: got %r want %r" % (
        shape, len(bad), tuple(bad[0]), g[tuple(bad[0])], want[tuple(bad[0])])
    return rest


def check_x_plane(got, x_in, t, f, mask_plane, state, shape):
    """One channel's X plane (rows, FS) complex64: untouched cells keep the caller's value (the prefill outside the data), every
    other cell is x_in * mask in fp32, component by component."""
    g2 = np.ascontiguousarray(got).view(np.float32).reshape(got.shape + (2,))
    assert np.all(bits(g2[t:]) == FILL) and np.all(bits(g2[:t, f:]) == FILL), "X outside the data was written: " + shape
    x2 = np.ascontiguousarray(x_in).view(np.float32).reshape(x_in.shape + (2,))
    g = g2[:t, :f]
    untouched = state == UNTOUCHED
    assert np.array_equal(bits(g)[untouched], bits(x2)[untouched]), "X outside the launch was changed: " + shape
    m = np.where(state == ZERO, np.float32(0), mask_plane[:t, :f]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        want = x2 * m[..., None]
    touched = ~untouched
    assert same_bits_or_both_nan(g[touched], want[touched]), "X is not X_in * mask bit for bit: " + shape
    note("all", "X = X_in * mask (bits)", 0.0, 0.0, shape)


def seen(report):
    if report["kernel"]:
        KERNELS_SEEN.add(report["kernel"])
    if report["nyquist"]:
        KERNELS_SEEN.add(report["nyquist"])


# ---- the period family -------------------------------------------------------------------------------------------------
def period_report(t, f, c, b, periods, device, min_period):
    pmin = min_period if device else periods[0]
    max_segments = -(-t // pmin)
    nfb, useful, parts = -(-f // 64), pmin * c * b, 1
    while parts < 4 and useful * parts < 2048 and 4 * parts < nfb:
        parts *= 2
    net = ref.net_for(max_segments) if max_segments <= 32 else -1
    return "mask_period_kernel<%d>" % net, parts, ((t // 3 + 2) if device else periods[0], c * parts, b)


def run_period(V, periods, device, want=("mask",), X=None, cutoff=0, min_period=1, tag=""):
    b, c, t, f = V.shape
    shape = "period T=%d F=%d C=%d B=%d p=%s %s cutoff=%d %s %s" % (t, f, c, b, periods, "device" if device else "host", cutoff, "+".join(want), tag)
    kw = dict(periods=periods, min_period=min_period) if device else dict(period=periods[0])
    r = repet._mask_stage("period", V, X, want=want, cutoff=cutoff, prefill=PREFILL, **kw)
    kernel, parts, grid = period_report(t, f, c, b, periods, device, min_period)
    rep = r["launch"]
    assert (rep["kernel"], rep["parts"], rep["grid"], rep["nyquist"]) == (kernel, parts, grid, ""), (rep, shape)
    seen(rep)
    KERNELS_SEEN.add("parts=%d" % parts)
    below = total = 0
    for clip in range(b):
        for ch in range(c):
            v, p = V[clip, ch], periods[clip] if device else periods[0]
            model, (m, one) = ref.mask_period(v, p, cutoff)
            state = np.full((t, f), REF)
            if "model" in want:
                got = r["model"][clip, ch]
                assert same_bits_or_both_nan(got[:p, :f], model), "model: " + shape
                assert np.all(bits(got[p:]) == FILL) and np.all(bits(got[:, f:]) == FILL), "model rows q >= period / pad bins: " + shape
                note(kernel, "model (bits)", 0.0, 0.0, shape)
            if "mask" in want:
                rest = check_mask_plane(r["mask"][clip, ch], t, f, m, one, state, kernel, shape)
                below += np.count_nonzero(rest)
                total += rest.size
            if "X" in want:
                check_x_plane(r["X"][clip, ch], X[clip, ch], t, f, r["mask"][clip, ch], state, shape)
    return r, (below / total if total else None)


@pytest.mark.parametrize("t", ref.PERIOD_FILL_T)
def test_period_single_network_fill_levels(t):
    """Host period 2, F = 65 (a second bin block with one live lane): positions with ceil(T / 2) and floor(T / 2) segments, on
    both sides of the network sizes 2 / 4 / 8 / 10 / 12 / 16 / 24 / 32."""
    r, share = run_period(ref.magnitudes((1, 1, t, 65), 300 + t), [2], False)
    assert r["launch"]["net"] == ref.net_for(-(-t // 2))
    assert t < 9 or share >= 0.25


@pytest.mark.parametrize("period,t", ref.PERIOD_SWITCH)
def test_period_switch_kernel(period, t):
    """Device period, min_period 1: the launcher cannot bound the segments (T > 32) and the kernel picks the network itself --
    8 / 16 / 32 / 64 / 100 / 128 and the bisection at 129 - 131 segments; the grid has T / 3 + 2 positions, most of which exit."""
    r, share = run_period(ref.magnitudes((1, 1, t, 65), 400 + t + period), [period], True)
    assert r["launch"]["net"] == (-1 if t > 32 else ref.net_for(t)) and share >= 0.25


@pytest.mark.parametrize("want", [("mask", "X"), ("model",)])
def test_period_batch_of_three_clips_with_their_own_periods(want):
    t = 40
    V = ref.magnitudes((3, 2, t, 65), 500)
    X = ref.spectra(V.shape, 501) if "X" in want else None
    run_period(V, [2, 7, t // 3 + 1], True, want=want, X=X, cutoff=3)


@pytest.mark.parametrize("f,parts", [(321, 2), (577, 4)])
def test_period_parts_share_the_bins(f, parts):
    for want in (("mask",), ("model",)):
        r, _ = run_period(ref.magnitudes((1, 1, 12, f), 600 + f), [3], False, want=want)
        assert r["launch"]["parts"] == parts


@pytest.mark.parametrize("cutoff", [0, 1, 7, 64, 70])
def test_period_cutoff(cutoff):
    """cutoff in {0, 1, 7, F - 1, F + 5}: bins 1 .. cutoff exactly 1 (a NaN model included), bin 0 never."""
    V = ref.magnitudes((1, 2, 21, 65), 700)
    V[0, 0, 4] = np.nan
    r, _ = run_period(V, [4], False, want=("mask", "X"), X=ref.spectra(V.shape, 701), cutoff=cutoff)
    m = r["mask"][0, 0, :21, :65]
    assert np.all(m[:, 1:min(cutoff, 64) + 1] == 1.0) and np.isnan(m[4, 0]) and not np.all(m[:, 0] == 1.0)


@pytest.mark.parametrize("t,device", [(21, False), (260, True)])
def test_period_nan_and_infinite_magnitudes(t, device):
    """A NaN frame, a NaN cell and +inf cells: the NaN marks its position in every period -- through the sums of the networks
    (11 segments) and through the bisection (130 segments)."""
    V = ref.magnitudes((1, 1, t, 65), 800 + t)
    V[0, 0, 6] = np.nan
    V[0, 0, 9, 4] = np.nan
    V[0, 0, [3, 7, 11], 8] = np.inf
    V[0, 0, 5, 9] = np.inf
    V[0, 0, 1::2, 10] = np.inf                   # a position that is infinite in every segment: model inf, mask exactly 1
    for want in (("mask",), ("model",)):
        r, _ = run_period(V, [2], device, want=want, tag="nan")
    assert r["launch"]["net"] == (-1 if device else 12)
    assert np.all(np.isnan(r["model"][0, 0, 0, :65])) and np.isnan(r["model"][0, 0, 1, 4]) and r["model"][0, 0, 1, 10] == np.inf


# ---- adaptive ------------------------------------------------------------------------------------------------------------
@np.errstate(all="ignore")
def run_adaptive(V, per, order, want=("mask",), X=None, cutoff=0, tag=""):
    _, c, t, f = V.shape
    shape = "adaptive T=%d F=%d C=%d order=%d cutoff=%d %s %s" % (t, f, c, order, cutoff, "+".join(want), tag)
    r = repet._mask_stage("adaptive", V, X, want=want, cutoff=cutoff, prefill=PREFILL, periods=per, order=order)
    kernel = "mask_adaptive_kernel<%d>" % ref.net_for(order)
    assert (r["launch"]["kernel"], r["launch"]["grid"], r["launch"]["nyquist"]) == (kernel, (t, c, 1), ""), (r["launch"], shape)
    seen(r["launch"])
    below = total = 0
    for ch in range(c):
        m, one = ref.mask_of(V[0, ch], ref.model_adaptive(V[0, ch], per, order), cutoff)
        state = np.full((t, f), REF)
        rest = check_mask_plane(r["mask"][0, ch], t, f, m, one, state, kernel, shape)
        below, total = below + np.count_nonzero(rest), total + rest.size
        if "X" in want:
            check_x_plane(r["X"][0, ch], X[0, ch], t, f, r["mask"][0, ch], state, shape)
    return r, below / total


@pytest.mark.parametrize("order", ref.ADAPTIVE_ORDERS)
def test_adaptive_orders(order):
    """Orders through every network size and into the bisection (129), periods 1, T - 1, T and beyond, taps off either end."""
    f = 257 if order in (5, 16, 129) else 65
    V = ref.magnitudes((1, 2, 150, f), 900 + order)
    per = ref.adaptive_periods(150, order)
    _, share = run_adaptive(V, per, order, want=("mask", "X"), X=ref.spectra(V.shape, 901), cutoff=2 if order == 5 else 0)
    assert order < 3 or share >= 0.25


@pytest.mark.parametrize("order", [9, 13, 100, 129])
def test_adaptive_nan_and_infinite_magnitudes(order):
    V = ref.magnitudes((1, 2, 150, 65), 950 + order)
    V[0, 0, 60] = np.nan
    V[0, 1, 75, 4] = np.nan
    V[0, 0, [30, 31, 33], 8] = np.inf
    V[0, 1, 90, 9] = np.inf
    per = ref.adaptive_periods(150, order)
    r, _ = run_adaptive(V, per, order, tag="nan")
    assert np.isnan(r["mask"][0, 0, 60, :65]).all() and np.isnan(r["mask"][0, 1, 75, 4])


# ---- sim -----------------------------------------------------------------------------------------------------------------
def sim_report(f, max_count, c, b, t, first_frame, n_launch, parts, idx_pitch, path):
    net, split = ref.net_for(max_count), f > 64 and (f - 1) % 64 == 0
    nyquist, nyquist_grid = "", (0, 0, 0)
    if split and parts & 2 and t - first_frame > 0:
        nyquist = "mask_sim_nyquist_kernel<%d, %s>" % (net, "true" if net >= 2 and idx_pitch % 4 == 0 else "false")
        nyquist_grid = (-(-(t - first_frame) // 64), c, b)
    if not parts & 1 or n_launch <= 0:
        return "", None, nyquist, nyquist_grid
    if not split:
        return "mask_sim_kernel<%d, false>" % net, (n_launch, c, b), nyquist, nyquist_grid
    if path == "bits":
        return "mask_sim_bits_kernel<%d, %d>" % (25 if max_count <= 100 else 32, max(11, int(t - 1).bit_length())), (8 * -(-n_launch // 8), 1, 1), nyquist, nyquist_grid
    if path == "rank":
        return "mask_sim_rank_kernel<%d>" % net, (8 * -(-(c * ((f - 1) // 128)) // 8) * -(-n_launch // 4), 1, 1), nyquist, nyquist_grid
    if 2 <= net <= 16 and (f - 1) % 256 == 0:
        return "mask_sim_wide_kernel<%d>" % net, (-(-n_launch // 16), c, b), nyquist, nyquist_grid
    return "mask_sim_kernel<%d, true>" % net, (n_launch, c, b), nyquist, nyquist_grid


def sim_states(t, f, first_frame, frame0, frame_end, parts, warm_end):
    """What a launch does to the cells (T, F) of one clip: REF, ZERO (warm-up rows) or UNTOUCHED."""
    split = f > 64 and (f - 1) % 64 == 0
    state = np.full((t, f), UNTOUCHED)
    main = f - 1 if split else f
    for row in range(frame0, frame_end):
        if row < warm_end:
            if parts & 1:
                state[row, :] = ZERO           # the main kernel zeroes a warm-up row whole, its Nyquist cell included
        else:
            if parts & 1:
                state[row, :main] = REF
            if split and parts & 2:
                state[row, f - 1] = REF
    return state


def run_sim(V, idx, cnt, max_count, refs, want=("mask",), X=None, cutoff=0, first_frame=0, frame0=0, frame_end=0, parts=3,
            slot_start=None, slot_bias=0, idx_pitch=None, path="float", tag=""):
    """refs[clip][channel] = (mask, exactly one) from ref.reference_sim, computed once by the caller and left unchanged."""
    b, c, t, f = V.shape
    end = frame_end or t
    pitch = idx_pitch or max(idx.shape[2], 128)
    shape = "sim T=%d F=%d C=%d B=%d n<=%d first=%d rows=[%d,%d) parts=%d pitch=%d %s %s cutoff=%d %s" % (
        t, f, c, b, max_count, first_frame, frame0, end, parts, pitch, path, "+".join(want), cutoff, tag)
    r = repet._mask_stage("sim", V, X, want=want, cutoff=cutoff, prefill=PREFILL, idx=idx, cnt=cnt, first_frame=first_frame,
                          max_count=max_count, frame0=frame0, frame_end=frame_end, parts=parts, slot_start=slot_start,
                          slot_bias=slot_bias, idx_pitch=idx_pitch, median_path=path)
    kernel, grid, nyquist, nyquist_grid = sim_report(f, max_count, c, b, t, first_frame, end - frame0, parts, pitch, path)
    rep = r["launch"]
    assert (rep["kernel"], rep["nyquist"], rep["nyquist_grid"]) == (kernel, nyquist, nyquist_grid), (rep, shape)
    assert grid is None or rep["grid"] == grid, (rep, shape)
    assert rep["lookups"] == (path == "bits" and bool(kernel))
    seen(rep)
    below = total = 0
    for clip in range(b):
        warm_end = first_frame if slot_start is None else max(first_frame, slot_start[clip] - slot_bias)
        state = sim_states(t, f, first_frame, frame0, end, parts, warm_end)
        for ch in range(c):
            m, one = refs[clip][ch]
            if "mask" in want:
                rest = check_mask_plane(r["mask"][clip, ch], t, f, m, one, state, kernel or nyquist, shape)
                if nyquist and kernel:       # the Nyquist cells once more under their own kernel's name
                    g, col = r["mask"][clip, ch, :t, f - 1].astype(np.float64), (state[:, f - 1] == REF) & ~one[:, f - 1] & ~np.isnan(m[:, f - 1])
                    note(nyquist, "mask", np.abs(g - m[:, f - 1])[col], ref.MASK_BAR * m[col, f - 1], shape)
                below, total = below + np.count_nonzero(rest), total + np.count_nonzero(state == REF)
            if "X" in want and "mask" in want:
                check_x_plane(r["X"][clip, ch], X[clip, ch], t, f, r["mask"][clip, ch], state, shape)
    return r, (below / total if total else None)


def sim_refs(V, idx, cnt, first_frame=0, cutoff=0):
    return [[ref.reference_sim(V[clip, ch], idx[clip], cnt[clip], first_frame, cutoff)[:2] for ch in range(V.shape[1])]
            for clip in range(V.shape[0])]


@pytest.mark.parametrize("max_count", ref.SIM_COUNTS)
@pytest.mark.parametrize("f", ref.SIM_FLOAT_F)
def test_sim_float_kernels(f, max_count):
    """mask_sim_kernel unsplit (F = 40, 100) and split with the Nyquist kernel (F = 65, 129, 193), every network size and the
    bisection (150), lists of every length 0 .. max_count, two channels, mask and X together."""
    t = ref.sim_frames(max_count)
    V, idx, cnt = ref.build_sim(1, 2, t, f, max_count, 1000 * f + max_count)
    assert set(range(max_count + 1)) <= set(cnt.ravel().tolist())
    cutoff = 3 if max_count == 10 else 0
    _, share = run_sim(V, idx, cnt, max_count, sim_refs(V, idx, cnt, 0, cutoff), want=("mask", "X"), X=ref.spectra(V.shape, f), cutoff=cutoff)
    assert share >= 0.25


@pytest.mark.parametrize("f,max_count", [(257, 2), (257, 4), (257, 8), (257, 10), (257, 12), (257, 16), (513, 10), (513, 16), (257, 24)])
def test_sim_wide_kernel_takes_short_lists(f, max_count):
    """F - 1 a multiple of 256 and lists of at most 16 entries: mask_sim_wide_kernel (four bins per lane, runs of 16 frames);
    longer lists on the same shape go back to mask_sim_kernel."""
    t = ref.sim_frames(max_count)
    V, idx, cnt = ref.build_sim(1, 2, t, f, max_count, 2000 * f + max_count)
    r, share = run_sim(V, idx, cnt, max_count, sim_refs(V, idx, cnt), want=("mask", "X"), X=ref.spectra(V.shape, f))
    assert r["launch"]["name"] == ("mask_sim_wide_kernel" if max_count <= 16 else "mask_sim_kernel") and share >= 0.25


WIDE = dict(t=56, f=257, max_count=10)


@pytest.fixture(scope="module")
def wide_case():
    """One input for the wide kernel's launch geometry: three clips with their own lists, list rows numbered from frame 0."""
    V, idx, cnt = ref.build_sim(3, 2, WIDE["t"], WIDE["f"], WIDE["max_count"], 3000)
    return V, ref.spectra(V.shape, 3001), idx, cnt, sim_refs(V, idx, cnt)


@pytest.mark.parametrize("n_launch", [1, 15, 16, 17, 33])
def test_sim_wide_runs_of_frames(wide_case, n_launch):
    """frame0 > 0 and frame_end < T: whole runs of 16 frames, a run of one, a last run of one; the rows outside keep the prefill,
    their Nyquist cells included (the Nyquist kernel covers [first_frame, T) and must leave them alone)."""
    V, X, idx, cnt, refs = wide_case
    r, _ = run_sim(V[:1], idx[:1], cnt[:1], 10, refs[:1], want=("mask", "X"), X=X[:1], frame0=3, frame_end=3 + n_launch)
    assert r["launch"]["grid"][0] == -(-n_launch // 16)


@pytest.mark.parametrize("first_frame,frame0", [(5, 0), (16, 0), (18, 2), (20, 2), (15, 0), (17, 0)])
def test_sim_wide_warm_up_rows(first_frame, frame0):
    """first_frame inside a run of 16, at a run's edge and either side of it: the rows before it are zero in every bin, the Nyquist
    cell included, and the list rows are numbered from first_frame."""
    t, f, n = WIDE["t"], WIDE["f"], WIDE["max_count"]
    V, idx, cnt = ref.build_sim(1, 2, t, f, n, 3100 + first_frame, first_frame=first_frame)
    refs = sim_refs(V, idx, cnt, first_frame)
    X = ref.spectra(V.shape, 3101)
    for want in (("mask", "X"), ("mask",)):
        r, _ = run_sim(V, idx, cnt, n, refs, want=want, X=X if "X" in want else None, first_frame=first_frame, frame0=frame0)
    m = r["mask"][0, :, frame0:first_frame, :f]
    assert np.all(bits(m) == 0)


@pytest.mark.parametrize("want", [("mask",), ("X",), ("mask", "X")])
def test_sim_wide_batch_with_slots(want):
    """Three clips with per-clip list strides; slot_start puts clip 0's warm-up end past first_frame inside a run, clip 1's before
    it (first_frame rules) and leaves clip 2 idle (every row a warm-up row). Mask only, X only (against the mask-only plane of the
    same input), both."""
    t, f, n, first_frame, bias = WIDE["t"], WIDE["f"], WIDE["max_count"], 4, 100
    V, idx, cnt = ref.build_sim(3, 2, t, f, n, 3200, first_frame=first_frame)
    X = ref.spectra(V.shape, 3201)
    refs = sim_refs(V, idx, cnt, first_frame, cutoff=2)
    starts = [bias + 9, bias + 1, IDLE]
    kw = dict(cutoff=2, first_frame=first_frame, slot_start=starts, slot_bias=bias)
    r, _ = run_sim(V, idx, cnt, n, refs, want=want, X=X if "X" in want else None, **kw)
    if want == ("X",):
        plane, _ = run_sim(V, idx, cnt, n, refs, want=("mask",), **kw)
        for clip in range(3):
            state = sim_states(t, f, first_frame, 0, t, 3, max(first_frame, starts[clip] - bias))
            for ch in range(2):
                check_x_plane(r["X"][clip, ch], X[clip, ch], t, f, plane["mask"][clip, ch], state, "X only, B=3 clip %d" % clip)
    else:
        m = r["mask"]
        assert np.all(bits(m[0, :, :9, :f]) == 0) and np.all(bits(m[1, :, :4, :f]) == 0) and np.all(bits(m[2, :, :t, :f]) == 0)
        assert not np.any(bits(m[0, :, 9, :f]) == 0) and not np.any(bits(m[1, :, 4, :f - 1]) == 0)


@pytest.mark.parametrize("rows", [63, 64, 65])
def test_sim_nyquist_kernels(rows):
    """The lane-per-frame Nyquist kernel with its list fetched up front (idx_pitch 128) and entry by entry (idx_pitch 130, no
    16-byte rows): the report names each and the planes are identical; 63 / 64 / 65 list rows around its 64-frame workgroup;
    parts 1, 2 and 3 write disjoint cells."""
    f, n = 129, 10
    V, idx, cnt = ref.build_sim(1, 2, rows, f, n, 4000 + rows)
    refs = sim_refs(V, idx, cnt)
    planes = {}
    for pitch in (128, 130):
        for parts in (1, 2, 3):
            r, _ = run_sim(V, idx, cnt, n, refs, parts=parts, idx_pitch=pitch)
            planes[pitch, parts] = r["mask"]
            assert r["launch"]["nyquist_preload"] == (pitch == 128 and parts != 1)
    for parts in (1, 2, 3):
        assert np.array_equal(bits(planes[128, parts]), bits(planes[130, parts]))
    both = np.where(bits(planes[128, 1]) == FILL, bits(planes[128, 2]), bits(planes[128, 1]))
    assert np.array_equal(both, bits(planes[128, 3]))
    # a window of frames with first_frame > 0: the same kernel leaves the rows outside [frame0, frame_end) alone
    V, idx, cnt = ref.build_sim(1, 2, rows, f, n, 4100 + rows, first_frame=7)
    run_sim(V, idx, cnt, n, sim_refs(V, idx, cnt, 7), first_frame=7, frame0=2, frame_end=rows - 5, parts=3)
    run_sim(V, idx, cnt, n, sim_refs(V, idx, cnt, 7), first_frame=7, frame0=2, frame_end=rows - 5, parts=2)


RANK_CASES = [(129, 100), (129, 128), (1025, 100)]
_rank_inputs = {}


def rank_input(f, max_count):
    """T = 1100, stereo: the input, the reference and the float kernel's plane, computed once per shape and left unchanged."""
    if (f, max_count) not in _rank_inputs:
        t = 1100
        V, idx, cnt = ref.build_sim(1, 2, t, f, max_count, 5000 + f + max_count)
        refs = sim_refs(V, idx, cnt, cutoff=2)
        X = ref.spectra(V.shape, 5001)
        r, share = run_sim(V, idx, cnt, max_count, refs, want=("mask", "X"), X=X, cutoff=2)
        assert share >= 0.25 and set(range(max_count + 1)) <= set(cnt.ravel().tolist())
        _rank_inputs[f, max_count] = (V, X, idx, cnt, refs, r["mask"], r["X"])
    return _rank_inputs[f, max_count]


@pytest.mark.parametrize("path", ["rank", "bits"])
@pytest.mark.parametrize("f,max_count", RANK_CASES)
def test_sim_rank_paths_stereo(f, max_count, path):
    """The packed-rank network and the bit-sliced selection at C = 2 -- 4 and 32 blocks of 64 bins, cells numbered channel-major
    -- against the reference, against the float kernel's plane bit for bit, and (bit-sliced) the code words against NumPy's sort."""
    V, X, idx, cnt, refs, float_mask, float_x = rank_input(f, max_count)
    t = V.shape[2]
    r, _ = run_sim(V, idx, cnt, max_count, refs, want=("mask", "X"), X=X, cutoff=2, path=path)
    assert np.array_equal(bits(r["mask"]), bits(float_mask)) and np.array_equal(bits(r["X"].view(np.float32)), bits(float_x.view(np.float32)))
    note(r["launch"]["kernel"], "mask == float kernel's (bits)", 0.0, 0.0, "T=%d F=%d C=2 n<=%d" % (t, f, max_count))
    if path == "bits":
        for ch in range(2):
            v = V[0, ch, :, :f - 1]
            ranks = np.stack([np.searchsorted(np.sort(v[:, k]), v[:, k], side="left") for k in range(f - 1)], axis=1)        # (T, F - 1)
            codes = r["codes"][ch, :t, :f - 1].astype(np.int64)
            for i in range(0, t, 5):
                n = int(cnt[0, i])
                if n == 0:
                    continue
                s = np.sort(ranks[idx[0, i, :n]], axis=0)
                lower, upper = s[(n - 1) // 2], s[n // 2]
                assert np.array_equal(codes[i] & 0x7fff, lower) and np.array_equal(codes[i] >> 16, upper), (ch, i)
                assert np.array_equal((codes[i] >> 15) & 1, (lower < ranks[i]).astype(np.int64)), (ch, i)
            assert np.all(r["codes"][ch, t:] == FILL) and np.all(r["codes"][ch, :, f - 1:] == FILL)
        note(r["launch"]["kernel"], "code words == NumPy's sort", 0.0, 0.0, "T=%d F=%d C=2 n<=%d" % (t, f, max_count))


def test_stage_entry_refuses_what_would_index_out_of_range():
    V, idx, cnt = ref.build_sim(1, 1, 20, 65, 4, 6000)
    bad = idx.copy()
    bad[0, 3, 1] = 20
    with pytest.raises(ValueError):
        repet._mask_stage("sim", V, idx=bad, cnt=cnt)
    bad[0, 3, 1] = -1
    with pytest.raises(ValueError):
        repet._mask_stage("sim", V, idx=bad, cnt=cnt)
    with pytest.raises(ValueError):
        repet._mask_stage("sim", V, idx=idx, cnt=cnt + 5)
    with pytest.raises(ValueError):
        repet._mask_stage("sim", V, idx=idx, cnt=cnt, frame0=9, frame_end=8)
    with pytest.raises(ValueError):
        repet._mask_stage("sim", V, idx=idx, cnt=cnt, frame_end=21)
    with pytest.raises(ValueError):
        repet._mask_stage("sim", V, idx=idx, cnt=cnt, idx_pitch=100)
    with pytest.raises(ValueError):
        repet._mask_stage("period", V, period=0)
    with pytest.raises(ValueError):
        repet._mask_stage("period", V, periods=[9], min_period=1)          # past T / 3 + 2
    with pytest.raises(ValueError):
        repet._mask_stage("adaptive", V, periods=np.zeros(20, dtype=np.int32), order=3)
    with pytest.raises(RuntimeError):
        repet._mask_stage("sim", V, idx=idx, cnt=cnt, median_path="rank")   # too short, F - 1 no multiple of 128: no silent fallback


def test_zz_parity_record():
    """Every kernel of the family was launched by the cases above; the largest error / bar per (kernel, check) is printed and
    written to $REPET_MASK_STAGE_PARITY_OUT."""
    families = {k.split("<")[0] for k in KERNELS_SEEN}
    assert {"mask_period_kernel", "mask_adaptive_kernel", "mask_sim_kernel", "mask_sim_wide_kernel", "mask_sim_nyquist_kernel",
            "mask_sim_rank_kernel", "mask_sim_bits_kernel", "parts=1", "parts=2", "parts=4"} <= families, sorted(KERNELS_SEEN)
    assert "mask_period_kernel<-1>" in KERNELS_SEEN and any(k.startswith("mask_period_kernel<") and "-1" not in k for k in KERNELS_SEEN)
    assert any(k.startswith("mask_sim_kernel<") and k.endswith("true>") for k in KERNELS_SEEN)
    assert any(k.startswith("mask_sim_kernel<") and k.endswith("false>") for k in KERNELS_SEEN)
    assert any(k.startswith("mask_sim_nyquist_kernel<") and k.endswith("true>") for k in KERNELS_SEEN)
    assert any(k.startswith("mask_sim_nyquist_kernel<") and k.endswith("false>") for k in KERNELS_SEEN)
    lines = ["%-44s %-34s %10s %12s %12s  %s" % ("kernel", "check", "err/bar", "error", "bar", "worst case")]
    for (kernel, check), (ratio, err, bar, shape) in sorted(PARITY.items()):
        lines.append("%-44s %-34s %10.4f %12.4e %12.4e  %s" % (kernel, check, ratio, err, bar, shape))
    lines.append("kernels launched: " + ", ".join(sorted(k for k in KERNELS_SEEN if not k.startswith("parts="))))
    text = "\n".join(lines) + "\n"
    print("\n" + text)
    out = os.environ.get("REPET_MASK_STAGE_PARITY_OUT")
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    assert all(ratio <= 1.0 for ratio, _, _, _ in PARITY.values())
