"""Float64 NumPy statement of the peak picking of ``sim``, ``simonline`` and the live handles, and the cases the GPU test
tests/test_gpu_peaks_stages.py runs through ``repet._peaks_stage`` (CPU only; checked by tests/test_peaks_reference.py).

What the kernels promise (peaks.h, peaks_exact.hip): the similar-frame lists are those of the float64 reference,
whatever the fp32 rounding of the similarity matrix. Three values of every similarity are involved:

  M    the fp32 matrix / band the first pass reads;
  e1   the float64 cosine of the FP32 unit rows, norms divided out (``exact_similarity2``): level 1;
  e2   the dot product of the FLOAT64 unit rows (``unit64``: float64 Hamming window, frames of hi + lo, magnitudes of bins
       0 .. W/2, channel mean, 2-norm): level 2, the reference's own value.

Tiered decisions. A kernel trusts an fp32 comparison whose gap exceeds ``delta`` and a level-1 comparison whose gap is at least
``delta2``. With |M - e1| <= 0.4 delta and |e1 - e2| <= 0.4 delta2 for every element a launch can read, a trusted fp32 gap
(> delta) leaves an e1 gap > 0.2 delta and -- delta being several times delta2 -- an e2 gap of the same sign; a trusted
level-1 gap (>= delta2) leaves an e2 gap >= 0.2 delta2 of the same sign; a comparison of a level-1 value with a level-2 value
of another element that is trusted has a gap >= delta2 against an error <= 0.4 delta2. So every trusted decision has the sign
of the e2 comparison, and the lists equal ``orc.localmaxima`` of the e2 row -- provided the e2 comparisons themselves do not
hinge on the last bits: every pair of e2 values that meets in a window, at the threshold or across the top-``number`` cut is
either exactly equal (frames that are identical sample for sample: one class, evaluated once) or at least ``SEPARATION``
apart. ``premises`` measures the three conditions; ``build`` refuses a case that violates one.

A launch without the second level (``refine`` 1) leaves its close level-1 verdicts as they are: its reference is the e1 row.
The cases that run at that level are built so that the e1 row and the e2 row give the same lists (asserted on the CPU), so
"the reference is ``orc.localmaxima`` of the e2 row" holds for them too. Rows with more near-ties than the first pass's lists
hold (``kAmbCap`` elements, ``kRivalCap`` pairs: "flat" rows) keep their fp32 decisions at that level by the kernels' own
contract (peaks.h); the cases that contain such rows run with both levels only.
"""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.signal.windows

from oracle import repet_oracle as orc

SEPARATION = 1e-11         # 250 x the bar of the float64 spectra at W = 256 (fft_bar): device-versus-NumPy rounding stays out
PLANT_SHARE = 0.35         # |M - fp32(e1 +- share * delta)|: the fp32 rounding of a value below 1 adds 3e-8, far inside 0.4 delta
K_AMB_CAP = 96             # peaks.h: kAmbCap, kRivalCap -- only to SIZE the stress rows; the test asserts the device counters
K_RIVAL_CAP = 96
K_MIN_IDX_PITCH = 128      # common.h


def round_up(x, m):
    return -(-x // m) * m


def fft_bar(W):
    """Bar for a float64 unit row, 2-norm and per component: Higham's norm-wise bound for the radix-2 FFT, about 8 u log2 N,
    doubled for the window product, magnitude, channel mean and normalisation: 16 log2(W) 2^-53."""
    return 16.0 * np.log2(W) * 2.0 ** -53


def design_deltas(F, f16_gram=True):
    """delta, delta2 as engine_sim.hip states them (peak_refine_delta in fp32 arithmetic, peak_exact_delta2). The CPU test
    builds the cases with these; the GPU test takes the two numbers from the stage's report and builds with those."""
    fs = np.float32(round_up(F, 32))
    delta = np.float32(2.0 if f16_gram else 4.0) * np.sqrt(fs, dtype=np.float32) * np.float32(5.9604645e-8)
    return float(delta), 2.5e-7


# ---- float64 unit rows ---------------------------------------------------------------------------------------------------
def frame_samples(hi, lo, W, H, frame_sample0, n_frames):
    """(n_frames, W, C) float64 samples of hi + lo, zero outside [0, n_samples)."""
    x = np.asarray(hi, dtype=np.float64)
    if lo is not None:
        x = x + np.asarray(lo, dtype=np.float64)
    n = x.shape[0]
    at = frame_sample0 + np.arange(n_frames)[:, None] * H + np.arange(W)[None, :]
    inside = (at >= 0) & (at < n)
    return np.where(inside[:, :, None], x[np.clip(at, 0, n - 1)], 0.0)


def frame_classes(frames):
    """(class of every frame, first frame of every class): frames equal sample for sample (as bytes) share a class."""
    flat = np.ascontiguousarray(frames.reshape(frames.shape[0], -1))
    keys = flat.view(np.dtype((np.void, flat.dtype.itemsize * flat.shape[1]))).ravel()
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    return inverse.ravel(), first


def unit_rows_of(frames, W):
    """Unit rows of (K, W, C) float64 frames, in the issue's order: window, magnitudes of bins 0 .. W/2, channel mean, 2-norm.
    A silent frame is a NaN row."""
    window = scipy.signal.windows.hamming(W, sym=False)
    mag = np.abs(np.fft.rfft(frames * window[None, :, None], axis=1))        # (K, F, C)
    mean = np.mean(mag, axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return mean / np.sqrt(np.sum(np.power(mean, 2), axis=1))[:, None]


def unit64_classes(hi, lo, W, H, frame_sample0, n_frames):
    """(unit rows of the classes, class of every frame): every class of identical frames is evaluated ONCE."""
    frames = frame_samples(hi, lo, W, H, frame_sample0, n_frames)
    cls, first = frame_classes(frames)
    return unit_rows_of(frames[first], W), cls


def unit64(hi, lo, W, H, frame_sample0, n_frames):
    rows, cls = unit64_classes(hi, lo, W, H, frame_sample0, n_frames)
    return rows[cls]


def unit_longdouble(frames, W):
    """The same rows from a direct DFT in np.longdouble (a handful of frames: O(W^2) each)."""
    ld = np.longdouble
    n = np.arange(W)
    two_pi = 2 * np.arctan2(ld(0), ld(-1))
    window = ld(0.54) - ld(0.46) * np.cos(two_pi * n.astype(ld) / W)
    turn = two_pi * n.astype(ld) / W
    cos_t, sin_t = np.cos(turn), np.sin(turn)
    F = W // 2 + 1
    out = []
    for fr in frames:                                                          # (W, C)
        x = fr.astype(ld) * window[:, None]
        mag = np.zeros((F, x.shape[1]), dtype=ld)
        for k0 in range(0, F, 128):
            k = np.arange(k0, min(F, k0 + 128))
            ph = (k[:, None] * n[None, :]) % W                                 # exact phase index
            re = cos_t[ph] @ x
            im = sin_t[ph] @ x
            mag[k] = np.sqrt(re * re + im * im)
        mean = np.sum(mag, axis=1) / ld(x.shape[1])
        out.append(mean / np.sqrt(np.sum(mean * mean)))
    return np.array(out)


class Spectra:
    """The unit rows of one clip at both levels, by class. ``e2(self, elems)`` / ``e1(self, elems)``: the values of frame rows
    ``elems`` against frame row ``self``, every class evaluated once and expanded (a BLAS product does not promise equal bits
    for equal rows at different positions)."""

    def __init__(self, hi, lo, W, frame_sample0, n_frames):
        H = W // 2
        self.W, self.H, self.F, self.n_frames = W, H, W // 2 + 1, n_frames
        self.u64c, self.cls2 = unit64_classes(hi, lo, W, H, frame_sample0, n_frames)
        u_hi, self.cls1 = unit64_classes(hi, None, W, H, frame_sample0, n_frames)
        self.u32c = u_hi.astype(np.float32)                # what the fp32 pipeline hands the peak picking: fp32(unit64) of hi
        self._u32c64 = self.u32c.astype(np.float64)
        with np.errstate(invalid="ignore"):
            self._n32 = np.sum(self._u32c64 * self._u32c64, axis=1)

    @property
    def unit32(self):
        return self.u32c[self.cls1]

    @property
    def unit64(self):
        return self.u64c[self.cls2]

    def e2(self, self_row, elems):
        cs = self.cls2[elems]
        uniq, inv = np.unique(cs, return_inverse=True)
        with np.errstate(invalid="ignore"):
            return (self.u64c[uniq] @ self.u64c[self.cls2[self_row]])[inv]

    def e1(self, self_row, elems):
        cs = self.cls1[elems]
        uniq, inv = np.unique(cs, return_inverse=True)
        me = self.cls1[self_row]
        with np.errstate(invalid="ignore"):
            return ((self._u32c64[uniq] @ self._u32c64[me]) / np.sqrt(self._n32[uniq] * self._n32[me]))[inv]


# ---- row geometry (peaks.h: the modes, row_columns, apply_origin; common.h: PeakBatch) --------------------------------------
def row_elements(mode, j, n_cols, start=0, origin=None, shift=0):
    """Row ``j`` (its global number: row0 + r) of a launch. None for an inactive row (a clip with an origin whose row is younger
    than start - 1 frames of its own stream). Else a namespace: ``n`` columns; ``lag`` of every column (modes 1, 2); ``rows`` the
    frame row (band row, unit row) each column holds; ``written`` the index the kernels write for it; ``self_row`` the row's own
    frame row; ``band`` (modes 1, 2) the (band row, lag) cell of every column in the layout of that mode."""
    if mode == 0:
        cols = np.arange(n_cols)
        return SimpleNamespace(n=n_cols, lag=None, rows=cols, written=cols, self_row=j, band=None)
    jl = j - (origin or 0)                                    # apply_origin: rows counted from the clip's own first frame
    if origin is not None and jl < (start or n_cols) - 1:
        return None
    assert jl >= 0
    n = min(n_cols, jl + 1)                                   # row_columns: the stream's own frames 0 .. jl while it fills
    cols = np.arange(n)
    lag = np.mod(jl - cols, n)
    rows = j - lag - shift                                    # the band rows stay where they are
    band = (rows, lag) if mode == 1 else (np.full(n, j - shift), lag)
    return SimpleNamespace(n=n, lag=lag, rows=rows, written=rows, self_row=j - shift, band=band)


def expected_list(values, min_value, d, number):
    """(kept values, kept columns) of a row: orc.localmaxima."""
    vals, cols = orc.localmaxima(values, min_value, d, number)
    return np.asarray(vals, dtype=np.float64), np.asarray(cols, dtype=np.int64)


def row_separation(values, classes, min_value, d, number):
    """Premise 3 for one row of level values: (SEPARATION / the smallest gap that is not an exact class tie -- inf when two
    DIFFERENT classes are exactly equal --, True when an exact tie sits among the kept values or across the cut)."""
    v = np.asarray(values, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        left = orc._trailing_max(v, d)
        right = orc._trailing_max(v[::-1], d)[::-1]
        top = np.maximum(left, right)
        gap = np.abs(v - top)
    worst = 0.0
    live = np.isfinite(gap)
    small = live & (gap < SEPARATION)
    for i in np.flatnonzero(small):
        lo, hi = max(i - d, 0), min(i + d + 1, len(v))
        rivals = [k for k in range(lo, hi) if k != i and v[k] == top[i]]
        if gap[i] != 0.0 or not all(classes[k] == classes[i] for k in rivals):
            worst = max(worst, np.inf if gap[i] == 0.0 else SEPARATION / gap[i])
    if np.any(live & ~small):
        worst = max(worst, SEPARATION / float(np.min(gap[live & ~small])))
    keep = orc.localmaxima_mask(v, min_value, d)
    cand = np.flatnonzero(keep)
    tie = False
    if len(cand):
        thr = np.abs(v[cand] - min_value)
        worst = max(worst, np.inf if np.min(thr) == 0.0 else SEPARATION / float(np.min(thr)))
        order = cand[np.argsort(v[cand], kind="stable")[::-1]][:number + 1]
        for at, (a, b) in enumerate(zip(order[:-1], order[1:])):
            g = v[a] - v[b]
            if g == 0.0 and classes[a] == classes[b]:
                tie = tie or at == number - 1             # an exact tie ACROSS the cut: the kept set itself is open
            else:
                worst = max(worst, np.inf if g == 0.0 else SEPARATION / g)
    # an element the threshold alone decides (no window rival near it) is a candidate above; one below the threshold that
    # would otherwise be a strict maximum must not sit on it either
    with np.errstate(invalid="ignore"):
        under = np.flatnonzero((v > top) & (v < min_value))
    if len(under):
        g = float(np.min(min_value - v[under]))
        worst = max(worst, SEPARATION / g)
    return worst, tie


def order_margin(values, classes, min_value, d, number, delta):
    """What the ORDER of a row's kept entries rests on. The refinement re-takes VERDICTS -- window maximum, threshold, cut --
    from float64 values; the ranking inside the kept set stays fp32's (peaks.hip: "ranked by counting"), and a refined winner
    enters it with its level-1 value beside the fp32 values of the others. The planted perturbation moves every kept entry by the
    same amount, so fp32 keeps their order as long as two kept values do not round to one fp32 number (2^-22 apart), and a
    kept entry with a window rival inside 2 delta (it may be refined) is more than delta from every other kept value. Returns
    the smallest such margin ratio (>= 1: the ordered comparison is safe), exact class ties aside."""
    v = np.asarray(values, dtype=np.float64)
    vals, cols = expected_list(v, min_value, d, number)
    if len(cols) < 2:
        return np.inf
    with np.errstate(invalid="ignore"):
        top = np.maximum(orc._trailing_max(v, d), orc._trailing_max(v[::-1], d)[::-1])
    refined = (v[cols] - top[cols]) < 2 * delta
    worst = np.inf
    for a in range(len(cols) - 1):
        g = vals[a] - vals[a + 1]
        if g == 0.0 and classes[cols[a]] == classes[cols[a + 1]]:
            continue
        need = delta if (refined[a] or refined[a + 1]) else 2.0 ** -22
        worst = min(worst, g / need)
    return worst


# ---- synthetic audio -------------------------------------------------------------------------------------------------------
def make_audio(n_frames, W, C, seed, frame_sample0=0, tail=None):
    """fp32 audio (n_samples, C): a few dozen partials plus noise, every frame different. frame_sample0 = -W/2: the first and
    the last frame lie partly outside the signal."""
    H = W // 2
    n = (n_frames - 1) * H + W + 2 * frame_sample0 if tail is None else tail
    rng = np.random.RandomState(seed)
    t = np.arange(n)[:, None]
    x = 0.25 * rng.standard_normal((n, C))
    for _ in range(24):
        f = rng.uniform(0.002, 0.45)
        x += rng.uniform(0.01, 0.08) * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28, (1, C))) * (1 + 0.5 * np.sin(t * rng.uniform(1e-4, 4e-3)))
    return (x / np.max(np.abs(x)) * 0.9).astype(np.float32)


class Planter:
    """Writes copies of frames into other frames of one clip's audio: exact copies (one class with their source: exact ties
    at every level), copies plus ``eps`` x a fixed noise (near-ties; the same (eps, key) is one class), and twins (the same hi,
    a remainder plane lo of half an fp32 ulp: bit-equal fp32 unit rows, float64 rows that differ by 1e-10 .. 1e-8)."""

    def __init__(self, hi, W, frame_sample0, with_lo):
        self.hi, self.W, self.H, self.s0 = hi, W, W // 2, frame_sample0
        self.lo = np.zeros_like(hi) if with_lo else None
        self.used = set()

    def span(self, frame):
        a = self.s0 + frame * self.H
        assert 0 <= a and a + self.W <= len(self.hi), "a planted frame lies inside the signal"
        return slice(a, a + self.W)

    def copy(self, dst, src, eps=0.0, key=0, twin=None):
        assert all(abs(dst - u) >= 2 for u in self.used - {dst}) and abs(dst - src) >= 2, "planted frames do not overlap"
        self.used.add(dst)
        x = self.hi[self.span(src)].astype(np.float64)
        if eps:
            x = x + eps * np.random.RandomState(1000 + key).standard_normal(x.shape)
        self.hi[self.span(dst)] = x.astype(np.float32)
        if self.lo is not None:
            self.lo[self.span(dst)] = 0.0 if twin is None else self.twin_plane(self.hi[self.span(dst)], twin)

    def protect(self, frame):
        self.used.add(frame)

    @staticmethod
    def twin_plane(hi, seed):
        ulp = np.spacing(np.abs(hi).astype(np.float32)).astype(np.float64)
        return (0.5 * ulp * np.random.RandomState(seed).uniform(-1, 1, hi.shape)).astype(np.float32)


def eps_for_gap(frame, W, target, key=0):
    """eps such that a copy of ``frame`` (W, C) plus eps x noise(key) has e2 = 1 - target against the frame (1 - e2 grows as
    eps^2: two secant steps from a first guess)."""
    noise = np.random.RandomState(1000 + key).standard_normal(frame.shape)
    base = frame.astype(np.float64)

    def gap(eps):
        u = unit_rows_of(np.stack([base, (base + eps * noise).astype(np.float32).astype(np.float64)]), W)
        d = u[0] - u[1]
        return 0.5 * float(d @ d)                      # 1 - cos of two unit vectors, without cancellation

    eps = 1e-3
    for _ in range(6):
        g = gap(eps)
        if g <= 0:
            eps *= 4
            continue
        eps *= np.sqrt(target / g)
    return eps


# ---- cases -----------------------------------------------------------------------------------------------------------------
class Clip:
    def __init__(self, hi, lo, W, frame_sample0, n_frames):
        self.hi, self.lo = hi, lo
        self.sp = Spectra(hi, lo, W, frame_sample0, n_frames)


def _signs_from(expected_cols, n):
    """Planted perturbation in units of share x delta: the reference's winners down, everything else up -- every fp32 decision
    within 2 x share x delta of a tie flips --, the losers by 1 or 0.3 in turn so that exact ties come apart in fp32 too."""
    s = np.where((np.arange(n) * 2654435761 >> 7) & 1, 1.0, 0.3)
    s[expected_cols] = -1.0
    return s


def build(spec, delta, delta2, attempts=6):
    """``build_once`` on the case's clip; a clip that violates a premise is refused and the next seed of the case is taken (the
    background of noise and partials puts two kept values inside the fp32 resolution of each other in one clip of five or so)."""
    for attempt in range(attempts):
        try:
            return build_once(spec, delta, delta2, attempt)
        except AssertionError as e:
            refused = e
    raise refused


def build_once(spec, delta, delta2, attempt=0):
    """A case ready for ``repet._peaks_stage``: spec (a namespace from CASES: geometry + a function that makes the clips) ->
    namespace with M (mode 0) or band1 / band2 (modes 1, 2; absent cells NaN), unit32, hi, lo, per (clip, row) the e1 / e2 rows,
    classes, geometry and expected lists, and ``premise`` = the three worst ratios. Raises AssertionError when a premise fails."""
    s = SimpleNamespace(**vars(spec))
    clips = s.make(delta, delta2, attempt)
    if getattr(s, "threshold_quantile", None):
        s.min_value = _threshold_near(next(c for c in clips if c is not None).sp, s.row0, s.threshold_quantile)
    nb = len(clips)
    n_frames = clips[0].sp.n_frames if clips[0] is not None else next(c for c in clips if c is not None).sp.n_frames
    F = s.W // 2 + 1
    origins = s.origin if s.origin is not None else [None] * nb
    rows = {}
    worst1 = worst2 = worst3 = 0.0
    margin = np.inf
    ties = 0
    if s.mode == 0:
        M = np.full((nb, s.row0 + s.n_rows, s.n_cols), np.nan, dtype=np.float32)
    else:
        band1 = np.full((nb, n_frames, s.n_cols), np.nan, dtype=np.float32)
        band2 = np.full((nb, n_frames, s.n_cols), np.nan, dtype=np.float32)
    for b in range(nb):
        for r in range(s.n_rows):
            j = s.row0 + r
            geo = row_elements(s.mode, j, s.n_cols, s.start, origins[b], s.shift)
            if geo is None:
                rows[(b, r)] = None
                continue
            sp = clips[b].sp
            e1 = sp.e1(geo.self_row, geo.rows)
            e2 = sp.e2(geo.self_row, geo.rows)
            cls1, cls2 = sp.cls1[geo.rows], sp.cls2[geo.rows]
            v2, c2 = expected_list(e2, s.min_value, s.d, s.number)
            v1, c1 = expected_list(e1, s.min_value, s.d, s.number)
            with np.errstate(invalid="ignore"):
                m = (e1 + PLANT_SHARE * delta * _signs_from(c2, geo.n)).astype(np.float32)
            if s.mode == 0:
                M[b, j] = m
            else:
                band1[b, geo.rows, geo.lag] = m
                band2[b, j - s.shift, geo.lag] = m
            ok = ~np.isnan(e2)
            assert np.array_equal(np.isnan(e1), ~ok) and np.array_equal(np.isnan(m), ~ok)
            if np.any(ok):
                worst1 = max(worst1, float(np.max(np.abs(m[ok].astype(np.float64) - e1[ok]))) / (0.4 * delta))
                worst2 = max(worst2, float(np.max(np.abs(e1[ok] - e2[ok]))) / (0.4 * delta2))
            w3, tie = row_separation(e2, cls2, s.min_value, s.d, s.number)
            if 1 in s.levels:                              # level 1 alone decides on e1: the same separation there
                w3 = max(w3, row_separation(e1, cls1, s.min_value, s.d, s.number)[0])
            worst3 = max(worst3, w3)
            margin = min(margin, order_margin(e2, cls2, s.min_value, s.d, s.number, delta))
            ties += bool(tie)
            rows[(b, r)] = SimpleNamespace(geo=geo, e1=e1, e2=e2, cls2=cls2, vals2=v2, cols2=c2, vals1=v1, cols1=c1, m=m)
    active = [k for k, v in rows.items() if v is not None]
    out = SimpleNamespace(spec=s, clips=clips, rows=rows, n_batch=nb, n_frames=n_frames, F=F, delta=delta, delta2=delta2,
                          premise=(worst1, worst2, worst3), order_margin=margin, tied_rows=ties, active=active,
                          KP=max(s.number, K_MIN_IDX_PITCH))
    if s.mode == 0:
        out.M = M
    else:
        out.band1, out.band2 = band1, band2
    live = [c for c in clips if c is not None]
    silent = np.zeros((n_frames, F), dtype=np.float32)
    out.unit32 = np.stack([c.sp.unit32 if c is not None else silent for c in clips])
    out.hi = np.stack([c.hi if c is not None else np.zeros_like(live[0].hi) for c in clips])
    out.lo = None if live[0].lo is None else np.stack([c.lo if c is not None else np.zeros_like(live[0].hi) for c in clips])
    assert worst1 <= 1.0, "%s: |M - e1| = %.3f x 0.4 delta" % (s.name, worst1)
    assert worst2 <= 1.0, "%s: |e1 - e2| = %.3f x 0.4 delta2" % (s.name, worst2)
    assert worst3 <= 1.0, "%s: a pair of values %.3g x closer than the separation" % (s.name, worst3)
    assert margin >= 1.0, "%s: the order of two kept entries rests on fp32 (margin %.3g)" % (s.name, margin)
    assert ties <= 0.1 * max(len(active), 1) or s.allow_ties, "%s: %d of %d rows tie at the cut" % (s.name, ties, len(active))
    return out


def premises(case):
    return case.premise


def check_row(got, count, row, level, number, d, written=None):
    """The issue's assert for one active row: ``got`` the row's ``number`` list cells, ``count`` its length. level 2: the e2 row
    decides, level 1: the e1 row. Equal ordered sequences where the kept values are distinct; with exact ties among them equal
    sorted values, indices valid and distinct, and equal sets when fewer than ``number`` survive. Returns an error string or None."""
    vals, cols, values = (row.vals2, row.cols2, row.e2) if level == 2 else (row.vals1, row.cols1, row.e1)
    written = row.geo.written if written is None else written
    if count != len(cols):
        return "count %d, reference %d (reference %s)" % (count, len(cols), written[cols][:8].tolist())
    mine = np.asarray(got[:count], dtype=np.int64)
    if len(np.unique(vals)) == len(vals):
        if not np.array_equal(mine, written[cols]):
            return "list %s, reference %s" % (mine[:10].tolist(), written[cols][:10].tolist())
    else:
        where = {int(w): c for c, w in enumerate(written.tolist())}
        if len(set(mine.tolist())) != count or any(int(k) not in where for k in mine):
            return "indices not valid and distinct: %s" % mine[:10].tolist()
        at = np.array([where[int(k)] for k in mine], dtype=np.int64)
        if not np.array_equal(values[at], vals):
            return "kept values differ from the reference's"
        if not set(at.tolist()) <= set(np.flatnonzero(orc.localmaxima_mask(values, -np.inf, d)).tolist()):
            return "a kept index is no strict maximum of its window"
        if count < number and set(at.tolist()) != set(cols.tolist()):
            return "fewer than `number` survive, yet the sets differ"
    if np.any(np.asarray(got[count:number]) != -1):
        return "cells count .. number-1 are not -1"
    return None


def _spec(name, **kw):
    base = dict(name=name, mode=0, W=256, C=1, row0=0, d=5, number=100, min_value=0.0, shift=0, origin=None, start=0, with_scratch=False,
                levels=(1,), frame_sample0=0, allow_ties=False, pitch=None, expect=None, qmax=None, planted=False, level2=None,
                threshold_quantile=None, flat_rows=0, hands_on=False)
    base.update(kw)
    return SimpleNamespace(**base)


def _threshold_near(sp, row, fraction):
    """An fp32-representable threshold inside the values of frame row `row`."""
    v = sp.e2(row, np.arange(sp.n_frames))
    return float(np.float32(np.quantile(v[np.isfinite(v)], fraction)))


def _pair_values(W, row_frame, hi, lo=None):
    """(e1, e2) of one frame (hi (+ lo), (W, C)) against the frame `row_frame` (hi only), as Spectra computes them."""
    x = hi.astype(np.float64)
    u_hi = unit_rows_of(np.stack([row_frame.astype(np.float64), x]), W)
    u_full = u_hi if lo is None else unit_rows_of(np.stack([row_frame.astype(np.float64), x + lo.astype(np.float64)]), W)
    a = u_hi.astype(np.float32).astype(np.float64)
    return float(a[0] @ a[1] / np.sqrt((a[0] @ a[0]) * (a[1] @ a[1]))), float(u_full[0] @ u_full[1])


def _clip(seed, n_frames, W=256, C=1, frame_sample0=0, with_lo=False, plants=(), silent=(), period=0):
    """make(delta, delta2) for one clip: noise + partials (period > 0: one period of that many hops, tiled bit for bit), silent
    frames, and planted frames (dst, src, kind, arg[, key]):
      "copy"   an exact copy (one class with its source);
      "near"   a copy + noise with e2 = 1 - arg x delta against the source (the same key: the same noise, one class);
      "close"  the same with arg x delta2;
      "twin"   the same hi as src, a remainder plane lo found (seeds from arg) such that, seen from frame `key`, the twin's e2
               is at least 1e-10 BELOW its source's: index order (the higher index first on an exact level-1 tie) is reversed;
      "far"    a copy + noise with e2 = 1 - arg against the source (arg of a few hundredths: a frame whose similarities to the
               source carry the first-order rounding of the fp32 spectra, about 1e-8, like any unrelated pair);
      "step"   a copy of src + noise whose e2, seen from frame `key`, lies arg x delta beside src's (first order in the noise);
      "rev"    a copy of src + a little noise found such that, seen from frame `key`, its e2 differs from src's by 1e-10 ..
               0.35 delta2 and the e1 order of the two is the OPPOSITE."""
    def make(delta, delta2, attempt=0):
        H = W // 2
        hi = make_audio(n_frames, W, C, seed + 7919 * attempt, frame_sample0)
        if period:
            one = hi[:period * H].copy()
            hi = np.tile(one, (-(-len(hi) // len(one)), 1))[:len(hi)].copy()
        for f in silent:
            a = frame_sample0 + f * H
            hi[max(a, 0):a + W] = 0.0
        need_lo = with_lo or any(p[2] == "twin" for p in plants)
        pl = Planter(hi, W, frame_sample0, need_lo)
        for p in plants:
            pl.protect(p[1])
        for k, p in enumerate(plants):
            dst, src, kind, arg = p[:4]
            key = p[4] if len(p) > 4 else k
            if kind == "copy":
                pl.copy(dst, src)
            elif kind in ("near", "close", "far"):
                target = arg * (delta if kind == "near" else delta2 if kind == "close" else 1.0)
                pl.copy(dst, src, eps=eps_for_gap(hi[pl.span(src)], W, target, key=key), key=key)
            elif kind == "twin":
                seen_from = hi[pl.span(key)]
                base = _pair_values(W, seen_from, hi[pl.span(src)])[1]
                for seed2 in range(arg, arg + 200):
                    lo = Planter.twin_plane(hi[pl.span(src)], seed2)
                    if 1e-10 <= base - _pair_values(W, seen_from, hi[pl.span(src)], lo)[1] <= 0.3 * delta2:
                        break
                else:
                    raise AssertionError("no twin remainder found")
                pl.copy(dst, src, twin=seed2)
            elif kind == "step":
                seen_from, other = hi[pl.span(key)], hi[pl.span(src)]
                e2o = _pair_values(W, seen_from, other)[1]
                noise = np.random.RandomState(1000 + 9000 + k).standard_normal(other.shape)
                eps = 1e-4
                for _ in range(4):                         # first order in eps
                    cand = (other.astype(np.float64) + eps * noise).astype(np.float32)
                    eps *= arg * delta / abs(_pair_values(W, seen_from, cand)[1] - e2o)
                pl.copy(dst, src, eps=eps, key=9000 + k)
            elif kind == "rev":
                seen_from, other = hi[pl.span(key)], hi[pl.span(src)]
                e1o, e2o = _pair_values(W, seen_from, other)
                found = False
                for key2 in range(5000 + 40 * k, 5120 + 40 * k):
                    noise = np.random.RandomState(1000 + key2).standard_normal(other.shape)
                    for eps in (2e-8, 5e-8, 1e-7, 2e-7, 5e-7, 1e-6):     # (first order: 0.1 eps; the fp32 spectra move e1 by 1e-9)
                        cand = (other.astype(np.float64) + eps * noise).astype(np.float32)
                        e1c, e2c = _pair_values(W, seen_from, cand)
                        if (e1c - e1o) * (e2c - e2o) < 0 and 1e-10 <= abs(e2c - e2o) <= 0.35 * delta2:
                            found = True
                            break
                    if found:
                        break
                assert found, "no reversed pair found"
                pl.copy(dst, src, eps=eps, key=key2)
            else:
                raise ValueError(kind)
        return [Clip(hi, pl.lo, W, frame_sample0, n_frames)]
    return make


def _join(*makers):
    """make() of a batch: one maker per clip (None: an idle clip)."""
    return lambda delta, delta2, attempt=0: [None if m is None else m(delta, delta2, attempt)[0] for m in makers]


def _place(sources, d, n_frames, taken, gaps=(0.25,), kind="near", direction=1, reach=None):
    """Planted near-copies of `sources`, each as far from its source as the window allows (direction +1: later frames, -1:
    earlier ones) and two frames clear of every other planted or source frame."""
    plants = []
    taken = set(taken) | set(sources)
    for n, src in enumerate(sources):
        for o in range(min(d, reach or d), 1, -1):
            dst = src + direction * o
            if 1 <= dst <= n_frames - 2 and all(abs(dst - u) >= 2 for u in taken):
                plants.append((dst, src, kind, gaps[n % len(gaps)]))
                taken.add(dst)
                break
    return plants, taken


def _cases():
    cases = []
    add = cases.append
    # ---- first pass and level 1, mode 0 (refine 0 against the fp32 matrix itself, refine 1 against the reference) ----------------
    # wave: the four d & 3 instantiations x three row lengths, the list lengths in turn; a near-copy of the row's own frame
    # at the edge of its window, 0.25 delta below it, in every (2 d + 7)th row; every other case a threshold inside the values
    numbers = (1, 3, 100, 130)
    k = 0
    for d in (4, 5, 6, 7):
        for T in (33, 200, 257):
            plants = [(r + d - 1, r, "near", 0.25) for r in range(3, T - d - 2, 2 * d + 7)][:12]
            silent = (150,) if (d, T) == (5, 200) else ()
            add(_spec("wave_d%d_T%d" % (d, T), n_cols=T, n_rows=T, d=d, number=numbers[k % 4], levels=(0, 1),
                      make=_clip(100 + k, T, plants=plants, silent=silent), expect="wave", planted=True,
                      threshold_quantile=0.55 if k % 2 else None))
            k += 1
    # wave + segment records: rows that end inside a 32-column segment
    for d in (31, 47, 63):
        for T in (96, 300, 700):
            n_rows = min(T, 40)
            plants, _ = _place(range(2, n_rows, 9), d, T, ())
            add(_spec("records_d%d_T%d" % (d, T), n_cols=T, n_rows=n_rows, d=d, number=100, levels=(0, 1),
                      make=_clip(200 + k, T, plants=plants), expect="wave+records", planted=True))
            k += 1
    # block: ceil(groups / 256) on each of 1, 2, 4, 8, 16, 32, the windows in turn. (d = 0 and 1 stop at 6 000 columns: without a
    # window every element is a candidate, and launch_by_size refuses a row whose candidate list does not fit the LDS beside it.)
    # d < 2 has no window to tie in: two near-copies of the row's frame 0.25 delta apart and a list of 2 put the tie on the cut.
    for T, d, qmax in ((300, 0, 1), (300, 200, 1), (1500, 1, 2), (1500, 64, 2), (3000, 3, 4), (3000, 0, 4), (6000, 64, 8), (6000, 1, 8),
                       (12000, 200, 16), (12000, 3, 16), (20000, 64, 32), (20000, 3, 32)):
        n_rows = 4 + (k % 5)
        if d < 2:
            plants = [(40 + 10 * r, r, "near", 0.25) for r in range(n_rows)] + [(T - 50 - 10 * r, r, "near", 0.5) for r in range(n_rows)]
        else:
            plants, _ = _place(range(n_rows - 1, -1, -1), d, T, (), reach=40)
        add(_spec("block_T%d_d%d" % (T, d), n_cols=T, n_rows=n_rows, d=d, number=2 if d < 2 else 100, levels=(0, 1),
                  make=_clip(300 + k, T, plants=plants), expect="block", qmax=qmax, planted=True))
        k += 1
    # block two-stage: rows of 9 000 columns in two segments of peak_segment_length(64) = 8 052 columns: candidates on both sides of
    # the border (row 3), and near-ties whose rival lies in the neighbouring segment (rows 2 and 4: one window across column 8 052):
    # a frame 0.04 below the row's own and a second one 0.25 delta beside THAT, so that the winner stays clear of every other kept value
    add(_spec("two_stage", n_cols=9000, n_rows=6, d=64, number=100, with_scratch=True, levels=(0, 1), expect="block two-stage", qmax=8,
              planted=True, make=_clip(400, 9000, plants=[(8040, 2, "far", 0.04), (8060, 8040, "step", 0.25, 2), (8000, 3, "far", 0.03),
                                                          (8120, 3, "far", 0.05), (8050, 4, "far", 0.04), (8054, 8050, "step", 0.25, 4),
                                                          (7900, 1, "far", 0.04), (7950, 7900, "step", 0.3, 1), (8200, 5, "far", 0.03)])))

    # ---- modes 1 and 2: the band (both layouts from the same values; absent cells NaN, then + 2.0) ------------------------------
    idle = 1 << 60
    for name, B, d, nb, shift, start, origin, row0, n_rows in (
            ("band_B40_d5", 40, 5, 1, 0, 0, None, 39, 30),
            ("band_B40_d2_start1", 40, 2, 1, 0, 1, None, 0, 60),
            ("band_B130_d31_start50", 130, 31, 1, 0, 50, None, 49, 110),
            ("band_B130_d70_batch", 130, 70, 3, 57, 40, [57, 82, idle], 96, 120),
            ("band_B431_d43_later", 431, 43, 1, 0, 0, None, 438, 24),
            ("band_B431_d2_batch", 431, 2, 3, 57, 200, [57, 117, idle], 256, 260),
            ("band_B40_d5_batch", 40, 5, 3, 57, 40, [57, 70, idle], 96, 30),
            ("band_B130_d5_origin", 130, 5, 1, 57, 1, [60], 60, 150)):
        n_frames = row0 - shift + n_rows
        makers = []
        for b in range(nb):
            if origin is not None and origin[b] == idle:
                makers.append(None)
                continue
            o_b = origin[b] if origin is not None else 0
            first = o_b - shift + 2
            reach = min(d, 12)

            def own_column(t):                      # the circular position of band row t's own frame in its row
                jl = t + shift - o_b
                return jl % min(B, jl + 1)
            # (a copy `reach` frames back sits in the row's window only if the columns do not wrap between the two)
            sources = [t for t in range(max(row0 - shift, first + d + 2), n_frames - 1) if own_column(t) >= reach][::d + 6][:10]
            plants, _ = _place(sources, d, n_frames, (), direction=-1, reach=reach)
            makers.append(_clip(500 + k + b, n_frames, plants=plants))
        add(_spec(name, mode=1, n_cols=B, n_rows=n_rows, row0=row0, d=d, number=100 if B < 431 else 3, shift=shift, start=start,
                  origin=origin, levels=(1,), make=_join(*makers), planted=True, expect="wave" if 4 <= d <= 63 else "block"))
        k += 1

    # ---- level 2 (refine 2): wave shapes take the fast path (records, unit_rows_f64_wg_kernel, the lite relaunch), block shapes
    # and flat rows the general kernel. The launch rows are frames 0 .. n_rows-1; the planted frames lie behind them. ----------
    def pairs(rows, n_rows, d, T, kind):
        """per row r: A = a copy of r with enough noise to sit 0.03 .. 0.1 below it (so that, seen from r, A and its partner
        differ at first order) and its partner -- in one window for even r (one of the two is a strict maximum), more than d
        apart for odd r (both are: with a list of 2 -- the row's own frame and one more -- the CUT falls between them)"""
        plants, lo_at, hi_at = [], n_rows + 2, T - 3
        for r in rows:
            a = lo_at
            a2 = a + 2 if r % 2 == 0 else hi_at
            if r % 2:
                hi_at -= 2
            lo_at += 4
            assert (a2 - a > d or r % 2 == 0) and lo_at < hi_at
            plants.append((a, r, "far", 0.03 + 0.009 * r))
            plants.append((a2, a, "twin", 10 * r, r) if kind == "twin" else (a2, a, "rev", 1 if r % 4 < 2 else -1, r))
        return plants

    for C in (1, 2, 3):
        add(_spec("twins_wave_C%d" % C, n_cols=120, n_rows=8, d=5 + C, C=C, number=2, levels=(2,), level2="lite",
                  make=_clip(600 + C, 120, C=C, plants=pairs(range(8), 8, 5 + C, 120, "twin")), expect="wave"))
    add(_spec("twins_block", n_cols=120, n_rows=8, d=3, C=2, number=2, levels=(2,), level2="general",
              make=_clip(610, 120, C=2, plants=pairs(range(8), 8, 3, 120, "twin")), expect="block"))
    for name, s0, with_lo in (("", 0, False), ("_lo", 0, True), ("_centred", -128, False)):
        add(_spec("reversed_wave" + name, n_cols=120, n_rows=8, d=6, number=2, levels=(2,), level2="lite", frame_sample0=s0,
                  make=_clip(620, 120, frame_sample0=s0, with_lo=with_lo, plants=pairs(range(1 if s0 else 0, 8), 8, 6, 120, "rev")), expect="wave"))
        add(_spec("reversed_block" + name, n_cols=120, n_rows=8, d=2, number=2, levels=(2,), level2="general", frame_sample0=s0,
                  make=_clip(630, 120, frame_sample0=s0, with_lo=with_lo, plants=pairs(range(1 if s0 else 0, 8), 8, 2, 120, "rev")), expect="block"))
    # a looped exact period: whole frame classes tie. Period above the window: every copy is kept, the ORDER of equal values
    # is open (the exact-tie rule) and nothing is near a tie inside a window, so no level has anything to decide; period inside the
    # window: no copy is a strict maximum.
    for name, s0 in (("", 0), ("_centred", -128)):
        add(_spec("loop_far" + name, n_cols=150, n_rows=150, d=5, number=100, levels=(2,), level2=None, frame_sample0=s0,
                  make=_clip(640, 150, period=10, frame_sample0=s0), expect="wave"))
        add(_spec("loop_flat" + name, n_cols=150, n_rows=150, d=6, number=100, levels=(2,), level2="lite", frame_sample0=s0,
                  make=_clip(641, 150, period=4, frame_sample0=s0), expect="wave"))
    add(_spec("loop_block", n_cols=120, n_rows=120, d=3, number=100, levels=(2,), level2="general", flat_rows=1,
              make=_clip(642, 120, period=2), expect="block"))
    # near-tie stress on row 0 (d = 6, 700 columns; 12 rows, so that the one row with exact ties among its kept values stays under
    # a tenth): exact copies of frame 0 in pairs 3 columns apart tie with each other -- 2 near-tied elements and 2 rival entries per pair
    def stress(n_pairs, n_triples):
        plants, at = [], 20
        for _ in range(n_pairs):
            plants += [(at, 0, "copy", 0), (at + 3, 0, "copy", 0)]
            at += 14
        for _ in range(n_triples):
            plants += [(at, 0, "copy", 0), (at + 2, 0, "copy", 0), (at + 4, 0, "copy", 0)]
            at += 14
        assert at < 698
        return plants
    add(_spec("stress_amb_cap", n_cols=700, n_rows=12, d=6, levels=(2,), level2="lite", make=_clip(650, 700, plants=stress(K_AMB_CAP // 2, 0)),
              expect="wave"))
    add(_spec("stress_amb_cap_plus_1", n_cols=700, n_rows=12, d=6, levels=(2,), level2="general", flat_rows=1,
              make=_clip(651, 700, plants=stress(K_AMB_CAP // 2 - 1, 1)), expect="wave"))
    add(_spec("stress_rival_cap", n_cols=700, n_rows=12, d=6, levels=(2,), level2="general", flat_rows=1,
              make=_clip(652, 700, plants=stress(0, K_RIVAL_CAP // 6 + 4)), expect="wave"))
    # more than kRivalCap level-2 items in a row the first pass could record (d = 4): 53 times an exact copy z of frame 0, then k and i
    # -- one class, 2 delta below it -- 4 and 8 columns on. z beats k by more than delta (k is no candidate), i ties with k exactly:
    # 53 near-tied elements with 53 unlisted rivals, 106 items for the second level -- the fast path hands the row on (counter [14])
    plants, at = [], 12
    for _ in range(53):
        plants += [(at, 0, "copy", 0), (at + 4, 0, "near", 2.0, 777), (at + 8, 0, "near", 2.0, 777)]
        at += 13
    add(_spec("stress_hand_on", n_cols=710, n_rows=12, d=4, levels=(2,), level2="general", hands_on=True,
              make=_clip(653, 710, plants=plants), expect="wave"))
    # a silent frame: its NaN row and column reach into the windows of the rows around it
    add(_spec("silent_level2", n_cols=120, n_rows=120, d=5, levels=(2,), level2=None, make=_clip(660, 120, silent=(60,), plants=[
        (57, 20, "close", 30.0), (63, 20, "close", 30.4), (80, 21, "close", 30.0), (83, 21, "close", 30.4)]), expect="wave"))
    # the two unit_rows_f64_wg_kernel variants and the two FFT plans of the exact kernel: W = 2048 and 4096, 60 frames
    for W in (2048, 4096):
        add(_spec("W%d_wave" % W, W=W, n_cols=60, n_rows=6, d=5, C=2, number=2, levels=(2,), level2="lite",
                  make=_clip(670, 60, W=W, C=2, plants=pairs(range(6), 6, 5, 60, "rev")), expect="wave"))
        add(_spec("W%d_block" % W, W=W, n_cols=60, n_rows=6, d=2, C=2, number=2, levels=(2,), level2="general",
                  make=_clip(671, 60, W=W, C=2, plants=pairs(range(6), 6, 2, 60, "rev")), expect="block"))
    # the band at level 2: a batch with origins (the fast path walks the diagonal / the look-back row through row_columns)
    # (the twins lie before the launch's first row: a twin seen from its own source is 1 - 1e-17, no comparison for anybody)
    makers = []
    for b, triples in enumerate((((39, 30, 27), (45, 22, 19), (51, 14, 16)), ((52, 44, 41), (56, 36, 33), (60, 28, 25)))):
        plants = []
        for n, (t, a, a2) in enumerate(triples):
            plants += [(a, t, "far", 0.03 + 0.01 * n), (a2, a, "twin", 10 * n, t)]
        makers.append(_clip(680 + b, 69, plants=plants))
    add(_spec("band_level2", mode=1, n_cols=40, n_rows=30, row0=96, d=5, shift=57, start=40, origin=[57, 70, idle], levels=(2,),
              level2="lite", make=_join(makers[0], makers[1], None), expect="wave"))
    return cases


CASES = {c.name: c for c in _cases()}


@functools.lru_cache(maxsize=None)
def built(name, delta, delta2):
    """The case `name` built with the launch's delta and delta2 (shared by the tests that run it)."""
    return build(CASES[name], delta, delta2)
