"""The arithmetic of the median-mask kernels (csrc/mask.hip, mask_bits.hip, rank.hip) in NumPy, and the inputs their stage tests
run on (tests/test_gpu_mask_stages.py; checked on the CPU by tests/test_mask_reference.py).

Which frames a cell's median is taken over is written from the rules of repet.py that the oracle restates, not from the kernels:
  period    position q of the period: the frames q, q + p, q + 2 p, ... below T (the segments that really hold s p + q)
  adaptive  frame t: the in-range taps t + (k + 1 - ceil(order / 2)) per[t], k = 0 .. order - 1
  sim       frame t: its list
The model is the kernels' own, in fp32 and bit for bit: a median is a selection, so it is exact; an even count gives
float32(0.5) * (a + b) with the sum rounded to fp32; an empty list gives NaN; in the period and adaptive families a NaN among the
gathered values gives NaN (np.median's rule). The mask the model implies is computed in float64: (min(v, m) + eps) / (v + eps)
with eps = kMaskEps = 2^-52, exactly 1 where m >= v, exactly 1 in bins 1 .. cutoff, NaN for a NaN model."""
import numpy as np

EPS = np.float32(2.220446049250313e-16)          # kMaskEps (common.h) = np.finfo(float).eps, exact in fp32
U = 2.0 ** -24
MASK_BAR = 3 * 2.0 ** -23                       # soft_mask: two additions and a product at 2^-24 each + a 1-ulp (2^-23) reciprocal
NET_SIZES = (2, 4, 8, 10, 12, 16, 24, 32, 48, 64, 80, 100, 128)        # dispatch_net (mask.hip); longer lists: bisection (0)


def net_for(n):
    return next((s for s in NET_SIZES if n <= s), 0)


# ---- which frames ------------------------------------------------------------------------------------------------------
def period_frames(t, period, q):
    return np.arange(q, t, period)


def adaptive_frames(t, i, per, order):
    taps = np.arange(1, order + 1) - int(np.ceil(order / 2))
    j = i + taps * int(per)
    return j[(j >= 0) & (j < t)]


# ---- the model, fp32 ---------------------------------------------------------------------------------------------------
def median32(values, nan_rule):
    """Median over axis 0 of values (n, F) fp32, as the kernels compute it."""
    values = np.asarray(values, dtype=np.float32)
    n, f = values.shape
    if n == 0:
        return np.full(f, np.nan, dtype=np.float32)
    s = np.sort(values, axis=0)                  # (NaN sorts last)
    with np.errstate(invalid="ignore", over="ignore"):
        med = s[(n - 1) // 2] if n & 1 else np.float32(0.5) * (s[n // 2 - 1] + s[n // 2]).astype(np.float32)
    med = med.astype(np.float32)
    if nan_rule:
        med = np.where(np.isnan(values).any(axis=0), np.float32(np.nan), med)
    return med


def model_period(v, period):
    """v (T, F) -> the repeating segment (period, F): row q is the median over the frames that hold position q."""
    t = v.shape[0]
    return np.stack([median32(v[period_frames(t, period, q)], True) for q in range(period)])


def model_adaptive(v, per, order):
    t = v.shape[0]
    return np.stack([median32(v[adaptive_frames(t, i, per[i], order)], True) for i in range(t)])


def model_sim(v, lists):
    """lists[r]: the frames of list row r; returns (len(lists), F)."""
    return np.stack([median32(v[np.asarray(ix, dtype=np.int64)], False) for ix in lists])


# ---- the mask, float64 -------------------------------------------------------------------------------------------------
def mask_of(v, model, cutoff=0):
    """v, model (T, F) fp32 -> (mask float64, exactly_one bool): the mask is exactly 1 where the model is not below the magnitude
    and in bins 1 .. cutoff; NaN where the model is NaN (outside those bins)."""
    v64, m64 = np.asarray(v, dtype=np.float64), np.asarray(model, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = (np.minimum(v64, m64) + float(EPS)) / (v64 + float(EPS))
        one = m64 >= v64
    m = np.where(one, 1.0, m)
    m = np.where(np.isnan(m64), np.nan, m)
    hi = min(int(cutoff), v.shape[1] - 1)
    if hi >= 1:
        m[:, 1:hi + 1] = 1.0
        one = one.copy()
        one[:, 1:hi + 1] = True
    return m, one


def mask_period(v, period, cutoff=0):
    model = model_period(v, period)
    return model, mask_of(v, model[np.arange(v.shape[0]) % period], cutoff)


# ---- inputs ------------------------------------------------------------------------------------------------------------
ZERO_BIN, CONST_BIN, TIE_BIN = 2, 3, 5             # bins with exact zeros, one value in every frame, few distinct values


def magnitudes(shape, seed):
    """(..., T, F) fp32, every value exact in fp32: bin f sits at the level 2^e(f), e spread over -40 .. 40 and shuffled, and frame
    t of a bin holds level * 2^(0..2) * (1 + j / 4096) with j different for every frame of the bin (T <= 4096): two values that can
    meet in one median differ by at least 2^-13 relative. Bin 2 is exactly zero in every third frame, bin 3 holds one value, bin 5
    only five different ones (exact ties)."""
    *lead, t, f = shape
    assert t <= 4096
    rs = np.random.RandomState(seed)
    n = int(np.prod(lead)) if lead else 1
    out = np.empty((n, t, f), dtype=np.float64)
    expo = np.round(np.linspace(-40, 40, f)).astype(np.int64) if f > 1 else np.array([0])
    for k in range(n):
        j = np.argsort(rs.rand(t, f), axis=0) * (4096 // t if t <= 4096 else 1)        # a permutation of distinct steps per bin
        level = np.exp2(rs.permutation(expo))[None, :]
        out[k] = level * np.exp2(rs.randint(0, 3, size=(t, f))) * (1.0 + j / 4096.0)
        if f > ZERO_BIN:
            out[k, rs.permutation(t)[: (t + 2) // 3], ZERO_BIN] = 0.0
        if f > CONST_BIN:
            out[k, :, CONST_BIN] = level[0, CONST_BIN] * 1.25
        if f > TIE_BIN:
            out[k, :, TIE_BIN] = level[0, TIE_BIN] * (1.0 + rs.randint(0, 5, size=t) / 8.0)
    v = out.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), out)
    return v.reshape(*lead, t, f)


def spectra(shape, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(*shape) + 1j * rs.randn(*shape)).astype(np.complex64)


def sim_lists(n_rows, t, max_count, seed, first_frame=0, width=None):
    """idx (n_rows, width), cnt (n_rows): list row r belongs to frame first_frame + r. The lengths run through every value 0 ..
    max_count (n_rows > max_count) with neighbours of different length, the entries are distinct frames drawn anew for every row,
    more than half of the rows leave their own frame out, and the entries past a list's end are valid frames that are not in it."""
    width = max_count if width is None else width
    assert n_rows > max_count and t >= max_count and width >= max_count
    rs = np.random.RandomState(seed)
    lengths = [int(n) for n in rs.permutation(max_count + 1)]
    while len(lengths) < n_rows:                  # (the rows beyond the first run of all lengths: no more empty lists)
        n = int(rs.randint(1, max_count + 1))
        if n != lengths[-1]:
            lengths.append(n)
    cnt = np.array(lengths[:n_rows], dtype=np.int32)
    idx = np.empty((n_rows, width), dtype=np.int32)
    own_in = np.zeros(n_rows, dtype=bool)
    for r in range(n_rows):
        own = first_frame + r
        order = rs.permutation(t)
        n = int(cnt[r])
        if n and rs.rand() < 0.4 and own < t:
            order = np.concatenate(([own], order[order != own]))
            own_in[r] = True
            order[:n] = rs.permutation(order[:n])
        else:
            order = order[order != own] if t > max_count else order
            own_in[r] = own in order[:n]
        idx[r] = np.resize(order, width)
    return idx, cnt, own_in


def raise_absent(v, own_in, first_frame=0):
    """Frames that are not in their own list get four times their magnitude (still exact, still distinct from the bin's others)."""
    v = v.copy()
    for r in np.flatnonzero(~own_in):
        if first_frame + r < v.shape[-2]:
            v[..., first_frame + r, :] *= np.float32(4.0)
    return v


def lists_of(idx, cnt):
    return [idx[r, :cnt[r]] for r in range(len(cnt))]


def input_conditions(cnt, max_count, mask, compared):
    """The two conditions every case is held to: every list length 0 .. max_count occurs, and at least a quarter of the compared
    cells have a reference mask below 1."""
    if cnt is not None:
        assert set(range(max_count + 1)) <= set(int(n) for n in np.ravel(cnt)), "a list length is missing"
    m = np.asarray(mask)[compared]
    with np.errstate(invalid="ignore"):
        share = np.count_nonzero(m < 1.0) / max(m.size, 1)
    assert share >= 0.25, "only %.3f of the compared cells have a mask below 1" % share
    return share


# ---- the cases both test modules walk through ----------------------------------------------------------------------------
PERIOD_FILL_T = (3, 4, 9, 17, 21, 25, 33, 49, 64)                   # host period 2, F = 65: n on both sides of every network size
PERIOD_SWITCH = [(2, t) for t in (17, 33, 65, 129, 201, 257, 261)] + [(5, 40), (13, 40)]      # (device period, T), min_period 1
ADAPTIVE_ORDERS = tuple(range(1, 14)) + (16, 17, 24, 25, 32, 33, 100, 129)
SIM_COUNTS = (2, 4, 8, 10, 12, 16, 24, 32, 48, 64, 80, 100, 128, 150)
SIM_FLOAT_F = (40, 100, 65, 129, 193)


def sim_frames(max_count):
    """T of a `sim` case: just above the longest list, and enough rows for the quarter condition when the lists are short."""
    return max(max_count + 3, 33)


def adaptive_periods(t, seed):
    """Periods (T,) holding 1, T - 1, T and more than T, small ones whose taps fall off either end or both, and random ones."""
    rs = np.random.RandomState(seed)
    per = rs.randint(1, max(t // 4, 2), size=t).astype(np.int32)
    per[::7] = 1
    per[3::11] = t - 1
    per[5::13] = t
    per[6::17] = t + 9
    per[t // 2] = 1
    per[0], per[t - 1] = 2, 3
    return per


def build_sim(b, c, t, f, max_count, seed, first_frame=0, width=None):
    """V (B, C, T, F), idx (B, T - first_frame, width), cnt (B, T - first_frame): every clip its own lists, the frames absent from
    their own list raised."""
    n_rows = t - first_frame
    V = magnitudes((b, c, t, f), seed)
    idx, cnt = [], []
    for clip in range(b):
        ix, n, own_in = sim_lists(n_rows, t, max_count, seed + 101 * clip + 1, first_frame, width)
        V[clip] = raise_absent(V[clip], own_in, first_frame)
        idx.append(ix)
        cnt.append(n)
    return V, np.stack(idx), np.stack(cnt)


def reference_sim(v, idx, cnt, first_frame=0, cutoff=0):
    """One channel v (T, F) and one clip's lists -> (mask float64 (T, F), exactly_one, model fp32); the rows before first_frame
    have no list: NaN in all three."""
    t, f = v.shape
    model = np.full((t, f), np.nan, dtype=np.float32)
    n_rows = min(len(cnt), t - first_frame)
    model[first_frame:first_frame + n_rows] = model_sim(v, lists_of(idx[:n_rows], cnt[:n_rows]))
    m, one = mask_of(v, model, cutoff)
    m[:first_frame] = np.nan
    one[:first_frame] = False
    return m, one, model
