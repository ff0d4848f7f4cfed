"""What a 16-bit destination of an emission holds: ``round_ref(v, dtype)`` of the float64 values ``v`` the engine forms.

A destination dtype is a cast of that float64 value, never a rescale, rounded ONCE:

* ``"float16"``: the nearest binary16, ties to even -- ``astype(np.float16)``, which NumPy rounds from float64 in one step.
* ``"bfloat16"``: the nearest bfloat16, ties to even, chosen between the two bfloat16 values either side of ``|v|`` by their
  float64 distances to it. Both neighbours are float64 values and both differences are exact (the neighbours lie within a
  factor of two of ``v`` and on its grid), so nothing here rounds but the choice itself. No float32 step, no torch conversion:
  ``torch.Tensor.to(torch.bfloat16)`` of a float64 tensor rounds twice.
* ``"int16"``: ``rint`` (ties to even), saturated to [-32768, 32767]; NaN is 0.

Beyond the largest finite value the floats become +-inf, subnormals are produced, NaN stays NaN, the sign of zero is kept.
``round_ref`` returns float16, uint16 (the bfloat16 bit patterns: NumPy has no such dtype) or int16; ``bits`` views any of them
as uint16, ``decode`` returns the float64 values they stand for."""
import numpy as np

DTYPES = ("int16", "float16", "bfloat16")

_BF16_FRACTION = 7
_DROP = 52 - _BF16_FRACTION                                        # fraction bits of a float64 that a bfloat16 does not have
_BF16_MIN_NORMAL = 2.0 ** -126
_BF16_QUANTUM = 2.0 ** -133                                        # the spacing of the subnormal bfloat16 values
_BF16_OVERFLOW = 2.0 ** 128


def _bf16_neighbours(a):
    """For float64 ``a`` >= 0 (finite): the bfloat16 values lo <= a < hi either side, as float64 (hi may be 2**128), and whether
    lo's last fraction bit is even."""
    u = a.view(np.uint64)
    lo_n = (u & ~np.uint64((1 << _DROP) - 1))
    hi_n = lo_n + np.uint64(1 << _DROP)                            # (the carry runs into the exponent: the next binade)
    even_n = (lo_n >> np.uint64(_DROP)) & np.uint64(1) == 0
    sub = a < _BF16_MIN_NORMAL
    k = np.floor(np.where(sub, a, 0.0) / _BF16_QUANTUM)            # (a power of two: the division is exact)
    lo = np.where(sub, k * _BF16_QUANTUM, lo_n.view(np.float64))
    hi = np.where(sub, (k + 1) * _BF16_QUANTUM, hi_n.view(np.float64))
    even = np.where(sub, k % 2 == 0, even_n)
    return lo, hi, even


def _bf16_values(v):
    """The float64 value of the bfloat16 nearest to each float64 ``v`` (ties to even, +-inf on overflow; NaN stays NaN)."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    a = np.abs(v)
    finite = np.isfinite(a)
    lo, hi, even = _bf16_neighbours(np.where(finite, a, 0.0))
    with np.errstate(invalid="ignore"):
        below, above = a - lo, hi - a                              # exact (inf and NaN are put back below)
    r = np.where((below < above) | ((below == above) & even), lo, hi)
    r = np.where(r >= _BF16_OVERFLOW, np.inf, r)
    r = np.where(finite, r, a)                                     # inf and NaN as they are
    return np.copysign(r, v)


def round_ref(v, dtype):
    v = np.ascontiguousarray(v, dtype=np.float64)
    if dtype == "float16":
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            return v.astype(np.float16)
    if dtype == "bfloat16":
        r = _bf16_values(v)
        with np.errstate(invalid="ignore"):
            f = r.astype(np.float32)
        assert np.array_equal(f.astype(np.float64), r, equal_nan=True)         # a bfloat16 value is a float32 value: exact
        b = f.view(np.uint32)
        assert not np.any((b & np.uint32(0xFFFF))[~np.isnan(f)])
        return (b >> np.uint32(16)).astype(np.uint16)
    if dtype == "int16":
        with np.errstate(invalid="ignore"):
            r = np.clip(np.rint(v), -32768.0, 32767.0)
        return np.where(np.isnan(v), 0.0, r).astype(np.int16)
    raise ValueError(dtype)


def bits(a):
    """A 16-bit array as uint16 bit patterns."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 2, a.dtype
    return a.view(np.uint16)


def decode(b, dtype):
    """The float64 values of 16-bit patterns ``b`` (uint16) of ``dtype``."""
    b = np.ascontiguousarray(b).view(np.uint16)
    if dtype == "float16":
        return b.view(np.float16).astype(np.float64)
    if dtype == "bfloat16":
        return (b.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    if dtype == "int16":
        return b.view(np.int16).astype(np.float64)
    raise ValueError(dtype)


def same_bits(got, want, dtype):
    """True where the patterns agree; for the float formats every quiet NaN pattern counts as NaN."""
    got, want = bits(got), bits(want)
    ok = got == want
    if dtype in ("float16", "bfloat16"):
        fraction = 10 if dtype == "float16" else 7
        quiet = lambda p: ((p & 0x7FFF) >> fraction == (1 << (15 - fraction)) - 1) & ((p >> (fraction - 1)) & 1 == 1)
        ok |= quiet(got) & quiet(want)
    return ok


# The values at which a conversion can go wrong, with the value each must become (float64; None: NaN).
TRAPS = {
    "float16": [
        (1 + 2.0 ** -11, 1.0), (1 + 3 * 2.0 ** -11, 1 + 2.0 ** -9),
        (1 + 2.0 ** -11 + 2.0 ** -40, 1 + 2.0 ** -10),             # through float32 this is rounded twice: 1.0
        (65504.0, 65504.0), (65519.99, 65504.0), (65520.0, np.inf), (-65520.0, -np.inf),
        (2.0 ** -24, 2.0 ** -24), (2.0 ** -25, 0.0), (2.0 ** -25 + 2.0 ** -60, 2.0 ** -24), (-(2.0 ** -25), -0.0),
        (-0.0, -0.0), (0.0, 0.0), (np.nan, None), (np.inf, np.inf), (-np.inf, -np.inf),
        (3 * 2.0 ** -25, 2.0 ** -23), (2.0 ** -14 - 2.0 ** -26, 2.0 ** -14), (1e300, np.inf), (5e-324, 0.0),
    ],
    "bfloat16": [
        (1 + 2.0 ** -8, 1.0), (1 + 2.0 ** -8 + 2.0 ** -40, 1 + 2.0 ** -7), (1 + 3 * 2.0 ** -8, 1 + 2.0 ** -6),
        ((2 - 2.0 ** -7) * 2.0 ** 127, (2 - 2.0 ** -7) * 2.0 ** 127),           # the largest finite bfloat16
        ((2 - 2.0 ** -8) * 2.0 ** 127, np.inf), (-(2 - 2.0 ** -8) * 2.0 ** 127, -np.inf),   # halfway above it
        ((2 - 2.0 ** -8) * 2.0 ** 127 * (1 - 2.0 ** -50), (2 - 2.0 ** -7) * 2.0 ** 127),
        (-0.0, -0.0), (0.0, 0.0), (np.nan, None), (np.inf, np.inf), (-np.inf, -np.inf),
        (2.0 ** -133, 2.0 ** -133), (2.0 ** -134, 0.0), (2.0 ** -134 + 2.0 ** -140, 2.0 ** -133), (3 * 2.0 ** -134, 2.0 ** -132),
        (1e300, np.inf), (5e-324, 0.0),
    ],
    "int16": [
        (2.5, 2.0), (3.5, 4.0), (-2.5, -2.0), (2.5 + 2.0 ** -40, 3.0), (32767.4, 32767.0), (32767.5, 32767.0),
        (-32768.5, -32768.0), (1e9, 32767.0), (-1e9, -32768.0), (np.nan, 0.0), (np.inf, 32767.0), (-np.inf, -32768.0),
        (0.5, 0.0), (-0.5, 0.0), (1.5, 2.0), (-0.0, 0.0), (1e300, 32767.0),
    ],
}


# the trailing entries of each list that go beyond the table every implementation must pass: a test that cannot deliver them to
# the conversion untouched (the engine holds a sample as fp32 + fp32) checks them against round_ref of what it did deliver
TRAPS_BEYOND = {"float16": 4, "bfloat16": 6, "int16": 5}


def trap_inputs(dtype):
    return np.array([v for v, _ in TRAPS[dtype]], dtype=np.float64)


def trap_bits(dtype):
    """The patterns the trap table must become, written down by hand (not by round_ref): from the expected float64 values,
    each of which the format holds exactly."""
    want = np.array([np.nan if w is None else w for _, w in TRAPS[dtype]], dtype=np.float64)
    if dtype == "float16":
        return bits(want.astype(np.float16))
    if dtype == "bfloat16":
        with np.errstate(invalid="ignore"):
            return (want.astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    return bits(want.astype(np.int16))
