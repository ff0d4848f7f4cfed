"""``emit_dtypes_reference.round_ref`` against exact rational arithmetic: the reference the GPU tests of the 16-bit destinations
compare with must itself round once, to nearest, ties to even. ``fractions.Fraction`` holds every float64 exactly, so the
nearest value of a format is found without any rounding of our own."""
import math
from fractions import Fraction

import numpy as np
import pytest

from emit_dtypes_reference import DTYPES, TRAPS, decode, round_ref, same_bits, trap_bits, trap_inputs

# (exponent bits, fraction bits) of the two float formats
FORMATS = {"float16": (5, 10), "bfloat16": (8, 7)}


def exact_float(v, dtype):
    """The value of the format nearest to the float64 ``v`` (ties to even), by rational arithmetic: a float, +-inf, or NaN."""
    if math.isnan(v) or math.isinf(v):
        return v
    e_bits, m_bits = FORMATS[dtype]
    bias = (1 << (e_bits - 1)) - 1
    e_min, e_max = 1 - bias, bias
    a = abs(Fraction(v))
    if a == 0:
        return v
    e = max(math.frexp(abs(v))[1] - 1, e_min) if abs(v) >= 5e-324 else e_min       # floor(log2 |v|), not below the smallest normal's
    quantum = Fraction(2) ** (e - m_bits)
    r = round(a / quantum) * quantum                                               # (round of a Fraction: half to even)
    out = math.inf if r >= Fraction(2) ** (e_max + 1) else float(r)
    return math.copysign(out, v)


def exact_int16(v):
    if math.isnan(v):
        return 0
    if math.isinf(v):
        return 32767 if v > 0 else -32768
    return min(max(round(Fraction(v)), -32768), 32767)


def exact(v, dtype):
    return float(exact_int16(v)) if dtype == "int16" else exact_float(v, dtype)


def agree(g, w, dtype):
    """Two float64 values a format holds are the same value of it: equal, with the sign of zero where the format has one."""
    if math.isnan(w):
        return math.isnan(g)
    return g == w and (dtype == "int16" or math.copysign(1.0, g) == math.copysign(1.0, w))


def check(values, dtype):
    got = decode(round_ref(values, dtype), dtype)
    for v, g in zip(values.tolist(), got.tolist()):
        assert agree(g, exact(v, dtype), dtype), (dtype, v, g, exact(v, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_trap_table(dtype):
    values = trap_inputs(dtype)
    check(values, dtype)
    # the table's own expected values, written by hand, say the same
    assert same_bits(round_ref(values, dtype), trap_bits(dtype), dtype).all()
    for (v, w), g in zip(TRAPS[dtype], decode(round_ref(values, dtype), dtype).tolist()):
        assert agree(g, math.nan if w is None else w, dtype), (v, w, g)


def test_the_double_rounding_trap_is_a_trap():
    """Through float32 the two marked table entries come out differently: the table tells one rounding from two."""
    v = np.array([1 + 2.0 ** -11 + 2.0 ** -40])
    assert v.astype(np.float32).astype(np.float16)[0] == 1.0 and round_ref(v, "float16")[0] == np.float16(1 + 2.0 ** -10)
    v = np.array([1 + 2.0 ** -8 + 2.0 ** -40])
    twice = v.astype(np.float32).view(np.uint32)
    twice = (twice + 0x7FFF + ((twice >> 16) & 1)) >> 16                        # float32 -> bfloat16, ties to even
    assert decode(twice.astype(np.uint16), "bfloat16")[0] == 1.0 and decode(round_ref(v, "bfloat16"), "bfloat16")[0] == 1 + 2.0 ** -7


def ranges(rng, n):
    """Five ranges of random float64 values, both signs."""
    sign = lambda: rng.choice([-1.0, 1.0], n)
    yield "normal", sign() * np.exp2(rng.uniform(-14, 15, n))
    yield "f16-subnormal", sign() * np.exp2(rng.uniform(-27, -13, n))
    yield "near the f16 overflow", sign() * rng.uniform(65000, 66000, n)
    top = (2 - 2.0 ** -7) * 2.0 ** 127
    yield "near the bf16 overflow", sign() * top * rng.uniform(1 - 2.0 ** -6, 1 + 2.0 ** -6, n)
    half = rng.integers(-33000, 33000, n) + rng.choice([0.0, 0.5, 0.25, 0.5 + 2.0 ** -30, 0.5 - 2.0 ** -30], n)
    yield "int16 range with half-integers", half


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_values_in_five_ranges(dtype):
    rng = np.random.default_rng(20240607)
    for name, values in ranges(rng, 10_000):
        # on the formats' own ties as well: a quarter of the values cut to a multiple of half a bfloat16 place (fraction bits
        # below the 8th cleared), another quarter to half a binary16 place (below the 11th)
        snapped = values.copy()
        u = snapped.view(np.uint64)
        u[::4] &= ~np.uint64((1 << 44) - 1)
        u[1::4] &= ~np.uint64((1 << 41) - 1)
        check(snapped, dtype)
