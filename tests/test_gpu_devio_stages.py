"""The kernels of csrc/devio.hip launch by launch: the strided ingest, the egress, the emission with its gain fade, the level
reduction, ``devio_tail_clear`` and every per-push data movement of the live handle, each through its production launcher
(repet._devio_stage -> repet_debug_devio_stage) on buffers this module owns, against tests/devio_reference.py -- plain NumPy and
exact rational arithmetic, checked on the CPU by tests/test_devio_reference.py, which also builds every case below and asserts
its premises.

How a case runs. Every buffer a launcher is given is an "arena": the entry uploads it into an allocation of its own, its first
byte at an offset from a 256-byte boundary that the case chooses (so the case, not the allocator, decides which vector paths are
legal), with the byte 0xA5 everywhere else, and returns it whole with 512 bytes of that prefill on either side. A case states
the content of every arena after the launch; destinations start as prefill, so a store outside what the reference writes --
in a guard, in the gap between a strided destination's rows, behind a ring's length, in an idle or held slot's share, at or
behind a run's length -- shows as a changed cell.

Bars (none fitted; the issue of this module sets them):
  bits       every comparison is on the bit patterns; for the float formats any quiet NaN counts as NaN.
  energies   the three level energies alone use levels_reference.check (4 n 2^-53 relative, derived there); peaks and counts are
             identical.
  decisions  what the launcher reports (dense per destination, src_vec / dst_vec / held_vec per part, the grid, the number of
             launches) equals what the case predicts from its own addresses and strides, and the last test fails unless every
             decision REQUIRED lists was seen.
Counts. Where the issue gives counts without a shape (ingest: 1 .. 1027, one workgroup is 1024 elements), they are samples per
clip: two clips for the counts up to 5 (so a run of four crosses a clip), one clip above, so C = 1 puts 1023 / 1024 / 1025 / 1027
elements on either side of the workgroup and C = 2, 3 put other residues there.
Out of reach here: the 64-bit division branch of the ragged ingest and of emit_body (planes above 2^32 elements need tens of
gigabytes) and the 65535 cap of grid y (as many streams).
The worst error / bar per (kernel, check) and the decisions seen are collected; the last test writes them to
$REPET_DEVIO_STAGE_PARITY_OUT: profiles/devio_stage_parity.txt is that output from an MI355X."""
import os

import numpy as np
import pytest

import repet
import devio_reference as ref
import emit_dtypes_reference as edr
import levels_reference as lr

pytestmark = pytest.mark.gpu

PREFILL = 0xA5
GUARD = repet.DEVIO_GUARD
IDLE, HELD = ref.IDLE, ref.HELD
NULL = [-1, 0]
DTYPES = ("float64", "float32", "int16", "float16", "bfloat16")
FLOAT_DTYPES = ("float64", "float32", "float16", "bfloat16")
PARITY = {}          # (kernel, check) -> (worst error / bar, cases)
DECISIONS = set()    # (op, what, value) as the launchers reported them


def prefilled(n, dtype):
    dtype = np.dtype(dtype)
    return np.frombuffer(bytes([PREFILL]) * (int(n) * dtype.itemsize), dtype=dtype).copy()


def ceil_div(a, b):
    return -(-a // b)


def fmt_of(a):
    return {"float32": "float32", "float64": "float64", "float16": "float16", "complex64": "float32"}.get(a.dtype.name, "bits")


_QUIET = {"float16": (np.uint16, 0x7E00), "bfloat16": (np.uint16, 0x7FC0), "float32": (np.uint32, 0x7FC00000), "float64": (np.uint64, 0x7FF8000000000000)}


def mismatches(got, want, fmt):
    """Indices where the bit patterns differ; for a float format two quiet NaNs agree."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.nbytes == want.nbytes, (got.nbytes, want.nbytes)
    if fmt in _QUIET:
        u, q = _QUIET[fmt]
        g, w = got.view(u).ravel(), want.view(u).ravel()
        ok = (g == w) | ((g & u(q) == u(q)) & (w & u(q) == u(q)))
    else:
        ok = got.view(np.uint8).ravel() == want.view(np.uint8).ravel()
    return np.flatnonzero(~ok)


class Case:
    """One launch: ``arenas`` before it, ``want[k]`` the content of arena k after it (not named: unchanged), ``expect`` the
    fields of the launcher's report the case predicts, ``formats[k]`` where an arena's float format is not its NumPy dtype's
    (bfloat16 in uint16), ``free`` the arenas whose content no reference states (scratch: only their guards are checked)."""

    def __init__(self, kernel, label, op, arenas, words, floats=(), shifts=None, want=None, expect=None, formats=None, free=()):
        self.kernel, self.label, self.op, self.arenas, self.words, self.floats = kernel, label, op, arenas, words, list(floats)
        self.shifts = [0] * len(arenas) if shifts is None else list(shifts)
        self.want, self.expect, self.formats, self.free = want or {}, expect or {}, formats or {}, set(free)
        for k, w in self.want.items():
            w = np.ascontiguousarray(w)
            assert w.nbytes == self.arenas[k].nbytes, (label, k, w.nbytes, self.arenas[k].nbytes)

    def __repr__(self):
        return self.label


def note(kernel, check, ratio=0.0):
    worst, count = PARITY.get((kernel, check), (0.0, 0))
    PARITY[(kernel, check)] = (max(worst, float(ratio)), count + 1)


def run_case(case):
    outs, report = repet._devio_stage(case.op, case.arenas, case.words, case.floats, case.shifts, PREFILL)
    gots = []
    for k, (o, a) in enumerate(zip(outs, case.arenas)):
        assert np.all(o[:GUARD] == PREFILL), "%s: the guard in front of arena %d was written" % (case.label, k)
        assert np.all(o[len(o) - GUARD:] == PREFILL), "%s: the guard behind arena %d was written" % (case.label, k)
        got = o[GUARD:len(o) - GUARD].view(a.dtype) if a.nbytes else a.copy()
        gots.append(got)
        if k in case.free:
            continue
        want = np.ascontiguousarray(case.want.get(k, a))
        fmt = case.formats.get(k, fmt_of(a))
        bad = mismatches(got, want, fmt)
        if len(bad):
            unit = _QUIET[fmt][0] if fmt in _QUIET else np.uint8
            first = int(bad[0]) * np.dtype(unit).itemsize
            i = first // a.dtype.itemsize
            raise AssertionError("%s: arena %d differs in %d places, the first in element %d (byte %d): got %r want %r%s" % (
                case.label, k, len(bad), i, first, got.ravel()[i], want.view(a.dtype).ravel()[i],
                "" if k in case.want else " (an arena the launch must leave alone)"))
    for field, value in case.expect.items():
        assert report[field] == value, "%s: the launcher reports %s = %r, the case predicts %r" % (case.label, field, report[field], value)
    for field in ("dense", "src_vec", "dst_vec", "held_vec"):
        for v in report[field]:
            if v >= 0:
                DECISIONS.add((case.op, field, v))
    for s, d in zip(report["src_vec"], report["dst_vec"]):
        if s >= 0:
            DECISIONS.add((case.op, "src_vec,dst_vec", (s, d)))
    DECISIONS.add((case.op, "launches", report["launches"]))
    note(case.kernel, "bits and untouched cells")
    return gots, report


# ---- inputs -------------------------------------------------------------------------------------------------------------
def samples(rng, shape, dtype):
    """Finite stored samples of ``dtype`` (bfloat16: uint16 patterns): wide in exponent, with what each type can get wrong --
    float64 values that need their remainder and one beyond float32's normal range downwards, the ends of int16, subnormal
    binary16."""
    n = int(np.prod(shape))
    v = rng.standard_normal(n) * 10.0 ** rng.uniform(-5, 5, n)
    if dtype == "float64":
        v[::7] = 1e-42                                            # a float32 subnormal with a remainder
        out = v
    elif dtype == "float32":
        out = v.astype(np.float32)
        out[::7] = np.float32(1e-42)
    elif dtype == "int16":
        out = rng.integers(-32768, 32768, n).astype(np.int16)
        out[:2] = (-32768, 32767)[:min(2, n)]
    elif dtype == "float16":
        with np.errstate(over="ignore"):
            out = (rng.standard_normal(n) * 10.0 ** rng.uniform(-7, 4, n)).astype(np.float16)
        out[::7] = np.float16(6e-8)
        out[~np.isfinite(out)] = np.float16(65504)
    else:
        out = (v.astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    return out.reshape(shape)


def not_a_number(dtype):
    return {"float64": np.float64(np.nan), "float32": np.float32(np.nan), "float16": np.float16(np.nan), "bfloat16": np.uint16(0x7FC0)}[dtype]


def special(dtype, name):
    v = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf}[name]
    if dtype == "bfloat16":
        return np.uint16(np.float32(v).view(np.uint32) >> np.uint32(16))
    return ref.STORAGE[dtype](v)


def fp32_signal(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale * 2.0 ** rng.integers(-3, 4, shape)).astype(np.float32)


LAYOUTS = ("dense", "dense_off1", "channels_first", "padded")


def layout(kind, B, n, C):
    """(element strides, elements of storage, element offset of the base) of a (B, n, C) source or destination."""
    if kind == "dense":
        return (n * C, C, 1), B * n * C, 0
    if kind == "dense_off1":
        return (n * C, C, 1), B * n * C + 1, 1
    if kind == "channels_first":
        return (C * n, 1, n), B * n * C, 0
    assert kind == "padded"
    st = (n * (C + 2) + 3, C + 2, 1)
    return st, ref.strided_span((B, n, C), st), 0


def predict_dense(shape, strides, addr, vec_bytes):
    """The dense layout itself (a dimension of one element has no stride to speak of) on a base aligned for the vector access."""
    B, n, C = shape
    return int(addr % vec_bytes == 0 and (C == 1 or strides[2] == 1) and (n == 1 or strides[1] == C) and (B == 1 or strides[0] == n * C))


def predict_vec(addr, block, stream):
    """One side of a part takes 16-byte accesses: a 16-byte base, every stride a multiple of four floats."""
    return int(addr % 16 == 0 and block % 4 == 0 and stream % 4 == 0)


def stored(values, shape, strides, elems, base, dtype):
    out = prefilled(elems, ref.STORAGE[dtype])
    out[ref.strided_index(shape, strides, base).ravel()] = np.asarray(values).ravel()
    return out


# ---- A. ingest ----------------------------------------------------------------------------------------------------------
INGEST_COUNTS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 1027)


def ingest_case(dtype, kind, B, n, C, seed, lengths=None, poke=None, shift=0, label=""):
    rng = np.random.default_rng(seed)
    x = samples(rng, (B, n, C), dtype)
    if lengths is not None and dtype != "int16":
        for b in range(B):
            x[b, lengths[b]:] = not_a_number(dtype)               # what lies behind a length is never looked at
    for at, value in (poke or []):
        x[at] = value
    strides, elems, base = layout(kind, B, n, C)
    size = np.dtype(ref.STORAGE[dtype]).itemsize
    count = B * n * C
    arenas = [stored(x, (B, n, C), strides, elems, base, dtype), prefilled(count, np.float32), prefilled(count, np.float32),
              np.zeros(1, dtype=np.uint32)]
    len_ref = NULL
    if lengths is not None:
        arenas.append(np.asarray(lengths, dtype=np.int64))
        len_ref = [4, 0]
    hi, lo, flag = ref.ingest(x, dtype, lengths)
    want = {1: hi.ravel(), 3: np.array([flag], dtype=np.uint32)}
    if lo is not None:
        want[2] = lo.ravel()
    words = [ref.DTYPE_CODES[dtype], B, n, C, *strides, 0, base, 1, 0, 2, 0, 3, 0, *len_ref]
    expect = {"dense": (predict_dense((B, n, C), strides, shift + base * size, 16 if dtype == "float64" else 4 * size), -1),
              "grid": (ceil_div(ceil_div(count, 4), 256), 1, 1), "launches": 1}
    kernel = "devio_ingest_%s%s" % ("ragged_" if lengths is not None else "", dtype)
    c = Case(kernel, "ingest %s %s B=%d n=%d C=%d %s" % (dtype, kind, B, n, C, label), "ingest", arenas, words,
             shifts=[shift, 0, 0, 0, 0][:len(arenas)], want=want, expect=expect)
    c.flag, c.x, c.lengths = flag, x, lengths
    return c


def ingest_equal(dtype):
    return [ingest_case(dtype, kind, 2 if n <= 5 else 1, n, C, 1000 * n + 10 * C + k)
            for k, kind in enumerate(LAYOUTS) for C in (1, 2, 3) for n in INGEST_COUNTS]


def ingest_ragged(dtype):
    out = []
    for kind in ("dense", "padded", "channels_first"):
        # C = 3: a length cuts inside a run of four; n * C = 21: a run spans two clips and the second length is loaded mid-run
        out.append(ingest_case(dtype, kind, 5, 7, 3, 31, lengths=[0, 1, 6, 7, 3], label="lengths 0 1 n-1 n mix"))
        out.append(ingest_case(dtype, kind, 5, 7, 3, 32, lengths=[7, 6, 0, 1, 7], label="lengths n n-1 0 1 n"))
        out.append(ingest_case(dtype, kind, 4, 8, 2, 33, lengths=[8, 0, 3, 7], label="whole runs"))
        out.append(ingest_case(dtype, kind, 3, 5, 1, 34, lengths=[2, 5, 4], label="C=1 n=5"))
        out.append(ingest_case(dtype, kind, 2, 1027, 1, 35, lengths=[1025, 3], label="two workgroups"))
    return out


def ingest_flags(dtype):
    """The flag: set exactly when a live float sample is NaN or infinite."""
    out = []
    if dtype == "int16":
        return [ingest_case(dtype, kind, 2, 9, 3, 41, label="int16 never sets it") for kind in ("dense", "padded")]
    for kind in ("dense", "padded"):
        for name in ("nan", "inf", "-inf"):
            for where, at in (("a whole run", (0, 1, 2)), ("the tail of the plane", (1, 8, 2))):      # 2 * 9 * 3 = 54 = 13 runs + 2
                out.append(ingest_case(dtype, kind, 2, 9, 3, 42, poke=[(at, special(dtype, name))], label="%s in %s" % (name, where)))
        # not live: the flag stays clear (dense runs wholly behind a length, and the run a length cuts)
        out.append(ingest_case(dtype, kind, 2, 9, 3, 43, lengths=[4, 9], poke=[((0, 4, 0), special(dtype, "inf")), ((0, 8, 2), special(dtype, "nan"))],
                               label="NaN and inf behind a length"))
        out.append(ingest_case(dtype, kind, 2, 9, 3, 44, lengths=[4, 9], poke=[((0, 3, 2), special(dtype, "inf"))], label="inf in the last live sample"))
    if dtype == "float64":
        for kind in ("dense", "padded"):
            out.append(ingest_case(dtype, kind, 2, 9, 3, 45, poke=[((0, 1, 2), 1e300), ((1, 8, 2), -1e300), ((1, 2, 0), 3.5e38)],
                                   label="finite doubles above FLT_MAX"))
    return out


INGEST = {}
for _d in DTYPES:
    INGEST["equal-" + _d] = (lambda d=_d: ingest_equal(d))
    INGEST["ragged-" + _d] = (lambda d=_d: ingest_ragged(d))
    INGEST["flags-" + _d] = (lambda d=_d: ingest_flags(d))


# ---- B. egress ----------------------------------------------------------------------------------------------------------
def ept(dtype):
    return 2 if dtype == "float64" else 4


def trap_values(dtype, rng, count):
    """fp32 inputs of an egress: the trap table of a 16-bit type as far as fp32 delivers it (the rest is checked against
    round_ref of what it did deliver), the special values of the wide types, then noise."""
    if dtype in edr.DTYPES:
        with np.errstate(over="ignore", under="ignore"):
            head = edr.trap_inputs(dtype).astype(np.float32)
    else:
        head = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 3.4028235e38, 1.17549435e-38, 1 + 2.0 ** -23], dtype=np.float32)
    scale = 3e4 if dtype == "int16" else 1.0
    body = fp32_signal(rng, max(count, len(head)), scale)
    body[:len(head)] = head
    return body[:count] if count < len(head) else body


def egress_case(dtype, kind, S, n, C, seed, shift=0):
    rng = np.random.default_rng(seed)
    count = S * n * C
    v = trap_values(dtype, rng, count)[:count].reshape(S, n, C)
    strides, elems, base = layout(kind, S, n, C)
    size = np.dtype(ref.STORAGE[dtype]).itemsize
    want = stored(ref.egress(v, dtype), (S, n, C), strides, elems, base, dtype)
    vec = 16 if dtype in ("float64", "float32") else 8
    words = [ref.DTYPE_CODES[dtype], S, n, C, *strides, 0, 0, 1, base]
    expect = {"dense": (predict_dense((S, n, C), strides, shift + base * size, vec), -1),
              "grid": (ceil_div(ceil_div(count, ept(dtype)), 256), 1, 1), "launches": 1}
    c = Case("devio_egress_" + dtype, "egress %s %s S=%d n=%d C=%d shift=%d" % (dtype, kind, S, n, C, shift), "egress",
             [v.ravel(), prefilled(elems, ref.STORAGE[dtype])], words, shifts=[0, shift], want={1: want}, expect=expect,
             formats={1: dtype} if dtype == "bfloat16" else None)
    c.values = v
    return c


def egress_cases(dtype):
    e, wg = ept(dtype), ept(dtype) * 256
    counts = sorted({1, e - 1, e, e + 1, 2 * e + 1, wg - 1, wg, wg + 1, wg + e - 1, 24})
    out = [egress_case(dtype, kind, 1, n, 1, 50 + n) for kind in ("dense", "padded") for n in counts if n >= 1]
    out += [egress_case(dtype, kind, 2, 7, 3, 77) for kind in LAYOUTS]
    if dtype in edr.DTYPES:
        # a dense 16-bit destination whose base is 2 bytes off an 8-byte boundary: not dense to the launcher, and still right
        out += [egress_case(dtype, "dense", 1, n, 1, 90 + n, shift=2) for n in (24, wg + 1)]
    return out


EGRESS = {d: (lambda d=d: egress_cases(d)) for d in DTYPES}


# ---- C. emission / D. levels: one description of an emission -------------------------------------------------------------
def emission(S, n, C, seed, lo=True, hi_off=0, in_pad=0, table=None, bg_fg=False, live_len=None, gain=None, scale=1.0, silent=None):
    """The planes of an emission and the arenas that hold them: bg 0, hi 1, lo 2, table 3, bg_fg 4, live_len 5, a_cur 6, a_tgt 7.
    Stream s of hi / lo starts hi_off + s * (n * C + in_pad) floats into its arena; the share of an idle slot is NaN in hi and
    bg. ``gain``: None, ("scalar", a) or ("tables", a_cur, a_tgt, ramp). ``silent``: a sample whose input is +0 under a background
    of 1 in every stream, so that its foreground is -a itself."""
    rng = np.random.default_rng(seed)
    per = n * C
    e = {"S": S, "n": n, "C": C, "in_stream": per + in_pad, "table": table, "live_len": live_len, "gain": gain}
    e["hi"], e["bg"] = fp32_signal(rng, (S, n, C), scale), fp32_signal(rng, (S, n, C), scale)
    e["lo"] = (e["hi"] * np.float32(2.0 ** -25) * rng.standard_normal((S, n, C)).astype(np.float32)) if lo else None
    if lo:
        e["lo"][:, ::3] = 0                                        # zero remainders among them
        e["hi"][0, 0, 0] = np.float32(-0.0)
        e["lo"][0, 0, 0] = 0                                       # the mixture of a negative zero is a negative zero
        if n > 2:
            e["hi"][S - 1, 2, 0], e["lo"][S - 1, 2, 0] = np.float32(np.inf), np.float32(np.nan)    # an infinite sample as the ingest leaves it
    e["bg_fg"] = fp32_signal(rng, (S, n, C), scale) if bg_fg else None
    if silent is not None:
        e["hi"][:, silent], e["bg"][:, silent] = 0, 1
        if lo:
            e["lo"][:, silent] = 0
        if bg_fg:
            e["bg_fg"][:, silent] = 1
    if table is not None:
        for s in range(S):
            if table[s] >= IDLE:
                e["hi"][s], e["bg"][s] = np.nan, np.nan
    plane = lambda v: stored(v, (S, n, C), (e["in_stream"], C, 1), hi_off + (S - 1) * e["in_stream"] + per, hi_off, "float32")
    one = np.zeros(1, dtype=np.float32)
    tables = gain is not None and gain[0] == "tables"
    e["arenas"] = [e["bg"].ravel(), plane(e["hi"]), plane(e["lo"]) if lo else one,
                   np.asarray(table, dtype=np.int64) if table is not None else np.zeros(1, dtype=np.int64),
                   e["bg_fg"].ravel() if bg_fg else one,
                   np.asarray(live_len, dtype=np.int64) if live_len is not None else np.zeros(1, dtype=np.int64),
                   np.asarray(gain[1], dtype=np.float32) if tables and gain[1] is not None else one,
                   np.asarray(gain[2], dtype=np.float32) if tables else one]
    e["refs"] = [0, 0, 1, hi_off, *([2, hi_off] if lo else NULL), *([3, 0] if table is not None else NULL), *([4, 0] if bg_fg else NULL),
                 *([5, 0] if live_len is not None else NULL)]
    mode = 0 if gain is None else 1 if gain[0] == "scalar" else 2
    e["gain_words"] = [mode, *([6, 0] if tables and gain[1] is not None else NULL), *([7, 0] if tables else NULL), gain[3] if tables else 0]
    e["floats"] = [float(np.float32(gain[1]))] if mode == 1 else []
    return e


def signals(e, pos0, hop):
    return ref.emit_signals(e["hi"], e["lo"], e["bg"], e["bg_fg"], e["table"], pos0, hop, e["live_len"], e["gain"])


POS0, HOP = 41, 4            # the emission's first sample and the hop of its table: slot_start 11 begins at sample 3 of it


def emit_case(dtype, label, outs, S=3, n=5, C=3, pos0=POS0, hop=HOP, hi_shift=0, **kw):
    e = emission(S, n, C, kw.pop("seed", 7), scale=3e3 if dtype == "int16" else 1.0, **kw)
    mix, bgv, fgv, _ = signals(e, pos0, hop)
    sig = {ref.BACKGROUND: bgv, ref.FOREGROUND: fgv, ref.MIXTURE: mix}
    arenas, want, words_out, dense = list(e["arenas"]), {}, [], [-1, -1]
    size = np.dtype(ref.STORAGE[dtype]).itemsize
    for k, (which, kind) in enumerate(outs):
        strides, elems, base = layout(kind, S, n, C)
        arenas.append(prefilled(elems, ref.STORAGE[dtype]))
        want[len(arenas) - 1] = stored(ref.narrow(sig[which], dtype), (S, n, C), strides, elems, base, dtype)
        words_out += [which, *strides, len(arenas) - 1, base]
        dense[k] = predict_dense((S, n, C), strides, base * size, 16 if dtype in ("float64", "float32") else 8)
    words = [ref.DTYPE_CODES[dtype], S, n, C, e["in_stream"], pos0, hop, *e["refs"], *e["gain_words"], len(outs), *words_out]
    expect = {"dense": tuple(dense), "grid": (ceil_div(ceil_div(S * n * C, ept(dtype)), 256), 1, 1), "launches": 1}
    shifts = [0] * len(arenas)
    shifts[1] = shifts[2] = hi_shift
    return Case("devio_emit_" + dtype, "emit %s %s" % (dtype, label), "emit", arenas, words, e["floats"], shifts=shifts, want=want,
                expect=expect, formats={k: dtype for k in want} if dtype == "bfloat16" else None)


TABLE = [0, IDLE, 11]        # a slot that started long ago, an idle one, one that starts at sample 3 of the emission
A_CUR, A_TGT = [1.0, 0.25, 0.7], [0.3, 0.8, 0.7]               # per stream: two different fades and a slot whose entries are equal


# a fade whose difference a_tgt - a_cur is not a float64: sample ramp - 1 is no longer inside the fade and takes a_tgt itself, which
# a_cur + (a_tgt - a_cur) * 1 computed in float64 is not (1 + (2^-60 - 1) is 0). Seen in the foreground of a silent sample there.
FAR_CUR, FAR_TGT = [1.0, 1.0, 0.5], [2.0 ** -60, 2.0 ** -70, 2.0 ** -90]


def gain_cases(n):
    """(label, gain) for an emission of n samples: none, scalar, tables with every position of the ramp."""
    f32 = lambda v: np.asarray(v, dtype=np.float32)
    return [("no gain", None), ("scalar gain", ("scalar", np.float32(0.3))), ("tables ramp 0", ("tables", None, f32(A_TGT), 0)),
            ("tables ramp inside a run", ("tables", f32(A_CUR), f32(A_TGT), 3)), ("tables ramp = n", ("tables", f32(A_CUR), f32(A_TGT), n)),
            ("tables ramp > n", ("tables", f32(A_CUR), f32(A_TGT), n + 6))]


def emit_cases(dtype):
    B, F, M = ref.BACKGROUND, ref.FOREGROUND, ref.MIXTURE
    out = []
    for lo in (True, False):
        for which, name in ((B, "background"), (F, "foreground"), (M, "mixture")):
            out.append(emit_case(dtype, "%s alone lo=%d" % (name, lo), [(which, "dense")], lo=lo))
            out.append(emit_case(dtype, "%s alone strided lo=%d" % (name, lo), [(which, "padded")], lo=lo, S=2, n=6, C=2))
        out.append(emit_case(dtype, "two destinations lo=%d" % lo, [(B, "dense"), (F, "padded")], lo=lo))
        out.append(emit_case(dtype, "two destinations, mixture first lo=%d" % lo, [(M, "channels_first"), (F, "dense")], lo=lo, table=TABLE))
    # hi misaligned: one float into its arena and streams 15 + 2 floats apart; n * C = 15 is odd, so a run holds two streams
    for label, gain in gain_cases(5):
        out.append(emit_case(dtype, label + ", table", [(F, "dense"), (B, "padded")], table=TABLE, gain=gain))
        out.append(emit_case(dtype, label + ", hi misaligned", [(F, "dense")], hi_off=1, in_pad=2, gain=gain))
        out.append(emit_case(dtype, label + ", shaped background", [(F, "dense"), (B, "dense")], bg_fg=True, gain=gain, table=TABLE))
        out.append(emit_case(dtype, label + ", C = 1", [(F, "dense"), (M, "padded")], S=3, n=9, C=1,
                             gain=None if gain is None or gain[0] == "scalar" else (gain[0], gain[1], gain[2], {5: 9, 11: 15}.get(gain[3], gain[3]))))
    for ramp in (3, 5):
        out.append(emit_case(dtype, "the last sample of a fade is the target itself, ramp %d" % ramp, [(F, "dense"), (F, "padded")], silent=ramp - 1,
                             gain=("tables", np.asarray(FAR_CUR, dtype=np.float32), np.asarray(FAR_TGT, dtype=np.float32), ramp)))
    out.append(emit_case(dtype, "hi 8 bytes off", [(M, "dense")], hi_shift=8, S=2, n=8, C=2))
    out.append(emit_case(dtype, "the mixture does not read the shaped background", [(M, "dense"), (B, "padded")], bg_fg=True))
    for label, lens in (("0", [0, 0, 0]), ("cutting runs", [2, 5, 3]), ("n", [5, 5, 5]), ("mixed", [5, 0, 1])):
        out.append(emit_case(dtype, "live_len %s, background only" % label, [(B, "dense"), (B, "padded")], live_len=lens))
        out.append(emit_case(dtype, "live_len %s, foreground" % label, [(F, "dense")], live_len=lens, gain=("scalar", np.float32(0.5))))
        out.append(emit_case(dtype, "live_len %s, hi misaligned" % label, [(M, "dense"), (F, "padded")], live_len=lens, hi_off=3, in_pad=1))
    # more than one workgroup, and a plane whose last run is short
    out.append(emit_case(dtype, "three workgroups", [(F, "dense"), (B, "padded")], S=3, n=683, C=1, table=TABLE,
                         gain=("tables", np.asarray(A_CUR, dtype=np.float32), np.asarray(A_TGT, dtype=np.float32), 6)))
    return out


EMIT = {d: (lambda d=d: emit_cases(d)) for d in DTYPES}


# ---- D. levels ----------------------------------------------------------------------------------------------------------
def level_tile(C):
    return 1024 // int(np.lcm(4, C)) * int(np.lcm(4, C))


def levels_case(label, S, n, C, pos0=POS0, hop=HOP, **kw):
    e = emission(S, n, C, kw.pop("seed", 11), **kw)
    chunks = ceil_div(n, ref.LEVEL_CHUNK)
    arenas = list(e["arenas"]) + [prefilled(S * C * lr.FIELDS, np.float64), prefilled(max(1, S * C * chunks * lr.FIELDS if chunks > 1 else 1), np.float64)]
    words = [S, n, C, e["in_stream"], pos0, hop, *e["refs"], *e["gain_words"], 8, 0, *([9, 0] if chunks > 1 else NULL)]
    c = Case("devio_levels", "levels %s S=%d n=%d C=%d" % (label, S, n, C), "levels", arenas, words, e["floats"], free={8, 9},
             expect={"grid": (S * C, 1, 1) if chunks > 1 else (1, S, 1), "launches": 2 if chunks > 1 else 1})
    c.emission, c.pos0, c.hop, c.shape = e, pos0, hop, (S, C, lr.FIELDS)
    return c


def levels_sizes(C):
    tile = level_tile(C)
    return [1, tile // C, tile // C + 1, 4095, 4096, 4097, 8 * 4096 + 1]


def levels_cases_sizes(C):
    return [levels_case("sizes", 2, n, C, hi_off=k % 2, in_pad=(k % 3), seed=100 + n % 97) for k, n in enumerate(levels_sizes(C))]


def levels_cases_options():
    out = []
    for label, gain in gain_cases(9):
        out.append(levels_case(label + ", table", 3, 9, 3, table=TABLE, gain=gain))
        out.append(levels_case(label + ", shaped, hi misaligned", 3, 9, 3, bg_fg=True, hi_off=1, in_pad=2, gain=gain))
    for label, lens in (("0", [0, 0, 0]), ("cutting runs", [2, 9, 3]), ("n", [9, 9, 9])):
        out.append(levels_case("live_len " + label, 3, 9, 3, live_len=lens, gain=("scalar", np.float32(0.5))))
    out.append(levels_case("no lo", 2, 300, 5, lo=False))
    out.append(levels_case("the last sample of a fade is the target itself", 3, 9, 3, silent=4,
                           gain=("tables", np.asarray(FAR_CUR, dtype=np.float32), np.asarray(FAR_TGT, dtype=np.float32), 5)))
    return out


LEVELS = {"sizes-C%d" % C: (lambda C=C: levels_cases_sizes(C)) for C in (1, 2, 3, 5)}
LEVELS["options"] = levels_cases_options


def levels_want(c):
    mix, bgv, fgv, live = signals(c.emission, c.pos0, c.hop)
    return lr.levels(mix, bgv, fgv, live)


# ---- E. append, feed, take ----------------------------------------------------------------------------------------------
def append_cases():
    out = []
    for dtype in ("float64", "int16"):
        for kind in ("dense", "padded"):
            for C, ns in ((1, (5, 6, 7, 8)), (3, (3, 4, 5, 6))):          # n * C % 4 takes 1, 2, 3, 0 (C = 3: 1, 0, 3, 2)
                for n in ns:
                    for d_off in (8, 9, 10, 11):
                        S, d_stream = 3, 40
                        x = samples(np.random.default_rng(n * 10 + d_off), (S, n, C), dtype)
                        strides, elems, base = layout(kind, S, n, C)
                        total = (S - 1) * d_stream + d_off + n * C + 5
                        arenas = [stored(x, (S, n, C), strides, elems, base, dtype), prefilled(total, np.float32), prefilled(total, np.float32)]
                        hi, lo = ref.append(arenas[1], arenas[2], x, dtype, d_stream, d_off)
                        words = [ref.DTYPE_CODES[dtype], S, n, C, *strides, 0, base, 1, 0, 2, 0, d_stream, d_off]
                        c = Case("online_append_" + dtype, "append %s %s n=%d C=%d d_off=%d" % (dtype, kind, n, C, d_off), "append", arenas,
                                 words, want={1: hi, 2: lo}, expect={"grid": (1, S, 1), "launches": 1})
                        c.classes = (d_off & 3, (n * C) % 4)
                        out.append(c)
    return out


def feed_case(label, dtype, kind, n, C, ring_len, ring_stride, rows, seed, n_slots=None):
    """rows: (slot, count, wpos) per row of the source."""
    R = len(rows)
    n_slots = n_slots or max(r[0] for r in rows) + 1
    x = samples(np.random.default_rng(seed), (R, n, C), dtype)
    strides, elems, base = layout(kind, R, n, C)
    arenas = [stored(x, (R, n, C), strides, elems, base, dtype), prefilled(n_slots * ring_stride, np.float32), prefilled(n_slots * ring_stride, np.float32)]
    slots, counts, wpos = ([r[k] for r in rows] for k in range(3))
    hi, lo = ref.feed(arenas[1], arenas[2], x, dtype, slots, counts, wpos, ring_stride, ring_len)
    words = [ref.DTYPE_CODES[dtype], R, n, C, *strides, 0, base, 1, 0, 2, 0, ring_stride, ring_len, *slots, *counts, *wpos]
    launches = sum(1 for first in range(0, R, 256) if max(counts[first:first + 256]) > 0)
    c = Case("online_feed_" + dtype, "feed %s %s %s" % (dtype, kind, label), "feed", arenas, words, want={1: hi, 2: lo}, expect={"launches": launches})
    c.rows, c.ring_len, c.ring_stride, c.C = rows, ring_len, ring_stride, C
    return c


def ring_rows(ring_len, C, n):
    """Rows that put a run of n samples at every write position around the wrap: every wpos & 3, the wrap cutting a slot after
    1, 2 and 3 floats (whatever ring_len % 4 is, some position does each), a run that ends exactly on ring_len, counts 0 and n."""
    starts = [p * C for p in range(ring_len // C)]
    rows = [(k, n, w) for k, w in enumerate(w for w in starts if w + n * C >= ring_len - 4 or w < 4 * C)]
    rows.append((len(rows), 0, starts[1]))
    rows.append((len(rows), n - 1, ring_len - (n - 1) * C))       # ends exactly on ring_len
    order = np.random.default_rng(ring_len).permutation(len(rows))
    return [(int(order[k]), rows[k][1], rows[k][2]) for k in range(len(rows))]


def feed_cases():
    out = []
    for dtype, kind in (("float64", "padded"), ("float64", "dense"), ("int16", "dense"), ("int16", "padded")):
        for C, ring_len, ring_stride in ((1, 20, 24), (1, 21, 24), (1, 22, 24), (1, 23, 24), (3, 21, 24), (2, 22, 28)):
            n = 9 // C + 1 if C > 1 else 9
            out.append(feed_case("ring %d C=%d" % (ring_len, C), dtype, kind, n, C, ring_len, ring_stride, ring_rows(ring_len, C, n), ring_len))
    out.append(feed_case("257 rows", "float64", "dense", 2, 1, 8, 12, [(256 - k, 1 + k % 2, k % 8) for k in range(257)], 5))
    out.append(feed_case("256 idle rows, then one", "int16", "dense", 2, 1, 8, 12, [(k, 0 if k < 256 else 2, 7) for k in range(257)], 6))
    return out


def take_case(label, ring_len, ring_stride, table, rpos, length, d_stream, d_off, seed):
    rng = np.random.default_rng(seed)
    S = len(rpos)
    hi, lo = fp32_signal(rng, S * ring_stride), fp32_signal(rng, S * ring_stride)
    arenas = [hi, lo, prefilled(S * d_stream, np.float32), prefilled(S * d_stream, np.float32), np.asarray(table, dtype=np.int64)]
    dhi, dlo = ref.take(arenas[2], arenas[3], hi, lo, table, rpos, length, ring_stride, ring_len, d_stream, d_off)
    words = [S, length, ring_stride, ring_len, d_stream, d_off, 0, 0, 1, 0, 2, 0, 3, 0, 4, 0, *rpos]
    c = Case("online_take", "take " + label, "take", arenas, words, want={2: dhi, 3: dlo},
             expect={"launches": ceil_div(S, 256), "grid": (1, min(256, S - 256 * (ceil_div(S, 256) - 1)), 1)})
    c.table, c.rpos, c.ring_len, c.length, c.d_off = table, rpos, ring_len, length, d_off
    return c


def take_cases():
    out = []
    for ring_len in (20, 21, 22, 23):
        for d_off in (8, 9, 10, 11):
            for length in (9, 12):
                rpos = list(range(ring_len - 13, ring_len)) + [0, 1, 2, 3, 4]
                table = [k % 5 for k in range(len(rpos))]
                table[2], table[7], table[11] = IDLE, HELD, IDLE
                out.append(take_case("ring %d d_off %d len %d" % (ring_len, d_off, length), ring_len, 24, table, rpos, length, 24, d_off,
                                     ring_len * 100 + d_off))
    out.append(take_case("257 slots", 8, 12, [IDLE if k % 7 == 3 else (HELD if k % 11 == 5 else k) for k in range(257)],
                         [k % 8 for k in range(257)], 5, 8, 2, 9))
    return out


MOVE_IN = {"append": append_cases, "feed": feed_cases, "take": take_cases}


# ---- F. the five movers on move_slot ------------------------------------------------------------------------------------
SIDES = {"aligned": (0, 12, 48), "base off": (1, 12, 48), "block odd": (0, 13, 48), "stream odd": (0, 12, 49)}      # (base, block, stream)


def part_arenas(rng, length, blocks, S, src_side, dst_side, null_src=False, lead=0, stream=None):
    """One part's source and destination: (src or None, src_off, src_block, src_stream, dst, dst_off, dst_block, dst_stream).
    ``lead`` floats of the source lie in front of the part's first element."""
    so, sb, ss = SIDES[src_side]
    do, db, ds = SIDES[dst_side]
    if stream is not None:                                        # (runs longer than the strides of SIDES: streams must not overlap)
        ss, ds = stream + ss % 4, stream + ds % 4
    so += lead
    src = None if null_src else fp32_signal(rng, so + (S - 1) * ss + (blocks - 1) * sb + length + 8)
    if src is not None:
        src[::5] = np.nan                                          # what a mover moves it moves bit for bit
    dst = prefilled(do + (S - 1) * ds + (blocks - 1) * db + length + 3, np.float32)
    return src, so, sb, ss, dst, do, db, ds


def row_copy_case(label, specs, S, table=None, op="row_copies", seed=3):
    """specs: dicts of len, blocks, src_side, dst_side and optionally null_src, row_len, frame0, delta, zero_below, lead."""
    rng = np.random.default_rng(seed)
    arenas, words, parts, want = [np.asarray(table if table is not None else [0], dtype=np.int64)], [], [], {}
    src_vec, dst_vec, held_vec = [-1] * 5, [-1] * 5, [-1] * 5
    most = 1
    for k, sp in enumerate(specs):
        src, so, sb, ss, dst, do, db, ds = part_arenas(rng, sp["len"], sp["blocks"], S, sp["src_side"], sp["dst_side"], sp.get("null_src", False),
                                                       sp.get("lead", 0), sp.get("stream"))
        si = -1
        if src is not None:
            arenas.append(src)
            si = len(arenas) - 1
        arenas.append(dst)
        di = len(arenas) - 1
        p = {"dst": dst, "src": src, "dst_off": do, "src_off": so, "len": sp["len"], "blocks": sp["blocks"], "src_block": sb, "dst_block": db,
             "src_stream": ss, "dst_stream": ds, "row_len": sp.get("row_len", 0), "frame0": sp.get("frame0", 0), "delta": sp.get("delta", 0),
             "zero_below": sp.get("zero_below", 0)}
        parts.append((p, di))
        words += [si, so if si >= 0 else 0, di, do, sp["len"], sp["blocks"], sb, db, ss, ds, p["row_len"], p["frame0"]]
        if op == "slide_held":
            words += [p["delta"], p["zero_below"]]
        src_vec[k] = 0 if src is None else predict_vec(4 * so, sb, ss)
        dst_vec[k] = predict_vec(4 * do, db, ds)
        if op == "slide_held":
            held_vec[k] = int(src_vec[k] and p["delta"] % 4 == 0)
        most = max(most, ceil_div(sp["len"], 4) * sp["blocks"])
    outs = ref.row_copies([p for p, _ in parts], S, table) if op == "row_copies" else ref.slide_held([p for p, _ in parts], S, table)
    for (p, di), o in zip(parts, outs):
        want[di] = o
    x_cap = max(1, 4096 // (S * len(specs)))
    expect = {"src_vec": tuple(src_vec), "dst_vec": tuple(dst_vec), "held_vec": tuple(held_vec), "launches": 1,
              "grid": (max(1, min(ceil_div(most, 256), x_cap)), S, len(specs))}
    c = Case("online_" + op, "%s %s" % (op.replace("_", " "), label), op, arenas, [len(specs), S, *([0, 0] if table is not None else NULL), *words],
             want=want, expect=expect)
    c.vec = list(zip(src_vec, dst_vec))[:len(specs)]
    c.held_vec = held_vec[:len(specs)]
    return c


def row_copies_cases():
    out = []
    for length in (1, 3, 4, 5, 8, 9):
        for blocks in (1, 3):
            for src_side in SIDES:
                specs = [dict(len=length, blocks=blocks, src_side=src_side, dst_side=d) for d in SIDES]
                specs.append(dict(len=length, blocks=blocks, src_side="aligned", dst_side="aligned" if length % 2 else "base off", null_src=True))
                out.append(row_copy_case("len=%d blocks=%d src %s" % (length, blocks, src_side), specs, 2, seed=length * 10 + blocks))
    # frame rows: of stream b only the rows of frames before slot_start[b] -- no rows, some rows, all rows, and an idle slot
    for src_side, dst_side in (("aligned", "aligned"), ("base off", "block odd")):
        specs = [dict(len=12, blocks=2, src_side=src_side, dst_side=dst_side, row_len=3, frame0=5),
                 dict(len=12, blocks=2, src_side=src_side, dst_side=dst_side, row_len=4, frame0=5, null_src=True),
                 dict(len=9, blocks=1, src_side=src_side, dst_side=dst_side)]
        out.append(row_copy_case("frame rows %s" % src_side, specs, 5, table=[4, 5, 7, 14, IDLE]))
    out.append(row_copy_case("frame rows, no table", [dict(len=12, blocks=2, src_side="aligned", dst_side="aligned", row_len=3, frame0=5)], 2))
    # 64 streams x 5 parts leave 12 workgroups in x: one slot more than 12 x 256 per stream, so the grid-stride loop runs
    big = [dict(len=4 * 12 * 256 + 2, blocks=1, src_side="aligned", dst_side="aligned", stream=4 * 12 * 256 + 4)]
    big += [dict(len=5, blocks=1, src_side="aligned", dst_side=d) for d in SIDES]
    c = row_copy_case("grid-stride in x", big, 64)
    assert c.expect["grid"] == (12, 64, 5)
    out.append(c)
    return out


SLIDE_LENS, SLIDE_BLOCKS = (1, 3, 4, 5, 8, 9), (1, 3)


def slide_cases():
    """Every len and blocks of the movers with every delta in {0, -1, -4, -len} and, as the parts of one launch, every zero_below
    in {0, 1, 4, 5, len} -- above len too, where the launcher cuts it to len --, each from an aligned and a misaligned source into a
    destination that takes whole slots in one store and one that does not; streams 0 and 2 held, stream 1 not."""
    out = []
    for length in SLIDE_LENS:
        for blocks in SLIDE_BLOCKS:
            for delta in sorted({0, -1, -4, -length}, reverse=True):
                for src_side, dst_side in (("aligned", "aligned"), ("base off", "aligned"), ("aligned", "block odd"), ("base off", "block odd")):
                    zbs = sorted({0, 1, 4, 5, length})
                    specs = [dict(len=length, blocks=blocks, src_side=src_side, dst_side=dst_side, delta=delta, zero_below=zb, lead=12) for zb in zbs]
                    c = row_copy_case("len=%d blocks=%d src %s dst %s delta=%d" % (length, blocks, src_side, dst_side, delta), specs, 3,
                                      table=[HELD, 5, HELD], op="slide_held", seed=length * 100 + blocks * 10 - delta)
                    c.slide = (length, blocks, delta, tuple(zbs))
                    out.append(c)
    c = row_copy_case("nobody held", [dict(len=8, blocks=3, src_side="aligned", dst_side="aligned", delta=-4, zero_below=4, lead=12)], 2,
                      table=[3, IDLE], op="slide_held")
    c.slide = None
    out.append(c)
    return out


def slot_move_case(label, specs, op, table=None, slot=0, value=0, shift=0, seed=5):
    """specs: dicts of len, blocks, src_side, dst_side, src_off, zero_below and optionally null_src, lead."""
    rng = np.random.default_rng(seed)
    arenas, words, parts = [np.asarray(table if table is not None else [0], dtype=np.int64)], [], []
    src_vec, dst_vec = [-1] * 5, [-1] * 5
    most = 1
    for k, sp in enumerate(specs):
        src, so, sb, _, dst, do, db, _ = part_arenas(rng, sp["len"], sp["blocks"], 1, sp["src_side"], sp["dst_side"], sp.get("null_src", False), sp.get("lead", 0))
        si = -1
        if src is not None:
            arenas.append(src)
            si = len(arenas) - 1
        arenas.append(dst)
        di = len(arenas) - 1
        zb = sp["zero_below"]
        parts.append(({"dst": dst, "dst_off": do, "src": src, "src_base": so, "src_off": sp["src_off"], "len": sp["len"], "blocks": sp["blocks"],
                       "src_block": sb, "dst_block": db, "zero_below": zb}, di))
        words += [si, so if si >= 0 else 0, di, do, sp["src_off"], sp["len"], sp["blocks"], sb, db, zb]
        reads = src is not None and zb < sp["len"]
        src_vec[k] = int(reads and predict_vec(4 * so, sb, 0) and sp["src_off"] % 4 == 0)
        dst_vec[k] = predict_vec(4 * do, db, 0)
        most = max(most, ceil_div(sp["len"], 4) * sp["blocks"])
    want = {di: o for (p, di), o in zip(parts, ref.slot_move([p for p, _ in parts]))}
    if op == "slot_import":
        want[0] = ref.import_table(arenas[0], slot, value, shift)
    head = [len(specs), *([0, 0] if op == "slot_import" else NULL), len(arenas[0]) if op == "slot_import" else 0, slot, value, shift]
    expect = {"src_vec": tuple(src_vec), "dst_vec": tuple(dst_vec), "launches": 1, "grid": (max(1, min(ceil_div(most, 256), 4096 // 5)), 5, 1)}
    return Case("online_" + op, "%s %s" % (op.replace("_", " "), label), op, arenas, head + words, want=want, expect=expect)


def slot_move_cases():
    out = []
    for op in ("slot_export", "slot_import"):
        kw = dict(table=[3, IDLE, HELD, 7], slot=1, value=9, shift=-2) if op == "slot_import" else {}
        for length in (1, 3, 4, 5, 8, 9):
            for blocks in (1, 3):
                specs = [dict(len=length, blocks=blocks, src_side=s, dst_side=d, src_off=0, zero_below=0) for s, d in
                         (("aligned", "aligned"), ("base off", "aligned"), ("aligned", "block odd"), ("block odd", "base off"))]
                specs.append(dict(len=length, blocks=blocks, src_side="aligned", dst_side="aligned", src_off=0, zero_below=length, null_src=True))
                out.append(slot_move_case("len=%d blocks=%d" % (length, blocks), specs, op, seed=length + blocks, **kw))
        # runs right-aligned on what the source holds: a negative offset with the elements in front of the source zero
        specs = [dict(len=9, blocks=2, src_side="aligned", dst_side="aligned", src_off=-3, zero_below=3),
                 dict(len=9, blocks=2, src_side="aligned", dst_side="base off", src_off=-4, zero_below=5),
                 dict(len=8, blocks=3, src_side="aligned", dst_side="aligned", src_off=-4, zero_below=4),
                 dict(len=8, blocks=1, src_side="aligned", dst_side="aligned", src_off=-8, zero_below=8),
                 dict(len=5, blocks=2, src_side="aligned", dst_side="aligned", src_off=4, zero_below=1, lead=0)]
        out.append(slot_move_case("negative src_off", specs, op, **kw))
    out.append(slot_move_case("shift 0 leaves the other slots", [dict(len=4, blocks=1, src_side="aligned", dst_side="aligned", src_off=0, zero_below=0)],
                              "slot_import", table=[3, IDLE, HELD, 7], slot=3, value=1 << 40, shift=0))
    out.append(slot_move_case("no parts, the table alone", [], "slot_import", table=[3, 5, HELD, IDLE], slot=3, value=2, shift=6))
    return out


def slot_reset_case(label, n_table, slots, value, specs, seed=8):
    rng = np.random.default_rng(seed)
    table = np.arange(n_table, dtype=np.int64) + 100
    arenas, words, parts = [table], [], []
    dst_vec = [-1] * 5
    most = 1
    for k, sp in enumerate(specs):
        do, db, ds = SIDES[sp["dst_side"]]
        ds = sp.get("stream", ds)
        dst = fp32_signal(rng, do + (n_table - 1) * ds + (sp["blocks"] - 1) * db + sp["len"] + 3)
        dst[::3] = np.nan
        arenas.append(dst)
        parts.append({"dst": dst, "dst_off": do, "len": sp["len"], "blocks": sp["blocks"], "dst_block": db, "dst_stream": ds})
        words += [len(arenas) - 1, do, sp["len"], sp["blocks"], db, ds]
        dst_vec[k] = predict_vec(4 * do, db, ds)
        most = max(most, ceil_div(sp["len"], 4) * sp["blocks"])
    new_table, outs = ref.slot_reset(table, value, slots, parts)
    want = {0: new_table}
    want.update({k + 1: o for k, o in enumerate(outs)})
    last = len(slots) - 256 * (ceil_div(len(slots), 256) - 1)
    expect = {"dst_vec": tuple(dst_vec), "src_vec": tuple(0 if v >= 0 else -1 for v in dst_vec), "launches": ceil_div(len(slots), 256),
              "grid": (max(1, min(ceil_div(most, 256), max(1, 4096 // (last * 5)))), last, 5)}
    return Case("online_slot_reset", "slot reset " + label, "slot_reset", arenas, [0, 0, n_table, value, len(slots), len(specs), *slots, *words],
                want=want, expect=expect)


def slot_reset_cases():
    out = []
    for length in (1, 3, 4, 5, 8, 9):
        specs = [dict(len=length, blocks=b, dst_side=d) for b in (1, 3) for d in ("aligned", "base off")] + [dict(len=length, blocks=1, dst_side="stream odd")]
        out.append(slot_reset_case("len=%d" % length, 6, [4, 1, 2], IDLE, specs, seed=length))
    out.append(slot_reset_case("no parts", 4, [3], 17, []))
    out.append(slot_reset_case("257 slots", 300, [299 - k for k in range(257)], 0,
                               [dict(len=5, blocks=1, dst_side="aligned", stream=8), dict(len=4, blocks=2, dst_side="base off", stream=25)]))
    return out


MOVERS = {"row_copies": row_copies_cases, "slide_held": slide_cases, "slot_move": slot_move_cases, "slot_reset": slot_reset_cases}


# ---- G. tables and tail_clear -------------------------------------------------------------------------------------------
def table_cases():
    out = []
    t = np.arange(300, dtype=np.int64) * 3
    slots = [(k * 7) % 300 for k in range(257)]
    values = [HELD if k % 5 == 0 else 1000 + k for k in range(257)]
    assert len(set(slots)) == 257
    out.append(Case("online_slot_set", "slot set 257 ids", "slot_set", [t], [0, 0, 300, 257, *slots, *values], want={0: ref.slot_set(t, slots, values)},
                    expect={"launches": 2, "grid": (1, 1, 1)}))
    out.append(Case("online_slot_set", "slot set 1 id", "slot_set", [t], [0, 0, 300, 1, 299, IDLE], want={0: ref.slot_set(t, [299], [IDLE])},
                    expect={"launches": 1}))
    g = prefilled(300, np.float32)
    for n in (1, 255, 256, 257, 300):
        out.append(Case("online_gain_fill", "gain fill n=%d" % n, "gain_fill", [g], [0, 0, n], [0.3], want={0: ref.gain_fill(g, n, 0.3)}, expect={"launches": 1}))
    a = [float(np.float32(1 - k / 300)) for k in range(257)]
    out.append(Case("online_gain_set", "gain set 257 ids", "gain_set", [g], [0, 0, 300, 257, *slots], a, want={0: ref.gain_set(g, slots, a)},
                    expect={"launches": 2}))
    out.append(Case("online_gain_set", "gain set 1 id", "gain_set", [g], [0, 0, 300, 1, 299], [0.5], want={0: ref.gain_set(g, [299], [0.5])},
                    expect={"launches": 1}))
    rng = np.random.default_rng(4)
    tgt, old = rng.random(300).astype(np.float32), rng.random(300).astype(np.float32)
    for n, slot in ((300, -1), (300, 0), (300, 299), (300, 256), (5, 3), (1, -1)):
        new = prefilled(300, np.float32)
        out.append(Case("online_gain_commit", "gain commit n=%d slot=%d" % (n, slot), "gain_commit", [tgt, old, new], [0, 0, 1, 0, 2, 0, n, slot],
                        want={2: ref.gain_commit(tgt, old, new, n, slot)}, expect={"launches": 1}))
    return out


def band_expand_case(label, FS, F, n_table, slots, rows_of, edges, gains, init):
    gains = np.asarray(gains, dtype=np.float32).reshape(-1, len(edges) - 1)
    tab = prefilled(n_table * ref.BAND_ROWS * FS, np.float32)
    job = np.concatenate([np.asarray(slots, dtype=np.int32), np.asarray(rows_of, dtype=np.int32), np.asarray(edges, dtype=np.int32),
                          gains.ravel().view(np.int32)])
    want = ref.band_expand(tab, FS, F, slots, rows_of, edges, gains, init)
    return Case("online_band_expand", "band expand " + label, "band_expand", [tab, job],
                [0, 0, 1, 0, n_table, FS, F, len(slots), len(edges) - 1, gains.shape[0], int(init)], want={0: want},
                expect={"launches": 1, "grid": (ceil_div(FS, 256), len(slots), 1)})


def band_cases():
    out = []
    rng = np.random.default_rng(12)
    for init in (False, True):
        # bins below edges[0] and at edges[n_bands], pad bins F .. FS - 1, a row below 0 and one past the rows
        out.append(band_expand_case("five bands init=%d" % init, 544, 513, 5, [3, 0, 4, 1], [1, 0, -1, 2], [2, 3, 10, 255, 256, 500],
                                    rng.random((2, 5)), init))
        out.append(band_expand_case("one band init=%d" % init, 32, 17, 2, [1], [0], [0, 17], [[0.25]], init))
        out.append(band_expand_case("one band inside init=%d" % init, 32, 17, 2, [0], [0], [5, 6], [[1.0]], init))
        out.append(band_expand_case("F bands init=%d" % init, 32, 17, 3, [2, 0], [0, 1], list(range(18)), rng.random((2, 17)), init))
    FS, n_slots = 288, 4
    tab = fp32_signal(rng, n_slots * ref.BAND_ROWS * FS)
    table = np.asarray([3, HELD, IDLE, 9], dtype=np.int64)
    for mode, name in ((ref.BAND_COMMIT, "commit"), (ref.BAND_SETTLE, "settle"), (ref.BAND_CARRY, "carry")):
        for slot, with_table in ((-1, True), (-1, False), (1, True), (3, False)):
            out.append(Case("online_band_commit", "band %s slot=%d table=%d" % (name, slot, with_table), "band_commit", [tab, table],
                            [0, 0, *([1, 0] if with_table else NULL), FS, n_slots, slot, mode],
                            want={0: ref.band_commit(tab, FS, n_slots, slot, mode, table if with_table else None)},
                            expect={"launches": 1, "grid": (2, n_slots if slot < 0 else 1, 1)}))
    return out


def tail_clear_cases():
    out = []
    rng = np.random.default_rng(21)
    W, H, FS, T, C, B = 64, 32, 32, 6, 2, 5
    chan, spec = (T + 2) * FS, C * (T + 2) * FS + 64
    # T_b = ceil((len - W) / H) + 1: 0 for a clip shorter than W - H, T - 1, T, more than T, and something between
    lengths = [W - H - 1, W + (T - 2) * H, W + (T - 1) * H, W + (T + 3) * H, W + H + 1]
    assert [ref.frame_count(v, W, H) for v in lengths] == [0, T - 1, T, T + 4, 3]
    cells = (B - 1) * spec + (C - 1) * chan + T * FS + 8
    for with_mask in (True, False):
        X = (rng.standard_normal(cells) + 1j * rng.standard_normal(cells)).astype(np.complex64)
        Mk = rng.random(cells).astype(np.float32)
        X[::3], Mk[::4] = np.nan, np.nan                          # NaN in the rows beforehand: a store, not a product
        wx, wm = ref.tail_clear(X, Mk if with_mask else None, spec, chan, B, C, T, FS, W, H, lengths)
        arenas = [X, Mk, np.asarray(lengths, dtype=np.int64)]
        longest = T
        groups = min(ceil_div(longest * FS, 1024), max(1, 4096 // (B * C)))
        out.append(Case("devio_tail_clear", "tail clear mask=%d" % with_mask, "tail_clear", arenas,
                        [B, C, T, FS, W, H, spec, chan, longest, 0, 0, *([1, 0] if with_mask else NULL), 2, 0],
                        want={0: wx, 1: wm} if with_mask else {0: wx}, expect={"launches": 1, "grid": (groups, B, C)}))
    # rows long enough that a workgroup's 1024 floats do not cover the tail: the loop in x runs
    T, FS, B, C = 40, 64, 1, 1
    cells = T * FS
    X = (rng.standard_normal(cells) + 1j * rng.standard_normal(cells)).astype(np.complex64)
    Mk = rng.random(cells).astype(np.float32)
    lengths = [W + 2 * H]
    wx, wm = ref.tail_clear(X, Mk, cells, cells, B, C, T, FS, W, H, lengths)
    out.append(Case("devio_tail_clear", "tail clear, a short grid", "tail_clear", [X, Mk, np.asarray(lengths, dtype=np.int64)],
                    [B, C, T, FS, W, H, cells, cells, 1, 0, 0, 1, 0, 2, 0], want={0: wx, 1: wm}, expect={"launches": 1, "grid": (1, 1, 1)}))
    return out


TABLES = {"tables": table_cases, "bands": band_cases, "tail_clear": tail_clear_cases}

GROUPS = {"ingest": INGEST, "egress": EGRESS, "emit": EMIT, "levels": LEVELS, "move_in": MOVE_IN, "movers": MOVERS, "tables": TABLES}

# the launcher decisions that must have been seen by the time the last test runs
REQUIRED = ([(op, "dense", v) for op in ("ingest", "egress", "emit") for v in (0, 1)] +
            [(op, "src_vec,dst_vec", (s, d)) for op in ("row_copies", "slide_held", "slot_export", "slot_import") for s in (0, 1) for d in (0, 1)] +
            [("slot_reset", "dst_vec", v) for v in (0, 1)] + [("slide_held", "held_vec", v) for v in (0, 1)] +
            [(op, "launches", 2) for op in ("slot_set", "feed", "take", "slot_reset", "gain_set", "levels")] +
            [(op, "launches", 1) for op in ("slot_set", "feed", "take", "slot_reset", "gain_set", "levels")])


# ---- the tests ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(INGEST))
def test_ingest(key):
    for case in INGEST[key]():
        run_case(case)


@pytest.mark.parametrize("dtype", DTYPES)
def test_egress(dtype):
    for case in EGRESS[dtype]():
        gots, _ = run_case(case)
        if dtype in edr.DTYPES and case.values.size >= len(edr.TRAPS[dtype]):
            # the hand-written patterns of the trap table, wherever fp32 delivers the trap itself
            traps = edr.trap_inputs(dtype)
            with np.errstate(over="ignore", under="ignore"):
                exact = traps.astype(np.float32).astype(np.float64) == traps
            exact |= np.isnan(traps)
            k = len(traps)
            if case.label.find("dense S=1") >= 0 and case.shifts[1] == 0:
                ok = edr.same_bits(gots[1][:k], edr.trap_bits(dtype), dtype)
                assert ok[exact].all(), "%s: trap table entries %s" % (case.label, np.flatnonzero(exact & ~ok))
                note(case.kernel, "trap table (hand-written bits)")


@pytest.mark.parametrize("dtype", DTYPES)
def test_emit(dtype):
    for case in EMIT[dtype]():
        run_case(case)


@pytest.mark.parametrize("key", sorted(LEVELS))
def test_levels(key):
    for case in LEVELS[key]():
        gots, _ = run_case(case)
        got = gots[8].reshape(case.shape)
        worst = lr.check(got, levels_want(case), case.label)
        note("devio_levels", "energies (levels_reference.check)", worst)
        note("devio_levels", "peaks and counts identical")
        again, _ = run_case(case)
        assert np.array_equal(again[8].view(np.uint64), gots[8].view(np.uint64)), case.label + ": two launches differ"
        note("devio_levels", "two launches, the same bits")


@pytest.mark.parametrize("C,n,lens", [(3, 9, [4, 9, 0]), (1, 4097, [4096, 1]), (3, 2 * 4096 + 5, [4097, 341]), (2, 8 * 4096 + 1, [8 * 4096, 4095])])
def test_a_ragged_clips_levels_are_the_one_clip_launch_of_that_length(C, n, lens):
    S = len(lens)
    ragged = levels_case("ragged", S, n, C, live_len=lens, seed=77, gain=("scalar", np.float32(0.5)))
    gots, _ = run_case(ragged)
    rec = gots[8].reshape(S, C, lr.FIELDS)
    lr.check(rec, levels_want(ragged), ragged.label)
    e = ragged.emission
    for s, length in enumerate(lens):
        if length == 0:
            assert not rec[s].any(), "an empty clip's record is zero"
            continue
        one = levels_case("one clip", 1, length, C, seed=77, gain=("scalar", np.float32(0.5)))
        o = one.emission
        for name in ("hi", "lo", "bg"):
            o[name][0] = e[name][s, :length]
        per = length * C
        one.arenas[0], one.arenas[1], one.arenas[2] = o["bg"].ravel(), o["hi"].ravel()[:per].copy(), o["lo"].ravel()[:per].copy()
        got, _ = run_case(one)
        assert np.array_equal(got[8].view(np.uint64), rec[s].ravel().view(np.uint64)), "clip %d of %s" % (s, ragged.label)
    note("devio_levels", "a ragged clip's record is the one-clip record (bits)")


@pytest.mark.parametrize("key", sorted(MOVE_IN))
def test_append_feed_take(key):
    for case in MOVE_IN[key]():
        run_case(case)


@pytest.mark.parametrize("key", sorted(MOVERS))
def test_movers(key):
    for case in MOVERS[key]():
        run_case(case)


@pytest.mark.parametrize("key", sorted(TABLES))
def test_tables_and_tail_clear(key):
    for case in TABLES[key]():
        run_case(case)


REFUSED = {
    "a source one element short": lambda c: c.arenas.__setitem__(0, c.arenas[0][:-1].copy()),
    "a destination one element short": lambda c: c.arenas.__setitem__(1, c.arenas[1][:-1].copy()),
    "an arena that is not there": lambda c: c.words.__setitem__(7, 9),
    "a negative element offset": lambda c: c.words.__setitem__(8, -1),
    "words that end early": lambda c: c.words.__delitem__(slice(10, None)),
    "a float arena 2 bytes off its alignment": lambda c: c.shifts.__setitem__(1, 2),
    "more samples than any arena holds": lambda c: c.words.__setitem__(2, 1 << 28),
    "a product of counts past int64": lambda c: (c.words.__setitem__(2, 1 << 28), c.words.__setitem__(3, 1 << 28)),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_stage_entry_refuses_what_would_index_out_of_range(what):
    case = ingest_case("float32", "padded", 2, 5, 3, 1)
    case.words = list(case.words)
    REFUSED[what](case)
    with pytest.raises(ValueError):
        repet._devio_stage(case.op, case.arenas, case.words, case.floats, case.shifts, PREFILL)


def refusals():
    """(label, case) pairs the entry must refuse, one per family of launchers: every one indexes outside an arena."""
    out = []
    c = append_cases()[0]
    c.words[-1] += 1000
    out.append(("append: d_off past the planes", c))
    c = feed_cases()[0]
    c.arenas[1] = c.arenas[1][:-1].copy()
    out.append(("feed: a ring plane short of its stride", c))
    c = take_cases()[0]
    c.arenas[4] = c.arenas[4][:-1].copy()
    out.append(("take: a table short of its slots", c))
    c = slide_cases()[0]
    c.words[5], c.words[16], c.words[17] = 0, -1, 0               # the first part's source at its arena's first float, delta in front of it
    out.append(("slide: a held source in front of its arena", c))
    c = slot_move_cases()[0]
    c.words[8], c.words[11] = 0, -1                               # the first part: src_off -1 from the arena's first float, zero_below 0
    out.append(("export: a negative offset that is read", c))
    c = slot_reset_case("bad id", 4, [3], 0, [])
    c.words[6] = 4
    out.append(("reset: a slot outside the table", c))
    c = table_cases()[0]
    c.words[4] = 300
    out.append(("slot set: a slot outside the table", c))
    c = table_cases()[0]
    c.words[3] = 1 << 27
    out.append(("slot set: more ids than words", c))
    c = take_cases()[0]
    c.words[0] = 1 << 27
    out.append(("take: more slots than words", c))
    c = band_cases()[0]
    c.arenas[1] = c.arenas[1].copy()
    c.arenas[1][0] = 5
    out.append(("band expand: a slot outside the table", c))
    c = emit_cases("float32")[0]
    c.words[4] += 1
    out.append(("emit: streams further apart than hi holds", c))
    c = tail_clear_cases()[0]
    c.words[2] += 1
    out.append(("tail clear: a frame more than X holds", c))
    return out


def test_every_family_refuses_an_arena_that_is_too_small():
    for label, case in refusals():
        with pytest.raises(ValueError):
            repet._devio_stage(case.op, case.arenas, case.words, case.floats, case.shifts, PREFILL)


def test_parity_record_and_the_decisions_seen():
    """Needs the whole module to have run before it, in one process: it reads what the tests above collected."""
    missing = [d for d in REQUIRED if d not in DECISIONS]
    lines = ["kernel | check | worst error / bar | launches checked"]
    lines += ["%s | %s | %.3f | %d" % (k, c, w, n) for (k, c), (w, n) in sorted(PARITY.items())]
    lines += ["", "launcher decisions seen (op, what, value):"] + ["%s | %s | %s" % d for d in sorted(DECISIONS, key=repr)]
    text = "\n".join(lines) + "\n"
    print(text)
    path = os.environ.get("REPET_DEVIO_STAGE_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            f.write(text)
    assert not missing, "launcher decisions never seen: %s" % missing
    grids = {c.expect["grid"] for c in row_copies_cases() if "grid-stride" in c.label}
    assert grids == {(12, 64, 5)}
