"""NumPy / Python reference of what the kernels of csrc/devio.hip must leave in memory, for tests/test_gpu_devio_stages.py: the
strided ingest, the egress and the emission with its gain fade, the signals the level reduction measures, the rows of the
spectra ``tail_clear`` zeroes, the live handle's per-push data movement and its gain and band tables. Written from what
csrc/engine.h and include/repet_hip.h promise, not from the kernels: no slots of four, no vector paths, no grid -- every function
is an index computation on whole arrays, and the two fused multiply-adds of a fade are exact rational arithmetic rounded once.
Checked on the CPU by tests/test_devio_reference.py.

Buffers are flat NumPy arrays as the device holds them. A function that writes takes the buffer's content before the launch and
returns its content after it, so a caller that compares whole buffers also checks every cell the launch must leave alone."""
from fractions import Fraction

import numpy as np

import emit_dtypes_reference as edr

IDLE = 1 << 60               # kSlotIdle: a slot without a stream
HELD = IDLE + 1              # kSlotHeld: a slot that sits pushes out
DTYPE_CODES = {"float32": 0, "float64": 1, "int16": 2, "float16": 3, "bfloat16": 4}        # REPET_F32 ..
STORAGE = {"float32": np.float32, "float64": np.float64, "int16": np.int16, "float16": np.float16, "bfloat16": np.uint16}
BACKGROUND, FOREGROUND, MIXTURE = 0, 1, 2                                                # REPET_OUT_*
BAND_CARRIED, BAND_NEW, BAND_PENDING, BAND_ROWS = 0, 1, 2, 3
BAND_COMMIT, BAND_SETTLE, BAND_CARRY = 0, 1, 2
LEVEL_CHUNK = 4096           # REPET_LEVEL_CHUNK


# ---- layouts -------------------------------------------------------------------------------------------------------------
def strided_index(shape, strides, base=0):
    """The flat element index of every (clip, sample, channel) of a strided ``shape`` = (B, n, C)."""
    b, n, c = (np.arange(k, dtype=np.int64) for k in shape)
    return base + b[:, None, None] * strides[0] + n[None, :, None] * strides[1] + c[None, None, :] * strides[2]


def strided_span(shape, strides):
    """One past the largest index ``strided_index`` reaches (base 0)."""
    return int(sum(st * (k - 1) for st, k in zip(strides, shape)) + 1) if all(k > 0 for k in shape) else 0


# ---- conversions ---------------------------------------------------------------------------------------------------------
def widen(x, dtype):
    """Stored samples of ``dtype`` (bfloat16: uint16 patterns) as the values they stand for: float64 for float64, else float32 --
    every 16-bit type and int16 widens exactly."""
    x = np.asarray(x)
    if dtype == "bfloat16":
        return (x.astype(np.uint32) << np.uint32(16)).view(np.float32)
    if dtype == "float64":
        return x.astype(np.float64)
    return x.astype(np.float32)


@np.errstate(over="ignore", invalid="ignore")
def split(x, dtype):
    """(hi, lo) fp32 of stored samples: hi = float32(x), lo = float32(x - float64(hi)) for float64, 0 for the other types."""
    v = widen(x, dtype)
    if dtype != "float64":
        return v, np.zeros(v.shape, dtype=np.float32)
    hi = v.astype(np.float32)
    return hi, (v - hi.astype(np.float64)).astype(np.float32)


def narrow(v, dtype):
    """float64 values -> what a destination of ``dtype`` stores (bfloat16: uint16 patterns), rounded once."""
    v = np.asarray(v, dtype=np.float64)
    if dtype == "float64":
        return v.copy()
    if dtype == "float32":
        with np.errstate(over="ignore", invalid="ignore"):
            return v.astype(np.float32)
    return edr.round_ref(v, dtype).reshape(v.shape)


# ---- ingest ---------------------------------------------------------------------------------------------------------------
def ingest(x, dtype, lengths=None):
    """``x`` (B, n, C) stored samples -> (hi, lo, flag): the fp32 planes (B, n, C) -- ``lo`` None unless float64, the plane is
    not written then -- and the non-finite flag. Clip b is live below sample ``lengths[b]``: a dead sample is +0 in both planes
    and is not looked at. The flag is set exactly when a live float sample is NaN or infinite: judged on the sample itself, so
    not by a finite double beyond float32's range, and never by int16."""
    B, n, C = x.shape
    hi, lo = split(x, dtype)
    live = np.ones((B, n), dtype=bool) if lengths is None else np.arange(n)[None, :] < np.asarray(lengths)[:, None]
    on = np.broadcast_to(live[:, :, None], x.shape)
    hi, lo = np.where(on, hi, np.float32(0)), np.where(on, lo, np.float32(0))
    flag = 0 if dtype == "int16" else int(np.any(~np.isfinite(widen(x, dtype)) & on))
    return hi, (lo if dtype == "float64" else None), flag


# ---- emission -------------------------------------------------------------------------------------------------------------
def fma_once(a, b, c):
    """a * b + c of three float64 values, rounded once."""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))              # NaN and infinities: no rounding to get wrong
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        # an exact zero: the sum of two zeros keeps their common sign, everything else that cancels is +0
        return a * b + c if (a == 0 or b == 0) else 0.0
    try:
        return float(exact)                                       # (a Fraction converts correctly rounded, subnormals included)
    except OverflowError:
        return np.inf if exact > 0 else -np.inf


def liveness(shape, table=None, pos0=0, hop=1, live_len=None):
    """(S, n) booleans: sample j of stream s is live when the slot has a stream (its first frame is below IDLE) and handle
    sample pos0 + j lies at or behind slot_start[s] * hop, and, for a ragged batch, j < live_len[s]."""
    S, n = shape
    j = np.arange(n, dtype=object)
    live = np.ones((S, n), dtype=bool)
    if table is not None:
        for s in range(S):
            start = int(table[s])
            live[s] = False if start >= IDLE else np.array([pos0 + int(q) >= start * hop for q in j], dtype=bool)
    if live_len is not None:
        live &= np.arange(n)[None, :] < np.asarray(live_len)[:, None]
    return live


@np.errstate(invalid="ignore", over="ignore")
def emit_signals(hi, lo, bg, bg_fg=None, table=None, pos0=0, hop=1, live_len=None, gain=None):
    """The three float64 signals (mix, bgv, fgv), each (S, n, C), and the liveness (S, n).
    ``hi`` / ``lo`` / ``bg`` / ``bg_fg`` fp32 (S, n, C), ``lo`` and ``bg_fg`` None where absent. ``gain``: None, ("scalar", a) or
    ("tables", a_cur, a_tgt, ramp) with fp32 values; a_cur None with ramp 0."""
    hi = np.asarray(hi, dtype=np.float32)
    S, n, C = hi.shape
    h = hi.astype(np.float64)
    x = h
    if lo is not None:
        l = np.asarray(lo, dtype=np.float32).astype(np.float64)
        x = np.where(~np.isinf(h) & (l != 0), h + l, h)           # an infinite hi stays hi; a zero remainder adds nothing
    b = np.asarray(bg, dtype=np.float32).astype(np.float64)
    bf = b if bg_fg is None else np.asarray(bg_fg, dtype=np.float32).astype(np.float64)
    if gain is None:
        fg = x - bf
    elif gain[0] == "scalar":
        fg = x - np.float64(np.float32(gain[1])) * bf             # (the product of two fp32 values is exact in float64)
    else:
        _, a_cur, a_tgt, ramp = gain
        at = np.asarray(a_tgt, dtype=np.float32).astype(np.float64)
        fg = x - at[:, None, None] * bf
        for s in range(S if ramp > 0 else 0):
            ac = float(np.float64(np.float32(a_cur[s])))
            if ac == at[s]:
                continue                                          # equal entries fade nowhere
            d = float(np.float64(at[s]) - np.float64(ac))         # (one IEEE subtraction)
            for j in range(min(n, ramp - 1)):                     # j + 1 < ramp
                ak = fma_once(d, float(j + 1) / float(ramp), ac)
                for c in range(C):
                    fg[s, j, c] = fma_once(-ak, bf[s, j, c], x[s, j, c])
    live = liveness((S, n), table, pos0, hop, live_len)
    on = np.broadcast_to(live[:, :, None], hi.shape)
    return np.where(on, x, 0.0), np.where(on, b, 0.0), np.where(on, fg, 0.0), live


def emit(which, dtype, *args, **kwargs):
    """What a destination of ``dtype`` taking signal ``which`` stores, (S, n, C)."""
    mix, bgv, fgv, _ = emit_signals(*args, **kwargs)
    return narrow({BACKGROUND: bgv, FOREGROUND: fgv, MIXTURE: mix}[which], dtype)


def egress(values, dtype):
    """fp32 values -> what a destination of ``dtype`` stores."""
    return narrow(np.asarray(values, dtype=np.float32).astype(np.float64), dtype)


# ---- tail clear -------------------------------------------------------------------------------------------------------------
def frame_count(n, W, H):
    """Frames of an uncentred STFT of n samples: ceil((n - W) / H) + 1, none below zero."""
    return max(0, -((W - n) // H) + 1)


def tail_clear(X, Mk, spec_stride, chan_stride, n_clips, C, T, FS, W, H, lengths):
    """Rows [T_b, T) of every clip's and channel's plane are zero in X (complex64, flat) and, where given, Mk (fp32, flat)."""
    X, Mk = X.copy(), None if Mk is None else Mk.copy()
    for b in range(n_clips):
        tb = frame_count(int(lengths[b]), W, H)
        for c in range(C):
            lo, hi = b * spec_stride + c * chan_stride + min(tb, T) * FS, b * spec_stride + c * chan_stride + T * FS
            X[lo:hi] = 0
            if Mk is not None:
                Mk[lo:hi] = 0
    return X, Mk


# ---- the live handle's data movement ----------------------------------------------------------------------------------------
def append(hi, lo, x, dtype, d_stream, d_off):
    """Stream b's chunk ``x[b]`` (n, C) goes to both planes at b * d_stream + d_off as fp32 + fp32 remainder."""
    hi, lo = hi.copy(), lo.copy()
    h, l = split(x, dtype)
    per = x.shape[1] * x.shape[2]
    for b in range(x.shape[0]):
        hi[b * d_stream + d_off:b * d_stream + d_off + per] = h[b].ravel()
        lo[b * d_stream + d_off:b * d_stream + d_off + per] = l[b].ravel()
    return hi, lo


def feed(hi, lo, x, dtype, slots, counts, wpos, ring_stride, ring_len):
    """Row r of ``x`` (rows, n, C) brings its first counts[r] samples to the ring of slots[r], from float wpos[r] on, wrapping."""
    hi, lo = hi.copy(), lo.copy()
    h, l = split(x, dtype)
    C = x.shape[2]
    for r in range(x.shape[0]):
        k = int(counts[r]) * C
        at = int(slots[r]) * ring_stride + (int(wpos[r]) + np.arange(k)) % ring_len
        hi[at] = h[r].ravel()[:k]
        lo[at] = l[r].ravel()[:k]
    return hi, lo


def take(dst_hi, dst_lo, hi, lo, table, rpos, length, ring_stride, ring_len, d_stream, d_off):
    """``length`` floats of both planes from float rpos[b] of slot b's ring go to b * d_stream + d_off, but for the slots that
    read idle or held in the table."""
    dst_hi, dst_lo = dst_hi.copy(), dst_lo.copy()
    for b in range(len(rpos)):
        if int(table[b]) >= IDLE:
            continue
        at = b * ring_stride + (int(rpos[b]) + np.arange(length)) % ring_len
        dst_hi[b * d_stream + d_off:b * d_stream + d_off + length] = hi[at]
        dst_lo[b * d_stream + d_off:b * d_stream + d_off + length] = lo[at]
    return dst_hi, dst_lo


def move_runs(dst, dst_base, src, src_base, length, blocks, src_block, dst_block, zero_below=0):
    """In place: element i < length of run blk is src[src_base + blk * src_block + i] for i >= zero_below and zero below it
    (``src`` None: zero everywhere); nothing at or behind ``length``."""
    i = np.arange(max(0, length))
    for blk in range(blocks):
        v = np.zeros(len(i), dtype=np.float32)
        if src is not None:
            copied = i >= zero_below
            v[copied] = src[src_base + blk * src_block + i[copied]]
        dst[dst_base + blk * dst_block + i] = v


def row_copies(parts, n_streams, table=None):
    """``parts``: dicts of dst, src (None: zeros), dst_off, src_off, len, blocks, src_block, dst_block, src_stream, dst_stream,
    row_len, frame0. Of a part with row_len > 0 stream b takes only the rows of frames before slot_start[b] (no table: none).
    Returns the destinations after the launch, one per part."""
    outs = []
    for p in parts:
        dst = p["dst"].copy()
        for b in range(n_streams):
            length = p["len"]
            if p["row_len"] > 0:
                rows = int(table[b]) - p["frame0"] if table is not None else 0
                length = 0 if rows <= 0 else rows * p["row_len"] if rows < p["len"] // p["row_len"] else p["len"]
            move_runs(dst, p["dst_off"] + b * p["dst_stream"], p["src"], p["src_off"] + b * p["src_stream"], length, p["blocks"],
                      p["src_block"], p["dst_block"])
        outs.append(dst)
    return outs


def slide_held(parts, n_streams, table):
    """The row copies, except that a stream whose entry is HELD takes element i of a run from ``delta`` floats further on for
    i >= zero_below and zero below it."""
    outs = []
    for p in parts:
        dst = p["dst"].copy()
        for b in range(n_streams):
            held = int(table[b]) == HELD
            move_runs(dst, p["dst_off"] + b * p["dst_stream"], p["src"], p["src_off"] + b * p["src_stream"] + (p["delta"] if held else 0),
                      p["len"], p["blocks"], p["src_block"], p["dst_block"], min(p["zero_below"], p["len"]) if held else 0)
        outs.append(dst)
    return outs


def slot_set(table, slots, values):
    table = table.copy()
    table[np.asarray(slots, dtype=np.int64)] = np.asarray(values, dtype=np.int64)
    return table


def slot_reset(table, value, slots, parts):
    """slot_start[slot] = value and runs of zeros in every named slot's share: ``parts`` dicts of dst, dst_off, len, blocks,
    dst_block, dst_stream. Returns (table, destinations)."""
    table = slot_set(table, slots, [value] * len(slots))
    outs = []
    for p in parts:
        dst = p["dst"].copy()
        for b in slots:
            move_runs(dst, p["dst_off"] + int(b) * p["dst_stream"], None, 0, p["len"], p["blocks"], 0, p["dst_block"])
        outs.append(dst)
    return table, outs


def slot_move(parts):
    """Export and import: ``parts`` dicts of dst, dst_off, src (None: zeros), src_base (the source pointer's element), src_off
    (may be negative), len, blocks, src_block, dst_block, zero_below."""
    outs = []
    for p in parts:
        dst = p["dst"].copy()
        move_runs(dst, p["dst_off"], p["src"], p["src_base"] + p["src_off"], p["len"], p["blocks"], p["src_block"], p["dst_block"],
                  min(p["zero_below"], p["len"]))
        outs.append(dst)
    return outs


def import_table(table, slot, value, shift):
    """The import writes the slot's first frame and adds ``shift`` to the first frame of every other live slot."""
    out = table.copy()
    for s in range(len(out)):
        if s == slot:
            out[s] = value
        elif shift != 0 and int(out[s]) < IDLE:
            out[s] += shift
    return out


# ---- gain and band tables ----------------------------------------------------------------------------------------------------
def gain_fill(table, n, a):
    table = table.copy()
    table[:n] = np.float32(a)
    return table


def gain_set(tgt, slots, a):
    tgt = tgt.copy()
    tgt[np.asarray(slots, dtype=np.int64)] = np.asarray(a, dtype=np.float32)
    return tgt


def gain_commit(tgt, cur_old, cur_new, n, slot):
    """cur_new[s] = tgt[s] for the slot named (slot < 0: all), cur_old[s] for the others."""
    out = cur_new.copy()
    s = np.arange(n)
    out[:n] = np.where((slot < 0) | (s == slot), tgt[:n], cur_old[:n])
    return out


def band_expand(tab, FS, F, slots, rows_of, edges, gains, init):
    """``tab`` flat (n_slots, 3, FS) fp32. The pending row of every named slot: float32(1 - float64(g)) of the band
    [edges[b], edges[b + 1]) that holds the bin, g = 0 outside every band, in pad bins and for a slot whose row is not one of
    ``gains`` (rows, n_bands). ``init``: the other two rows of the named slots become 1."""
    out = tab.copy().reshape(-1, BAND_ROWS, FS)
    gains = np.asarray(gains, dtype=np.float32)
    for slot, r in zip(slots, rows_of):
        g = np.zeros(FS, dtype=np.float32)
        if 0 <= r < gains.shape[0]:
            for b in range(len(edges) - 1):
                lo, hi = max(0, int(edges[b])), min(F, int(edges[b + 1]))
                if lo < hi:
                    g[lo:hi] = gains[r, b]
        out[slot, BAND_PENDING] = (1.0 - g.astype(np.float64)).astype(np.float32)
        if init:
            out[slot, BAND_CARRIED] = 1
            out[slot, BAND_NEW] = 1
    return out.reshape(-1)


def band_commit(tab, FS, n_slots, slot, mode, table=None):
    """commit: carried = new, new = pending. settle: carried = new = pending. carry: carried = new. Every slot that is not held
    (slot < 0), or the one slot named."""
    out = tab.copy().reshape(-1, BAND_ROWS, FS)
    for s in (range(n_slots) if slot < 0 else [slot]):
        if slot < 0 and table is not None and int(table[s]) == HELD:
            continue
        pending, new = out[s, BAND_PENDING].copy(), out[s, BAND_NEW].copy()
        out[s, BAND_CARRIED] = pending if mode == BAND_SETTLE else new
        if mode != BAND_CARRY:
            out[s, BAND_NEW] = pending
    return out.reshape(-1)
