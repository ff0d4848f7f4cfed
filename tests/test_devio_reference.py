"""tests/devio_reference.py on the CPU: the reference the GPU stage tests hold the kernels of csrc/devio.hip to
(tests/test_gpu_devio_stages.py) against hand-worked values and independent formulations, and every case of that module built
here, with the premises its docstring and the issue behind it promise: the shapes, alignment classes and launcher decisions the
cases are there to reach are reached by construction, not by accident."""
import math
from fractions import Fraction

import numpy as np
import pytest

import devio_reference as ref
import emit_dtypes_reference as edr
import levels_reference as lr
import test_gpu_devio_stages as gpu

IDLE, HELD = ref.IDLE, ref.HELD


# ---- the reference itself -------------------------------------------------------------------------------------------------
def test_split_is_the_nearest_fp32_and_the_fp32_of_what_is_left():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(4000) * 10.0 ** rng.uniform(-20, 20, 4000)
    hi, lo = ref.split(x, "float64")
    assert hi.dtype == lo.dtype == np.float32
    # hi is a nearest fp32: no neighbour is closer
    for step in (np.float32(np.inf), np.float32(-np.inf)):
        other = np.nextafter(hi, step).astype(np.float64)
        assert np.all(np.abs(x - hi.astype(np.float64)) <= np.abs(x - other))
    # the two planes carry 48 bits of the sample
    assert np.all(np.abs(x - (hi.astype(np.float64) + lo.astype(np.float64))) <= 2.0 ** -47 * np.abs(x))
    # the wide ends: beyond float32 hi is infinite and the remainder its opposite; an infinite sample has a NaN remainder
    hi, lo = ref.split(np.array([1e300, -1e300, np.inf, np.nan, 0.0, -0.0]), "float64")
    assert hi[0] == np.inf and lo[0] == -np.inf and hi[1] == -np.inf and lo[1] == np.inf
    assert hi[2] == np.inf and np.isnan(lo[2]) and np.isnan(hi[3]) and np.isnan(lo[3])
    assert not np.signbit(hi[4]) and np.signbit(hi[5]) and not lo[4] and not lo[5]


@pytest.mark.parametrize("dtype", ("int16", "float16", "bfloat16"))
def test_the_16_bit_types_widen_exactly(dtype):
    every = np.arange(65536, dtype=np.uint16)
    stored = every.view(ref.STORAGE[dtype]) if dtype != "bfloat16" else every
    hi, lo = ref.split(stored, dtype)
    assert not lo.any() and hi.dtype == np.float32
    with np.errstate(invalid="ignore"):
        back = ref.narrow(hi.astype(np.float64), dtype)
    number = ~np.isnan(hi)
    assert edr.same_bits(back, stored, dtype)[number].all()       # what widens exactly narrows back to itself
    assert np.isnan(edr.decode(back, dtype)[~number]).all()


def test_the_ingest_flag_looks_at_live_float_samples_alone():
    x = np.ones((2, 4, 3))
    assert ref.ingest(x, "float64")[2] == 0
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1, 3, 2] = bad
        assert ref.ingest(y, "float64")[2] == 1
        assert ref.ingest(y, "float64", [4, 3])[2] == 0           # behind its clip's length
        assert ref.ingest(y, "float64", [0, 4])[2] == 1
        assert ref.ingest(y.astype(np.float32), "float32")[2] == 1
        assert ref.ingest(y.astype(np.float16), "float16")[2] == 1
    y = x.copy()
    y[0, 0, 0] = 1e300                                            # finite, though its fp32 is not
    hi, lo, flag = ref.ingest(y, "float64")
    assert flag == 0 and hi[0, 0, 0] == np.inf and lo[0, 0, 0] == -np.inf
    assert ref.ingest(np.full((1, 3, 1), -32768, dtype=np.int16), "int16")[2] == 0
    hi, lo, _ = ref.ingest(np.full((2, 4, 3), np.nan), "float64", [1, 0])
    assert np.isnan(hi[0, 0]).all() and not hi[0, 1:].view(np.uint32).any() and not lo[1].view(np.uint32).any()      # dead: +0 in both planes
    assert ref.ingest(x.astype(np.float32), "float32")[1] is None


def test_fma_once_rounds_once():
    e = 2.0 ** -30
    assert ref.fma_once(1 + e, 1 + e, -1.0) == 2.0 ** -29 + 2.0 ** -60      # (two roundings give 2^-29)
    assert (1 + e) * (1 + e) - 1.0 == 2.0 ** -29
    rng = np.random.default_rng(2)
    for a, b, c in rng.standard_normal((300, 3)) * 10.0 ** rng.uniform(-3, 3, (300, 3)):
        r = ref.fma_once(a, b, c)
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        assert abs(Fraction(r) - exact) <= min(abs(Fraction(np.nextafter(r, np.inf)) - exact), abs(Fraction(np.nextafter(r, -np.inf)) - exact))
        assert ref.fma_once(a, b, -a * b) == float(Fraction(a) * Fraction(b) - Fraction(a * b))      # the error of a product, exactly
    sign = lambda v: math.copysign(1.0, v)
    assert sign(ref.fma_once(-0.0, 5.0, -0.0)) == -1 and sign(ref.fma_once(0.0, 5.0, -0.0)) == 1 and sign(ref.fma_once(3.0, 2.0, -6.0)) == 1
    assert ref.fma_once(1e308, 10.0, 0.0) == np.inf and ref.fma_once(-1e308, 10.0, 0.0) == -np.inf
    assert np.isnan(ref.fma_once(np.inf, 0.0, 1.0)) and ref.fma_once(np.inf, 1.0, 1.0) == np.inf
    assert ref.fma_once(2.0 ** -600, 2.0 ** -600, 0.0) == 0.0 and ref.fma_once(2.0 ** -537, 2.0 ** -537, 0.0) == 2.0 ** -1074


def test_the_emission_on_hand_worked_samples():
    f = np.float32
    hi = np.array([[[1.0], [-0.0], [np.inf], [2.0], [4.0]]], dtype=f)
    lo = np.array([[[2.0 ** -30], [0.0], [np.nan], [0.0], [-(2.0 ** -28)]]], dtype=f)
    bg = np.array([[[0.5], [0.0], [1.0], [3.0], [1.0]]], dtype=f)
    mix, bgv, fgv, live = ref.emit_signals(hi, lo, bg)
    assert mix[0, 0, 0] == 1 + 2.0 ** -30 and np.signbit(mix[0, 1, 0]) and mix[0, 2, 0] == np.inf and mix[0, 4, 0] == 4 - 2.0 ** -28
    assert fgv[0, 0, 0] == 0.5 + 2.0 ** -30 and fgv[0, 3, 0] == -1.0 and np.array_equal(bgv[0, :, 0], [0.5, 0, 1, 3, 1]) and live.all()
    # a scalar gain: x - a * bg with a the fp32 value
    a = f(0.3)
    _, _, fgv, _ = ref.emit_signals(hi, lo, bg, gain=("scalar", a))
    assert fgv[0, 3, 0] == 2.0 - float(a) * 3.0 and fgv[0, 0, 0] == float(Fraction(1 + 2.0 ** -30) - Fraction(float(a)) * Fraction(0.5))
    # the fade: sample j takes a_cur + (a_tgt - a_cur) (j + 1) / ramp while j + 1 < ramp, a_tgt from there on
    cur, tgt = np.array([1.0], dtype=f), np.array([0.25], dtype=f)
    _, _, fgv, _ = ref.emit_signals(hi, None, bg, gain=("tables", cur, tgt, 4))
    want = [1.0 - (1 - 0.75 * 0.25) * 0.5, -0.0 - (1 - 0.75 * 0.5) * 0.0, np.inf, 2.0 - 0.25 * 3.0, 4.0 - 0.25]
    assert np.array_equal(fgv[0, :, 0], want)
    for ramp in (0, 1):
        _, _, fgv, _ = ref.emit_signals(hi, None, bg, gain=("tables", cur if ramp else None, tgt, ramp))
        assert fgv[0, 0, 0] == 1.0 - 0.25 * 0.5
    # the shaped background shows in the foreground alone
    mix2, bgv2, fgv2, _ = ref.emit_signals(hi, lo, bg, bg_fg=bg * f(2))
    assert np.array_equal(mix2, mix, equal_nan=True) and np.array_equal(bgv2, bgv) and fgv2[0, 3, 0] == 2.0 - 6.0
    # liveness: slot_start * hop against pos0 + j; an idle or held slot never; a ragged clip below its length; dead is +0 everywhere
    live = ref.liveness((4, 5), [0, IDLE, 11, HELD], 41, 4)
    assert live[0].all() and not live[1].any() and np.array_equal(live[2], [False, False, False, True, True]) and not live[3].any()
    assert np.array_equal(ref.liveness((2, 3), None, 0, 1, [2, 0]), [[True, True, False], [False, False, False]])
    mix, bgv, fgv, _ = ref.emit_signals(np.full((1, 2, 1), np.nan, dtype=f), None, np.full((1, 2, 1), np.nan, dtype=f), table=[IDLE])
    assert not (mix.view(np.uint64).any() or bgv.view(np.uint64).any() or fgv.view(np.uint64).any())


def test_narrow_is_round_ref_and_the_cpp_conversions():
    for dtype in edr.DTYPES:
        assert edr.same_bits(ref.narrow(edr.trap_inputs(dtype), dtype), edr.trap_bits(dtype), dtype).all()
    v = np.array([1 + 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, 1e300, -0.0])
    assert np.array_equal(ref.narrow(v, "float32"), np.array([1.0, 1 + 2.0 ** -23, np.inf, -0.0], dtype=np.float32))
    assert ref.narrow(v, "float64") is not v and np.array_equal(ref.narrow(v, "float64"), v)


def test_frame_count_is_the_librarys():
    lib = gpu.repet._native.lib()
    for W, H in ((64, 32), (64, 16), (128, 100)):
        for n in range(0, 5 * W):
            assert ref.frame_count(n, W, H) == max(0, lib.repet_frame_count(n, W, H, 0)), (n, W, H)


def test_the_movers_on_hand_worked_buffers():
    f = np.float32
    src = np.arange(100, dtype=f)
    dst = np.full(40, -1, dtype=f)
    ref.move_runs(dst, 2, src, 10, 5, 2, 20, 8, zero_below=2)
    assert np.array_equal(dst[:16], [-1, -1, 0, 0, 12, 13, 14, -1, -1, -1, 0, 0, 32, 33, 34, -1])
    ref.move_runs(dst, 0, None, 0, 3, 1, 0, 0)
    assert np.array_equal(dst[:4], [0, 0, 0, 0])
    # a ring wraps modulo its length, and what lies behind a count is not brought
    hi, lo = ref.feed(np.full(24, -1, dtype=f), np.full(24, -1, dtype=f), np.arange(1, 7, dtype=np.float64).reshape(1, 6, 1), "float64", [1], [5], [9], 12, 11)
    assert np.array_equal(hi[12:], [3, 4, 5, -1, -1, -1, -1, -1, -1, 1, 2, -1]) and not lo[[21, 22, 12, 13, 14]].any() and lo[23] == -1
    ring = np.arange(24, dtype=f)
    dh, dl = ref.take(np.full(16, -1, dtype=f), np.full(16, -1, dtype=f), ring, ring + 100, [3, HELD], [9, 0], 4, 12, 11, 8, 1)
    assert np.array_equal(dh, [-1, 9, 10, 0, 1, -1, -1, -1] + [-1] * 8) and np.array_equal(dl[1:5], [109, 110, 100, 101])
    # frame rows: only the rows of frames before the slot's own first frame
    part = dict(dst=np.full(30, -1, dtype=f), src=src, dst_off=0, src_off=0, len=6, blocks=1, src_block=0, dst_block=0, src_stream=10, dst_stream=10,
                row_len=2, frame0=5)
    out, = ref.row_copies([part], 3, [5, 6, 20])
    assert np.array_equal(out[:10], [-1] * 10) and np.array_equal(out[10:20], [10, 11] + [-1] * 8) and np.array_equal(out[20:26], src[20:26])
    part.update(delta=-2, zero_below=3, row_len=0)
    out, = ref.slide_held([part], 2, [HELD, 7])
    assert np.array_equal(out[:7], [0, 0, 0, 1, 2, 3, -1]) and np.array_equal(out[10:16], src[10:16])
    assert np.array_equal(ref.import_table(np.array([3, IDLE, HELD, 7]), 1, 9, -2), [1, 9, HELD, 5])
    # band tables
    tab = ref.band_expand(np.full(2 * 3 * 8, -1, dtype=f), 8, 6, [1], [0], [1, 3, 5], [[0.25, 1.0]], True)
    assert np.array_equal(tab[24:], [1] * 16 + [1, 0.75, 0.75, 0, 0, 1, 1, 1]) and np.all(tab[:24] == -1)
    t = np.arange(24, dtype=f)
    assert np.array_equal(ref.band_commit(t, 4, 2, 1, ref.BAND_COMMIT)[12:], [16, 17, 18, 19, 20, 21, 22, 23, 20, 21, 22, 23])
    assert np.array_equal(ref.band_commit(t, 4, 2, 0, ref.BAND_SETTLE)[:12], [8, 9, 10, 11] * 3)
    assert np.array_equal(ref.band_commit(t, 4, 2, -1, ref.BAND_CARRY, [HELD, 0]), list(range(12)) + [16, 17, 18, 19] + list(range(16, 24)))


def test_the_levels_of_an_emission_come_from_its_signals():
    e = gpu.emission(2, 7, 3, 5, table=[IDLE, 0], gain=("scalar", np.float32(0.5)))
    mix, bgv, fgv, live = gpu.signals(e, 0, 1)
    rec = lr.levels(mix, bgv, fgv, live)
    assert not rec[0].any() and np.all(rec[1, :, lr.LIVE] == 7)


# ---- the cases of the GPU module ---------------------------------------------------------------------------------------------
def built(group):
    return {key: fn() for key, fn in gpu.GROUPS[group].items()}


def common_premises(cases):
    for c in cases:
        assert 1 <= len(c.arenas) <= 16 and len(c.shifts) == len(c.arenas) and all(s in (0, 2, 4, 8, 12) for s in c.shifts), c.label
        assert all(isinstance(w, (int, np.integer)) for w in c.words), c.label
        assert c.op in gpu.repet.DEVIO_OPS
    assert len({c.label for c in cases}) == len(cases), "two cases of one name"


def predicted(cases):
    seen = set()
    for c in cases:
        for field in ("dense", "src_vec", "dst_vec", "held_vec"):
            seen |= {(c.op, field, v) for v in c.expect.get(field, ()) if v >= 0}
        seen |= {(c.op, "src_vec,dst_vec", (s, d)) for s, d in zip(c.expect.get("src_vec", ()), c.expect.get("dst_vec", ())) if s >= 0}
        if "launches" in c.expect:
            seen.add((c.op, "launches", c.expect["launches"]))
    return seen


def test_ingest_cases():
    groups = built("ingest")
    for dtype in gpu.DTYPES:
        equal = groups["equal-" + dtype]
        common_premises(equal + groups["ragged-" + dtype] + groups["flags-" + dtype])
        assert len(equal) == 4 * 3 * len(gpu.INGEST_COUNTS)
        for c in equal:
            assert c.flag == 0 and ("dense_off1" not in c.label or c.expect["dense"][0] == 0)
        assert {c.expect["dense"][0] for c in equal} == {0, 1}
        assert any(c.expect["grid"][0] == 1 for c in equal) and any(c.expect["grid"][0] == 2 for c in equal)      # either side of 1024 elements
        ragged = groups["ragged-" + dtype]
        lens = set()
        for c in ragged:
            B, n, C = c.x.shape
            lens |= {("0", "1", "n-1", "n").index(k) for k, v in (("0", 0), ("1", 1), ("n-1", n - 1), ("n", n)) if v in c.lengths}
            assert c.flag == 0
            if dtype != "int16":
                w = ref.widen(c.x, dtype)
                assert all(np.isnan(w[b, c.lengths[b]:]).all() for b in range(B)), "the source behind a length holds NaN"
        assert lens == {0, 1, 2, 3}
        assert any(c.x.shape[2] == 3 and (c.x.shape[1] * 3) % 4 for c in ragged)                     # a run of four spans two clips
        flags = groups["flags-" + dtype]
        assert {c.flag for c in flags} == ({0} if dtype == "int16" else {0, 1})
        assert {c.expect["dense"][0] for c in flags} == {0, 1}


def test_egress_cases():
    for dtype, cases in built("egress").items():
        common_premises(cases)
        e, wg = gpu.ept(dtype), gpu.ept(dtype) * 256
        counts = {c.values.size for c in cases}
        assert {e - 1, e, e + 1, wg - 1, wg, wg + 1} - {0} <= counts
        assert {c.expect["dense"][0] for c in cases} == {0, 1}
        assert all(c.expect["dense"][0] == 0 for c in cases if c.shifts[1] == 2) and (dtype not in edr.DTYPES or any(c.shifts[1] == 2 for c in cases))
        if dtype in edr.DTYPES:
            assert any(c.values.size >= len(edr.TRAPS[dtype]) for c in cases)


def test_emit_and_levels_cases():
    for dtype, cases in built("emit").items():
        common_premises(cases)
        assert {c.expect["dense"] for c in cases} >= {(1, -1), (0, -1), (1, 0), (0, 1)}
        assert any(c.expect["grid"][0] >= 3 for c in cases)
        assert sum("the last sample of a fade" in c.label for c in cases) == 2
    # what tells the end of a fade from its inside: a_cur + (a_tgt - a_cur) in float64 is not a_tgt for these tables
    for cur, tgt in zip(gpu.FAR_CUR, gpu.FAR_TGT):
        assert float(np.float32(tgt)) == tgt and cur + (tgt - cur) != tgt
    for cur, tgt in zip(gpu.A_CUR, gpu.A_TGT):
        c, t = float(np.float32(cur)), float(np.float32(tgt))
        assert c + (t - c) == t                                   # ... and is for gains a handle can hold
    levels = built("levels")
    for key, cases in levels.items():
        common_premises(cases)
    for C in (1, 2, 3, 5):
        assert gpu.level_tile(C) == {1: 1024, 2: 1024, 3: 1020, 5: 1020}[C]
        assert [c.emission["n"] for c in levels["sizes-C%d" % C]] == [1, gpu.level_tile(C) // C, gpu.level_tile(C) // C + 1, 4095, 4096, 4097, 32769]
        assert any(c.words[9] % 4 for c in levels["sizes-C%d" % C]), "hi misaligned (word 9: the element offset of hi)"
    assert {1, 2} == {c.expect["launches"] for cs in levels.values() for c in cs}


def test_append_feed_take_cases():
    groups = built("move_in")
    for cases in groups.values():
        common_premises(cases)
    for C in (1, 3):
        classes = {c.classes for c in groups["append"] if c.words[3] == C}
        assert classes == {(a, b) for a in range(4) for b in range(4)}
    assert {c.kernel for c in groups["append"]} == {"online_append_float64", "online_append_int16"}
    feeds = groups["feed"]
    cut, wpos_low, exact, counts = set(), set(), False, set()
    for c in feeds:
        assert c.ring_stride >= c.ring_len + 1 and c.ring_stride % 4 == 0
        for slot, count, w in c.rows:
            length = count * c.C
            counts.add("0" if count == 0 else "n" if count == c.words[2] else "some")
            wpos_low.add(w & 3)
            exact |= length > 0 and w + length == c.ring_len
            if w + length > c.ring_len:
                # the aligned slot of four that holds the ring's last float: how many of its floats lie in front of the wrap
                cut.add(c.ring_len - (c.ring_len & ~3))
    assert cut >= {1, 2, 3} and wpos_low == {0, 1, 2, 3} and exact and counts >= {"0", "n"}
    assert any(len(c.rows) == 257 and c.expect["launches"] == 2 for c in feeds)
    takes = groups["take"]
    assert {c.ring_len % 4 for c in takes} == {0, 1, 2, 3} and {c.d_off & 3 for c in takes} == {0, 1, 2, 3}
    assert all(IDLE in c.table and HELD in c.table for c in takes)
    assert any(r & 3 for c in takes for r in c.rpos) and any(not r & 3 for c in takes for r in c.rpos)
    assert any(r + c.length > c.ring_len for c in takes for r in c.rpos) and any(len(c.rpos) == 257 for c in takes)


def test_mover_and_table_cases_reach_every_decision():
    groups = {name: built(name) for name in gpu.GROUPS}
    every = [c for g in groups.values() for cs in g.values() for c in cs]
    movers = groups["movers"]
    for cs in list(movers.values()) + list(groups["tables"].values()):
        common_premises(cs)
    seen = predicted(every)
    assert not [d for d in gpu.REQUIRED if d not in seen]
    assert any(c.expect["grid"] == (12, 64, 5) for c in movers["row_copies"])
    # the held slide: every len and blocks of the movers, with every delta and every zero_below (above len too), held and
    # not-held streams in one launch, held_vec both ways at every len
    slides = [c for c in movers["slide_held"] if c.slide is not None]
    assert {c.slide[:2] for c in slides} == {(n, b) for n in gpu.SLIDE_LENS for b in gpu.SLIDE_BLOCKS}
    for n in gpu.SLIDE_LENS:
        for b in gpu.SLIDE_BLOCKS:
            mine = [c for c in slides if c.slide[:2] == (n, b)]
            assert {c.slide[2] for c in mine} == {0, -1, -4, -n}
            assert all(set(c.slide[3]) == {0, 1, 4, 5, n} for c in mine)
            assert {v for c in mine for v in c.held_vec} == {0, 1}
            for c in mine:
                k = len(c.slide[3])
                assert c.words[0] == k and [c.words[4 + 14 * q + 13] for q in range(k)] == list(c.slide[3])       # zero_below as the launcher gets it
                assert [c.words[4 + 14 * q + 12] for q in range(k)] == [c.slide[2]] * k and [c.words[4 + 14 * q + 4] for q in range(k)] == [n] * k
                assert list(c.arenas[0]) == [HELD, 5, HELD]
    # the boundary cuts a slot that is stored whole (zero_below inside four floats that lie below len, dst_vec set), at every len
    # that has such a slot, and the same boundary meets the element path (dst_vec clear)
    for n in (4, 5, 8, 9):
        for vec in (0, 1):
            assert any(c.slide[0] == n and c.expect["dst_vec"][q] == vec and zb % 4 and (zb // 4) * 4 + 4 <= n
                       for c in slides for q, zb in enumerate(c.slide[3])), (n, vec)
    assert any(max(c.slide[3]) > c.slide[0] for c in slides) and any(c.slide[0] % 4 == 0 and c.slide[0] in c.slide[3] for c in slides)


def test_the_refusals_are_built():
    assert len(gpu.refusals()) == 12 and len(gpu.REFUSED) == 8
