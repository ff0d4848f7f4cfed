"""The read-back calls of a live handle at the C ABI (include/repet_hip.h: repet_online_last_emission, last_levels, last_frames,
last_band_energies, last_matches, export_stream, import_stream and the _device form of each): what each of the fourteen entry
points refuses, in which order, with which words and with what left in ``*n_written`` / ``*n_rows``, and that the host form and
the device form of a record hand out the same bits.

One geometry, the smallest the suite uses (8 kHz: window 512, hop 256; 2 streams, 2 channels, start_length of 33 frames: M_YOUNG
of tests/test_gpu_online_frames.py), 40 hops plus 77 samples in two uneven pushes, so the last push completes nine frames, seven
of them past the warm-up. The library is called through ``_native.lib()``; only the pushes go through the Python handle.

The refusal texts below were recorded from the library as it stood BEFORE the host and device forms of these calls were given one
body each; they are constants of this file and are never read from the tree under test. Every bad argument here is one the
library refuses on the host before any launch, and every destination is pre-filled with a sentinel that a refusal must leave.

Host form equals device form, bit for bit: asserted here for last_emission (three signals, float64), last_levels,
last_band_energies (3 bands) and the export payload and header (and a host import followed by an export reproduces the payload).
For last_frames (a dense destination and a stride-permuted one) the same equality is asserted by
tests/test_gpu_online_frames.py::test_host_and_device_forms_and_strided_destinations, for last_matches (all three arrays) by
tests/test_gpu_online_matches.py::test_host_and_device_forms_give_identical_bits: they are not repeated here."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet import _native
from repet._native import ptr
from repet_synth import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS, W, H, F = 8000, 512, 256, 257
S, CH, M = 2, 2, 33
PUSHES = (31 * H + 5, 9 * H + 72)                 # 40 hops + 77 samples: 30 frames, then 9 more (frames 30 .. 38)
N_EMIT, N_FRAMES = 9 * H, 9
BAD_ARG, LIMIT = -1, -5
EDGES = np.array([0, 7, 100, F], dtype=np.int32)  # 3 bands
SENT = -7.0                                       # what every destination holds before a call
KEEP = 99                                         # what *n_written / *n_rows hold before a call

NULL = "null argument"
NULL_DST = "null destination"
SMALL = "online: output capacity too small"
WHICH = "which must be REPET_OUT_BACKGROUND, REPET_OUT_FOREGROUND or REPET_OUT_MIXTURE"
STALE_EMISSION = "online: the last emission is stale (a push, finish, restart or release came after it)"
STALE_FRAMES = "online: the last frames are stale (a push, finish, finish_stream, restart, release, import, hold or resume came after them)"
STALE_MATCHES = "online: the last matches are stale (a push, finish, finish_stream, restart, release, import, hold or resume came after them)"
DTYPE = "the result is float64, float32, int16, float16 or bfloat16"
NO_STRIDES = "strides is null"
NEG_STRIDE = "negative stride (make the tensor contiguous first)"
OVERLAP = "the destination's elements overlap (an expanded or aliasing view)"
MANY_BANDS = "online: at most REPET_MAX_BANDS (128) bands"
NO_BANDS = "online: at least one band and its edges"
BAD_EDGES = "online: band edges are ascending bins in [0, window_length / 2 + 1]"
ALIGN = "online: the payload must be 4-byte aligned"
SLOT = "online: slot out of range"
OFF_GRID = "online: a stream can only be exported on a hop boundary (samples pushed % step_length == 0)"
MAGIC = "online: not a stream state (unknown magic word)"


def lib():
    return _native.lib()


@functools.lru_cache(maxsize=None)
def signal():
    """The two streams' samples (S, n, CH): computed once, shared, left unchanged."""
    n = sum(PUSHES) + 10
    x = np.stack([synth(n / FS + 0.01, FS, CH, seed)[:n] for seed in (61, 62)])
    x.setflags(write=False)
    return x


def open_handle():
    return repet.online_streams(FS, CH, S, start_length=M * H / FS)


def pushed(extra=0):
    """A handle after the two pushes (and a third of ``extra`` samples); its raw handle beside it."""
    x, handle, pos = signal(), open_handle(), 0
    for n in PUSHES + ((extra,) if extra else ()):
        handle.push(x[:, pos:pos + n])
        pos += n
    return handle, handle._handle()


def stream():
    return _native._stream_handle(torch.cuda.current_stream(torch.device(DEV)))


def dev(shape, dtype=torch.float64):
    return torch.full(shape, SENT, dtype=dtype, device=DEV)


def dptr(t):
    return C.c_void_p(t.data_ptr())


def i64(*values):
    return (C.c_int64 * len(values))(*values)


def untouched(*dsts):
    torch.cuda.synchronize()
    for d in dsts:
        a = d.cpu().numpy() if isinstance(d, torch.Tensor) else d
        assert (a == a.dtype.type(SENT)).all()


def refused(call, text, left=KEEP, code=BAD_ARG, dsts=()):
    """``call(counter)`` is refused with ``code`` and ``text``, leaves ``left`` in the counter and the destinations alone."""
    n = C.c_int64(KEEP)
    assert call(C.byref(n)) == code
    assert lib().repet_last_error().decode() == text
    assert n.value == left
    untouched(*dsts)


def accepted(call, left, dsts=()):
    n = C.c_int64(KEEP)
    assert call(C.byref(n)) == 0, lib().repet_last_error().decode()
    assert n.value == left
    untouched(*dsts)


def same_bits(a, b):
    torch.cuda.synchronize()
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.tobytes() == b.tobytes()


def stale_handles():
    """[(handle, raw)] before the first push, and after a restart that followed a push (of whole hops: a restart's grid)."""
    fresh, handle = open_handle(), open_handle()
    handle.push(signal()[:, :40 * H])
    handle.restart([1])
    return [(fresh, fresh._handle()), (handle, handle._handle())]


def test_last_emission_refusals():
    L = lib()
    handle, h = pushed()
    out = np.full((S, N_EMIT, CH), SENT)
    dst, dense = dev((S, N_EMIT, CH)), i64(N_EMIT * CH, CH, 1)
    host = lambda n, o=h, which=1, a=out, cap=N_EMIT: L.repet_online_last_emission(o, which, None if a is None else ptr(a), cap, n)
    device = lambda n, o=h, which=1, d=dst, dtype=_native.F64, st=dense: L.repet_online_last_emission_device(
        o, which, None if d is None else dptr(d), dtype, st, stream(), n)
    stales = stale_handles()
    for form in (host, device):
        refused(lambda n: form(n, o=None), NULL, dsts=(out, dst))
        assert form(None) == BAD_ARG and L.repet_last_error().decode() == NULL
        refused(lambda n: form(n, which=3), WHICH, 0, dsts=(out, dst))
        refused(lambda n: form(n, which=-1), WHICH, 0, dsts=(out, dst))
        for _, hs in stales:
            refused(lambda n: form(n, o=hs), STALE_EMISSION, 0, dsts=(out, dst))
            refused(lambda n: form(n, o=hs, which=3), WHICH, 0)                   # which comes before stale
    refused(lambda n: host(n, cap=N_EMIT - 1), SMALL, 0, dsts=(out,))
    refused(lambda n: host(n, a=None), SMALL, 0)
    refused(lambda n: host(n, a=None, cap=0), SMALL, 0)                           # asking: the emission's call has no count to tell
    refused(lambda n: device(n, dtype=99), DTYPE, 0, dsts=(dst,))
    refused(lambda n: device(n, dtype=99, st=None), DTYPE, 0, dsts=(dst,))        # dtype comes before strides
    refused(lambda n: device(n, st=None), NO_STRIDES, 0, dsts=(dst,))
    refused(lambda n: device(n, st=i64(N_EMIT * CH, -CH, 1)), NEG_STRIDE, 0, dsts=(dst,))
    refused(lambda n: device(n, st=i64(0, CH, 1)), OVERLAP, 0, dsts=(dst,))
    refused(lambda n: device(n, st=i64(0, CH, 1), d=None), OVERLAP, 0)            # strides come before the destination
    refused(lambda n: device(n, d=None), NULL_DST, 0)
    for closing in [handle] + [st for st, _ in stales]:
        closing.close()
    # an empty emission (a push that completes no frame): the host form takes a null array, the device form a null destination
    handle, h = pushed(extra=10)
    accepted(lambda n: host(n, o=h, a=None, cap=0), 0)
    accepted(lambda n: device(n, o=h, d=None), 0)
    handle.close()


def test_last_levels_refusals():
    L = lib()
    handle, h = pushed()
    count = S * CH * _native.LEVEL_FIELDS
    out, dst = np.full(count, SENT), dev((count,))
    host = lambda n, o=h, a=out, cap=count: L.repet_online_last_levels(o, None if a is None else ptr(a), cap, n)
    device = lambda o=h, d=dst: L.repet_online_last_levels_device(o, None if d is None else dptr(d), stream())

    def refused_device(call, text):
        assert call() == BAD_ARG and L.repet_last_error().decode() == text
        untouched(dst)

    refused(lambda n: host(n, o=None), NULL, dsts=(out,))
    assert host(None) == BAD_ARG and L.repet_last_error().decode() == NULL
    refused_device(lambda: device(o=None), NULL)
    for stale, hs in stale_handles():
        refused(lambda n: host(n, o=hs), STALE_EMISSION, 0, dsts=(out,))
        refused_device(lambda: device(o=hs), STALE_EMISSION)
        refused_device(lambda: device(o=hs, d=None), STALE_EMISSION)              # stale comes before the destination
        stale.close()
    refused(lambda n: host(n, cap=count - 1), SMALL, count, dsts=(out,))          # a short array is told the count
    refused(lambda n: host(n, a=None), SMALL, count)
    refused(lambda n: host(n, a=None, cap=0), SMALL, count)                       # asking
    refused_device(lambda: device(d=None), NULL_DST)
    handle.close()


def frame_forms(h, bands):
    """(host, device) callers of last_frames (``bands`` false) or last_band_energies over shared sentinel destinations."""
    L = lib()
    last = len(EDGES) - 1 if bands else F
    count = S * N_FRAMES * CH * last
    out = np.full(count, SENT, dtype=np.float64 if bands else np.float32)
    dst = dev((count,), torch.float64 if bands else torch.float32)
    dense = i64(N_FRAMES * CH * last, CH * last, last, 1)
    if bands:
        host = lambda n, o=h, which=1, a=out, cap=count, e=EDGES, nb=3: L.repet_online_last_band_energies(
            o, which, None if e is None else ptr(e), nb, None if a is None else ptr(a), cap, n)
        device = lambda o=h, which=1, d=dst, e=EDGES, nb=3, st=None: L.repet_online_last_band_energies_device(
            o, which, None if e is None else ptr(e), nb, None if d is None else dptr(d), stream())
    else:
        host = lambda n, o=h, which=1, a=out, cap=count: L.repet_online_last_frames(o, which, None if a is None else ptr(a), cap, n)
        device = lambda o=h, which=1, d=dst, st=dense: L.repet_online_last_frames_device(o, which, None if d is None else dptr(d), st, stream())
    return host, device, out, dst, count


@pytest.mark.parametrize("bands", [False, True], ids=["frames", "bands"])
def test_last_frames_and_band_energies_refusals(bands):
    L = lib()
    handle, h = pushed()
    host, device, out, dst, count = frame_forms(h, bands)

    def refused_device(call, text, code=BAD_ARG):
        assert call() == code and L.repet_last_error().decode() == text
        untouched(dst)

    refused(lambda n: host(n, o=None), NULL, dsts=(out,))
    assert host(None) == BAD_ARG and L.repet_last_error().decode() == NULL
    refused_device(lambda: device(o=None), NULL)
    refused(lambda n: host(n, which=3), WHICH, 0, dsts=(out,))
    refused_device(lambda: device(which=3), WHICH)
    if bands:
        refused(lambda n: host(n, which=3, nb=129), WHICH, 0)                     # which comes before the edges
        refused(lambda n: host(n, nb=129), MANY_BANDS, 0, code=LIMIT, dsts=(out,))
        refused(lambda n: host(n, nb=0), NO_BANDS, 0, dsts=(out,))
        refused(lambda n: host(n, e=None), NO_BANDS, 0, dsts=(out,))
        refused(lambda n: host(n, e=np.array([0, 9, 8, F], dtype=np.int32)), BAD_EDGES, 0, dsts=(out,))
        refused(lambda n: host(n, e=np.array([0, 7, 100, F + 1], dtype=np.int32)), BAD_EDGES, 0, dsts=(out,))
        refused_device(lambda: device(nb=129), MANY_BANDS, LIMIT)
        refused_device(lambda: device(nb=0), NO_BANDS)
        refused_device(lambda: device(e=None), NO_BANDS)
        refused_device(lambda: device(e=np.array([0, 9, 8, F], dtype=np.int32)), BAD_EDGES)
    for stale, hs in stale_handles():
        refused(lambda n: host(n, o=hs), STALE_FRAMES, 0, dsts=(out,))
        refused_device(lambda: device(o=hs), STALE_FRAMES)
        refused_device(lambda: device(o=hs, d=None), STALE_FRAMES)                # stale comes before the destination
        if bands:
            refused(lambda n: host(n, o=hs, nb=0), NO_BANDS, 0)                   # the edges come before stale
            refused_device(lambda: device(o=hs, nb=0), NO_BANDS)
        stale.close()
    refused(lambda n: host(n, cap=count - 1), SMALL, count, dsts=(out,))          # a short array is told the count
    refused(lambda n: host(n, a=None), SMALL, count)
    refused(lambda n: host(n, a=None, cap=0), SMALL, count)                       # asking
    if not bands:
        last = F
        refused_device(lambda: device(st=None), NO_STRIDES)
        refused_device(lambda: device(st=i64(N_FRAMES * CH * last, CH * last, -last, 1)), NEG_STRIDE)
        refused_device(lambda: device(st=i64(0, CH * last, last, 1)), OVERLAP)
        refused_device(lambda: device(st=i64(0, CH * last, last, 1), d=None), OVERLAP)    # strides come before the destination
    refused_device(lambda: device(d=None), NULL_DST)
    handle.close()
    # an empty record (a push that completes no frame): OK from either form, nothing written; the device form still checks first
    handle, h = pushed(extra=10)
    accepted(lambda n: host(n, o=h), 0, dsts=(out,))
    accepted(lambda n: host(n, o=h, a=None, cap=0), 0)
    assert device(o=h) == 0
    untouched(dst)
    refused_device(lambda: device(o=h, d=None), NULL_DST)
    handle.close()


def test_last_matches_refusals():
    L = lib()
    handle, h = pushed()
    k = handle.match_capacity
    rows = S * N_FRAMES
    outs = (np.full(rows, SENT, dtype=np.int32), np.full(rows * k, SENT, dtype=np.int32), np.full(rows * k, SENT, dtype=np.float32))
    dsts = (dev((rows,), torch.int32), dev((rows * k,), torch.int32), dev((rows * k,), torch.float32))
    p = lambda a: None if a is None else ptr(a)
    d = lambda t: None if t is None else dptr(t)
    host = lambda n, o=h, a=outs, cap=rows: L.repet_online_last_matches(o, p(a[0]), p(a[1]), p(a[2]), cap, n)
    device = lambda o=h, t=dsts: L.repet_online_last_matches_device(o, d(t[0]), d(t[1]), d(t[2]), stream())

    def refused_device(call, text):
        assert call() == BAD_ARG and L.repet_last_error().decode() == text
        untouched(*dsts)

    refused(lambda n: host(n, o=None), NULL, dsts=outs)
    assert host(None) == BAD_ARG and L.repet_last_error().decode() == NULL
    refused_device(lambda: device(o=None), NULL)
    for stale, hs in stale_handles():
        refused(lambda n: host(n, o=hs), STALE_MATCHES, 0, dsts=outs)
        refused_device(lambda: device(o=hs), STALE_MATCHES)
        refused_device(lambda: device(o=hs, t=(None, None, None)), STALE_MATCHES)  # stale comes before the destination
        stale.close()
    accepted(lambda n: host(n, a=(None, None, None), cap=0), rows, dsts=outs)     # asking
    refused(lambda n: host(n, cap=rows - 1), SMALL, rows, dsts=outs)
    for missing in range(3):
        part = tuple(None if j == missing else a for j, a in enumerate(outs))
        refused(lambda n: host(n, a=part), SMALL, rows, dsts=outs)
        refused_device(lambda: device(t=tuple(None if j == missing else t for j, t in enumerate(dsts))), NULL_DST)
    handle.close()
    # an empty record: OK from either form with nothing written; the device form still checks its destinations first
    handle, h = pushed(extra=10)
    accepted(lambda n: host(n, o=h), 0, dsts=outs)
    accepted(lambda n: host(n, o=h, a=(None, outs[1], outs[2])), 0, dsts=outs)
    assert device(o=h) == 0
    untouched(*dsts)
    refused_device(lambda: device(o=h, t=(dsts[0], None, dsts[2])), NULL_DST)
    handle.close()


def state_sizes(h):
    hb, pb = C.c_int64(), C.c_int64()
    assert lib().repet_online_stream_state_size(h, C.byref(hb), C.byref(pb)) == 0
    return hb.value, pb.value


def test_export_and_import_refusals():
    L = lib()
    handle, h = pushed()                          # 40 hops + 77 samples: off the hop grid
    hb, pb = state_sizes(h)
    header = np.full(hb, 0x55, dtype=np.uint8)
    payload = np.full(pb // 4, SENT, dtype=np.float32)
    dst = dev((pb // 4 + 1,), torch.float32)

    def refused_plain(call, text):
        assert call() == BAD_ARG and L.repet_last_error().decode() == text
        untouched(payload, dst)
        assert (header == 0x55).all()

    exp = lambda o=h, slot=0, hd=header, p=payload: L.repet_online_export_stream(o, slot, None if hd is None else ptr(hd), None if p is None else ptr(p))
    exp_dev = lambda o=h, slot=0, hd=header, p=dst.data_ptr(): L.repet_online_export_stream_device(
        o, slot, None if hd is None else ptr(hd), None if p is None else C.c_void_p(p), stream())
    imp = lambda o=h, slot=0, hd=header, p=payload: L.repet_online_import_stream(o, slot, None if hd is None else ptr(hd), None if p is None else ptr(p))
    imp_dev = lambda o=h, slot=0, hd=header, p=dst.data_ptr(): L.repet_online_import_stream_device(
        o, slot, None if hd is None else ptr(hd), None if p is None else C.c_void_p(p), stream())
    for form in (exp, exp_dev, imp, imp_dev):
        refused_plain(lambda: form(o=None), NULL)
        refused_plain(lambda: form(hd=None), NULL)
        refused_plain(lambda: form(p=None), NULL)
    for form in (exp_dev, imp_dev):
        refused_plain(lambda: form(p=dst.data_ptr() + 2), ALIGN)
        refused_plain(lambda: form(p=dst.data_ptr() + 2, slot=S), ALIGN)          # the alignment comes before the plan / the check
    for form in (exp, exp_dev):
        refused_plain(lambda: form(slot=S), SLOT)
        refused_plain(lambda: form(slot=-1), SLOT)
        refused_plain(lambda: form(), OFF_GRID)
    for form in (imp, imp_dev):
        refused_plain(lambda: form(slot=S), SLOT)
        refused_plain(lambda: form(), MAGIC)                                      # a header of 0x55 bytes
    handle.close()


def test_host_form_equals_device_form():
    L = lib()
    handle, h = pushed()
    n = C.c_int64()
    # last_emission: the three signals, float64
    for which in (0, 1, 2):
        out, dst = np.full((S, N_EMIT, CH), SENT), dev((S, N_EMIT, CH))
        assert L.repet_online_last_emission(h, which, ptr(out), N_EMIT, C.byref(n)) == 0 and n.value == N_EMIT
        assert L.repet_online_last_emission_device(h, which, dptr(dst), _native.F64, i64(N_EMIT * CH, CH, 1), stream(), C.byref(n)) == 0
        assert n.value == N_EMIT and np.isfinite(out).all() and (out != SENT).any()
        same_bits(dst, out)
    # last_levels
    count = S * CH * _native.LEVEL_FIELDS
    out, dst = np.full(count, SENT), dev((count,))
    assert L.repet_online_last_levels(h, ptr(out), count, C.byref(n)) == 0 and n.value == count
    assert L.repet_online_last_levels_device(h, dptr(dst), stream()) == 0
    same_bits(dst, out)
    # last_band_energies, 3 bands (last_frames and last_matches: see the module docstring)
    host, device, out, dst, count = frame_forms(h, True)
    assert host(C.byref(n)) == 0 and n.value == count
    assert device() == 0
    assert np.isfinite(out).all() and (out != SENT).all()
    same_bits(dst, out)
    handle.close()
    # export: payload and header of either form; a host import followed by an export reproduces the payload
    x = signal()[:, :40 * H]
    handle, twin = open_handle(), open_handle()
    handle.push(x)
    twin.push(x[::-1])
    h, t = handle._handle(), twin._handle()
    hb, pb = state_sizes(h)
    headers = [np.zeros(hb, dtype=np.uint8) for _ in range(3)]
    host_payload, again = np.full(pb // 4, SENT, dtype=np.float32), np.full(pb // 4, SENT, dtype=np.float32)
    dev_payload = dev((pb // 4,), torch.float32)
    assert L.repet_online_export_stream(h, 1, ptr(headers[0]), ptr(host_payload)) == 0
    assert L.repet_online_export_stream_device(h, 1, ptr(headers[1]), dptr(dev_payload), stream()) == 0
    same_bits(dev_payload, host_payload)
    assert headers[0].tobytes() == headers[1].tobytes() and headers[0].any()
    assert L.repet_online_import_stream(t, 0, ptr(headers[0]), ptr(host_payload)) == 0, L.repet_last_error().decode()
    assert L.repet_online_export_stream(t, 0, ptr(headers[2]), ptr(again)) == 0, L.repet_last_error().decode()
    assert headers[2].tobytes() == headers[0].tobytes() and again.tobytes() == host_payload.tobytes()
    handle.close()
    twin.close()


@pytest.mark.parametrize("lead", [1, 2, 3])
def test_a_payload_that_is_only_4_byte_aligned_carries_the_same_bits(lead):
    """A device payload that begins ``lead`` floats behind a 16-byte boundary: the export stores it element by element, the import
    gathers its loads one by one. Both hand on the bits of the host forms, and the export writes nothing around the payload."""
    L = lib()
    x = signal()[:, :40 * H]
    handle, twin = open_handle(), open_handle()
    handle.push(x)
    twin.push(x[::-1])
    h, t = handle._handle(), twin._handle()
    hb, pb = state_sizes(h)
    headers = [np.zeros(hb, dtype=np.uint8) for _ in range(3)]
    host_payload, again = np.full(pb // 4, SENT, dtype=np.float32), np.full(pb // 4, SENT, dtype=np.float32)
    room = dev((pb // 4 + 4,), torch.float32)
    assert room.data_ptr() % 16 == 0
    odd = room[lead:lead + pb // 4]
    assert L.repet_online_export_stream(h, 1, ptr(headers[0]), ptr(host_payload)) == 0
    assert L.repet_online_export_stream_device(h, 1, ptr(headers[1]), dptr(odd), stream()) == 0
    assert host_payload.any() and (host_payload != np.float32(SENT)).all()
    same_bits(odd, host_payload)
    untouched(room[:lead], room[lead + pb // 4:])
    assert headers[0].tobytes() == headers[1].tobytes()
    assert L.repet_online_import_stream_device(t, 0, ptr(headers[1]), dptr(odd), stream()) == 0, L.repet_last_error().decode()
    assert L.repet_online_export_stream(t, 0, ptr(headers[2]), ptr(again)) == 0, L.repet_last_error().decode()
    assert headers[2].tobytes() == headers[0].tobytes() and again.tobytes() == host_payload.tobytes()
    handle.close()
    twin.close()
