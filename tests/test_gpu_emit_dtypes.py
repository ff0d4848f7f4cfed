"""int16, float16 and bfloat16 destinations of the device-side egress: live handles (``push`` / ``finish`` / ``finish_stream`` /
``last_emission``) and tensor calls (``repet.separate``).

A destination dtype is a cast of the float64 value the engine holds, rounded ONCE (``emit_dtypes_reference.round_ref``, which
``test_emit_dtypes_reference.py`` checks against rational arithmetic). Expected values are never taken from the 16-bit code
under test: they are ``round_ref`` of float64 values the same samples have -- ``last_emission(..., out=float64 tensor)`` of the
same handle, the float64 result of a twin handle fed the same chunks, or the float64 result of the same tensor call -- which
the older tests pin to the oracle. Every comparison is on the bits (the 16-bit tensors viewed as uint16; for the two float
formats any quiet NaN counts as NaN). All at 8 kHz (W = 512, H = 256)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet import _native
from emit_dtypes_reference import DTYPES, TRAPS_BEYOND, bits, round_ref, same_bits, trap_bits, trap_inputs
from test_gpu_online_streams import signals
from test_gpu_online_foreground import to_numpy

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 8000
H = 256
TORCH = {"int16": torch.int16, "float16": torch.float16, "bfloat16": torch.bfloat16}
SIGNALS = ("background", "foreground", "mixture")
PCM = 20000.0                                  # the streams are at PCM scale: rounding to integers leaves signal
SENTINEL = 0x5A5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits_of(t):
    """The bit patterns of a 16-bit tensor (any layout) as a uint16 array of its shape."""
    assert t.element_size() == 2, t.dtype
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def check_bits(got, want64, name, label=""):
    """``got`` (a tensor of TORCH[name]) holds round_ref of the float64 values ``want64``, bit for bit."""
    assert got.dtype == TORCH[name], (label, got.dtype)
    want64 = to_numpy(want64)
    assert want64.dtype == np.float64 and tuple(got.shape) == want64.shape, (label, tuple(got.shape), want64.shape)
    g, w = bits_of(got), bits(round_ref(want64, name)).reshape(want64.shape)
    ok = same_bits(g, w, name)
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{label}: {int((~ok).sum())} of {ok.size} {name} values differ; at {i}: float64 {want64[i]!r} "
                             f"became 0x{int(g[i]):04x}, expected 0x{int(w[i]):04x}")


def f64(shape):
    return torch.empty(shape, dtype=torch.float64, device=DEV)


def streams(channels, seconds, seeds):
    """float64 streams at PCM scale with fractional parts (not fp32-exact: the engine holds 48 bits of each), odd in length."""
    xs = signals(FS, channels, seconds, seeds) * PCM
    return xs[:, :xs.shape[1] - (1 - xs.shape[1] % 2)]


def open_pair(channels, n_streams, **kw):
    p = repet.derive_params(FS)
    assert (p.window_length, p.step_length) == (2 * H, H)
    return repet.online_streams(FS, channels, n_streams, **kw), repet.online_streams(FS, channels, n_streams, **kw)


# ---- 1. the trap table, through the mixture -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DTYPES)
def test_trap_table_through_the_mixture(name):
    """The mixture of a live sample is its input (fp32 sample + fp32 remainder: every entry of the table proper is exactly
    that), so the table reaches the last store untouched. Slot 0 carries it after its first hop, at an odd offset; slot 1 at
    another one; slot 2 is idle and its share of every chunk is NaN."""
    table, want = trap_inputs(name), trap_bits(name)
    S, ch, at0, at1 = 3, 1, H + 3, 2 * H - 7
    x = np.random.RandomState(5).uniform(-3, 3, (S, 4 * H, ch))
    x[0, at0:at0 + len(table), 0] = table
    x[1, at1:at1 + len(table), 0] = table
    x[2] = np.nan
    h = repet.online_streams(FS, ch, S, start_length=0.5)
    h.release([2])
    xd = dev(x)
    first = h.push(xd[:, :2 * H], which="mixture", dtype=TORCH[name])
    assert first.shape == (S, H, ch) and first.dtype == TORCH[name]
    got = h.push(xd[:, 2 * H:], which="mixture", dtype=TORCH[name])
    assert got.shape == (S, 2 * H, ch) and got.dtype == TORCH[name]
    mix = to_numpy(h.last_emission("mixture", out=f64((S, 2 * H, ch))))      # the float64 values of the same samples
    again = h.last_emission("mixture", dtype=TORCH[name])
    h.close()
    g = bits_of(got)
    assert not g[2].any() and not bits_of(first)[2].any() and not mix[2].any()          # the idle slot: zero bits, NaN or not
    check_bits(got, mix, name, "push")
    check_bits(again, mix, name, "last_emission")
    n_proper = len(table) - TRAPS_BEYOND[name]
    for s, at in ((0, at0 - H), (1, at1 - H)):
        seen, reached = g[s, at:at + len(table), 0], np.ascontiguousarray(mix[s, at:at + len(table), 0])
        untouched = (reached.view(np.uint64) == table.view(np.uint64)) | (np.isnan(reached) & np.isnan(table))
        # the table proper arrives as it is (two entries with more than 48 significant bits arrive within 2**-48 of themselves,
        # nowhere near a tie); beyond it, what did not arrive untouched was checked against round_ref of what did arrive
        proper = np.arange(len(table)) < n_proper
        with np.errstate(invalid="ignore"):
            near = np.abs(reached - table) <= 2.0 ** -48 * np.abs(table)
        assert (untouched | near)[proper].all(), (name, s, table[proper & ~untouched])
        assert untouched[table == 0].all()                         # (the sign of a zero included)
        must = proper | untouched
        ok = same_bits(seen, want, name)
        assert ok[must].all(), (name, s, [(float(v), hex(int(a)), hex(int(b))) for v, a, b in zip(table[must & ~ok], seen[must & ~ok], want[must & ~ok])])
        print(f"trap table, {name}, slot {s}: {int(must.sum())} of {len(table)} entries delivered untouched and equal to the table")


# ---- 2. every signal, every emitting call, every dtype --------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_every_signal_every_call_every_dtype(channels):
    S = 3
    xs = streams(channels, 3.3, [3, 5, 7])
    N = xs.shape[1]
    sizes = [5 * H + 77, 3 * H - 5, H, 2 * H + 1, 31 * H + 3, 9 * H - 75, 17 * H, 6 * H + 129]
    sizes.append(N - sum(sizes))
    assert N % 2 == 1 and sizes[-1] > 3 * H
    fade_before, end_slot_before = 6, 7                    # a gain change in front of push 6; slot 1 ends in front of push 7
    xd = dev(xs)
    whiches = ["both", "foreground", "mixture", "background"]
    some_background = some_foreground = False
    for d, name in enumerate(DTYPES):
        dt = TORCH[name]
        h, twin = open_pair(channels, S, start_length=0.5)
        pos = 0
        for k, n in enumerate(sizes + [None]):
            which = whiches[(k + d) % 4]
            label = f"C = {channels}, {name}, call {k} ({which})"
            if k == fade_before:
                for a in (h, twin):
                    a.set_background_gain([0.5, 0.25], slots=[0, 2])
            if k == end_slot_before:
                n_rest = h.stream_emit_count(1)
                tail = h.finish_stream(1, which="both", dtype=dt)
                tail64 = twin.finish_stream(1, which="both")
                assert n_rest % 4 and tail[0].shape == (n_rest, channels)
                for t, t64, sig in zip(tail, tail64, SIGNALS):
                    check_bits(t, t64, name, f"{label}: finish_stream {sig}")
            if n is None:
                got, got64 = h.finish(which=which, dtype=dt), twin.finish(which=which)
            else:
                got, got64 = h.push(xd[:, pos:pos + n], which=which, dtype=dt), twin.push(xd[:, pos:pos + n], which=which)
                pos += n
            names = ("background", "foreground") if which == "both" else (which,)
            got, got64 = (got, got64) if which == "both" else ((got,), (got64,))
            n_emit = got[0].shape[1]
            assert got[0].shape == (S, n_emit, channels) and (n is not None or (S * n_emit * channels) % 4)
            # the float64 values of the same samples, from this handle itself: what the twin returned, and what each tensor rounds
            own = {sig: h.last_emission(sig, out=f64(got[0].shape)) for sig in SIGNALS}
            for t, t64, sig in zip(got, got64, names):
                assert to_numpy(own[sig]).tobytes() == to_numpy(t64).tobytes(), label
                check_bits(t, own[sig], name, f"{label}: {sig}")
            other = SIGNALS[(k + d) % 3]                   # another signal of the same samples, straight into the 16-bit dtype
            check_bits(h.last_emission(other, dtype=dt), own[other], name, f"{label}: last_emission {other}")
            bg, fg, mix = (to_numpy(own[sig]) for sig in SIGNALS)
            some_background |= bool(np.any(bg != 0))
            some_foreground |= bool(np.any(fg != 0) and np.any(fg != mix))
        h.close()
        twin.close()
    assert some_background and some_foreground, "no emission with a background and a foreground of its own: the test saw a bypass"


# ---- 3. layouts ----------------------------------------------------------------------------------------------------------------
def layout(kind, shape, dt, pad=24):
    """A destination of ``shape`` (S, n, C) in a padded buffer full of SENTINEL: (the buffer, the view, the buffer positions the
    view covers). The buffer starts 16-byte aligned (torch allocates in 512-byte blocks); ``pad`` elements lie either side."""
    S, n, ch = shape
    dense = (n * ch, ch, 1)
    offset, strides = {
        "dense16": (pad, dense),                           # 16-byte aligned
        "dense8": (pad + 4, dense),                        # aligned for the 8-byte store, not for 16
        "dense4": (pad + 2, dense),                        # 4-byte aligned only: the element path
        "offset1": (pad + 1, dense),                       # 2-byte aligned only: the element path
        "channels_first": (pad, (ch * n, 1, n)),           # an (S, C, n) tensor, .transpose(1, 2)
        "step2": (pad, (2 * n * ch, 2 * ch, 1)),           # an (S, 2 n, C) tensor, [:, ::2]
    }[kind]
    span = sum(st * (d - 1) for st, d in zip(strides, shape)) + 1
    total = offset + span + pad
    buf = torch.full((total,), SENTINEL, dtype=torch.int16, device=DEV).view(dt)
    view = buf.as_strided(shape, strides, offset)
    where = np.lib.stride_tricks.as_strided(np.arange(total)[offset:], shape, tuple(8 * st for st in strides))
    return buf, view, np.ascontiguousarray(where)


def check_layout(buf, view, where, want_bits, name, label):
    flat = bits_of(buf)
    ok = same_bits(flat[where], want_bits, name)
    assert ok.all(), f"{label}: {int((~ok).sum())} of {ok.size} values differ from the dense aligned result"
    rest = np.ones(flat.size, dtype=bool)
    rest[where.reshape(-1)] = False
    assert (flat[rest] == SENTINEL).all(), f"{label}: {int((flat[rest] != SENTINEL).sum())} elements outside the destination were written"
    assert view.data_ptr() % 2 == 0


@pytest.mark.parametrize("name", DTYPES)
def test_layouts(name):
    dt, S, ch = TORCH[name], 3, 2
    xs = streams(ch, 2.6, [11, 12, 13])
    xd = dev(xs)
    h, twin = open_pair(ch, S, start_length=0.5)
    first = 50 * H + 3
    for a in (h, twin):
        a.push(xd[:, :first])
    kinds = ["dense16", "dense8", "dense4", "offset1", "channels_first", "step2"]
    pos, checked = first, 0
    for k, kind in enumerate(kinds):
        n = (2 + k % 2) * H
        chunk = xd[:, pos:pos + n]
        pos += n
        shape = (S, h.emit_count(n), ch)
        assert shape[1] == n
        # the dense aligned result of the twin: a fresh tensor of the dtype, for "both" a pair
        ref_bg, ref_fg = (bits_of(t) for t in twin.push(chunk, which="both", dtype=dt))
        (b0, v0, w0), (b1, v1, w1) = layout(kind, shape, dt), layout(kinds[(k + 3) % len(kinds)], shape, dt)
        out = h.push(chunk, which="both", out=(v0, v1))
        assert out[0] is v0 and out[1] is v1
        check_layout(b0, v0, w0, ref_bg, name, f"{name}, push into {kind}, background")
        check_layout(b1, v1, w1, ref_fg, name, f"{name}, push into {kinds[(k + 3) % len(kinds)]}, foreground")
        assert ref_bg.any() and (ref_fg != ref_bg).any()
        # one signal into the same kind of view (the background alone takes the plain egress kernel), and last_emission
        b, v, w = layout(kind, shape, dt)
        h.last_emission("background", out=v)
        check_layout(b, v, w, ref_bg, name, f"{name}, last_emission into {kind}, background")
        b, v, w = layout(kind, shape, dt)
        h.last_emission("foreground", out=v)
        check_layout(b, v, w, ref_fg, name, f"{name}, last_emission into {kind}, foreground")
        checked += 4
    # a pair that shares one buffer, the second tensor beginning where the first one ends: disjoint at 2-byte granularity
    n = H
    chunk = xd[:, pos:pos + n]
    shape = (S, n, ch)
    count = S * n * ch
    ref_bg, ref_fg = (bits_of(t) for t in twin.push(chunk, which="both", dtype=dt))
    buf = torch.full((count * 2 + 2,), SENTINEL, dtype=torch.int16, device=DEV).view(dt)
    pair = (buf[1:1 + count].view(shape), buf[1 + count:1 + 2 * count].view(shape))
    h.push(chunk, which="both", out=pair)
    flat = bits_of(buf)
    assert flat[0] == SENTINEL and flat[-1] == SENTINEL
    assert same_bits(flat[1:1 + count].reshape(shape), ref_bg, name).all() and same_bits(flat[1 + count:-1].reshape(shape), ref_fg, name).all()
    # the plain background egress of a push and of a finish, dense and 2-byte aligned
    pos += n
    rest = xd[:, pos:]
    ref = bits_of(twin.push(rest, dtype=dt))
    b, v, w = layout("offset1", tuple(ref.shape), dt)
    h.push(rest, out=v)
    check_layout(b, v, w, ref, name, f"{name}, background push into offset1")
    ref = bits_of(twin.finish(dtype=dt))
    assert ref.size % 4
    b, v, w = layout("dense8", tuple(ref.shape), dt)
    h.finish(out=v)
    check_layout(b, v, w, ref, name, f"{name}, background finish into dense8")
    h.close()
    twin.close()
    print(f"layouts, {name}: {checked + 4} destinations equal to the dense aligned result, nothing outside them written")


# ---- 4. refusals, before anything runs -----------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_untouched():
    S, ch = 3, 2
    xs = streams(ch, 2.2, [21, 22, 23])
    xd = dev(xs)
    h, twin = open_pair(ch, S, start_length=0.5)
    first = 40 * H + 9                                      # (the background is there by now; the foreground is still next to nothing)
    for a in (h, twin):
        emitted = tuple(a.push(xd[:, :first], which="both")[0].shape)
    n = 3 * H
    x = xd[:, first:first + n]
    m = h.emit_count(n)
    i16 = lambda *shape: torch.empty(shape, dtype=torch.int16, device=DEV)
    shared = i16(S, m + 1, ch)
    refused = [
        lambda: h.push(x, which="both", out=(i16(S, m, ch), torch.empty((S, m, ch), dtype=torch.float16, device=DEV))),   # two dtypes
        lambda: h.push(x, out=torch.empty((S, m, ch), dtype=torch.int32, device=DEV)),                                   # not a destination dtype
        lambda: h.push(x, out=i16(S, m, ch), dtype=torch.float16),                                                      # dtype= beside another out=
        lambda: h.push(x, which="both", out=(i16(S, m, ch), i16(S, m, ch)), dtype=torch.bfloat16),
        lambda: h.push(x, dtype=torch.int32),
        lambda: h.push(x.cpu().numpy(), dtype=torch.int16),                                                             # dtype= with a host chunk
        lambda: h.push(x.cpu(), dtype=torch.int16),
        lambda: h.push(x, which="both", out=(shared[:, :m], shared[:, 1:])),          # the pair overlaps (all but one sample)
        lambda: h.push(x, out=i16(1, m, ch).expand(S, m, ch)),                        # the elements of out overlap
        lambda: h.last_emission("mixture", out=i16(*emitted), dtype=torch.float32),
        lambda: h.last_emission("mixture", dtype=torch.int64),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
        assert h.samples_pushed == first, k
    # the library's own checks, under the binding's: a dtype code it does not know, and two int16 destinations one element apart
    lib, handle = _native.lib(), h._handle()
    stream = torch.cuda.current_stream(x.device)
    written = C.c_int64()
    a, b = i16(S, m, ch), i16(S * m * ch + 1)
    dense = (m * ch, ch, 1)
    push = lambda dst, code: lib.repet_online_push_device(handle, C.c_void_p(x.data_ptr()), _native.F64, n, _native._strides(tuple(x.stride())),
                                                          _native._stream_handle(stream), C.c_void_p(dst), code, _native._strides(dense),
                                                          _native._stream_handle(stream), C.byref(written))
    for code in (5, -1):
        assert push(a.data_ptr(), code) == _native.ERR_BAD_ARG and written.value == 0
    assert lib.repet_online_also_emit(handle, _native.OUT_FOREGROUND, C.c_void_p(a.data_ptr()), 5, _native._strides(dense)) == _native.ERR_BAD_ARG
    for code in (_native.I16, _native.F16, _native.BF16):
        # the second destination one element (2 bytes) into the first one's last element's neighbourhood: they share all but one
        _native.check(lib.repet_online_also_emit(handle, _native.OUT_FOREGROUND, C.c_void_p(b.data_ptr() + 2), code, _native._strides(dense)))
        assert push(b.data_ptr(), code) == _native.ERR_BAD_ARG and b"overlap" in lib.repet_last_error()
        # one dtype for both
        _native.check(lib.repet_online_also_emit(handle, _native.OUT_FOREGROUND, C.c_void_p(a.data_ptr()), _native.F32, _native._strides(dense)))
        assert push(b.data_ptr(), code) == _native.ERR_BAD_ARG and b"one dtype" in lib.repet_last_error()
    # nothing ran: the next push equals the twin's
    got, want = h.push(x, which="both", dtype=torch.int16), twin.push(x, which="both", dtype=torch.int16)
    for g, w in zip(got, want):
        assert bits_of(g).tobytes() == bits_of(w).tobytes()
    assert bits_of(got[0]).any()
    assert h.samples_pushed == twin.samples_pushed == first + n
    h.close()
    twin.close()


# ---- 5. tensor calls -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clips():
    """(sim clip (N, C), simonline batch (2, N, C)) as float64 at PCM scale, N odd, and their int16 forms."""
    one = streams(2, 6.0, [31])[0]
    two = streams(2, 10.6, [32, 33])
    pcm = lambda a: np.clip(np.round(a), -32768, 32767).astype(np.int16)
    return {"sim": (one, pcm(one)), "simonline": (two, pcm(two))}


@pytest.mark.parametrize("algo", ["sim", "simonline"])
def test_tensor_calls(algo, clips):
    x64, x16 = clips[algo]
    records = []
    for name in DTYPES:
        dt = TORCH[name]
        x = dev(x16 if name == "int16" else x64)           # int16 in, int16 out: PCM scale, so integers leave signal
        (bg64, fg64), rec64 = repet.separate(algo, x, FS, which="both", levels=True)
        assert bg64.dtype == torch.float64 and to_numpy(bg64).any() and (to_numpy(fg64) != to_numpy(x)).any()
        (bg, fg), rec = repet.separate(algo, x, FS, which="both", levels=True, dtype=dt)
        check_bits(bg, bg64, name, f"{algo} both, background")
        check_bits(fg, fg64, name, f"{algo} both, foreground")
        assert bits_of(bg).any() and bits_of(fg).any()
        assert to_numpy(rec).tobytes() == to_numpy(rec64).tobytes()                     # the levels do not notice the dtype
        records.append(to_numpy(rec64) if name != "int16" else None)
        # out=: a channels-first view for one signal, a pair for both; with a gain
        out = torch.empty(tuple(x.shape[:-2]) + (x.shape[-1], x.shape[-2]), dtype=dt, device=DEV).transpose(-1, -2)
        got = repet.separate(algo, x, FS, out=out, which="foreground", background_gain=0.5)
        assert got is out
        check_bits(out, repet.separate(algo, x, FS, which="foreground", background_gain=0.5), name, f"{algo} foreground with a gain")
        pair = (torch.empty(x.shape, dtype=dt, device=DEV), torch.empty(x.shape, dtype=dt, device=DEV))
        got, rec = repet.separate(algo, x, FS, out=pair, which="both", levels=True, dtype=dt)
        assert got[0] is pair[0] and bits_of(pair[0]).tobytes() == bits_of(bg).tobytes() and bits_of(pair[1]).tobytes() == bits_of(fg).tobytes()
        assert to_numpy(rec).tobytes() == to_numpy(rec64).tobytes()
        check_bits(repet.separate(algo, x, FS, which="mixture", dtype=dt), repet.separate(algo, x, FS, which="mixture"), name, f"{algo} mixture")
        with pytest.raises(ValueError):
            repet.separate(algo, x, FS, out=pair[0], dtype=torch.float32)
        with pytest.raises(ValueError):
            repet.separate(algo, x, FS, which="both", out=(pair[0], torch.empty(x.shape, dtype=torch.float32, device=DEV)))
        with pytest.raises(ValueError):
            repet.separate(algo, x, FS, out=torch.empty(x.shape, dtype=torch.int32, device=DEV))
    assert records[1].tobytes() == records[2].tobytes()


# ---- 6. levels and state untouched ---------------------------------------------------------------------------------------------
def test_levels_and_state_do_not_notice_the_dtype():
    S, ch = 3, 2
    xs = streams(ch, 2.4, [41, 42, 43])
    xd = dev(xs)
    h, twin = open_pair(ch, S, start_length=0.5)
    sizes = [44 * H, 3 * H, 5 * H, 2 * H]
    pos, measured = 0, 0
    for k, n in enumerate(sizes):
        chunk = xd[:, pos:pos + n]
        pos += n
        which = ("both", "foreground", "background", "mixture")[k]
        h.push(chunk, which=which, dtype=torch.int16)
        twin.push(chunk, which=which)
        a, b = to_numpy(h.last_levels()), to_numpy(twin.last_levels())
        assert a.tobytes() == b.tobytes() and a.shape == (S, ch, 8)
        measured += int(a[..., 1].any() and a[..., 2].any())              # background and foreground energy
        for slot in range(S):
            sa, sb = h.export_stream(slot), twin.export_stream(slot)
            assert sa.header == sb.header and np.asarray(sa.payload).tobytes() == np.asarray(sb.payload).tobytes()
    assert measured >= 2
    tail, tail64 = h.finish(which="both", dtype=torch.bfloat16), twin.finish(which="both")
    assert to_numpy(h.last_levels()).tobytes() == to_numpy(twin.last_levels()).tobytes()
    for t, t64 in zip(tail, tail64):
        check_bits(t, t64, "bfloat16", "finish")
    h.close()
    twin.close()
