"""A live stream moved between streaming handles (``export_stream`` / ``import_stream`` of ``repet.online_streams`` and
``repet.online``). The guarantee: what the exporting slot emitted before the export, then what the importing slot emits in
lockstep from the import on, then its ``finish_stream`` / ``finish`` tail, equal ``repet.simonline`` of the stream's whole input
bit for bit, NaN positions equal -- on a target handle of any age, whatever its other slots do and whatever lived in the slot.

All streams are 8 kHz stereo (W = 512, H = 256, B = 312) of at most about 500 hops. Pushes come from ``plan_sizes`` of the
slots tests (off-grid pushes that regain the grid, one push longer than B * H) wherever a timeline has the B + 6 hops in one
piece that helper needs; the shorter timelines (a 100-hop warm-up, a 155-hop continuation) take ``hop_sizes``: seeded pushes of
1 .. 6 hops with one off-grid pair."""
import functools
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet import _native
from oracle import repet_oracle as orc
from repet_synth import synth
from helpers import rms_err
from test_gpu_online_streams import same, sleep_cycles
from test_gpu_online_slots import as_numpy, plan_sizes
from test_gpu_variants import RMS_TOL

pytestmark = pytest.mark.gpu

FS, CH = 8000, 2
H, B = 256, 312
P = 345 * H                      # the export: past the warm-up, age % B != 0
N = 500 * H + 77                 # a whole stream: it ends off the hop grid


@functools.lru_cache(maxsize=None)
def signal(seed, n):
    x = synth(n / FS + 0.01, FS, CH, seed)[:n]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(seed, n):
    """repet.simonline of signal(seed, n): computed once, shared, left unchanged."""
    want = repet.simonline(np.array(signal(seed, n)), FS)
    want.setflags(write=False)
    return want


def hop_sizes(total, seed):
    """Seeded pushes of 1 .. 6 hops up to `total`, the second and third of them an off-grid pair (100 samples, then back)."""
    rs = np.random.RandomState(seed)
    sizes, pos = [], 0
    while pos < total:
        if len(sizes) == 1 and total - pos > 2 * H:
            sizes += [100, 2 * H - 100]
            pos += 2 * H
            continue
        n = min(int(rs.randint(1, 7)) * H, total - pos)
        sizes.append(n)
        pos += n
    return sizes


class Run:
    """A handle, its position and every slot's lockstep output so far."""

    def __init__(self, h, which="background"):
        self.h, self.pos, self.emitted, self.pieces, self.which = h, 0, 0, [], which
        self.fg = []

    def push(self, chunk):
        n = chunk.shape[1]
        expect = self.h.emit_count(n)
        got = self.h.push(chunk, which=self.which)
        if self.which == "both":
            got, fg = got
            self.fg.append(as_numpy(fg))
        assert tuple(got.shape) == (chunk.shape[0], expect, chunk.shape[2])
        self.pieces.append(as_numpy(got))
        self.pos += n
        self.emitted += expect
        assert self.h.samples_pushed == self.pos

    def feed(self, xs, sizes, upto=None):
        """Pushes xs[:, pos:...] in the given sizes until the handle stands at `upto`; returns the sizes left over."""
        sizes = list(sizes)
        while sizes and (upto is None or self.pos < upto):
            n = sizes.pop(0)
            self.push(xs[:, self.pos:self.pos + n])
        assert upto is None or self.pos == upto
        return sizes

    def out(self, slot, first=0):
        return np.concatenate([p[slot] for p in self.pieces])[first:]

    def fg_out(self, slot, first=0):
        return np.concatenate([p[slot] for p in self.fg])[first:]


def exported(seed=301, slots=3, slot=1, upto=P, sizes=None, device=False, dtype=None):
    """A handle of `slots` slots whose slot `slot` carries signal(seed, N)[:upto], and the state exported there."""
    xs = np.stack([signal(seed if s == slot else 310 + s, N)[:upto] for s in range(slots)])
    if dtype is not None:
        xs = xs.astype(dtype)
    a = Run(repet.online_streams(FS, CH, slots))
    a.feed(xs, sizes or plan_sizes(upto, [5 * H + 77], H, B, seed))
    state = a.h.export_stream(slot, device=device)
    assert a.h.stream_samples(slot) == upto and state.length_samples == upto
    return a, state


@functools.lru_cache(maxsize=None)
def mature_export():
    """(what the exporting slot emitted, the state) of signal(301, N) exported at P from slot 1 of three, host payload."""
    a, state = exported()
    before = a.out(1)
    a.h.close()
    assert len(before) == P - H
    return before, state


def test_mature_stream_into_a_mature_handle():
    x, pre = signal(301, N), 401 * H
    before, state = mature_export()
    total = pre + N - P
    y = signal(302, total)
    xs = np.stack([np.concatenate([np.full((pre, CH), np.nan), x[P:]]), y])
    b = Run(repet.online_streams(FS, CH, 2))
    b.h.release(0)
    left = b.feed(xs, plan_sizes(total, [pre, pre + 20 * H + 100], H, B, 2), upto=pre)
    b.h.import_stream(0, state)
    mark = b.emitted
    assert b.h.stream_samples(0) == P and b.h.stream_samples(1) == pre
    b.feed(xs, left)
    tail = b.h.finish_stream(0)
    rest = b.h.finish()
    b.h.close()
    got = np.concatenate([before, b.out(0, mark), tail])
    same(got, reference(301, N))
    assert rms_err(got, orc.simonline(np.array(x), FS)) <= RMS_TOL
    same(np.concatenate([b.out(1), rest[1]]), reference(302, total))
    assert not b.out(0)[:mark].any()


@pytest.mark.parametrize("target", ["fresh", "young", "young_restarted"])
def test_young_and_fresh_targets(target):
    """The handle is younger than the stream: its epoch moves back, its live slot never notices. (An untouched handle holds
    no sample yet, the moved stream one hop that was never emitted: the next push emits that hop, in lockstep a hop of zeros
    for the other slot, whose own output begins behind it.)"""
    x = signal(301, N)
    before, state = mature_export()
    pre = 0 if target == "fresh" else 20 * H
    first = 8 * H if target == "young_restarted" else 0            # where the live slot's own stream begins
    end = pre + N - P                                              # the moved stream ends here, off the grid
    total = end + 330 * H + 50
    y = signal(305, total - first)
    xs = np.stack([np.concatenate([np.zeros((pre, CH)), x[P:], np.zeros((total - end, CH))]),
                   np.concatenate([signal(306, N)[:first], y])])
    b = Run(repet.online_streams(FS, CH, 2))
    marks = [m for m in (first, pre, end) if m]
    sizes = plan_sizes(total, marks, H, B, 7)
    if first:
        sizes = b.feed(xs, sizes, upto=first)
        b.h.restart(1)
    sizes = b.feed(xs, sizes, upto=pre)
    b.h.import_stream(0, state)
    mark = b.emitted
    assert b.h.samples_pushed == pre and b.h.stream_samples(0) == P and b.h.stream_samples(1) == pre - first
    sizes = b.feed(xs, sizes, upto=end)
    tail = b.h.finish_stream(0)
    moved = b.out(0, mark)
    b.feed(xs, sizes)
    rest = b.h.finish()
    b.h.close()
    assert not b.out(0, mark + len(moved)).any() and not rest[0].any()       # idle since its finish_stream
    same(np.concatenate([before, moved, tail]), reference(301, N))
    lead = H if target == "fresh" else 0
    live = np.concatenate([b.out(1), rest[1]])
    assert not live[:lead].any()
    same(live[first + lead:], reference(305, total - first))


def test_warm_up_stream():
    age = 100 * H
    x = signal(301, N)
    a, state = exported(slots=2, slot=0, upto=age, sizes=hop_sizes(age, 3))
    before = a.out(0)
    a.h.close()
    assert not before.any() and state.age_frames == 99 and state.history_rows == 99
    pre = 150 * H
    total = pre + N - age
    y = signal(302, total)
    xs = np.stack([np.concatenate([np.full((pre, CH), np.nan), x[age:]]), y])
    b = Run(repet.online_streams(FS, CH, 2))
    b.h.release(0)
    left = b.feed(xs, plan_sizes(total, [pre], H, B, 4), upto=pre)
    b.h.import_stream(0, state)
    mark = b.emitted
    assert b.h.stream_samples(0) == age
    b.feed(xs, left)
    tail = b.h.finish_stream(0)
    rest = b.h.finish()
    b.h.close()
    got = np.concatenate([before, b.out(0, mark), tail])
    assert not got[:(B - 1) * H].any() and got[(B - 1) * H:].any()       # zeros until ITS warm-up ends
    same(got, reference(301, N))
    same(np.concatenate([b.out(1), rest[1]]), reference(302, total))


def test_snapshot_and_fork():
    x = signal(301, N)
    a, state = exported(slots=1, slot=0)
    x2a, x2b = signal(320, N - P), signal(321, N - P)
    assert not np.array_equal(x2a, x2b)
    fork = Run(repet.online_streams(FS, CH, 1))
    fork.h.import_stream(0, state)
    assert fork.h.samples_pushed == 0 and fork.h.stream_samples(0) == P
    before = a.out(0)
    fork.feed(x2a[None], hop_sizes(N - P, 5))
    a.feed(np.concatenate([x[:P], x2b])[None], hop_sizes(N - P, 6))
    got_fork = np.concatenate([before, fork.out(0), fork.h.finish()[0]])
    got_orig = np.concatenate([a.out(0), a.h.finish()[0]])
    a.h.close()
    fork.h.close()
    same(got_fork, repet.simonline(np.concatenate([x[:P], x2a]), FS))
    same(got_orig, repet.simonline(np.concatenate([x[:P], x2b]), FS))
    assert not np.array_equal(got_fork[P:], got_orig[P:])


def test_state_round_trip():
    x = signal(301, N)
    assert not np.array_equal(x.astype(np.float32).astype(np.float64), x)          # float64 that is not fp32-exact
    a, state = exported(slots=2, slot=1)
    on_device = a.h.export_stream(1, device=True)
    before = a.out(1)
    assert isinstance(state.header, bytes) and len(state.header) == repet.StreamState.HEADER_BYTES
    assert state.payload.dtype == np.uint8 and state.payload.shape == (a.h.stream_state_nbytes,)
    assert on_device.payload.dtype == torch.uint8 and on_device.payload.device == torch.device("cuda", 0)
    assert on_device.header == state.header and np.array_equal(on_device.payload.cpu().numpy(), state.payload)
    a.h.close()
    samples = (B - 1 + 1) * H * CH                                                  # held samples of the payload: (B - 1 + W / H - 1) hops
    lo = state.payload.view(np.float32)[-samples:]
    assert lo.any(), "the remainder plane of a float64 stream is zero"
    assert (state.window_length, state.step_length, state.buffer_frames, state.number_channels) == (512, H, B, CH)
    assert (state.age_frames, state.length_samples, state.history_rows, state.pending_samples) == (P // H - 1, P, B - 1, H)
    b = Run(repet.online_streams(FS, CH, 2))
    b.h.import_stream(1, state)
    again = b.h.export_stream(1)
    assert again.header == state.header and np.array_equal(again.payload, state.payload)
    c = Run(repet.online_streams(FS, CH, 1))
    c.h.import_stream(0, repet.StreamState.from_bytes(state.to_bytes()))
    cont = np.array(x[P:])
    sizes = hop_sizes(N - P, 8)
    b.feed(np.stack([cont, cont]), sizes)
    c.feed(cont[None], sizes)
    got_b = np.concatenate([before, b.out(1), b.h.finish()[1]])
    got_c = np.concatenate([before, c.out(0), c.h.finish()[0]])
    b.h.close()
    c.h.close()
    same(got_b, reference(301, N))
    same(got_c, got_b)


@pytest.mark.parametrize("dtype", ["f32", "i16"])
def test_device_path_equals_the_host_chunk_run(dtype):
    """Chunks, results (out=, float32) and the payload stay on the device; the stream equals an unmoved run of host chunks."""
    if dtype == "i16":
        host = np.clip(np.round(signal(301, N) * 20000.0), -32768, 32767).astype(np.int16)
    else:
        host = signal(301, N).astype(np.float32)
    plain = Run(repet.online_streams(FS, CH, 1))
    plain.feed(host[None], plan_sizes(N, [P], H, B, 12))
    want = np.concatenate([plain.out(0), plain.h.finish()[0]])
    plain.h.close()
    same(want, repet.simonline(host, FS))
    full = torch.tensor(host, device="cuda:0")
    pieces = []

    def push(h, slot, slots, a, b):
        chunk = torch.zeros((slots, b - a, CH), dtype=full.dtype, device="cuda:0")
        chunk[slot] = full[a:b]
        out = torch.full((slots, h.emit_count(b - a), CH), 7.0, dtype=torch.float32, device="cuda:0")
        assert h.push(chunk, out=out) is out
        pieces.append(out[slot])

    src = repet.online_streams(FS, CH, 2)
    pos = 0
    for n in plan_sizes(P, [5 * H + 77], H, B, 13):
        push(src, 1, 2, pos, pos + n)
        pos += n
    state = src.export_stream(1, device=True)
    src.release(1)
    assert state.payload.is_cuda and state.payload.dtype == torch.uint8
    dst = repet.online_streams(FS, CH, 3)
    dst.import_stream(2, state)
    for n in hop_sizes(N - P, 14):
        push(dst, 2, 3, pos, pos + n)
        pos += n
    tail = torch.full((dst.stream_emit_count(2), CH), 7.0, dtype=torch.float32, device="cuda:0")
    assert dst.finish_stream(2, out=tail) is tail
    src.close()
    dst.close()
    same(torch.cat(pieces + [tail]), want.astype(np.float32))


def test_migration_between_device_pushes_does_not_wait_on_the_host():
    S = 8
    xs = np.stack([signal(330 + s, 500 * H) for s in range(S)])
    total = xs.shape[1]
    full = torch.tensor(xs, device="cuda:0")
    h = repet.online_streams(FS, CH, S, max_push_samples=4 * H)
    h.release([5, 6])
    pieces, pos = [], 0

    def push(n):
        nonlocal pos
        chunk = full[:, pos:pos + n].clone()
        chunk[5] = full[1, pos:pos + n]                       # slot 5 is fed what slot 1 is: the stream will move there
        chunk[6] = full[2, pos:pos + n]
        pieces.append(h.push(chunk))
        pos += n

    while pos < 340 * H:
        push(4 * H)
    h.import_stream(6, h.export_stream(2, device=True))       # (both launches have been made once: their code is loaded)
    push(2 * H)
    torch.cuda.synchronize()
    torch.cuda._sleep(sleep_cycles(100))
    t0 = time.perf_counter()
    push(2 * H)
    state = h.export_stream(1, device=True)
    h.import_stream(5, state)
    h.release(1)
    moved = pos
    push(2 * H)
    elapsed = time.perf_counter() - t0
    assert elapsed < 0.05, f"two device pushes, an export and an import took {elapsed * 1e3:.1f} ms behind a 100-ms sleep: a host wait"
    torch.cuda.synchronize()
    assert isinstance(state.header, bytes) and state.length_samples == moved
    while pos < total:
        push(min(4 * H, total - pos))
    pieces.append(h.finish())
    h.close()
    got = torch.cat(pieces, dim=1).cpu().numpy()
    for s in (0, 2, 3, 4, 7):
        same(got[s], reference(330 + s, 500 * H))
    same(np.concatenate([got[1, :moved - H], got[5, moved - H:]]), reference(331, 500 * H))
    same(np.concatenate([got[2, :339 * H], got[6, 339 * H:]]), reference(332, 500 * H))
    assert not got[1, moved - H:].any() and not got[5, :moved - H].any() and not got[6, :339 * H].any()


def test_foreground_travels():
    """fp32-exact input: the foreground of every sample emitted after the import is x - background bit for bit, the hop that
    was pushed into the exporting handle included -- the delay line moved with the stream."""
    x = signal(301, N).astype(np.float32).astype(np.float64)
    a = Run(repet.online_streams(FS, CH, 1))
    a.feed(x[None], plan_sizes(P, [5 * H + 77], H, B, 15))
    state = a.h.export_stream(0)
    before = a.out(0)
    a.h.close()
    b = Run(repet.online_streams(FS, CH, 2), which="both")
    b.h.import_stream(1, state)
    b.feed(np.stack([np.zeros((N - P, CH)), x[P:]]), hop_sizes(N - P, 16))
    tail_bg, tail_fg = b.h.finish_stream(1, which="both")
    b.h.close()
    bg = np.concatenate([b.out(1), tail_bg])
    fg = np.concatenate([b.fg_out(1), tail_fg])
    assert len(before) == P - H and len(bg) == N - (P - H)
    same(fg, x[P - H:] - bg)
    same(np.concatenate([before, bg]), repet.simonline(x, FS))
    assert np.any(bg) and np.any(fg)


def test_nothing_of_the_slot_leaks():
    """Import over a live slot that held another signal, and into a slot that was fed NaN while idle."""
    x, pre = signal(301, N), 330 * H
    before, state = mature_export()
    total = pre + N - P
    dirty = np.array(signal(340, pre))
    dirty[pre - FS // 2:pre - H, 0] = np.nan                     # past its warm-up, up to the hop before the import
    dirty[pre - H:] = np.inf
    xs = np.stack([np.concatenate([dirty, x[P:]]), np.concatenate([np.full((pre, CH), np.nan), x[P:]]), signal(341, total)])
    b = Run(repet.online_streams(FS, CH, 3))
    b.h.release(1)
    left = b.feed(xs, plan_sizes(total, [pre], H, B, 17), upto=pre)
    b.h.import_stream(0, state)
    b.h.import_stream(1, state)
    mark = b.emitted
    b.feed(xs, left)
    tails = [b.h.finish_stream(0), b.h.finish_stream(1)]
    rest = b.h.finish()
    b.h.close()
    assert np.isnan(b.out(0)[:mark]).any()                      # the slot's previous life did carry them
    for slot in (0, 1):
        got = np.concatenate([before, b.out(slot, mark), tails[slot]])
        assert not np.isnan(got).any()
        same(got, reference(301, N))
    same(np.concatenate([b.out(2), rest[2]]), reference(341, total))


def test_refusals_change_nothing(monkeypatch):
    before, state = mature_export()
    others = {}
    for name, (fs, ch) in {"fs": (16000, CH), "channels": (FS, 1)}.items():
        h = repet.online_streams(fs, ch, 1)
        others[name] = h.export_stream(0)                        # (an untouched handle's slot is a live stream of length 0)
        h.close()
    for name, value in {"similarity_number": 50, "buffer_length": 8}.items():
        with monkeypatch.context() as m:
            m.setattr(repet, name, value)
            h = repet.online_streams(FS, CH, 1)
            others[name] = h.export_stream(0)
            h.close()
    flipped = bytearray(state.header)
    flipped[0] ^= 0xFF
    version = bytearray(state.header)
    version[4] ^= 0x02
    bad = dict(others,
               short=repet.StreamState(state.header, state.payload[:-1]),
               dtype=repet.StreamState(state.header, state.payload.view(np.int8)),
               floats=repet.StreamState(state.header, state.payload.view(np.float32)),
               magic=repet.StreamState.__new__(repet.StreamState),
               tensor=repet.StreamState(state.header, torch.tensor(state.payload.view(np.int8), device="cuda:0")))
    bad["magic"].header, bad["magic"].payload = bytes(flipped), state.payload
    with pytest.raises(ValueError):
        repet.StreamState(bytes(flipped), state.payload)
    with pytest.raises(ValueError):
        repet.StreamState(bytes(version), state.payload)
    with pytest.raises(ValueError):
        repet.StreamState.from_bytes(state.to_bytes()[:-1])

    total = 440 * H + 31
    off, on = 20 * H + 100, 380 * H
    xs = np.stack([signal(350, total), signal(351, total), signal(352, total)])
    b = Run(repet.online_streams(FS, CH, 3))
    b.h.release(2)
    sizes = b.feed(xs, plan_sizes(total, [off, on], H, B, 18), upto=off)
    with pytest.raises(ValueError):
        b.h.export_stream(0)                                     # off the hop grid
    with pytest.raises(ValueError):
        b.h.import_stream(0, state)
    sizes = b.feed(xs, sizes, upto=on)
    with pytest.raises(ValueError):
        b.h.export_stream(2)                                     # idle
    for slot in (3, -1):
        with pytest.raises(ValueError):
            b.h.export_stream(slot)
        with pytest.raises(ValueError):
            b.h.import_stream(slot, state)
    for name, s in bad.items():
        with pytest.raises(ValueError):
            b.h.import_stream(0, s)
        with pytest.raises(ValueError):
            b.h.import_stream(2, s)
    with pytest.raises(ValueError):
        b.h.import_stream(0, state.to_bytes())                   # not a StreamState
    lib, handle = _native.lib(), b.h._handle()                   # the library refuses what the Python layer refused first
    for header in (bytes(flipped), bytes(version)):
        assert lib.repet_online_import_stream(handle, 0, header, _native.ptr(state.payload)) == _native.ERR_BAD_ARG
    assert lib.repet_online_import_stream(handle, 3, state.header, _native.ptr(state.payload)) == _native.ERR_BAD_ARG
    assert lib.repet_online_import_stream(handle, 0, state.header, None) == _native.ERR_BAD_ARG
    assert b.h.stream_samples(0) == on and b.h.stream_samples(2) is None and b.h.samples_pushed == on
    b.feed(xs, sizes)
    rest = b.h.finish()
    with pytest.raises(ValueError):
        b.h.export_stream(0)                                     # a finished handle
    with pytest.raises(ValueError):
        b.h.import_stream(0, state)
    b.h.close()
    for slot in (0, 1):
        same(np.concatenate([b.out(slot), rest[slot]]), reference(350 + slot, total))
    assert not b.out(2).any() and not rest[2].any()


def test_online_separator_moves_too():
    """repet.online: the single-slot separator exports and imports through the same entry points."""
    x = signal(301, N)
    a = repet.online(FS, CH)
    pieces, pos = [], 0
    for n in plan_sizes(P, [5 * H + 77], H, B, 19):
        pieces.append(a.push(x[pos:pos + n]))
        pos += n
    state = a.export_stream()
    a.close()
    b = repet.online(FS, CH)
    b.import_stream(state)
    for n in hop_sizes(N - P, 20):
        pieces.append(b.push(x[pos:pos + n]))
        pos += n
    pieces.append(b.finish())
    b.close()
    same(np.concatenate(pieces), reference(301, N))
