"""Slots fed at their own pace (``enable_feed`` / ``feed`` / ``tick`` of ``repet.online_streams``). A tick is a lockstep push whose
chunk the handle assembles from per-slot inboxes, with the slots that are short held for that push. In every comparison a twin
handle is driven only through ``hold`` / ``resume`` / ``push``, told what to do by the scheduler model of
``tests/feed_reference.py``: every tick must equal the twin's push bit for bit, and per slot the pieces of the ticks that consumed
it, then its tail, equal ``simonline`` of the samples it consumed. 8 kHz: H = 256, W = 512, B = 312; start_frames 40 unless a
test says otherwise."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from helpers import rms_err
from feed_reference import FeedModel
from simonline_start_reference import simonline_from
from test_gpu_online_streams import same
from test_gpu_online_start import offline_run
from test_gpu_online_hold import FS, H, B, M, Run, as_numpy, open_streams, sig
from test_gpu_variants import RMS_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class Feeder:
    """A handle with inboxes, the scheduler model beside it, and the twin (a ``Run`` of the hold tests on a handle without
    inboxes). Every slot has a signal of its own; packets are cut from it in order, so what a slot has consumed is the front
    of its signal, which is also what the twin's cursor has pushed."""

    def __init__(self, ch, S, m, capacity, sigs, device=True, released=()):
        self.h, twin = open_streams(ch, S, m), open_streams(ch, S, m)
        self.model = FeedModel(S, H)
        for s in released:
            self.h.release(s)
            twin.release(s)
            self.model.release(s)
        self.h.enable_feed(capacity)
        self.model.enable_feed(capacity)
        assert self.h.feed_capacity == capacity
        self.S, self.C, self.device = S, ch, device
        self.sigs = [None if s in released else sigs[s] for s in range(S)]
        self.twin = Run(twin, self.sigs, device=device)
        self.cur = [0] * S                      # samples of each slot's signal fed so far
        self.first = {}                         # slot -> True where its very first piece came out of the handle's first push
        self.ticks = 0

    def tensor(self, a):
        return torch.tensor(a, device=DEV) if self.device else a

    def feed(self, sizes):
        """sizes: slot -> samples. One call for all of them, with counts and NaN behind the counts (one slot: its packet alone)."""
        slots = sorted(sizes)
        if not slots:
            return
        if len(slots) == 1:
            (s,) = slots
            self.h.feed(s, self.tensor(np.array(self.sigs[s][self.cur[s]:self.cur[s] + sizes[s]])))
            self.model.feed(s, sizes[s])
        else:
            n = max(sizes.values()) + 3
            x = np.full((len(slots), n, self.C), np.nan)
            for i, s in enumerate(slots):
                x[i, :sizes[s]] = self.sigs[s][self.cur[s]:self.cur[s] + sizes[s]]
            counts = [sizes[s] for s in slots]
            self.h.feed(slots, self.tensor(x), counts)
            self.model.feed(slots, n, counts)
        for s in slots:
            self.cur[s] += sizes[s]
        self.check_counters()

    def check_counters(self):
        assert list(self.h.queued()) == self.model.queued()
        assert self.h.samples_pushed == self.model.P == self.twin.pos
        for s in range(self.S):
            assert self.h.queued(s) == self.model.queued(s)
            assert self.h.held(s) == self.model.held(s)
            assert self.h.stream_samples(s) == (None if self.sigs[s] is None else self.twin.cur[s])

    def note_first(self, consumed):
        for s in consumed:
            self.first.setdefault(s, self.twin.pos == 0 and self.twin.cur[s] == 0)

    def tick(self, hops=1, compare=True, **kw):
        """(mine, the twin's) or (None, None) where nobody was ready; the twin's background piece is recorded per slot"""
        t = self.model.tick(hops)
        got = self.h.tick(hops, **kw)
        assert list(self.h.last_consumed) == self.model.last_consumed
        if t is None:
            assert got is None
            self.check_counters()
            return None, None
        self.note_first(t.ready)
        self.twin.set_held(self.model.device_held())
        want = self.twin.push(hops * H, record=False, **kw)
        self.twin.record(as_numpy(want[0] if isinstance(want, tuple) else want))
        self.ticks += 1
        self.check_counters()
        assert isinstance(got if not isinstance(got, tuple) else got[0], torch.Tensor if self.device or "out" in kw else np.ndarray)
        if compare:
            for a, b in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
                same(a, b)
        return got, want

    def push(self, n):
        """a plain lockstep push between ticks (the inboxes are empty): the starved slots take part again"""
        self.model.push(n)
        self.twin.set_held(self.model.device_held())
        x = self.twin.chunk(n)
        self.note_first([s for s in range(self.S) if self.twin.listens(s)])
        got = self.h.push(self.tensor(x))
        for s in range(self.S):
            if self.twin.listens(s):
                self.cur[s] += n
        want = self.twin.push(n)
        same(got, want)
        self.check_counters()

    def restart(self, s, signal):
        self.h.restart(s)
        self.twin.h.restart(s)
        self.model.restart(s)
        self.sigs[s] = signal
        self.twin.begin(s, signal)
        self.cur[s] = 0
        self.first.pop(s, None)

    def drain(self):
        """pad every queue to the hop grid and tick until the inboxes are empty; the pad counts"""
        pads = [int(k) for k in self.h.pad_feed()]
        assert pads == self.model.pad_feed()
        assert all(q % H == 0 for q in self.h.queued())
        self.pads = pads
        # the twin's signals end in the same zeros
        for s in range(self.S):
            if self.sigs[s] is not None:
                x = np.concatenate([self.sigs[s][:self.cur[s]], np.zeros((pads[s], self.C))])
                self.sigs[s] = self.twin.sigs[s] = x
                self.cur[s] += pads[s]
        while any(self.model.queued()):
            assert self.tick()[0] is not None
        return pads

    def end(self, s, m):
        """finish_stream of slot s on both handles; the stream's whole output without the pad, checked against simonline"""
        tail, want = self.h.finish_stream(s), self.twin.h.finish_stream(s)
        same(tail, want)
        pieces = self.twin.out[s] + [as_numpy(want)]
        got = np.concatenate(pieces)
        lead = 0 if self.first.get(s, False) else H
        assert not got[:lead].any()
        got = got[lead:]
        n = self.twin.cur[s]
        assert got.shape[0] == n == self.cur[s]
        pad = self.pads[s]
        x = np.array(self.sigs[s][:n - pad])
        same(got[:n - pad], repet.simonline(x, FS) if m is None else offline_run(x, FS, m))
        self.sigs[s] = self.twin.sigs[s] = None
        self.twin.held.discard(s)
        self.model.finish_stream(s)
        return got[:n - pad], x

    def close(self):
        self.h.close()
        self.twin.h.close()


def typed(x, dtype):
    """the (S, n, C) float64 signal as a device tensor of an ingest dtype, and the values the handle then holds"""
    if dtype == "float64":
        x = x * (1.0 + 2.0 ** -30)              # not fp32-exact: the remainder plane matters
        assert (x.astype(np.float32).astype(np.float64) != x).any()
        return torch.tensor(x, device=DEV)
    if dtype == "int16":
        return torch.tensor(np.rint(x * 20000.0).astype(np.int16), device=DEV)
    return torch.tensor(x, device=DEV).to(getattr(torch, dtype))


@pytest.mark.parametrize("dtype", ["float32", "float64", "int16", "float16", "bfloat16"])
def test_lockstep_feed_equals_push(dtype):
    """Every slot is fed the same 1 .. 3 whole hops before every tick of that many hops: the tick is the twin's push of the same
    tensor, bit for bit, for every ingest dtype -- background, which="both", the level and match records, an int16 out."""
    S, ch, hops_total = 3, 2, M + 20
    x = typed(np.stack([sig(500 + s, hops_total * H, ch) for s in range(S)]), dtype)
    h, twin = open_streams(ch, S, M), open_streams(ch, S, M)
    h.enable_feed(3 * H)
    rs = np.random.RandomState(3)
    pos, k = 0, 0
    while pos < hops_total * H:
        n = min(int(rs.randint(1, 4)) * H, hops_total * H - pos)
        chunk = x[:, pos:pos + n]
        if k % 3 == 0:
            for s in range(S):                  # one slot at a time, as strided views of the whole signal
                h.feed(s, chunk[s])
        else:
            h.feed([2, 0, 1], chunk[[2, 0, 1]])
        assert list(h.queued()) == [n] * S
        if k == 12:
            outs = [torch.empty((S, n if pos >= 2 * H else 0, ch), dtype=torch.int16, device=DEV) for _ in range(2)]
            assert h.tick(n // H, out=outs[0]) is outs[0]
            twin.push(chunk, out=outs[1])
            same(outs[0], outs[1])
        elif k % 2:
            got, want = h.tick(n // H, which="both"), twin.push(chunk, which="both")
            same(got[0], want[0])
            same(got[1], want[1])
        else:
            got = h.tick(n // H)
            assert isinstance(got, torch.Tensor) and got.dtype == torch.float64
            same(got, twin.push(chunk))
        assert h.last_consumed.all() and not h.queued().any()
        if k % 4 == 0 or pos >= (M - 1) * H:
            same(h.last_levels(), twin.last_levels())
            for a, b in zip(h.last_matches(), twin.last_matches()):
                same(a, b)
        pos += n
        k += 1
        assert h.samples_pushed == twin.samples_pushed == pos
    assert k > 12
    same(h.finish(), twin.finish())
    h.close()
    twin.close()


def ragged_sizes(t, f, rs):
    """what arrives for slots 0 .. 4 before tick t"""
    sizes = {}
    sizes[0] = 160 * ((t + 1) * H // 160 - t * H // 160)                 # 160-sample packets at the handle's pace
    k = int(rs.randint(1, 701))                                          # seeded sizes, as far as the inbox has room
    if f.model.queued(1) + k <= f.model.capacity:
        sizes[1] = k
    if t % 9 == 8:
        sizes[2] = 3 * H                                                 # nothing for 8 ticks, then a burst
    sizes[3] = H
    if t >= 25:
        sizes[4] = 200                                                   # restarted at hop 25
    return {s: k for s, k in sizes.items() if k > 0}


@pytest.mark.parametrize("ch", [1, 2])
def test_ragged_packets(ch):
    """Five slots, five arrival patterns, one tick per hop time: 160-sample packets, seeded sizes of 1 .. 700, bursts of three hops
    after eight empty ticks, exactly a hop per tick, and a slot released at the start and restarted at handle hop 25. Every tick
    equals the twin's push, starved slots are exact zeros, and every life with its padded tail is simonline of what it consumed."""
    ticks, total = 126, 140 * H
    sigs = [sig(510 + s, total, ch) for s in range(5)]
    f = Feeder(ch, 5, M, 8 * H, sigs, released=[4])
    rs = np.random.RandomState(11 + ch)
    starved_ticks = 0
    for t in range(ticks):
        if t == 25:
            f.restart(4, sigs[4])
        f.feed(ragged_sizes(t, f, rs))
        got, want = f.tick()
        assert got is not None and f.h.samples_pushed == (t + 1) * H      # slot 3 is always ready
        starved = [s for s in range(5) if f.sigs[s] is not None and not f.model.last_consumed[s]]
        starved_ticks += len(starved)
        for s in starved:
            assert not as_numpy(got)[s].any()
    assert starved_ticks > 100 and f.model.writes > 40
    f.drain()
    assert any(f.pads)
    for s in range(5):
        assert f.twin.cur[s] >= (M - 2) * H + 2 * H
        got, x = f.end(s, M)
        assert got[M * H:].any()
        if s == 0 and ch == 1:
            assert rms_err(got, simonline_from(x, FS, M)) <= RMS_TOL
    f.close()


def test_ring_wrap_and_a_full_buffer():
    """An inbox of three hops on the reference start (M = B), until the slot that is starved on a seeded third of the ticks has
    consumed B + 60 hops: its circular positions (own frame % B) wrap while the handle's frames and the ring's positions do."""
    ch, cap = 2, 3 * H
    total = (2 * B + 60) * H
    sigs = [sig(520 + s, total, ch) for s in range(2)]
    f = Feeder(ch, 2, None, cap, sigs)
    rs = np.random.RandomState(5)
    full = wrapped = 0
    while f.twin.cur[1] < (B + 60) * H:
        sizes = {}
        k = 0
        while f.model.queued(0) + k < H:                                 # odd packets: unaligned ring positions
            k += 161
        sizes[0] = k
        q = f.model.queued(1)
        if f.ticks % 40 == 5:
            sizes[1] = cap - q                                           # to the brim
        elif rs.rand() >= 1 / 3:
            sizes[1] = min(cap - q, max(H - q, 0) + int(rs.randint(0, 120)))
        before = f.cur[1] % cap
        f.feed({s: k for s, k in sizes.items() if k > 0})
        wrapped += f.cur[1] % cap < before
        full += f.model.queued(1) == cap
        assert f.tick()[0] is not None
    starved = f.ticks - f.twin.cur[1] // H
    assert full > 5 and wrapped > 20 and starved > f.ticks // 5 and f.ticks < 2 * B + 50
    f.drain()
    for s in range(2):
        f.end(s, None)
    f.close()


def test_refusals_change_nothing():
    """Handle a sees every refused call, handle b none of them: queued, samples_pushed and every later tick are equal."""
    S, ch, ticks = 3, 2, M + 12
    sigs = [sig(530 + s, (ticks + 2) * H, ch) for s in range(S)]
    a, b = open_streams(ch, S, M), open_streams(ch, S, M)
    packet = torch.tensor(np.array(sigs[0][:100]), device=DEV)
    with pytest.raises(ValueError):
        a.feed(0, packet)                                                # before enable_feed
    with pytest.raises(ValueError):
        a.tick()
    for h in (a, b):
        h.release(2)
        h.enable_feed(2 * H)
    with pytest.raises(ValueError):
        a.enable_feed(2 * H)                                             # a second one
    two = torch.tensor(np.stack([sigs[0][:2 * H], sigs[1][:2 * H]]), device=DEV)
    refused = {
        3: [lambda: a.feed([0, 1], two, [0, 2 * H - 99]),                # overflow of slot 1 alone
            lambda: a.feed([0, 2], two[:, :10]),                         # an idle slot
            lambda: a.feed([0, 0], two[:, :10]),                         # a slot named twice
            lambda: a.feed([0, 1], two[:, :10], [10, 11]),               # a count above n
            lambda: a.feed([0, 1], two[:, :10], [-1, 10]),
            lambda: a.feed(3, packet)],
        7: [lambda: a.push(two[:, :H].new_zeros((S, H, ch)))],           # a push with a queue
        M + 5: [lambda: a.finish_stream(0),                              # the streams could end here, but for their queues
                lambda: a.finish()],
    }
    cur = [0, 0]
    for t in range(ticks):
        for h in (a, b):
            h.feed([0, 1], torch.tensor(np.stack([sigs[s][cur[s]:cur[s] + H + 100 * (t in (3, 7))] for s in range(2)]), device=DEV))
        for s in range(2):
            cur[s] += H + 100 * (t in (3, 7))
        for call in refused.get(t, []):
            with pytest.raises(ValueError):
                call()
            assert list(a.queued()) == list(b.queued()) and a.samples_pushed == b.samples_pushed
            assert not a.held(0) and a.stream_samples(0) == b.stream_samples(0)
        if t == 10:                                                      # off the hop grid: no tick
            for h in (a, b):
                h.clear_feed()
                h.push(torch.zeros((S, 100, ch), device=DEV))
            with pytest.raises(ValueError):
                a.tick()
            for h in (a, b):
                h.push(torch.zeros((S, H - 100, ch), device=DEV))
                h.feed([0, 1], torch.tensor(np.stack([sigs[s][cur[s] - H:cur[s]] for s in range(2)]), device=DEV))
        got, want = a.tick(), b.tick()
        same(got, want)
        same(a.last_emission("foreground"), b.last_emission("foreground"))
        assert list(a.last_consumed) == list(b.last_consumed) == [True, True, False]
        assert list(a.queued()) == list(b.queued()) and a.samples_pushed == b.samples_pushed
    assert as_numpy(got)[:2].any()
    for h in (a, b):
        h.clear_feed()
    same(a.finish(), b.finish())
    with pytest.raises(ValueError):
        a.feed(0, packet)                                                # finished
    a.close()
    b.close()


def test_nobody_ready():
    """A tick that finds nobody ready returns None and leaves the handle, its last emission and its records as they were."""
    S, ch = 2, 2
    sigs = [sig(540 + s, (M + 6) * H, ch) for s in range(S)]
    f = Feeder(ch, S, M, 2 * H, sigs)
    for t in range(M + 3):
        f.feed({0: H, 1: H})
        f.tick()
    fg, frames, rng = f.h.last_emission("foreground"), f.h.last_frames(), f.h.last_frame_range
    levels, pushed = f.h.last_levels(), f.h.samples_pushed
    assert as_numpy(fg).any()
    f.feed({0: H - 1, 1: 10})
    assert f.tick() == (None, None)
    assert f.h.tick(2, which="both") is None and not f.h.last_consumed.any()
    assert f.h.samples_pushed == pushed and list(f.h.queued()) == [H - 1, 10]
    same(f.h.last_emission("foreground"), fg)
    same(f.h.last_frames(), frames)
    same(f.h.last_levels(), levels)
    assert f.h.last_frame_range == rng
    f.feed({0: 1})
    got, want = f.tick()
    assert list(f.h.last_consumed) == [True, False] and not as_numpy(got)[1].any()
    f.close()


def test_caller_holds():
    """A slot the caller holds is fed and not consumed, and consumed again by the tick after its resume; held() reports the
    caller's holds, never starvation; a starved slot that is held and resumed stays out until it is ready."""
    S, ch = 3, 2
    sigs = [sig(550 + s, (M + 30) * H, ch) for s in range(S)]
    f = Feeder(ch, S, M, 4 * H, sigs)
    for t in range(M + 23):
        if t == M + 2:
            f.h.hold(1)
            f.model.hold(1)
        if t == M + 8:
            assert f.h.queued(1) == 4 * H and f.h.held(1)
            f.h.resume(1)
            f.model.resume(1)
        sizes = {0: H, 1: H, 2: H if t % 3 else 0}                       # slot 2 starves on every third tick
        if f.model.queued(1) + H > 4 * H:
            del sizes[1]
        f.feed({s: k for s, k in sizes.items() if k})
        got, want = f.tick()
        held = M + 2 <= t < M + 8
        assert list(f.h.last_consumed) == [True, not held, bool(t % 3)]
        assert f.h.held(1) == held and not f.h.held(2) and not f.h.held(0)      # held() never reports starvation
        if held:
            assert not as_numpy(got)[1].any()
    # a starved slot that the caller holds and resumes stays out until it is ready
    f.feed({0: H})
    f.tick()
    f.h.hold(2), f.model.hold(2)
    f.h.resume(2), f.model.resume(2)
    f.feed({0: H})
    got, _ = f.tick()
    assert list(f.h.last_consumed) == [True, True, False] and not as_numpy(got)[2].any()
    f.drain()
    for s in range(S):
        f.end(s, M)
    f.close()


def test_host_arrays():
    """The NumPy forms against the device forms, bit for bit, on one schedule with starving and a plain push between ticks."""
    S, ch, ticks = 3, 2, M + 14
    sigs = [sig(560 + s, (ticks + 10) * H, ch) for s in range(S)]
    runs = [Feeder(ch, S, M, 3 * H, sigs, device=dev) for dev in (True, False)]
    rs = np.random.RandomState(9)
    plan = []
    for t in range(ticks):
        plan.append({0: H, 1: int(rs.randint(100, 400)), 2: 2 * H if t % 2 else 0})
    pieces = [[], []]
    for i, f in enumerate(runs):
        for t, sizes in enumerate(plan):
            if t in (M + 4, M + 9):
                # the inboxes are emptied and slot 1 was starved on the tick before: a plain push resumes it first
                f.h.clear_feed(), f.model.clear_feed()
                for s in range(S):
                    f.cur[s] = f.twin.cur[s]
                f.feed({0: H, 2: H})
                f.tick()
                assert f.model.starved[1] and not any(f.model.queued())
                f.push(H + 50)
                f.push(H - 50)
            f.feed({s: k for s, k in sizes.items() if k and f.model.queued(s) + k <= 3 * H})
            got, _ = f.tick()
            assert isinstance(got, torch.Tensor if f.device else np.ndarray)
            pieces[i].append(as_numpy(got))
            assert isinstance(f.h.last_levels(), torch.Tensor if f.device else np.ndarray)
    assert len(pieces[0]) == len(pieces[1]) == ticks
    for a, b in zip(*pieces):
        same(a, b)
    assert np.concatenate(pieces[0], axis=1)[:, M * H:].any()
    for f in runs:
        f.h.clear_feed(), f.model.clear_feed()
        same(f.h.finish(), f.twin.h.finish())
        f.close()
