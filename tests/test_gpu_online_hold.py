"""Slots that sit out pushes (``hold`` / ``resume`` of single slots of ``repet.online_streams``). The guarantee, per slot: the
output pieces of the pushes during which the slot was not held, in order, followed by its ``finish_stream`` / ``finish`` tail,
equal ``repet.simonline`` of the input pieces of those same pushes, bit for bit, NaN positions equal -- whatever the other
slots do and whatever the held chunks carried. Held shares of the chunks are NaN throughout, and a held slot's share of every
emission is exact zeros."""
import functools
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from oracle import repet_oracle as orc
from repet_synth import synth
from helpers import rms_err
from test_gpu_online_streams import same, sleep_cycles
from test_gpu_online_start import offline_run, start_length
from test_gpu_variants import RMS_TOL

pytestmark = pytest.mark.gpu

FS, H, B = 8000, 256, 312
M = 40                    # start_frames of the short scenarios: a slot separates from its own frame 39 on
LIVE = repet.LEVELS.index("live_samples")


def as_numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


@functools.lru_cache(maxsize=None)
def sig(seed, n, ch, scale=1.0):
    """A float32-exact signal of n samples: shared, left unchanged."""
    x = (synth(n / FS + 0.01, FS, ch, seed)[:n] * scale).astype(np.float32).astype(np.float64)
    x.setflags(write=False)
    return x


def oracle(x, m):
    """simonline of one stream on the device, with start_frames m (None: the reference's)."""
    return repet.simonline(np.array(x), FS) if m is None else offline_run(np.array(x), FS, m)


def open_streams(ch, S, m):
    p = repet.derive_params(FS)
    assert (p.window_length, p.step_length, p.buffer_frames) == (2 * H, H, B)
    return repet.online_streams(FS, ch, S, start_length=None if m is None else start_length(m, FS, H))


def make_plan(total, stretches, seed, dtx=None, quiet=(), big_at=None):
    """Seeded pushes [(n, held slots)] of 1 .. 6 hops up to `total` samples. stretches: slot -> [(first hop, end hop)] during
    which it is held; dtx = (slot, first hop, end hop): held on every other push in there; quiet: [(first hop, end hop)] in
    which nobody is held and pushes leave the hop grid and regain it; big_at: the hop at which one push of B + 2 hops is made.
    No push crosses a boundary of any of these, so every hold and resume falls between two pushes, on the grid."""
    rs = np.random.RandomState(seed)
    marks = {h for v in stretches.values() for ab in v for h in ab} | {h for ab in quiet for h in ab}
    if dtx:
        marks |= {dtx[1], dtx[2]}
    if big_at is not None:
        marks |= {big_at, big_at + B + 2}
    steps, pos = [], 0
    while pos < total:
        hop, on_grid = pos // H, pos % H == 0
        held = {s for s, v in stretches.items() for a, b in v if a <= hop < b}
        if dtx and dtx[1] <= hop < dtx[2] and len(steps) % 2:
            held.add(dtx[0])
        nxt = min([m for m in marks if m > hop] + [1 << 40]) * H
        if not on_grid:
            n = int(rs.randint(1, 4)) * H - pos % H
        elif hop == big_at:
            n = (B + 2) * H
        elif any(a <= hop <= b - 3 for a, b in quiet) and rs.rand() < 0.4:
            n = int(rs.randint(1, 2 * H))
        else:
            n = int(rs.randint(1, 7)) * H
        n = min(n, nxt - pos, total - pos)
        assert not held or (on_grid and n % H == 0)
        steps.append((n, frozenset(held)))
        pos += n
    return steps


class Run:
    """Every live slot has a signal of its own and a cursor into it: a push of n samples brings each slot that is neither held
    nor idle its next n samples and NaN to the others. Keeps, per slot, what it was fed and what came out while it was not held;
    checks that held and idle slots emit exact zeros and that nothing emitted is NaN.
    lead[s]: a stream that begins at handle sample P > 0 (a restart), or is held before its first sample, has nothing pending:
    the hop the next push emits for it first lies before its sample 0 and is zero, and is not part of its life."""

    def __init__(self, h, sigs, device=False, lead=None):
        self.h, self.sigs, self.device = h, list(sigs), device
        self.lead = dict(lead or {})
        self.S, self.C = h.shape
        self.cur = [0] * self.S
        self.held = set()
        self.fed = [[] for _ in range(self.S)]
        self.out = [[] for _ in range(self.S)]
        self.pos = 0
        self.last_held = set()

    def set_held(self, want):
        want = set(want)
        if want - self.held:
            self.h.hold(sorted(want - self.held))
        if self.held - want:
            self.h.resume(sorted(self.held - want))
        self.held = want

    def listens(self, s):
        return self.sigs[s] is not None and s not in self.held

    def chunk(self, n):
        x = np.full((self.S, n, self.C), np.nan)
        for s in range(self.S):
            if self.listens(s):
                x[s] = self.sigs[s][self.cur[s]:self.cur[s] + n]
        return x

    def begin(self, s, signal, lead=0):
        """a new stream in slot s (after the restart / import / release that the caller made)"""
        self.sigs[s], self.cur[s], self.fed[s], self.out[s] = signal, 0, [], []
        self.lead[s] = lead
        self.held.discard(s)

    def push(self, n, record=True, **kw):
        x = self.chunk(n)
        got = self.h.push(torch.tensor(x, device="cuda:0") if self.device else x, **kw)
        self.last_held = set(self.held)
        for s in range(self.S):
            if self.listens(s):
                self.fed[s].append(x[s])
                self.cur[s] += n
        self.pos += n
        assert self.h.samples_pushed == self.pos
        for s in range(self.S):
            assert self.h.stream_samples(s) == (None if self.sigs[s] is None else self.cur[s])
            assert self.h.held(s) == (s in self.held)
        if record:
            self.record(as_numpy(got))
        return got

    def record(self, piece):
        assert not np.isnan(piece).any()
        for s in range(self.S):
            if s in self.last_held or self.sigs[s] is None:
                assert not piece[s].any(), f"slot {s} is held or idle and emitted something"
            else:
                self.out[s].append(piece[s])

    def play(self, steps, actions=None):
        for k, (n, held) in enumerate(steps):
            if actions and k in actions:
                actions[k](self)
            self.set_held(held)
            self.push(n)
        return self

    def finish(self):
        rest = as_numpy(self.h.finish())
        assert not np.isnan(rest).any()
        for s in range(self.S):
            assert not self.h.held(s)
            if self.sigs[s] is None:
                assert not rest[s].any()
            else:
                self.out[s].append(rest[s])
        self.h.close()
        return self

    def life(self, s):
        got, lead = np.concatenate(self.out[s]), self.lead.get(s, 0)
        assert not got[:lead].any()
        return got[lead:]

    def input(self, s):
        return np.concatenate(self.fed[s])

    def check(self, s, m):
        got, x = self.life(s), self.input(s)
        assert got.shape == x.shape
        same(got, oracle(x, m))
        return got


PARITY_TOTAL = 800 * H + 77


def parity_plan(seed):
    stretches = {4: [(0, 60)], 3: [(10, 25), (100, 150)], 1: [(360, 372), (380, 381), (450, 450 + B + 2), (770, 772)]}
    steps = make_plan(PARITY_TOTAL, stretches, seed, dtx=(2, 270, 440), quiet=[(200, 262), (776, 800)], big_at=450)
    assert any(n % H for n, held in steps) and all(not held for n, held in steps if n % H)
    assert any(n == (B + 2) * H and 1 in held for n, held in steps)
    assert any(n == H and 1 in held for n, held in steps) and any(n > H and 1 in held for n, held in steps)
    assert sum(1 for n, held in steps if 2 in held) > 15
    return steps


@pytest.mark.parametrize("ch,m", [(1, None), (2, None), (2, M)])
def test_parity(ch, m):
    """Slot 0 is never held; 1 for stretches in steady state, across single-hop, multi-hop and longer-than-the-buffer pushes;
    2 on every other push; 3 inside its warm-up, while the handle's history still grows; 4 from P = 0 on; 5 is idle."""
    steps = parity_plan(17 + ch)
    total = PARITY_TOTAL
    sigs = [sig(300 + s, total, ch) for s in range(5)] + [None]
    h = open_streams(ch, 6, m)
    h.release(5)
    run = Run(h, sigs, lead={4: H}).play(steps).finish()
    assert run.pos == total and run.cur[0] == total and run.cur[4] == total - 60 * H
    for s in range(5):
        got = run.check(s, m)
        assert got.any()
    # slot 0 on a handle where nobody is ever held, and slot 4 against a restart where it was resumed
    ref = open_streams(ch, 2, m)
    ref.release(1)
    ref_run = Run(ref, [sigs[0], None])
    for n, held in steps:
        if ref_run.pos == 60 * H:
            ref.restart(1)
            ref_run.begin(1, sigs[4], lead=H)
        ref_run.push(n)
    ref_run.finish()
    for a, b in zip(run.out[0], ref_run.out[0]):
        same(a, b)
    same(run.life(4), ref_run.life(1))
    if ch == 1:
        assert rms_err(run.life(1), orc.simonline(np.array(run.input(1)), FS)) <= RMS_TOL


def test_young_handle():
    """Slots held while the handle has seen fewer than B - 1 frames: its history grows during the hold, so the rows and
    samples in front of a held slot's content are new and zero. With start_frames 40 the slots separate all the while."""
    ch, total = 2, 200 * H
    stretches = {1: [(50, 90), (120, 121)], 2: [(0, 1), (45, 47), (60, 140)], 3: [(1, 2), (41, 44)]}
    steps = make_plan(total, stretches, 5)
    sigs = [sig(320 + s, total, ch) for s in range(4)]
    run = Run(open_streams(ch, 4, M), sigs, lead={2: H}).play(steps).finish()
    assert steps[0] == (H, frozenset({2})) and steps[1] == (H, frozenset({3}))
    for s in range(4):
        assert run.check(s, M)[40 * H:].any()


def int16_of(a):
    return np.clip(np.rint(a), -32768, 32767).astype(np.int16)


def test_signals_and_records():
    """Every signal, the second destination and both a float32 and an int16 destination are zero for a held slot; the pieces
    of the pushes a slot took part in are the signals of its own stream; the level records count nothing for a held slot."""
    ch, total = 2, 150 * H
    stretches = {1: [(60, 75), (100, 104)], 2: [(5, 8), (90, 120)]}
    steps = make_plan(total, stretches, 8, dtx=(3, 50, 140))
    sigs = [sig(330 + s, total, ch, 20000.0) for s in range(4)]
    run = Run(open_streams(ch, 4, M), sigs, device=True)
    ref = Run(open_streams(ch, 1, M), sigs[:1], device=True)
    fg, mix, fg16, seen = [[] for _ in sigs], [[] for _ in sigs], [[] for _ in sigs], 0
    for n, held in steps:
        run.set_held(held)
        n_emit = run.h.emit_count(n)
        outs = tuple(torch.full((4, n_emit, ch), 7.0, dtype=torch.float32, device="cuda:0") for _ in range(2))
        run.push(n, record=False, which="both", out=outs)
        run.record(as_numpy(outs[0]))
        levels = as_numpy(run.h.last_levels())
        out16 = torch.full((4, n_emit, ch), 7, dtype=torch.int16, device="cuda:0")
        pieces = [as_numpy(outs[1]), as_numpy(run.h.last_emission("mixture")), as_numpy(run.h.last_emission("foreground", out=out16))]
        ref.push(n)
        ref_levels = as_numpy(ref.h.last_levels())
        assert np.array_equal(levels[0], ref_levels[0])
        for s in range(4):
            if s in held:
                assert not any(p[s].any() for p in pieces) and not levels[s].any()
                seen += n_emit
            else:
                assert levels[s, :, LIVE].tolist() == [n_emit] * ch
                for keep, p in zip((fg, mix, fg16), pieces):
                    keep[s].append(p[s])
    assert seen > 60 * H
    both = run.h.finish(which="both")
    ref.finish()
    for s in range(4):
        x = run.input(s)
        bg = oracle(x, M)
        got_bg = np.concatenate(run.out[s] + [as_numpy(both[0])[s].astype(np.float32)])
        got_fg = np.concatenate(fg[s] + [as_numpy(both[1])[s].astype(np.float32)])
        n = sum(len(p) for p in mix[s])
        same(got_bg, bg.astype(np.float32))
        same(got_fg, (x - bg).astype(np.float32))
        same(np.concatenate(mix[s]), x[:n])
        same(np.concatenate(fg16[s]), int16_of((x - bg)[:n]))
        assert got_fg.any() and got_bg.any()
    run.h.close()


def test_lifecycle_calls_on_held_slots():
    ch, total = 2, 170 * H
    sigs = [sig(340 + s, total, ch) for s in range(5)]
    a = Run(open_streams(ch, 5, M), sigs)
    b = Run(open_streams(ch, 2, M), [None, sig(349, total, ch)])
    b.h.release(0)
    for n in (2 * H, H):
        b.push(n)
    for n in (3 * H, 50 * H, 7 * H):
        a.push(n)
    a.set_held({1, 2, 3, 4})
    a.push(4 * H)
    a.push(H)
    # export of a held slot: the stream as it stands, and it goes on elsewhere
    state = a.h.export_stream(1)
    assert a.h.held(1) and a.h.stream_samples(1) == 60 * H
    b.h.import_stream(0, state)
    b.begin(0, sigs[1])                                       # the stream so far travels with it: 60 hops in, 59 out
    b.cur[0], b.fed[0], b.out[0] = 60 * H, [sigs[1][:60 * H]], list(a.out[1])
    assert sum(len(p) for p in b.out[0]) == 59 * H
    # a gain set during the hold: its fade elapses unheard
    a.h.set_background_gain(0.5, [1])
    a.push(2 * H)
    # finish_stream of a held slot: the tail of the stream as it stands; the hold has ended
    tail = a.h.finish_stream(2)
    assert not a.h.held(2) and a.h.stream_samples(2) is None
    same(np.concatenate(a.out[2] + [tail]), oracle(a.input(2), M))
    a.begin(2, None)
    # restart and release of held slots end the hold
    a.h.restart(3)
    a.h.release(4)
    assert not a.h.held(3) and not a.h.held(4) and a.h.stream_samples(3) == 0
    a.begin(3, sig(347, total, ch), lead=H)
    a.begin(4, None)
    a.push(3 * H)
    a.h.restart(4)
    a.begin(4, sig(348, total, ch), lead=H)
    assert a.held == {1} and a.h.held(1)
    a.push(H)
    a.set_held(set())
    bg, fg = a.push(2 * H, record=False, which="both")
    x = a.h.last_emission("mixture")
    assert bg[1].any() and np.array_equal(x[1, H:], sigs[1][60 * H:61 * H])
    same(fg[1], x[1] - 0.5 * bg[1])                           # in force from the first sample after the resume
    same(fg[0], x[0] - bg[0])
    a.record(bg)
    for n in (5 * H, 60 * H, 2 * H + 9):
        a.push(n)
        b.push(n)
    a.finish()
    b.finish()
    for s in (0, 1, 3, 4):
        assert a.check(s, M).any()
    assert b.check(0, M).any() and b.check(1, M).any()


def test_refusals_change_nothing():
    ch, S, total = 2, 3, 160 * H + 31
    sigs = [sig(350, total, ch), sig(351, total, ch), None]
    steps = make_plan(total, {1: [(70, 90)]}, 12, quiet=[(100, 130)])
    off = next(k for k, (n, held) in enumerate(steps) if sum(m for m, _ in steps[:k]) % H)
    inside = next(k for k, (n, held) in enumerate(steps) if 1 in held) + 1
    assert 1 in steps[inside][1]

    def refused_off(r):
        for call in (r.h.hold, r.h.resume):
            with pytest.raises(ValueError):
                call(0)                                      # off the hop grid
        assert not r.h.held(0)

    def refused_inside(r):
        assert r.h.held(1)
        for n in (H - 1, 1, 2 * H + 5):
            with pytest.raises(ValueError):
                r.h.push(r.chunk(n))                         # not a whole number of hops while a slot is held
        with pytest.raises(ValueError):
            r.h.hold(2)                                      # idle
        with pytest.raises(ValueError):
            r.h.hold([0, 2])                                 # (and nothing done for slot 0)
        for call in (r.h.hold, r.h.resume, r.h.held):
            with pytest.raises(ValueError):
                call(S)
            with pytest.raises(ValueError):
                call(-1)
        with pytest.raises(ValueError):
            r.h.resume([1, S])
        r.h.hold(1)                                          # held already: nothing happens
        r.h.resume(0)                                        # not held: nothing happens
        assert r.h.held(1) and not r.h.held(0) and not r.h.held(2)
        assert r.h.samples_pushed == r.pos and r.h.stream_samples(0) == r.cur[0] and r.h.stream_samples(1) == r.cur[1]

    def both(r):
        r.h.release(2)

    plain = Run(open_streams(ch, S, M), sigs).play(steps, {0: both})
    tried = Run(open_streams(ch, S, M), sigs).play(steps, {0: both, off: refused_off, inside: refused_inside})
    closed = tried.h
    rest = closed.finish()
    for call in (closed.hold, closed.resume):
        with pytest.raises(ValueError):
            call(0)                                          # after finish
    for s in (0, 1):
        tried.out[s].append(rest[s])
    closed.close()
    plain.finish()
    for s in (0, 1):
        same(tried.life(s), plain.life(s))
        assert tried.check(s, M).any()


def test_device_chunks_give_the_bits_of_host_chunks():
    ch, total = 2, 150 * H
    stretches = {0: [(0, 4), (80, 81)], 1: [(60, 100)]}
    steps = make_plan(total, stretches, 21, dtx=(2, 40, 130))
    sigs = [sig(360 + s, total, ch) for s in range(3)]
    host = Run(open_streams(ch, 3, M), sigs, lead={0: H}).play(steps).finish()
    dev = Run(open_streams(ch, 3, M), sigs, device=True, lead={0: H}).play(steps).finish()
    for s in range(3):
        same(dev.life(s), host.life(s))
        assert host.check(s, M).any()


def test_hold_and_resume_between_device_pushes_do_not_wait_on_the_host():
    ch, S = 2, 8
    xs = np.stack([sig(370 + s, 120 * H, ch) for s in range(S)])
    full = torch.tensor(xs, device="cuda:0")
    h = repet.online_streams(FS, ch, S, max_push_samples=4 * H, start_length=start_length(M, FS, H))
    cur, out = [0] * S, [[] for _ in range(S)]
    held = set()

    def push(n):
        chunk = torch.full((S, n, ch), float("nan"), dtype=torch.float64, device="cuda:0")
        for s in range(S):
            if s not in held:
                chunk[s] = full[s, cur[s]:cur[s] + n]
        got = h.push(chunk)
        for s in range(S):
            if s not in held:
                cur[s] += n
                out[s].append(got[s])

    for _ in range(30):
        push(2 * H)
    h.hold([1])                                      # (every launch has been made once: its code object is loaded)
    held.add(1)
    push(2 * H)
    h.resume([1])
    held.discard(1)
    push(2 * H)
    torch.cuda.synchronize()
    torch.cuda._sleep(sleep_cycles(100))
    t0 = time.perf_counter()
    push(2 * H)
    h.hold([2, 5])
    held.update({2, 5})
    push(2 * H)
    h.resume([5])
    held.discard(5)
    push(2 * H)
    elapsed = time.perf_counter() - t0
    assert elapsed < 0.05, f"three device pushes, two holds and a resume took {elapsed * 1e3:.1f} ms behind a 100-ms sleep: a host wait"
    torch.cuda.synchronize()
    for _ in range(3):
        push(4 * H)
    h.resume([2])
    held.discard(2)
    for _ in range(5):
        push(3 * H)
    rest = h.finish()
    h.close()
    for s in range(S):
        got = torch.cat(out[s] + [rest[s]]).cpu().numpy()
        same(got, oracle(xs[s, :cur[s]], M))
    assert cur[2] < cur[5] == cur[1] < cur[0]


def test_hold_and_resume_with_no_push_in_between_change_no_bit():
    ch, total = 2, 120 * H + 50
    sigs = [sig(380 + s, total, ch) for s in range(2)]
    steps = make_plan(total, {}, 4)
    at = [k for k, (n, _) in enumerate(steps) if sum(m for m, _ in steps[:k]) % H == 0][::3]

    def blink(r):
        r.h.hold([0, 1])
        assert r.h.held(0) and r.h.held(1)
        r.h.resume([1])
        r.h.resume(0)

    plain = Run(open_streams(ch, 2, M), sigs).play(steps).finish()
    blinked = Run(open_streams(ch, 2, M), sigs).play(steps, {k: blink for k in at}).finish()
    assert len(at) > 5
    for s in range(2):
        same(blinked.life(s), plain.life(s))
        for a, b in zip(blinked.out[s], plain.out[s]):
            same(a, b)
        assert plain.check(s, M).any()
