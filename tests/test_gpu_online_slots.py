"""Streams that join and leave a batched streaming handle one by one (``restart`` / ``release`` / ``finish_stream`` of single
slots of ``repet.online_streams``). The guarantee, per life (slot, P, Q, x): the slot's lockstep output from handle sample P
on, followed by its ``finish_stream`` / ``finish`` tail, equals ``repet.simonline(x[:Q - P], fs)`` bit for bit, NaN positions
equal -- whatever the other slots do meanwhile and whatever lived in the slot before."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from oracle import repet_oracle as orc
from repet_synth import synth
from helpers import rms_err
from test_gpu_online_streams import same, sleep_cycles
from test_gpu_variants import RMS_TOL

pytestmark = pytest.mark.gpu


def as_numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def plan_sizes(total, marks, H, B, seed):
    """Seeded pushes of k * H samples (k = 1 .. 6, one push longer than B * H) that stop at every mark; a mark off the hop grid
    is reached by a push of n = mark % H samples and left by one of m * H - n, so that the grid is regained."""
    rs = np.random.RandomState(seed)
    sizes, pos, big = [], 0, False
    for mark in sorted(set(marks) | {total}):
        while pos < mark:
            grid = mark - mark % H
            if pos % H:
                n = int(rs.randint(1, 4)) * H - pos % H
            elif pos == grid:
                n = mark - pos
            elif not big and grid - pos > (B + 6) * H:
                n, big = (B + int(rs.randint(1, 5))) * H, True
            else:
                n = int(rs.randint(1, 7)) * H
            n = min(n, (grid if pos < grid else mark) - pos)
            sizes.append(n)
            pos += n
    assert big and pos == total
    return sizes


class Drive:
    """Pushes xs (S, N, C) through a handle in the given sizes; actions[pos] is called once the handle stands at sample pos
    (before the first push for pos 0). Keeps every slot's lockstep output and what the actions record."""

    def __init__(self, h, xs, chunk_of=None, out_dtype=None):
        self.h, self.xs, self.pieces, self.pos, self.emitted = h, xs, [], 0, 0
        self.chunk_of = chunk_of or (lambda a, b: xs[:, a:b])
        self.out_dtype = out_dtype
        self.tails = {}                          # (slot, Q) -> (lockstep samples emitted when the life ended, its tail)

    def finish_stream(self, slot):
        n = self.h.stream_emit_count(slot)
        assert self.h.stream_samples(slot) is not None
        if self.out_dtype is not None:
            out = torch.full((n, self.xs.shape[2]), 7.0, dtype=self.out_dtype, device="cuda:0")
            assert self.h.finish_stream(slot, out=out) is out
            tail = out
        else:
            tail = self.h.finish_stream(slot)
        assert tuple(tail.shape) == (n, self.xs.shape[2]) and self.emitted + n == self.pos
        assert self.h.stream_samples(slot) is None
        self.tails[(slot, self.pos)] = (self.emitted, as_numpy(tail))

    def run(self, sizes, actions):
        S, C = self.xs.shape[0], self.xs.shape[2]
        if 0 in actions:
            actions[0](self)
        for n in sizes:
            expect = self.h.emit_count(n)
            if self.out_dtype is not None:
                out = torch.full((S, expect, C), 7.0, dtype=self.out_dtype, device="cuda:0")
                got = self.h.push(self.chunk_of(self.pos, self.pos + n), out=out)
            else:
                got = self.h.push(self.chunk_of(self.pos, self.pos + n))
            assert tuple(got.shape) == (S, expect, C)
            self.pieces.append(as_numpy(got))
            self.pos += n
            self.emitted += expect
            assert self.h.samples_pushed == self.pos
            if self.pos in actions:
                actions[self.pos](self)
        self.lockstep = np.concatenate(self.pieces, axis=1)
        if self.out_dtype is not None:
            out = torch.empty((S, self.h.emit_count(0, True), C), dtype=self.out_dtype, device="cuda:0")
            self.rest = as_numpy(self.h.finish(out=out))
        else:
            self.rest = as_numpy(self.h.finish())
        assert self.emitted + self.rest.shape[1] == self.pos
        self.whole = np.concatenate([self.lockstep, self.rest], axis=1)
        self.h.close()
        return self

    def life(self, slot, P, Q):
        """Output of the life (slot, P, Q): lockstep samples from P on, then the tail of its finish_stream / of finish."""
        if (slot, Q) in self.tails:
            emitted, tail = self.tails[(slot, Q)]
            return np.concatenate([self.lockstep[slot, P:emitted], tail])
        assert Q == self.pos
        return self.whole[slot, P:]


def churn_scenario(fs, ch, filler, scale=1.0):
    """Five slots: 0 untouched from open to finish; 1 released at open, restarted, ends in
    finish; 2 from open, finish_stream off the grid, restarted with another signal; 3 restarted while live, once inside its
    warm-up and once after; 4 idle, fed `filler`. Returns xs, the pushes, the actions and the lives (slot, P, Q, x, whole):
    whole = False for a life cut short by a restart (its lockstep output alone, up to the last full hop, is compared)."""
    p = repet.derive_params(fs)
    H, B = p.step_length, p.buffer_frames
    P3a, Q2, P1, P3b, P2b, total = 100 * H, 330 * H + 100, 340 * H, 445 * H, 460 * H, 790 * H + 77
    sig = lambda seed, n: synth(n / fs + 0.01, fs, ch, seed)[:n] * scale
    xs = np.full((5, total, ch), filler, dtype=np.float64)
    lives = []

    def put(slot, P, Q, seed, whole=True):
        x = sig(seed, Q - P)
        xs[slot, P:Q] = x
        lives.append((slot, P, Q, x, whole))

    put(0, 0, total, 201)
    put(1, P1, total, 202)
    put(2, 0, Q2, 203)
    put(2, P2b, total, 204)
    xs[3, :P3a] = sig(205, P3a)                          # (never leaves its warm-up: zeros)
    put(3, P3a, P3b, 206, whole=False)
    put(3, P3b, total, 207)
    actions = {0: lambda d: d.h.release([1, 4]),
               P3a: lambda d: d.h.restart(3),
               Q2: lambda d: d.finish_stream(2),
               P1: lambda d: d.h.restart([1]),
               P3b: lambda d: d.h.restart([3]),
               P2b: lambda d: d.h.restart(2)}
    sizes = plan_sizes(total, list(actions), H, B, seed=fs + ch)
    assert any(0 < n < H for n in sizes) and any(n > B * H for n in sizes) and all(n % H == 0 or n < 3 * H for n in sizes)
    return xs, sizes, actions, lives, (H, B, P3a)


def test_lives_equal_simonline():
    fs, ch = 8000, 2
    xs, sizes, actions, lives, (H, B, P3a) = churn_scenario(fs, ch, np.nan)
    d = Drive(repet.online_streams(fs, ch, 5), xs).run(sizes, actions)
    assert not np.isnan(d.whole).any()
    assert not d.whole[4].any()                                            # idle and fed NaN: zeros
    assert not d.whole[1, :lives[1][1]].any()                              # idle until its restart
    assert not d.whole[3, :P3a - H].any()                                  # a life that never left its warm-up
    for slot, P, Q, x, whole in lives:
        want = repet.simonline(x, fs)
        if whole:
            same(d.life(slot, P, Q), want)
        else:                                      # cut short by a restart: every hop that was final before it
            same(d.lockstep[slot, P:Q - H], want[:Q - P - H])
            assert np.any(want[:Q - P - H])
    slot, P, Q, x, _ = lives[3]                                            # the life that followed a finish_stream in its slot
    assert rms_err(d.life(slot, P, Q), orc.simonline(np.array(x), fs)) <= RMS_TOL


@pytest.mark.parametrize("dtype", ["f32", "i16"])
def test_lives_through_rocm_tensors_equal_host_chunks(dtype):
    fs, ch = 8000, 2
    if dtype == "i16":
        xs, sizes, actions, lives, _ = churn_scenario(fs, ch, 31000.0, scale=20000.0)
        host = np.clip(np.round(xs), -32768, 32767).astype(np.int16)
    else:
        xs, sizes, actions, lives, _ = churn_scenario(fs, ch, np.nan)
        host = xs.astype(np.float32)
    want = Drive(repet.online_streams(fs, ch, 5), host).run(sizes, actions)
    full = torch.tensor(host, device="cuda:0")
    got = Drive(repet.online_streams(fs, ch, 5), host, chunk_of=lambda a, b: full[:, a:b], out_dtype=torch.float32).run(sizes, actions)
    same(got.whole, want.whole.astype(np.float32))
    assert set(got.tails) == set(want.tails)
    for key in want.tails:
        assert got.tails[key][0] == want.tails[key][0]
        same(got.tails[key][1], want.tails[key][1].astype(np.float32))
    slot, P, Q, x, _ = lives[1]
    same(want.life(slot, P, Q), repet.simonline(host[slot, P:Q], fs))


def test_restart_between_device_pushes_does_not_wait_on_the_host():
    fs, ch, S = 8000, 2, 8
    hop = repet.derive_params(fs).step_length
    seconds = 23.0
    xs = np.stack([synth(seconds, fs, ch, s) for s in range(60, 60 + S)])
    N = (xs.shape[1] // hop) * hop
    xs = xs[:, :N]
    full = torch.tensor(xs, device="cuda:0")
    h = repet.online_streams(fs, ch, S, max_push_samples=4 * hop)
    pieces, pos = [], 0

    def push(n):
        nonlocal pos
        pieces.append(h.push(full[:, pos:pos + n]))
        pos += n

    while pos < 11 * fs // (2 * hop) * (2 * hop):
        push(2 * hop)
    h.restart([1])                                   # (the launch has been made once: its code object is loaded)
    P1 = pos
    push(2 * hop)
    torch.cuda.synchronize()
    torch.cuda._sleep(sleep_cycles(100))
    t0 = time.perf_counter()
    push(2 * hop)
    h.restart([2, 5])
    P2 = pos
    push(2 * hop)
    elapsed = time.perf_counter() - t0
    assert elapsed < 0.05, f"two device pushes and a restart took {elapsed * 1e3:.1f} ms behind a 100-ms sleep: a host wait"
    torch.cuda.synchronize()
    while pos < N:
        push(min(4 * hop, N - pos))
    pieces.append(h.finish())
    h.close()
    got = torch.cat(pieces, dim=1).cpu().numpy()
    for s in range(S):
        P = P1 if s == 1 else (P2 if s in (2, 5) else 0)
        same(got[s, P:], repet.simonline(xs[s, P:], fs))


def test_nothing_of_the_previous_life_leaks():
    fs, ch = 8000, 2
    H = repet.derive_params(fs).step_length
    P, total = 345 * H, 345 * H + 330 * H + 50
    first = synth(P / fs + 0.01, fs, ch, 71)[:P]
    first[P - fs:P - fs // 2, 0] = np.nan                       # NaN and infinite samples in its last second, up to its
    first[P - fs // 2:P - H, 1] = np.inf                        # very last sample: the frame that straddles the restart
    first[P - H:, :] = np.nan
    first[P - 3, 1] = -np.inf
    second = synth((total - P) / fs + 0.01, fs, ch, 72)[:total - P]
    xs = np.stack([synth(total / fs + 0.01, fs, ch, 73)[:total], np.concatenate([first, second])])
    B = repet.derive_params(fs).buffer_frames
    d = Drive(repet.online_streams(fs, ch, 2), xs).run(plan_sizes(total, [P], H, B, 3), {P: lambda d: d.h.restart(1)})
    assert np.isnan(d.whole[1, :P - H]).any()                   # the first life did carry them
    got = d.life(1, P, total)
    assert not np.isnan(got).any()
    same(got, repet.simonline(second, fs))
    same(d.whole[0], repet.simonline(xs[0], fs))


def test_second_level_reads_a_restarted_slots_own_samples():
    """float64 lives whose near-ties need the float64 spectra of the second level (a looped exact period; a twin that differs
    only below the fp32 rounding), in slots restarted at P > 0: the second level must read that life's samples at the right
    offset of the pending history."""
    fs, ch = 8000, 2
    p = repet.derive_params(fs)
    H, B = p.step_length, p.buffer_frames
    P1, P2 = 37 * H, 90 * H
    total = P2 + int(12.2 * fs)
    base = synth(total / fs + 0.01, fs, ch, 21)[:total]
    period = base[:int(1.5 * fs)]
    rs = np.random.RandomState(4)
    centre = np.tile(period, (total // len(period) + 1, 1))[:total].astype(np.float32)
    ulp = np.spacing(np.abs(centre)).astype(np.float64)
    looped = centre.astype(np.float64) + 0.2 * ulp * rs.uniform(-1, 1, size=centre.shape)
    nudged = centre.astype(np.float64) + 0.2 * ulp * rs.uniform(-1, 1, size=centre.shape)
    assert np.array_equal(looped.astype(np.float32), nudged.astype(np.float32)) and not np.array_equal(looped, nudged)
    noisy = base + 1e-7 * rs.standard_normal(base.shape)
    xs = np.stack([noisy, np.roll(looped, P1, axis=0), np.roll(nudged, P2, axis=0)])
    lives = [(0, 0, noisy), (1, P1, looped[:total - P1]), (2, P2, nudged[:total - P2])]
    actions = {P1: lambda d: d.h.restart(1), P2: lambda d: d.h.restart(2)}
    d = Drive(repet.online_streams(fs, ch, 3), xs).run(plan_sizes(total, list(actions), H, B, 9), actions)
    for slot, P, x in lives:
        assert np.array_equal(xs[slot, P:], x)
        same(d.life(slot, P, total), repet.simonline(x, fs))


def test_refusals_change_nothing():
    fs, ch, S = 8000, 2, 3
    p = repet.derive_params(fs)
    H, B = p.step_length, p.buffer_frames
    total = 700 * H + 31
    xs = np.stack([synth(total / fs + 0.01, fs, ch, s)[:total] for s in (81, 82, 83)])
    P, off, Q = 40 * H, 200 * H + 100, 380 * H
    sizes = plan_sizes(total, [P, off, Q], H, B, 11)

    def at_P(d):
        d.h.release(2)
        d.h.restart(1)

    def refused_off(d):
        with pytest.raises(ValueError):
            d.h.restart(0)                                   # off the hop grid
        with pytest.raises(ValueError):
            d.h.restart([0, S])                              # slot out of range (and nothing done for slot 0)
        with pytest.raises(ValueError):
            d.h.release(-1)
        with pytest.raises(ValueError):
            d.h.finish_stream(2)                             # idle
        with pytest.raises(ValueError):
            d.h.stream_emit_count(2)
        with pytest.raises(ValueError):
            d.h.finish_stream(1)                             # 160 hops old: shorter than the buffer
        assert d.h.stream_samples(0) == d.pos and d.h.stream_samples(1) == d.pos - P and d.h.stream_samples(2) is None

    def at_Q(d, refuse):
        if refuse:
            with pytest.raises(ValueError):
                d.h.finish_stream(S)
            with pytest.raises(ValueError):
                d.h.finish_stream(2)
        d.finish_stream(1)
        if refuse:
            with pytest.raises(ValueError):
                d.h.finish_stream(1)                         # idle now
        d.h.restart(2)

    plain = Drive(repet.online_streams(fs, ch, S), xs).run(sizes, {P: at_P, Q: lambda d: at_Q(d, False)})
    tried = Drive(repet.online_streams(fs, ch, S), xs).run(sizes, {P: at_P, off: refused_off, Q: lambda d: at_Q(d, True)})
    same(tried.whole, plain.whole)
    same(tried.tails[(1, Q)][1], plain.tails[(1, Q)][1])
    same(tried.life(0, 0, total), repet.simonline(xs[0], fs))
    same(tried.life(1, P, Q), repet.simonline(xs[1, P:Q], fs))
    same(tried.life(2, Q, total), repet.simonline(xs[2, Q:], fs))
    h = repet.online_streams(fs, ch, S)
    h.push(xs[:, :5 * H])
    h.release([0, 1, 2])
    with pytest.raises(ValueError):
        h.finish()                                           # the handle itself is shorter than the buffer, as before
    h.close()


def test_scale_64_slots_rolling_finish_and_restart():
    """64 stereo slots at 44.1 kHz, one hop per push, max_push_samples set. Every slot lives from open; from hop 440 on, every
    third hop one slot is finished and restarted with another clip, and all second lives end in finish(). The lifecycle calls
    allocate nothing: device memory is measured, as tools/online_streams_bench.py measures a handle, once the per-push
    workspaces have taken their size (the first pushes with active frames, before any lifecycle call), and has not grown at
    the end. Eight of the 128 completed lives, chosen by a seeded draw, equal simonline."""
    fs, ch, S = 44100, 2, 64
    p = repet.derive_params(fs)
    H, B = p.step_length, p.buffer_frames
    first_event, every = 440, 3
    total_hops = first_event + every * (S - 1) + B + 1
    dev = torch.device("cuda", 0)
    clips = np.stack([synth(15.0, fs, ch, 100 + s) for s in range(S)]).astype(np.float32)
    assert clips.shape[1] >= (first_event + every * S) * H and clips.shape[1] >= (total_hops - first_event) * H
    second_of = lambda s: (s + 17) % S
    ends = {first_event + every * s: s for s in range(S)}                 # hop -> the slot finished and restarted there
    src = torch.tensor(clips, device=dev)
    chunk = torch.empty((S, H, ch), dtype=torch.float32, device=dev)
    out = torch.empty((S, H, ch), dtype=torch.float64, device=dev)
    tail = torch.empty((H, ch), dtype=torch.float64, device=dev)
    keep = sorted(int(k) for k in np.random.RandomState(6).choice(2 * S, size=8, replace=False))   # life k: slot k % S, first / second
    kept = {k: [] for k in keep}
    begun = [0] * S
    h = repet.online_streams(fs, ch, S, max_push_samples=H)
    free_ref = None
    for hop in range(total_hops):
        for s in range(S):                       # (device-side gathers: slot s reads its current clip at its own position)
            clip = s if begun[s] == 0 else second_of(s)
            chunk[s] = src[clip, (hop - begun[s]) * H:(hop - begun[s] + 1) * H]
        n_emit = h.emit_count(H)
        assert n_emit == (H if hop >= 1 else 0)
        h.push(chunk, out=out[:, :n_emit])
        if hop >= 1:
            for k in keep:
                s, second = k % S, k >= S
                if (begun[s] > 0) == second:
                    kept[k].append(out[s].cpu().numpy().copy())
        if hop == B + 2:
            torch.cuda.synchronize()
            free_ref = torch.cuda.mem_get_info(0)[0]
        if hop + 1 in ends:
            s = ends[hop + 1]
            assert h.stream_emit_count(s) == H and h.finish_stream(s, out=tail) is tail
            if s in kept:
                kept[s].append(tail.cpu().numpy().copy())
            h.restart(s)
            begun[s] = hop + 1
    torch.cuda.synchronize()
    grown = free_ref - torch.cuda.mem_get_info(0)[0]
    rest = h.finish(out=torch.empty((S, H, ch), dtype=torch.float64, device=dev)).cpu().numpy()
    h.close()
    assert grown <= 0, f"the handle's device memory grew by {grown} bytes through the lifecycle calls"
    for k in keep:
        s, second = k % S, k >= S
        if second:
            P = begun[s]
            pieces = np.concatenate(kept[k] + [rest[s]])          # lockstep hops from P - H on (one hop behind), then the finish tail
            got = pieces[H:]
            want = repet.simonline(clips[second_of(s), :(total_hops - P) * H], fs)
        else:
            Q = first_event + every * s
            got = np.concatenate(kept[k])
            want = repet.simonline(clips[s, :Q * H], fs)
        same(got, want)
