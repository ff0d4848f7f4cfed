"""Separation that starts before the 10-s buffer is full (``start_length`` of ``repet.online`` / ``repet.online_streams``,
``Context.set_online_start``; include/repet_hip.h: repet_online_set_start_frames). With M = start_frames, a stream's frame
j >= M - 1 is separated on the min(B, j + 1) frames it has heard so far. The reference is the float64 statement of
tests/simonline_start_reference.py (tied to the oracle by tests/test_simonline_start_reference.py): the offline engine must give
its similar-frame lists on EVERY row and its samples within RMS_TOL, and every live form -- one stream, slots restarted among
old ones, short calls, a migrated stream -- must equal the offline engine bit for bit.

8 kHz stereo unless stated: W = 512, H = 256, B = 312, similarity_distance2 = 31; streams of (B + 20) H + 77 samples."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet import _native
from oracle import repet_oracle as orc
from repet_synth import synth
from helpers import rms_err
from simonline_start_reference import simonline_from
from test_gpu_online_streams import same
from test_gpu_variants import RMS_TOL

pytestmark = pytest.mark.gpu

FS, CH = 8000, 2
W, H, B = 512, 256, 312
N = (B + 20) * H + 77


def fp32_exact(a):
    return a.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def signal(seed, n=N, fs=FS, ch=CH):
    x = fp32_exact(synth(n / fs + 0.01, fs, ch, seed)[:n])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def restated(seed, m, n=N, fs=FS, ch=CH, number=100):
    """The float64 statement for signal(seed, ...): (samples, lists), computed once, shared, left unchanged."""
    trace = orc.Trace()
    want = simonline_from(np.array(signal(seed, n, fs, ch)), fs, m, orc.Params(similarity_number=number), trace=trace)
    want.setflags(write=False)
    return want, trace.items["similarity_indices"]


def offline_run(x, fs, m, number=None, lists=False):
    """simonline of one clip on a context of its own with start_frames m (None: a fresh context, nothing set)."""
    p = repet.derive_params(fs)
    if number is not None:
        p.sim_number = number
    ctx = repet.Context(0)
    if m is not None:
        ctx.set_online_start(m)
    ctx.upload(np.array(x))
    ctx.execute("simonline", p)
    got = ctx.download()
    out = got
    if lists:
        t = ctx.last_frame_count()
        rows = t - (m or p.buffer_frames) + 1
        out = (got, ctx.last_sim_indices(rows, p.sim_number), t)
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def offline(seed, m, a=0, b=N):
    """The offline engine's result for samples [a, b) of signal(seed) with start_frames m: shared, left unchanged."""
    got = offline_run(signal(seed)[a:b], FS, m)
    got.setflags(write=False)
    return got


def start_length(m, fs=FS, h=H):
    return m * h / fs


def check_against_restatement(seed, m, n, fs, ch, number=100):
    p = repet.derive_params(fs)
    h, b = p.step_length, p.buffer_frames
    want, lists = restated(seed, m, n, fs, ch, number)
    got, (idx, cnt), t = offline_run(signal(seed, n, fs, ch), fs, m, number=number, lists=True)
    assert t == orc.online_frame_count(n, p.window_length, h) and len(lists) == t - m + 1 == len(cnt)
    wrong = [k for k, row in enumerate(lists)
             if cnt[k] != len(row) or set(idx[k, :cnt[k]].tolist()) != set(int(v) for v in row)]
    err = rms_err(got, want)
    young = [k for k in wrong if k + m - 1 < b - 1]
    print(f"fs {fs} ch {ch} M {m} number {number}: rms {err:.3e}, rows that differ {len(wrong)} of {len(lists)} (young: {len(young)})")
    assert not wrong, f"rows {wrong[:8]} (frames from {m - 1}) differ from the float64 statement"
    assert err <= RMS_TOL, f"rms {err:.3e}"
    assert not got[: (m - 1) * h].any()
    return got


@pytest.mark.parametrize("m", [1, 32, 33, 64, 65, 311])
def test_offline_equals_the_float64_statement(m):
    check_against_restatement(31, m, N, FS, CH)


def test_offline_16k_mono():
    p = repet.derive_params(16000)
    assert (p.window_length, p.step_length, p.buffer_frames) == (1024, 512, 312)
    check_against_restatement(32, 64, (p.buffer_frames + 20) * p.step_length + 77, 16000, 1)


def test_offline_44k_stereo_register_fft():
    p = repet.derive_params(44100)
    assert (p.window_length, p.step_length, p.buffer_frames) == (2048, 1024, 431)
    check_against_restatement(33, 100, (p.buffer_frames + 10) * p.step_length, 44100, 2)


def test_offline_top_k_cut():
    want, lists = restated(31, 33, N, FS, CH, 4)
    assert max(len(row) for row in lists) == 4 and any(len(row) < 4 for row in lists)      # the cut is active, and not everywhere
    check_against_restatement(31, 33, N, FS, CH, number=4)


def test_zero_and_buffer_length_are_the_reference():
    x = signal(31)
    fresh = offline_run(x, FS, None)
    assert np.array_equal(offline_run(x, FS, 0), fresh)
    assert np.array_equal(offline_run(x, FS, B), fresh)
    assert np.array_equal(fresh, repet.simonline(np.array(x), FS))
    ctx = repet.Context(0)
    ctx.set_online_start(B + 1)
    ctx.upload(np.array(x))
    with pytest.raises(ValueError):
        ctx.execute("simonline", repet.derive_params(FS))
    with pytest.raises(ValueError):
        ctx.set_online_start(-1)
    ctx.set_online_start(0)
    ctx.execute("simonline", repet.derive_params(FS))
    assert np.array_equal(ctx.download(), fresh)
    ctx.close()


def test_batched_offline():
    m = 33
    clips = np.stack([signal(s) for s in (31, 41, 42)])
    p = repet.derive_params(FS)
    ctx = repet.Context(0)
    ctx.set_online_start(m)
    ctx.upload_batch(clips)
    ctx.execute("simonline", p)
    got = ctx.download()
    rows = ctx.last_frame_count() - m + 1
    idx, cnt = ctx.last_sim_indices(rows * len(clips), p.sim_number)
    ctx.close()
    assert got.shape == clips.shape
    for k, seed in enumerate((31, 41, 42)):
        one, (i1, c1), _ = offline_run(clips[k], FS, m, lists=True)
        assert np.array_equal(got[k], one), k
        assert np.array_equal(cnt[k * rows:(k + 1) * rows], c1), k
        for r in range(rows):
            assert np.array_equal(idx[k * rows + r, :c1[r]], i1[r, :c1[r]]), (k, r)
    same(got[0], offline(31, m))


def push_sizes(kind, total, seed=5):
    if kind == "hops":
        return [H] * (total // H) + ([total % H] if total % H else [])
    if kind == "big":                                  # one push across both M - 1 and B - 1
        first = (B + 5) * H
        return [first, total - first]
    rs = np.random.RandomState(seed)                   # off the hop grid
    sizes, pos = [], 0
    while pos < total:
        n = min(int(rs.choice([1, 100, 255, 257, 700, 3000, 9000])), total - pos)
        sizes.append(n)
        pos += n
    return sizes


@pytest.mark.parametrize("kind", ["hops", "big", "offgrid"])
def test_live_equals_offline(kind):
    m = 33
    x = np.array(signal(31))
    h = repet.online(FS, CH, start_length=start_length(m))
    assert h.start_frames == m
    bgs, fgs, pos = [], [], 0
    for n in push_sizes(kind, N):
        bg, fg = h.push(x[pos:pos + n], which="both")
        bgs.append(bg)
        fgs.append(fg)
        pos += n
    bg, fg = h.finish(which="both")
    h.close()
    bg, fg = np.concatenate(bgs + [bg]), np.concatenate(fgs + [fg])
    same(bg, offline(31, m))
    same(fg[: (m - 1) * H], x[: (m - 1) * H])          # below start_length the foreground is the input
    assert not bg[: (m - 1) * H].any() and bg[(m - 1) * H: m * H].any()
    assert np.array_equal(bg + fg, x)
    same(fg, x - bg)


@functools.lru_cache(maxsize=None)
def one_stream(seed, a, b, m):
    """The one-stream handle's output for samples [a, b) of signal(seed, TOTAL): pushed whole, then finished."""
    x = np.array(signal(seed, TOTAL)[a:b])
    h = repet.online(FS, CH, start_length=None if m is None else start_length(m))
    out = np.concatenate([h.push(x), h.finish()])
    h.close()
    out.setflags(write=False)
    return out


P1, P2 = (B + 30) * H, (B + 40) * H
TOTAL = (B + 110) * H + 77


def grid_sizes(total, marks, seed):
    """Seeded pushes of 1 .. 6 hops that stop at every mark, the second and third an off-grid pair; the rest in one push."""
    rs = np.random.RandomState(seed)
    sizes, pos = [], 0
    stops = sorted(marks) + [total - total % H]
    for stop in stops:
        while pos < stop:
            if len(sizes) == 1 and stop - pos > 2 * H:
                sizes += [100, 2 * H - 100]
                pos += 2 * H
                continue
            n = min(int(rs.randint(1, 7)) * H, stop - pos)
            sizes.append(n)
            pos += n
    if total > pos:
        sizes.append(total - pos)
    return sizes


def drive(h, xs, sizes, actions=None):
    """Push xs (S, N, C) in lockstep; actions: {position: fn(h)} run before the push that starts there. (S, emitted, C)."""
    actions = dict(actions or {})
    pieces, pos = [], 0
    for n in sizes:
        if pos in actions:
            actions.pop(pos)(h)
        pieces.append(h.push(xs[:, pos:pos + n]))
        pos += n
    assert not actions and pos == xs.shape[1]
    return np.concatenate(pieces, axis=1)


def test_young_slots_among_old_ones():
    m, S = 40, 4
    xs = np.stack([signal(s, TOTAL) for s in (51, 52, 53, 54)])
    xs[3] = np.nan
    sizes = grid_sizes(TOTAL, [P1, P2], 7)
    actions = {0: lambda h: h.release(3), P1: lambda h: h.restart(1), P2: lambda h: h.restart(2)}
    h = repet.online_streams(FS, CH, S, start_length=start_length(m))
    assert h.start_frames == m
    lock = drive(h, xs, sizes, actions)
    tail = h.finish()
    h.close()
    whole = np.concatenate([lock, tail], axis=1)
    assert whole.shape == xs.shape and not np.isnan(whole).any()
    assert not whole[3].any()                                              # idle and fed NaN
    same(whole[0], one_stream(51, 0, TOTAL, m))
    same(whole[1, : P1 - H], one_stream(52, 0, P1, m)[: P1 - H])          # a life cut short by its restart
    assert not whole[1, P1 - H: P1].any()                                  # the hop emitted behind the restart
    same(whole[1, P1:], one_stream(52, P1, TOTAL, m))                     # a young life among full buffers
    same(whole[2, : P2 - H], one_stream(53, 0, P2, m)[: P2 - H])
    same(whole[2, P2:], one_stream(53, P2, TOTAL, m))
    assert whole[1, P1 + (m - 1) * H: P1 + m * H].any() and not whole[1, P1: P1 + (m - 1) * H].any()
    # slot 0 on a handle where nothing is restarted
    h = repet.online_streams(FS, CH, S, start_length=start_length(m))
    quiet = np.concatenate([drive(h, xs, sizes, {0: lambda h: h.release(3)}), h.finish()], axis=1)
    h.close()
    same(whole[0], quiet[0])


def test_short_calls():
    m = 40
    age, begun = 100, 63                               # slot 0 is finished when it is 100 frames old; slot 1 begins at hop 63
    at = (age + 1) * H                                 # (one hop is held: W = 2 H)
    later = at + 30 * H
    xs = np.stack([signal(61, later), signal(62, later)])
    h = repet.online_streams(FS, CH, 2, start_length=start_length(m))
    lock = drive(h, xs[:, :at], grid_sizes(at, [begun * H], 3), {begun * H: lambda h: h.restart(1)})
    assert h.stream_samples(1) == (m - 2) * H          # M - 3 whole frames: the rule asks for (M - 2) H + W samples
    with pytest.raises(ValueError, match="shorter"):
        h.finish_stream(1)
    with pytest.raises(ValueError, match="shorter"):
        h.stream_emit_count(1)
    assert h.stream_samples(1) == (m - 2) * H
    tail = h.finish_stream(0)
    same(np.concatenate([lock[0], tail]), offline_run(xs[0, :at], FS, m))
    more = drive(h, xs[:, at:], grid_sizes(later - at, [], 4))
    tail = h.finish_stream(1)                          # it stayed as it was: the life goes on and ends whole
    life = np.concatenate([lock[1, begun * H:], more[1], tail])
    same(life, offline_run(xs[1, begun * H:], FS, m))
    assert not more[0].any()                           # slot 0 is idle now
    h.close()
    # the same ages on a default handle: too short, as before
    h = repet.online_streams(FS, CH, 1)
    assert h.start_frames == B
    h.push(xs[:1, : (m - 2) * H])
    with pytest.raises(ValueError, match="shorter"):
        h.finish_stream(0)
    h.push(xs[:1, (m - 2) * H: at])
    with pytest.raises(ValueError, match="shorter"):
        h.finish_stream(0)
    h.close()


@pytest.mark.parametrize("lead_hops", [80, 20])
def test_migration_of_a_young_stream(lead_hops):
    """lead_hops = 80: the target handle is older than the stream. 20: it is younger, so the import first reads the handle as
    opened earlier (online_shift_epoch) -- the stream's own frame numbers, hence its young rows, must not move with the epoch."""
    m, age = 40, 60
    total = (age + 1 + 90) * H + 77
    x = np.array(signal(71, total))
    other = np.array(signal(72, 200 * H))
    cut = (age + 1) * H                                # the export: 60 frames done, one hop held
    a = repet.online_streams(FS, CH, 2, start_length=start_length(m))
    first = drive(a, np.stack([x[:cut], other[:cut]]), grid_sizes(cut, [], 8))
    state = a.export_stream(0)
    assert state.age_frames == age
    a.close()
    b = repet.online_streams(FS, CH, 2, start_length=start_length(m))
    lead = lead_hops * H
    b.push(np.stack([other[:lead], other[:lead]]))
    b.import_stream(1, state)
    rest = np.stack([other[lead: lead + total - cut], x[cut:]])
    lock = drive(b, rest, grid_sizes(total - cut, [], 9))
    tail = b.finish_stream(1)
    b.close()
    # whatever b had emitted at the import, its next emitted sample is the stream's sample cut - H
    life = np.concatenate([first[0], lock[1], tail])
    assert first[0].shape[0] == cut - H and life.shape[0] == total
    same(life, offline_run(x, FS, m))


def test_refusals_change_nothing():
    m = 40
    lib = _native.lib()
    x = np.array(signal(31))
    h = repet.online(FS, CH, start_length=start_length(m))
    for bad in (0, B + 1, -5):
        assert lib.repet_online_set_start_frames(h._h, bad) == _native.ERR_BAD_ARG
        assert h.start_frames == m
    assert lib.repet_online_set_start_frames(h._h, m + 1) == 0 and h.start_frames == m + 1      # still before the first push
    assert lib.repet_online_set_start_frames(h._h, m) == 0
    pieces = [h.push(x[: 5 * H])]
    for value in (m + 1, B, 1, 0):
        assert lib.repet_online_set_start_frames(h._h, value) == _native.ERR_BAD_ARG
        assert b"first push" in lib.repet_last_error() or value == 0
        assert h.start_frames == m
    pieces += [h.push(x[5 * H:]), h.finish()]
    h.close()
    same(np.concatenate(pieces), offline(31, m))
    for length, frames in ((0.0, 1), (0.001, 1), (H / FS * 0.4, 1), (10.0, B), (60.0, B), (None, B)):
        h = repet.online(FS, CH, start_length=length)
        assert h.start_frames == frames, length
        h.close()
    h = repet.online_streams(FS, CH, 3, start_length=1e-6)
    assert h.start_frames == 1
    h.close()


def test_default_handles_are_untouched():
    S = 3
    total = (B + 60) * H + 77
    xs = np.stack([signal(s, TOTAL)[:total] for s in (51, 52, 53)])
    marks = [20 * H, 100 * H, (B + 10) * H]
    sizes = grid_sizes(total, marks, 12)
    actions = lambda: {marks[0]: lambda h: h.restart([1, 2]), marks[1]: lambda h: h.restart(2), marks[2]: lambda h: h.restart(1)}
    outs = []
    for explicit in (False, True):
        h = repet.online_streams(FS, CH, S)
        if explicit:
            assert _native.lib().repet_online_set_start_frames(h._h, B) == 0
        assert h.start_frames == B
        outs.append(np.concatenate([drive(h, xs, sizes, actions()), h.finish()], axis=1))
        h.close()
    same(outs[1], outs[0])
    same(outs[0][0], repet.simonline(xs[0], FS))
    assert not outs[0][1, marks[2]: marks[2] + 40 * H].any()                # a restarted slot is silent through its warm-up


def test_both_peak_kernels_and_both_band_layouts(tmp_path):
    """The kernels behind the switches: REPET_PEAKS=block (one workgroup per row and the general second level instead of one
    wavefront per row and its record path) and REPET_GRAM=f32 (the band as band[t][l] = sim(t, t + l) instead of the look-back
    layout). Each in a process of its own, since the switches are read once: the offline lists at M = 33 are the float64
    statement's on every row in all four, and the two peak kernels give the same samples bit for bit, offline and for a slot
    restarted among full buffers. A child pays the import, the first use of the device, one offline case and one whole live
    run of 422 hops -- a few seconds in all -- so one limit of 120 s per child is generous; a child that meets it has hung."""
    import os
    import subprocess
    import sys
    code = ("import sys, numpy as np; sys.path[:0] = [%r, %r, %r]; import repet; import test_gpu_online_start as t; "
            "x = np.array(t.signal(31)); got, (idx, cnt), n = t.offline_run(x, t.FS, 33, lists=True); "
            "xs = np.stack([t.signal(51, t.TOTAL), t.signal(52, t.TOTAL)]); "
            "h = repet.online_streams(t.FS, t.CH, 2, start_length=t.start_length(40)); "
            "live = np.concatenate([t.drive(h, xs, t.grid_sizes(t.TOTAL, [t.P1], 7), {t.P1: lambda h: h.restart(1)}), h.finish()], axis=1); "
            "np.savez(sys.argv[1], got=got, idx=idx, cnt=cnt, live=live)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = code % (os.path.join(root, "repet-python_amd"), root, os.path.join(root, "tests"))
    want, lists = restated(31, 33)
    runs = {}
    for peaks, gram in (("", ""), ("block", ""), ("", "f32"), ("block", "f32")):
        out = str(tmp_path / f"start_{peaks or 'wave'}_{gram or 'f16'}.npz")
        env = dict(os.environ)
        if peaks:
            env["REPET_PEAKS"] = peaks
        if gram:
            env["REPET_GRAM"] = gram
        subprocess.check_call([sys.executable, "-c", code, out], env=env, timeout=120)
        with np.load(out) as z:
            runs[(peaks, gram)] = {k: z[k] for k in z.files}
    for key, r in runs.items():
        wrong = [k for k, row in enumerate(lists)
                 if r["cnt"][k] != len(row) or set(r["idx"][k, :r["cnt"][k]].tolist()) != set(int(v) for v in row)]
        err = rms_err(r["got"], want)
        print(f"peaks {key[0] or 'wave'} gram {key[1] or 'f16'}: rms {err:.3e}, rows that differ {len(wrong)} of {len(lists)}")
        assert not wrong, (key, wrong[:8])
        assert err <= RMS_TOL, (key, err)
    for gram in ("", "f32"):
        same(runs[("block", gram)]["got"], runs[("", gram)]["got"])
        same(runs[("block", gram)]["live"], runs[("", gram)]["live"])
    same(runs[("", "")]["got"], offline(31, 33))
    same(runs[("", "")]["live"][1, P1:], one_stream(52, P1, TOTAL, 40))
