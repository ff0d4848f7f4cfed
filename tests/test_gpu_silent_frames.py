"""Live streams and ``simonline`` separated through digital silence (``silent_frames="zero"`` of ``repet.online``,
``repet.online_streams`` and ``repet.separate``; include/repet_hip.h: REPET_FLAG_SILENT_FRAMES_ZERO). The reference is the float64
statement of tests/silence_reference.py (tied to ``simonline_from`` and the oracle by tests/test_silence_reference.py): the
offline engine with the bit must give its similar-frame lists on EVERY processed row -- the silent rows empty -- and its samples
within RMS_TOL, without a NaN; every live form must equal that offline run bit for bit; a clip without a silent frame and a
handle without the option must give the bits they gave before.

8 kHz, W = 512, H = 256, B = 312, similarity_distance = 31 frames; clips of (B + 20) H + 77 samples, the silence layouts of
tests/silence_reference.py (A: inside the first buffer, off the hop grid, exactly one frame, one channel only; B: among young
rows; C: a call that begins muted; D: a mute longer than 2 d + 1 frames; E: A plus a NaN sample)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet import _native
from oracle import repet_oracle as orc
from repet_synth import synth
from helpers import rms_err
from silence_reference import mute, silent_frames_of, simonline_silence
from test_gpu_online_streams import same
from test_gpu_online_start import grid_sizes, push_sizes, start_length
from test_gpu_variants import RMS_TOL

pytestmark = pytest.mark.gpu

FS, CH = 8000, 2
W, H, B = 512, 256, 312
N = (B + 20) * H + 77
T = B + 20
PCM = 4000                                             # int16 clips: the float clip (peaks below 0.1) at a speech level in PCM units


@functools.lru_cache(maxsize=None)
def signal(seed, n=N, ch=CH):
    x = synth(n / FS + 0.01, FS, ch, seed)[:n].astype(np.float32).astype(np.float64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def clip(name, ch=CH, pcm=False):
    """(samples, start_frames) of layout `name` on synth seed 5: float32-exact float64, or int16 PCM. Shared, left unchanged."""
    x = signal(5, N, ch)
    assert not silent_frames_of(x, W, H).any()         # the clip has no silent frame of its own
    if pcm:
        x = np.round(x * PCM)
        assert np.abs(x).max() < 32768 and not silent_frames_of(x, W, H).any()
    y, m = mute(x, name, W, H, B)
    if pcm:
        y = y.astype(np.int16)
    y.setflags(write=False)
    return y, m


@functools.lru_cache(maxsize=None)
def restated(name, ch=CH, pcm=False):
    """The float64 statement for clip(name, ...): (samples, lists, silent frames), computed once, shared, left unchanged."""
    x, m = clip(name, ch, pcm)
    trace = orc.Trace()
    want = simonline_silence(np.array(x, dtype=np.float64), FS, m, trace=trace)
    want.setflags(write=False)
    return want, trace.items["similarity_indices"], trace.items["silent"]


def params(rule):
    p = repet.derive_params(FS)
    assert (p.window_length, p.step_length, p.buffer_frames, p.sim_distance_frames) == (W, H, B, 31)
    if rule is not None:
        p.flags |= _native.silent_frames_flag(rule)
    return p


def offline_run(x, m, rule, lists=False):
    """simonline of one clip on a context of its own: start_frames m, silent_frames rule (None: the flags as derived)."""
    p = params(rule)
    ctx = repet.Context(0)
    if m != B:
        ctx.set_online_start(m)
    ctx.upload(np.array(x))
    ctx.execute("simonline", p)
    got = ctx.download()
    out = got
    if lists:
        rows = ctx.last_frame_count() - m + 1
        out = (got, ctx.last_sim_indices(rows, p.sim_number))
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def offline(name, rule="zero", ch=CH, pcm=False):
    x, m = clip(name, ch, pcm)
    got = offline_run(x, m, rule)
    got.setflags(write=False)
    return got


def length(m):
    return None if m == B else start_length(m)


# ---- 1. offline against the statement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ch,pcm", [("A", 2, False), ("B", 2, False), ("C", 2, False), ("D", 2, False), ("E", 2, False),
                                         ("A", 1, False), ("A", 2, True)])
def test_offline_equals_the_float64_statement(name, ch, pcm):
    x, m = clip(name, ch, pcm)
    want, lists, silent = restated(name, ch, pcm)
    got, (idx, cnt) = offline_run(x, m, "zero", lists=True)
    assert len(lists) == T - m + 1 == len(cnt) and silent.any()             # (layout C: the silent frames are columns only)
    wrong = [k for k, row in enumerate(lists)
             if cnt[k] != len(row) or set(idx[k, :cnt[k]].tolist()) != set(int(v) for v in row)]
    nan_w, nan_g = np.isnan(want), np.isnan(got)
    err = rms_err(got[~nan_w & ~nan_g], want[~nan_w & ~nan_g])
    print(f"layout {name} ch {ch} pcm {pcm}: rms {err:.3e}, rows that differ {len(wrong)} of {len(lists)}, "
          f"silent rows {int(silent[m - 1:].sum())}, NaN {int(nan_g.sum())} against {int(nan_w.sum())}")
    assert not wrong, f"rows {wrong[:8]} (frames from {m - 1}) differ from the float64 statement"
    for k in np.flatnonzero(silent[m - 1:]):
        assert cnt[k] == 0 and (idx[k] == -1).all()                         # no allowance for silent rows: they are empty
    assert all(not silent[idx[k, :cnt[k]]].any() for k in range(len(cnt)))  # and in nobody's list
    assert np.array_equal(nan_g, nan_w)
    assert err <= RMS_TOL, f"rms {err:.3e}"
    if name != "E":
        assert not nan_g.any()
    else:                                                                   # the NaN frames: exactly where the reference rule puts them
        with np.errstate(all="ignore"):
            ref = np.isnan(orc.simonline(np.array(x), FS))
        at = np.flatnonzero(np.isnan(x[:, 0]))[0]
        assert nan_g[(at // H - 1) * H: (at // H) * H + W].all() and nan_g.sum() == 3 * H * ch      # its two frames, both channels
        assert ref[nan_g].all() and ref.sum() > nan_g.sum()
    assert not got[: (m - 1) * H].any()


def test_offline_44k_stereo_register_fft():
    """W = 2048: the forward kernel of stft_reg.hip (the 8-kHz cases run stft_pair_kernel for stereo and stft_kernel for mono;
    stft_wave_kernel is behind REPET_FFT_PATH=wave in the last test). A mute of three windows off the hop grid and one of
    exactly one frame behind the warm-up; the statement's lists on every row, its samples within RMS_TOL, no NaN."""
    fs = 44100
    p = repet.derive_params(fs)
    w, h, b = p.window_length, p.step_length, p.buffer_frames
    assert (w, h, b) == (2048, 1024, 431)
    n = (b + 10) * h
    x = synth(n / fs + 0.01, fs, 2, 7)[:n].astype(np.float32).astype(np.float64)
    assert not silent_frames_of(x, w, h).any()
    x[(b + 1) * h + 7: (b + 1) * h + 7 + 3 * w] = 0                         # frames b + 2 .. b + 5
    x[(b + 8) * h: (b + 8) * h + w] = 0                                     # frame b + 8, the last
    x[300 * h + 5: 340 * h] = 0                                             # and a long one inside the first buffer
    trace = orc.Trace()
    want = simonline_silence(x, fs, b, trace=trace)
    lists, silent = trace.items["similarity_indices"], trace.items["silent"]
    assert silent[b - 1:].sum() == 5 and silent[:b - 1].sum() > 31
    p.flags |= _native.FLAG_SILENT_FRAMES_ZERO
    ctx = repet.Context(0)
    ctx.upload(x)
    ctx.execute("simonline", p)
    got = ctx.download()
    idx, cnt = ctx.last_sim_indices(len(lists), p.sim_number)
    ctx.close()
    wrong = [k for k, row in enumerate(lists)
             if cnt[k] != len(row) or set(idx[k, :cnt[k]].tolist()) != set(int(v) for v in row)]
    err = rms_err(got, want)
    print(f"44.1 kHz stereo: rms {err:.3e}, rows that differ {len(wrong)} of {len(lists)}")
    assert not wrong, wrong[:8]
    assert np.isfinite(got).all() and err <= RMS_TOL
    h1 = repet.online(fs, 2, silent_frames="zero")
    live = np.concatenate([h1.push(x[: (b + 3) * h + 100]), h1.push(x[(b + 3) * h + 100:]), h1.finish()])
    h1.close()
    same(live, got)


# ---- 2. every live form equals the offline run bit for bit -------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("A", "hops"), ("A", "big"), ("A", "offgrid"), ("B", "offgrid"), ("C", "hops"), ("D", "big"),
                                       ("E", "offgrid")])
def test_one_stream_equals_offline(name, kind):
    x, m = clip(name)
    x = np.array(x)
    h = repet.online(FS, CH, start_length=length(m), silent_frames="zero")
    assert h.silent_frames == "zero" and h.start_frames == m
    bgs, fgs, pos = [], [], 0
    for n in push_sizes(kind, N):
        bg, fg = h.push(x[pos:pos + n], which="both")
        bgs.append(bg)
        fgs.append(fg)
        pos += n
    bg, fg = h.finish(which="both")
    h.close()
    bg, fg = np.concatenate(bgs + [bg]), np.concatenate(fgs + [fg])
    same(bg, offline(name))
    same(fg, x - bg)                                                        # a finite foreground that is the input minus the background
    if name != "E":
        assert np.isfinite(bg).all() and np.isfinite(fg).all()


def drive(h, xs, sizes, actions=None, **kw):
    """Push xs (S, N, C) in lockstep; actions: {position: fn(h)} run before the push that starts there. (S, emitted, C)."""
    actions = dict(actions or {})
    pieces, pos = [], 0
    for n in sizes:
        if pos in actions:
            actions.pop(pos)(h)
        pieces.append(h.push(xs[:, pos:pos + n], **kw))
        pos += n
    assert not actions and pos == xs.shape[1]
    return np.concatenate(pieces, axis=1)


@pytest.mark.parametrize("name", ["A", "B"])
def test_a_slot_restarted_among_older_slots(name):
    x, m = clip(name)
    P1 = 30 * H
    total = P1 + N
    xs = np.stack([signal(51, total), np.concatenate([signal(52, P1), x]), signal(53, total)])
    xs[2, 50 * H: 60 * H] = 0                                              # an older slot with a mute of its own
    h = repet.online_streams(FS, CH, 3, start_length=length(m), silent_frames="zero")
    assert h.silent_frames == "zero"
    lock = drive(h, xs, grid_sizes(total, [P1], 7), {P1: lambda h: h.restart(1)})
    whole = np.concatenate([lock, h.finish()], axis=1)
    h.close()
    assert np.isfinite(whole).all()
    same(whole[1, P1:], offline(name))
    same(whole[0], offline_run(xs[0], m, "zero"))
    same(whole[2], offline_run(xs[2], m, "zero"))


def test_feed_and_tick_with_160_sample_packets():
    x, m = clip("A")
    other = signal(61)
    h = repet.online_streams(FS, CH, 2, silent_frames="zero")
    h.enable_feed(4 * H)
    pieces = []
    for at in range(0, N, 160):
        h.feed([0, 1], np.stack([x[at:at + 160], other[at:at + 160]]))
        while h.queued(0) >= H:
            out = h.tick(1)
            assert h.last_consumed.all()
            pieces.append(out)
    pads = h.pad_feed()
    assert pads[0] == pads[1] == (-N) % H
    pieces.append(h.tick(1))
    assert h.queued(0) == 0
    tails = [h.finish_stream(0), h.finish_stream(1)]
    h.close()
    lock = np.concatenate(pieces, axis=1)
    same(np.concatenate([lock[0], tails[0]])[:N], offline("A"))
    same(np.concatenate([lock[1], tails[1]])[:N], offline_run(other, B, "zero"))


def test_a_slot_held_across_part_of_a_silence():
    x, m = clip("A")
    x = np.array(x)
    hold_at, held_hops = (B + 6) * H, 5                                     # inside [(B + 4) H + 7, (B + 10) H + 7): frames B + 5 .. B + 8 are silent
    other = signal(62, N + held_hops * H)
    h = repet.online_streams(FS, CH, 2, silent_frames="zero")
    mine, pos, cur = [], 0, 0
    sizes = [hold_at] + [H] * held_hops + [3 * H, N - hold_at - 3 * H]
    for k, n in enumerate(sizes):
        held = 1 <= k <= held_hops
        if k == 1:
            h.hold(0)
        if k == held_hops + 1:
            h.resume(0)
        chunk = np.full((2, n, CH), np.nan)
        chunk[1] = other[pos:pos + n]
        if not held:
            chunk[0] = x[cur:cur + n]
            cur += n
        got = h.push(chunk)
        pos += n
        if held:
            assert not got[0].any()
        else:
            mine.append(got[0])
    tail = h.finish()
    h.close()
    assert cur == N
    same(np.concatenate(mine + [tail[0]]), offline("A"))


def test_a_stream_exported_mid_silence_and_imported_elsewhere():
    x, m = clip("A")
    x = np.array(x)
    cut = (B + 7) * H                                                       # frames B + 5 .. B + 8 are silent: two done, two to come
    other = signal(63, N)
    a = repet.online_streams(FS, CH, 2, silent_frames="zero")
    first = drive(a, np.stack([x[:cut], other[:cut]]), grid_sizes(cut, [], 8))
    state = a.export_stream(0)
    assert state.flags & _native.FLAG_SILENT_FRAMES_ZERO
    a.close()
    b = repet.online_streams(FS, CH, 2, silent_frames="zero")
    lead = 20 * H
    b.push(np.stack([other[:lead], other[:lead]]))
    b.import_stream(1, state)
    rest = np.stack([other[lead: lead + N - cut], x[cut:]])
    lock = drive(b, rest, grid_sizes(N - cut, [], 9))
    tail = b.finish_stream(1)
    b.close()
    life = np.concatenate([first[0], lock[1], tail])
    assert first[0].shape[0] == cut - H and life.shape[0] == N
    same(life, offline("A"))


# ---- 3. / 4. nothing moves without silence, and nothing moves without the option ---------------------------------------
def test_without_a_silent_frame_both_rules_give_the_same_bits():
    x = np.array(signal(5))
    plain = offline_run(x, B, "reference")
    same(offline_run(x, B, "zero"), plain)
    same(offline_run(x, 64, "zero"), offline_run(x, 64, "reference"))
    for rule in ("reference", "zero"):
        h = repet.online(FS, CH, silent_frames=rule)
        got = np.concatenate([h.push(x[: (B + 5) * H]), h.push(x[(B + 5) * H:]), h.finish()])
        h.close()
        same(got, plain)
    xt = torch.tensor(x, device="cuda:0")
    same(repet.separate("simonline", xt, FS, silent_frames="zero"), plain)
    same(repet.separate("simonline", xt, FS), plain)


def test_the_default_still_answers_silence_with_nan():
    x, m = clip("A")
    x = np.array(x)
    with np.errstate(all="ignore"):
        want = orc.simonline(x, FS)
    nan = np.isnan(want)
    assert nan.sum() == 1792 * CH                                           # seven hops in both channels
    fresh = offline_run(x, B, None)
    assert np.array_equal(np.isnan(fresh), nan)
    assert rms_err(fresh[~nan], want[~nan]) <= RMS_TOL
    same(offline_run(x, B, "reference"), fresh)
    same(repet.simonline(x, FS), fresh)
    for kw in ({}, {"silent_frames": "reference"}):
        h = repet.online(FS, CH, **kw)
        assert h.silent_frames == "reference"
        got = np.concatenate([h.push(x[: (B + 5) * H]), h.push(x[(B + 5) * H:]), h.finish()])
        h.close()
        same(got, fresh)
    h = repet.online_streams(FS, CH, 1)
    assert h.silent_frames == "reference"
    same(np.concatenate([h.push(x[None]), h.finish()], axis=1)[0], fresh)
    h.close()
    xt = torch.tensor(x, device="cuda:0")
    same(repet.separate("simonline", xt, FS), fresh)
    same(repet.separate("simonline", xt, FS, silent_frames="zero"), offline("A"))


# ---- 5. the read-outs -----------------------------------------------------------------------------------------------
def test_read_outs_on_silent_frames():
    x, m = clip("A")
    x = np.array(x)
    _, lists, silent = restated("A")
    h = repet.online(FS, CH, silent_frames="zero")
    K = h.match_capacity
    sizes = [(B - 2) * H] + [H] * 4 + [3 * H] + [H] * 14 + [N - (B + 19) * H]
    assert sum(sizes) == N
    pos, seen, bgs = 0, 0, []
    for n in sizes:
        bg, fg = h.push(x[pos:pos + n], which="both")
        bgs.append(bg)
        pos += n
        assert np.isfinite(bg).all() and np.isfinite(fg).all()
        levels = h.last_levels()
        assert np.isfinite(levels).all()
        first, count = h.last_frame_range
        if count == 0:
            continue
        frames = {which: h.last_frames(which) for which in ("mixture", "background", "foreground")}
        matches = h.last_matches()
        for k in range(count):
            j = first + k
            assert all(np.isfinite(frames[w][k]).all() for w in frames)
            if silent[j]:
                assert all(not frames[w][k].any() for w in frames), j       # zero in all three signals
            if j < B - 1:
                continue
            want = sorted(int(v) for v in lists[j - (B - 1)])
            got = sorted(j - int(a) for a in matches.age[k, :matches.count[k]])
            assert got == want, (j, got, want)
            assert not silent[got].any()                                    # no silent frame in any list
            if silent[j]:
                seen += 1
                assert matches.count[k] == 0 and (matches.age[k] == -1).all() and not matches.similarity[k].any()
            else:
                assert matches.count[k] >= 1 and frames["mixture"][k].any()
    bg = h.finish()
    h.close()
    assert seen == 5                                                        # frames B + 5 .. B + 8 and B + 14
    same(np.concatenate(bgs + [bg]), offline("A"))


def test_shaped_foreground_and_narrow_destinations():
    x, m = clip("A")
    xs = np.array(x)[None]
    # band gains: half of the background's bass stays in the foreground -- shaped from a background that is 0 on the silent frames
    h = repet.online_streams(FS, CH, 1, silent_frames="zero")
    F = W // 2 + 1
    h.set_background_band_gains([0.5, 0.0, 1.0], edges=[0, 8, 64, F])
    bg, fg = h.push(xs, which="both")
    tb, tf = h.finish(which="both")
    h.close()
    bg, fg = np.concatenate([bg, tb], axis=1)[0], np.concatenate([fg, tf], axis=1)[0]
    same(bg, offline("A"))
    assert np.isfinite(fg).all()
    quiet = slice((B + 6) * H, (B + 9) * H)                                 # samples only silent frames cover: input, background, shaped background 0
    assert not xs[0, quiet].any() and not bg[quiet].any() and not fg[quiet].any()
    # float16 out of a float clip, int16 out of a PCM clip: the cast of the float64 result, which holds no NaN to hide
    xt = torch.tensor(xs, device="cuda:0")
    h = repet.online_streams(FS, CH, 1, silent_frames="zero")
    got = torch.cat([h.push(xt, dtype=torch.float16), h.finish(dtype=torch.float16)], dim=1)[0]
    h.close()
    assert got.dtype == torch.float16 and bool(torch.isfinite(got).all())
    assert torch.equal(got.cpu(), torch.tensor(np.array(offline("A"))).to(torch.float16))
    pcm, _ = clip("A", CH, True)
    pt = torch.tensor(np.array(pcm)[None], device="cuda:0")
    assert pt.dtype == torch.int16
    h = repet.online_streams(FS, CH, 1, silent_frames="zero")
    got = torch.cat([h.push(pt, dtype=torch.int16), h.finish(dtype=torch.int16)], dim=1)[0]
    h.close()
    want = offline("A", "zero", CH, True)
    assert np.isfinite(want).all()
    assert np.array_equal(got.cpu().numpy(), np.rint(want).astype(np.int16))


# ---- 6. refusals change nothing ------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    """One refusal at a time, each followed by a push of one hop on a handle of either rule: what the handle has emitted so far
    must still be the front of the uninterrupted run, so no refusal can hide what another one disturbed."""
    x, m = clip("A")
    x = np.array(x)
    lib = _native.lib()
    cut = (B + 7) * H                                                       # mid-silence: frames B + 5 .. B + 8 are silent
    handles = {"zero": repet.online_streams(FS, CH, 1, silent_frames="zero"), "reference": repet.online_streams(FS, CH, 1)}
    pieces = {rule: [h.push(x[None, :cut])] for rule, h in handles.items()}
    pos = cut
    xt = torch.tensor(x, device="cuda:0")
    p = params("zero")

    def import_across_rules():
        states = {rule: h.export_stream(0) for rule, h in handles.items()}
        assert states["zero"].flags & _native.FLAG_SILENT_FRAMES_ZERO and not states["reference"].flags & _native.FLAG_SILENT_FRAMES_ZERO
        for rule, other in (("zero", "reference"), ("reference", "zero")):
            with pytest.raises(ValueError):
                handles[rule].import_stream(0, states[other])

    def sim_with_the_keyword():
        with pytest.raises(ValueError, match="simonline"):
            repet.separate("sim", xt, FS, silent_frames="zero")

    def an_unknown_string():
        with pytest.raises(ValueError, match="silent_frames"):
            repet.separate("simonline", xt, FS, silent_frames="Zero")
        with pytest.raises(ValueError, match="silent_frames"):
            repet.online(FS, CH, silent_frames="0")

    def the_bit_on_repet_run_with_original():
        out = np.full(x.shape, 7.0)
        rc = lib.repet_run(_native.ALGO_IDS["original"], _native.ptr(x), _native.F64, x.shape[0], CH, p, _native.ptr(out), 0, None)
        assert rc == _native.ERR_BAD_ARG and b"REPET_FLAG_SILENT_FRAMES_ZERO" in lib.repet_last_error() and (out == 7.0).all()

    def the_bit_on_a_context_with_the_other_variants():
        ctx = repet.Context(0)
        ctx.upload(x)
        for algo in ("original", "extended", "adaptive", "sim"):
            with pytest.raises(ValueError, match="REPET_FLAG_SILENT_FRAMES_ZERO"):
                ctx.execute(algo, p)
        ctx.execute("simonline", p)                                         # the context is as good as new
        same(ctx.download(), offline("A"))
        ctx.close()

    for refusal in (import_across_rules, sim_with_the_keyword, an_unknown_string, the_bit_on_repet_run_with_original,
                    the_bit_on_a_context_with_the_other_variants):
        refusal()
        for rule, h in handles.items():                                     # the next push of either handle
            pieces[rule].append(h.push(x[None, pos:pos + H]))
            so_far = np.concatenate(pieces[rule], axis=1)[0]
            same(so_far, offline("A", rule)[: so_far.shape[0]])
        pos += H
    for rule, h in handles.items():
        pieces[rule] += [h.push(x[None, pos:]), h.finish()]
        h.close()
        same(np.concatenate(pieces[rule], axis=1)[0], offline("A", rule))


def test_a_batch_context_honours_the_bit():
    names = ("A", "D", "E")
    clips = np.stack([clip(n)[0] for n in names])
    ctx = repet.Context(0)
    ctx.upload_batch(clips)
    ctx.execute("simonline", params("zero"))
    got = ctx.download()
    ctx.close()
    for k, n in enumerate(names):
        same(got[k], offline(n))


# ---- 7. both peak kernels, both band layouts -----------------------------------------------------------------------------
def test_both_peak_kernels_and_both_band_layouts(tmp_path):
    """The kernels behind the switches, as tests/test_gpu_online_start.py reaches them: REPET_PEAKS=block (one workgroup per row
    and the general second level) and REPET_GRAM=f32 (the band as band[t][l] = sim(t, t + l)), each in a process of its own since
    the switches are read once. In all four the offline lists of layouts B (young rows) and D (the long mute) are the float64
    statement's on every row, and the two peak kernels give the same samples bit for bit, offline and for a live stream; a
    fifth child runs the same through REPET_FFT_PATH=wave, the one forward STFT kernel no other case reaches. A child
    pays the import, the first use of the device, two offline cases and one live run -- a few seconds -- so a limit of 120 s is
    generous; a child that meets it has hung."""
    code = ("import sys, numpy as np; sys.path[:0] = [%r, %r, %r]; import repet; import test_gpu_silent_frames as t; "
            "out = {}\n"
            "for name in 'BD':\n"
            "    x, m = t.clip(name); got, (idx, cnt) = t.offline_run(x, m, 'zero', lists=True)\n"
            "    out['got' + name], out['idx' + name], out['cnt' + name] = got, idx, cnt\n"
            "x, m = t.clip('D'); x = np.array(x); h = repet.online(t.FS, t.CH, silent_frames='zero')\n"
            "out['live'] = np.concatenate([h.push(x[:t.N // 2]), h.push(x[t.N // 2:]), h.finish()])\n"
            "np.savez(sys.argv[1], **out)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = code % (os.path.join(root, "repet-python_amd"), root, os.path.join(root, "tests"))
    runs = {}
    for peaks, gram in (("", ""), ("block", ""), ("", "f32"), ("block", "f32"), ("fft-wave", "")):
        out = str(tmp_path / f"silent_{peaks or 'wave'}_{gram or 'f16'}.npz")
        env = dict(os.environ)
        if peaks == "fft-wave":                        # a fifth child: the forward STFT through stft_wave_kernel, all else default
            env["REPET_FFT_PATH"] = "wave"
        elif peaks:
            env["REPET_PEAKS"] = peaks
        if gram:
            env["REPET_GRAM"] = gram
        subprocess.check_call([sys.executable, "-c", code, out], env=env, timeout=120)
        with np.load(out) as z:
            runs[(peaks, gram)] = {k: z[k] for k in z.files}
    for key, r in runs.items():
        for name in "BD":
            want, lists, silent = restated(name)
            idx, cnt = r["idx" + name], r["cnt" + name]
            wrong = [k for k, row in enumerate(lists)
                     if cnt[k] != len(row) or set(idx[k, :cnt[k]].tolist()) != set(int(v) for v in row)]
            err = rms_err(r["got" + name], want)
            print(f"peaks {key[0] or 'wave'} gram {key[1] or 'f16'} layout {name}: rms {err:.3e}, rows that differ {len(wrong)} of {len(lists)}")
            assert not wrong, (key, name, wrong[:8])
            assert err <= RMS_TOL and np.isfinite(r["got" + name]).all(), (key, name, err)
        same(r["live"], r["gotD"])
    for gram in ("", "f32"):
        for k in ("gotB", "gotD", "live"):
            same(runs[("block", gram)][k], runs[("", gram)][k])
    same(runs[("", "")]["gotD"], offline("D"))
    # (the wave-synchronous FFT kernels round differently from the block kernels: its samples are held to the statement above,
    # its lists to every row, not to the default path's bits)
