"""Latency per push of S live 44.1-kHz stereo streams: one ``repet.online_streams`` handle (host chunks and ROCm-tensor
chunks) against S separate ``repet.online`` handles pushed one after another, at 1 and 4 hops per push. Each latency is one
call plus, for device chunks, a synchronize; the streams are first pushed past the 10-s warm-up buffer so that every frame
is active. Prints one JSON document (median and p95 in ms per push, and the audio it carries).

``--churn K``: instead, streams that leave and join one by one. One handle of S slots, device chunks of one hop; on every
K-th push one slot's stream is ended with ``finish_stream`` and a new one begun in it with ``restart`` (round robin over
the slots). Reported: the latency of the pushes without a lifecycle call, of ``restart`` and of ``finish_stream`` (each
call plus a synchronize), beside the same schedule on S separate ``repet.online`` handles, the only other way to end one
stream and keep the rest: every hop is S pushes, a departure is one handle's ``finish`` and a new ``repet.online``.

``--which background,foreground,both``: the one-handle device-chunk cases once per selection, one after another in the same
session (``one_handle_device_chunks`` is the background's; the others carry their name).

``--migrate 1``: instead, a stream moved between slots. One handle of S slots past its warm-up, device chunks of one hop; after
every timed push one slot's stream is exported (``export_stream(slot, device=True)``) and imported into the spare slot
(``import_stream``), each call timed with a synchronize; the host forms (payload through host memory) a few times beside them.
In the same run, what a caller without these calls would do to keep a stream's background: replay its last ``buffer_frames``
hops, here as one device push into a restarted one-slot handle (the cheapest form: on the S-slot handle the replay would be
pushed in lockstep through every slot).

``--hold K``: instead, slots that sit out pushes. One handle of S slots past its warm-up, device chunks of one hop into a
preallocated ``out``, each push timed with a synchronize: first on the handle as it is (no ``hold`` was ever called), then, four
times over, ``hold`` of K slots spread over the handle, pushes with them held, ``resume``, pushes with nobody held; ``hold`` and
``resume`` are each timed as one call plus a synchronize.

``--feed 1``: instead, slots fed at their own pace. One handle of S slots past its warm-up, device chunks into a preallocated
``out``, every call timed with a synchronize: plain pushes of one hop before ``enable_feed`` was ever called; then, on the handle
with inboxes of four hops, ``feed`` of one hop to all slots and ``tick`` (each timed alone) alternating with plain pushes; then
packets of 882 samples (20 ms) per slot at staggered phases, one ``feed`` of all packets plus one ``tick`` per packet time, with
the share of slots each tick consumed.

``--start-length SECONDS``: the one-handle cases on handles opened with ``start_length`` (separation from that age on, before
the 10-s buffer has filled). The streams are then pushed only half a second past the start length, so the timed pushes are
those of YOUNG frames, each decided on the frames heard so far; keep ``--timed`` x hops inside the buffer's first 10 s.

``--background-gain G``: the one-handle cases with ``set_background_gain(G)`` made right after the open, so every timed push is
one of the steady state with gains set. ``--gain-change-every K`` (with it): a new gain is also set before every K-th timed push
(outside the clock), so those pushes are each the first one after a set, the ones that fade.

``--levels host|device``: the one-handle cases with a levels call after every timed push, inside the clock: ``device`` is
``last_levels()`` into a preallocated tensor on the device (no host wait of its own), ``host`` the C ABI's host form (one copy
through the pinned buffer and one wait), whatever the chunks are.

``--frames frames|bands``: the one-handle cases with a ``last_frames`` call after every timed push, inside the clock, into a
preallocated tensor on the device (no host wait of its own): ``frames`` the foreground magnitudes ``(S, T, C, F)``, ``bands`` the
foreground's energies in the 32 bands of ``repet.band_edges(fs, 32)``.

``--matches``: the one-handle cases with a ``last_matches`` call after every timed push, inside the clock, into three
preallocated tensors on the device (no host wait of its own).

``--band-gains N``: the one-handle cases with ``set_background_band_gains`` of N mel bands (``repet.band_edges(fs, N)``) with
distinct gains made right after the open, so every timed push carries the second, shaped inverse STFT (use it with ``--which
foreground`` or ``both``). ``--band-gains-change-every K`` (with it): the bands are set again, with the gains rotated, before
every K-th timed push (outside the clock), so those pushes also bring the tables up to date.

``--silent-frames LEGS`` (a comma list of ``off``, ``zero``, ``zero-muted``): instead, what ``silent_frames="zero"`` costs. One
handle of S slots per leg, device chunks of one hop, each push timed with a synchronize, the legs taking turns for ``--rounds``
rounds of ``--timed`` pushes each (every handle goes on with its own streams): ``off`` never names the option, ``zero`` sets it on
streams without silence, ``zero-muted`` sets it on streams of which a quarter of the 10-s buffer -- the frames from 207 to 97
before the end of the warm-up, layout D of tests/silence_reference.py at this rate -- is digital silence and stays in the buffer
through every timed push; a ``--timed`` x ``--rounds`` that would let the mute leave the buffer is refused before anything runs.
The legs take turns in the order given, and rotate by one from round to round so that no leg always runs first. ``--label TEXT``
goes into the document as ``build`` (the commit that was measured). Reported per leg: the median of every round, their range, and the ratio of the medians over all rounds
to the ``off`` leg's. ``REPET_PACKAGE_DIR`` (environment): the directory of the package to time in place of ``repet-python_amd``
-- the ``off`` leg runs on a build without the option, which is how a parent commit is timed on the same machine."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path[:0] = [os.environ.get("REPET_PACKAGE_DIR", "repet-python_amd"), "."]
import repet  # noqa: E402
from repet_synth import synth  # noqa: E402


def stream_signals(S, seconds, fs, ch):
    """S distinct streams from a few synthesised clips (rolled and scaled: synthesis of 256 clips would dominate the run)."""
    base = [synth(seconds, fs, ch, seed) for seed in range(4)]
    return np.stack([np.roll(base[s % 4], 997 * s, axis=0) * (1.0 - 0.001 * s) for s in range(S)])


def stats(lat_s, n, fs):
    lat = np.array(lat_s) * 1e3
    return {"latency_ms_median": round(float(np.median(lat)), 3), "latency_ms_p95": round(float(np.percentile(lat, 95)), 3),
            "audio_ms_per_push": round(1e3 * n / fs, 2), "pushes_timed": len(lat)}


def one_handle(xs, fs, hops, device, timed, warm_s, which="background", start_length=None, gain=None, gain_every=0, levels=None,
               out_dtype=None, frames=None, band_gains=0, band_every=0, matches=False):
    import ctypes
    import torch
    from repet import _native
    S, N, ch = xs.shape
    hop = repet.derive_params(fs).step_length
    n = hops * hop
    # --out-dtype: the hop-sized device pushes fill out= tensors of that torch dtype, allocated once (None: every push returns
    # a fresh float64 tensor, as ever)
    as_dtype = {}
    if out_dtype and device:
        outs = [torch.empty((S, n, ch), dtype=getattr(torch, out_dtype), device="cuda:0") for _ in range(2 if which == "both" else 1)]
        as_dtype = {"out": tuple(outs) if which == "both" else outs[0]}
    src = torch.tensor(xs, device="cuda:0") if device else xs
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    h = repet.online_streams(fs, ch, S, max_push_samples=n, start_length=start_length)
    if gain is not None:
        h.set_background_gain(gain)
    if band_gains > 0:
        band_edges = repet.band_edges(fs, band_gains)
        band_values = (np.arange(band_gains) + 1.0) / (band_gains + 1.0)
        h.set_background_band_gains(band_values, band_edges)
    if start_length is not None:
        warm_s = start_length + 0.5                            # past the start length, far from a full buffer
    pos = 0
    while pos < warm_s * fs:                                   # fill the buffer in half-second pushes
        h.push(src[:, pos:pos + fs // 2], which=which)
        pos += fs // 2
    for _ in range(3):                                         # the per-push workspaces take their size
        h.push(src[:, pos:pos + n], which=which, **as_dtype)
        pos += n
    torch.cuda.synchronize()
    held = free0 - torch.cuda.mem_get_info(0)[0]            # the handle's device memory (and the results torch keeps cached)
    record_dev = torch.empty((S, ch, len(repet.LEVELS)), dtype=torch.float64, device="cuda:0") if levels == "device" else None
    record_host, written = np.empty((S, ch, len(repet.LEVELS))), ctypes.c_int64()
    edges = repet.band_edges(fs, 32) if frames == "bands" else None
    if frames:
        last = 32 if frames == "bands" else repet.derive_params(fs).window_length // 2 + 1
        spectra = torch.empty((S, hops, ch, last), dtype=torch.float64 if frames == "bands" else torch.float32, device="cuda:0")
    if matches:
        cap = h.match_capacity
        lists = (torch.empty((S, hops), dtype=torch.int32, device="cuda:0"), torch.empty((S, hops, cap), dtype=torch.int32, device="cuda:0"),
                 torch.empty((S, hops, cap), dtype=torch.float32, device="cuda:0"))
    lat = []
    for k in range(timed):
        if pos + n > N:
            break
        if gain is not None and gain_every > 0 and k % gain_every == 0:
            h.set_background_gain((gain + 0.01 * (k + 1)) % 1.0)
        if band_gains > 0 and band_every > 0 and k % band_every == 0:
            h.set_background_band_gains(np.roll(band_values, k + 1), band_edges)
        t0 = time.perf_counter()
        h.push(src[:, pos:pos + n], which=which, **as_dtype)
        if levels == "device":
            h.last_levels(out=record_dev)
        elif levels == "host":
            _native.check(_native.lib().repet_online_last_levels(h._handle(), _native.ptr(record_host), record_host.size,
                                                                 ctypes.byref(written)))
        if frames:
            h.last_frames("foreground", bands=edges, out=spectra)
        if matches:
            h.last_matches(out=lists)
        if device:
            torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
        pos += n
    h_start = h.start_frames
    h.close()
    out = stats(lat, n, fs)
    out["device_mb_per_stream"] = round(held / S / 2**20, 1)
    if start_length is not None:
        out["start_frames"] = h_start
        out["stream_age_s_at_last_timed_push"] = round(pos / fs, 2)
    return out


def separate_handles(xs, fs, hops, timed, warm_s):
    S, N, ch = xs.shape
    hop = repet.derive_params(fs).step_length
    n = hops * hop
    hs = [repet.online(fs, ch) for _ in range(S)]
    pos = 0
    while pos < warm_s * fs:
        for s, h in enumerate(hs):
            h.push(xs[s, pos:pos + fs // 2])
        pos += fs // 2
    lat = []
    for _ in range(timed + 3):
        if pos + n > N:
            break
        t0 = time.perf_counter()
        for s, h in enumerate(hs):
            h.push(xs[s, pos:pos + n])
        lat.append(time.perf_counter() - t0)
        pos += n
    for h in hs:
        h.close()
    return stats(lat[3:], n, fs)


def churn_one_handle(xs, fs, every, timed, warm_s):
    import torch
    S, N, ch = xs.shape
    hop = repet.derive_params(fs).step_length
    src = torch.tensor(xs, device="cuda:0")
    h = repet.online_streams(fs, ch, S, max_push_samples=hop)
    pos = 0
    while pos < warm_s * fs // hop * hop:
        n = min(fs // 2 // hop * hop, warm_s * fs // hop * hop - pos)
        h.push(src[:, pos:pos + n])
        pos += n
    out = torch.empty((S, hop, ch), dtype=torch.float64, device="cuda:0")
    tail = torch.empty((hop, ch), dtype=torch.float64, device="cuda:0")
    for _ in range(3):
        h.push(src[:, pos:pos + hop], out=out)
        pos += hop
    # one departure and arrival before the clock starts (the single-slot sequence and the reset kernel have run once); the
    # slots that leave during the run are the oldest ones, so every stream that is finished is longer than the buffer
    h.finish_stream(S - 1, out=tail)
    h.restart(S - 1)
    torch.cuda.synchronize()
    plain, restart, finish, k, slot = [], [], [], 0, 0
    while k < timed and pos + hop <= N:
        t0 = time.perf_counter()
        h.push(src[:, pos:pos + hop], out=out)
        torch.cuda.synchronize()
        plain.append(time.perf_counter() - t0)
        pos += hop
        k += 1
        if k % every == 0 and slot < S - 1:
            t0 = time.perf_counter()
            h.finish_stream(slot, out=tail)
            torch.cuda.synchronize()
            finish.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            h.restart(slot)
            torch.cuda.synchronize()
            restart.append(time.perf_counter() - t0)
            slot += 1
    h.close()
    ms = lambda v: round(float(np.median(np.array(v) * 1e3)), 3) if v else None
    return {"push_ms_median": ms(plain), "push_ms_p95": round(float(np.percentile(np.array(plain) * 1e3, 95)), 3),
            "finish_stream_ms_median": ms(finish), "restart_ms_median": ms(restart), "pushes_timed": len(plain),
            "lifecycle_pairs": len(finish)}


def churn_separate_handles(xs, fs, every, timed, warm_s):
    S, N, ch = xs.shape
    hop = repet.derive_params(fs).step_length
    hs = [repet.online(fs, ch) for _ in range(S)]
    pos = 0
    while pos < warm_s * fs // hop * hop:
        n = min(fs // 2 // hop * hop, warm_s * fs // hop * hop - pos)
        for s, h in enumerate(hs):
            h.push(xs[s, pos:pos + n])
        pos += n
    for _ in range(3):
        for s, h in enumerate(hs):
            h.push(xs[s, pos:pos + hop])
        pos += hop
    plain, finish, reopen, k, slot = [], [], [], 0, 0
    while k < timed and pos + hop <= N:
        t0 = time.perf_counter()
        for s, h in enumerate(hs):
            h.push(xs[s, pos:pos + hop])
        plain.append(time.perf_counter() - t0)
        pos += hop
        k += 1
        if k % every == 0 and slot < S - 1:
            t0 = time.perf_counter()
            hs[slot].finish()
            finish.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            hs[slot].close()
            hs[slot] = repet.online(fs, ch)
            reopen.append(time.perf_counter() - t0)
            slot += 1
    for h in hs:
        h.close()
    ms = lambda v: round(float(np.median(np.array(v) * 1e3)), 3) if v else None
    return {"hop_ms_median": ms(plain), "finish_ms_median": ms(finish), "close_and_open_ms_median": ms(reopen),
            "hops_timed": len(plain), "lifecycle_pairs": len(finish)}


def migrate_one_handle(xs, fs, timed, warm_s):
    import torch
    S, N, ch = xs.shape
    p = repet.derive_params(fs)
    hop, B = p.step_length, p.buffer_frames
    src = torch.tensor(xs, device="cuda:0")
    h = repet.online_streams(fs, ch, S, max_push_samples=hop)
    h.release(S - 1)                                           # the spare slot every export is imported into
    pos = 0
    while pos < warm_s * fs // hop * hop:
        n = min(fs // 2 // hop * hop, warm_s * fs // hop * hop - pos)
        h.push(src[:, pos:pos + n])
        pos += n
    out = torch.empty((S, hop, ch), dtype=torch.float64, device="cuda:0")
    for _ in range(3):
        h.push(src[:, pos:pos + hop], out=out)
        pos += hop
    h.import_stream(S - 1, h.export_stream(0, device=True))    # (both launches have run once before the clock starts)
    torch.cuda.synchronize()
    plain, export, load, k = [], [], [], 0
    while k < timed and pos + hop <= N:
        t0 = time.perf_counter()
        h.push(src[:, pos:pos + hop], out=out)
        torch.cuda.synchronize()
        plain.append(time.perf_counter() - t0)
        pos += hop
        t0 = time.perf_counter()
        state = h.export_stream(k % (S - 1), device=True)
        torch.cuda.synchronize()
        export.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        h.import_stream(S - 1, state)
        torch.cuda.synchronize()
        load.append(time.perf_counter() - t0)
        k += 1
    export_host, load_host = [], []
    for k in range(5):
        t0 = time.perf_counter()
        state = h.export_stream(k, device=False)
        export_host.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        h.import_stream(S - 1, state)
        torch.cuda.synchronize()
        load_host.append(time.perf_counter() - t0)
    nbytes = h.stream_state_nbytes
    h.close()
    one = repet.online_streams(fs, ch, 1, max_push_samples=B * hop)
    back = torch.empty((1, B * hop, ch), dtype=torch.float64, device="cuda:0")
    one.push(src[:1, pos - B * hop:pos], out=back[:, :one.emit_count(B * hop)])
    torch.cuda.synchronize()
    replay = []
    for _ in range(5):
        t0 = time.perf_counter()
        one.restart(0)
        one.push(src[:1, pos - B * hop:pos], out=back[:, :one.emit_count(B * hop)])
        torch.cuda.synchronize()
        replay.append(time.perf_counter() - t0)
    one.close()
    ms = lambda v: round(float(np.median(np.array(v) * 1e3)), 3) if v else None
    return {"payload_bytes": nbytes, "hop_ms": round(1e3 * hop / fs, 2), "push_ms_median": ms(plain),
            "export_device_ms_median": ms(export), "import_device_ms_median": ms(load),
            "export_host_ms_median": ms(export_host), "import_host_ms_median": ms(load_host),
            "replay_buffer_one_slot_ms_median": ms(replay), "replay_hops": B, "calls_timed": len(export)}


def hold_one_handle(xs, fs, n_held, timed, warm_s):
    import torch
    S, N, ch = xs.shape
    hop = repet.derive_params(fs).step_length
    src = torch.tensor(xs, device="cuda:0")
    h = repet.online_streams(fs, ch, S, max_push_samples=hop)
    pos = 0
    while pos < warm_s * fs // hop * hop:
        n = min(fs // 2 // hop * hop, warm_s * fs // hop * hop - pos)
        h.push(src[:, pos:pos + n])
        pos += n
    out = torch.empty((S, hop, ch), dtype=torch.float64, device="cuda:0")
    for _ in range(3):
        h.push(src[:, pos:pos + hop], out=out)
        pos += hop
    torch.cuda.synchronize()

    def pushes(count):
        nonlocal pos
        lat = []
        while len(lat) < count and pos + hop <= N:
            t0 = time.perf_counter()
            h.push(src[:, pos:pos + hop], out=out)
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t0)
            pos += hop
        return lat

    def call(fn, slots):
        t0 = time.perf_counter()
        fn(slots)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    never = pushes(timed)                                      # no hold call was ever made on this handle
    slots = list(range(0, S, max(1, S // n_held)))[:n_held]    # (spread over the handle)
    h.hold(slots)
    pushes(3)                                                  # (the held slide has run once before the clock starts)
    h.resume(slots)
    held, hold, resume, after = [], [], [], []
    for _ in range(4):
        hold.append(call(h.hold, slots))
        held += pushes(timed // 4)
        resume.append(call(h.resume, slots))
        after += pushes(timed // 4)
    h.close()
    ms = lambda v: round(float(np.median(np.array(v) * 1e3)), 3) if v else None
    return {"hop_ms": round(1e3 * hop / fs, 2), "slots_held": len(slots), "push_ms_median_no_hold_call": ms(never),
            "push_ms_p95_no_hold_call": round(float(np.percentile(np.array(never) * 1e3, 95)), 3),
            "push_ms_median_slots_held": ms(held), "push_ms_median_after_resume": ms(after),
            "hold_ms_median": ms(hold), "resume_ms_median": ms(resume), "pushes_timed": len(never)}


def feed_one_handle(xs, fs, timed, warm_s, packet=882):
    import torch
    S, N, ch = xs.shape
    hop = repet.derive_params(fs).step_length
    src = torch.tensor(xs, device="cuda:0")
    h = repet.online_streams(fs, ch, S, max_push_samples=hop)
    pos = 0
    while pos < warm_s * fs // hop * hop:
        n = min(fs // 2 // hop * hop, warm_s * fs // hop * hop - pos)
        h.push(src[:, pos:pos + n])
        pos += n
    out = torch.empty((S, hop, ch), dtype=torch.float64, device="cuda:0")
    for _ in range(3):
        h.push(src[:, pos:pos + hop], out=out)
        pos += hop
    torch.cuda.synchronize()
    slots = list(range(S))
    clock = lambda t0: (torch.cuda.synchronize(), time.perf_counter() - t0)[1]
    before = []                                                # plain pushes before enable_feed was ever called
    for _ in range(timed):
        t0 = time.perf_counter()
        h.push(src[:, pos:pos + hop], out=out)
        before.append(clock(t0))
        pos += hop
    h.enable_feed(4 * hop)
    plain, feed, tick, both = [], [], [], []
    for k in range(2 * timed + 6):
        chunk = src[:, pos:pos + hop]
        pos += hop
        if k % 2:                                              # plain pushes between the ticks, on the handle with inboxes
            t0 = time.perf_counter()
            h.push(chunk, out=out)
            plain.append(clock(t0))
            continue
        t0 = time.perf_counter()
        h.feed(slots, chunk)
        t1 = clock(t0)
        t2 = time.perf_counter()
        h.tick(out=out)
        t3 = clock(t2)
        if k >= 6:                                             # (the take and feed kernels have run before the clock starts)
            feed.append(t1), tick.append(t3), both.append(t1 + t3)
    # packets that never match the hop: every slot gets `packet` samples per packet time, at a phase of its own
    for s in range(S):
        lead = (s * 131) % hop
        if lead:
            h.feed(s, src[s, pos:pos + lead])
    cursor = [pos + (s * 131) % hop for s in range(S)]
    ragged, share, writes = [], [], 0
    staged = torch.empty((S, packet, ch), dtype=torch.float64, device="cuda:0")
    for k in range(timed + 3):
        if max(cursor) + packet > N:
            break
        for s in range(S):
            staged[s] = src[s, cursor[s]:cursor[s] + packet]
            cursor[s] += packet
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.feed(slots, staged)
        h.tick(out=out)
        t1 = clock(t0)
        if k >= 3:
            ragged.append(t1)
            share.append(float(h.last_consumed.mean()))
    h.close()
    ms = lambda v: round(float(np.median(np.array(v) * 1e3)), 3) if v else None
    p95 = lambda v: round(float(np.percentile(np.array(v) * 1e3, 95)), 3) if v else None
    return {"hop_ms": round(1e3 * hop / fs, 2), "inbox_hops": 4,
            "push_ms_median_no_enable_feed": ms(before), "push_ms_p95_no_enable_feed": p95(before),
            "push_ms_median_with_inboxes": ms(plain),
            "feed_ms_median": ms(feed), "feed_ms_p95": p95(feed), "tick_ms_median": ms(tick), "tick_ms_p95": p95(tick),
            "feed_plus_tick_ms_median": ms(both),
            "packet_samples": packet, "ragged_feed_plus_tick_ms_median": ms(ragged), "ragged_feed_plus_tick_ms_p95": p95(ragged),
            "ragged_share_of_slots_consumed": round(float(np.mean(share)), 3) if share else None,
            "calls_timed": len(both), "ragged_ticks_timed": len(ragged)}


def silent_frames_legs(xs, fs, legs, timed, warm_s, rounds):
    import torch
    S, N, ch = xs.shape
    p = repet.derive_params(fs)
    hop, B = p.step_length, p.buffer_frames
    warm = int(round(warm_s * fs / hop)) * hop
    muted = np.array(xs)
    first = warm - 207 * hop + 3
    muted[:, first: first + 110 * hop + p.window_length] = 0
    end = warm + (3 + rounds * timed) * hop                    # the last timed push ends here
    if end > N or first < end - B * hop:                       # (before anything runs on the device)
        raise SystemExit("--silent-frames: %d rounds of %d pushes leave the clip, or let the mute leave the 10-s buffer" % (rounds, timed))
    handles, sources, lat = {}, {}, {}
    for leg in legs:
        kw = {} if leg == "off" else {"silent_frames": "zero"}
        handles[leg] = repet.online_streams(fs, ch, S, max_push_samples=hop, **kw)
        sources[leg] = torch.tensor(muted if leg == "zero-muted" else xs, device="cuda:0")
        lat[leg] = []
        pos = 0
        while pos < warm:                                      # fill the buffer in half-second pushes
            n = min(fs // 2, warm - pos)
            handles[leg].push(sources[leg][:, pos:pos + n])
            pos += n
        for _ in range(3):                                     # the per-push workspaces take their size
            handles[leg].push(sources[leg][:, pos:pos + hop])
            pos += hop
    torch.cuda.synchronize()
    for r in range(rounds):
        start = pos + r * timed * hop
        for leg in legs[r % len(legs):] + legs[:r % len(legs)]:
            h, src, at, mine = handles[leg], sources[leg], start, []
            for _ in range(timed):
                t0 = time.perf_counter()
                h.push(src[:, at:at + hop])
                torch.cuda.synchronize()
                mine.append(time.perf_counter() - t0)
                at += hop
            lat[leg].append(mine)
    out = {}
    for leg in legs:
        handles[leg].close()
        medians = [round(float(np.median(np.array(m) * 1e3)), 4) for m in lat[leg]]
        out[leg] = {"per_hop_ms_median_by_round": medians, "per_hop_ms_range": [min(medians), max(medians)],
                    "per_hop_ms_median": round(float(np.median(np.concatenate(lat[leg]) * 1e3)), 4), "pushes_timed": rounds * timed}
    if "off" in out:
        for leg in legs:
            out[leg]["ratio_to_off"] = round(out[leg]["per_hop_ms_median"] / out["off"]["per_hop_ms_median"], 4)
    if "zero" in out and "zero-muted" in out:
        out["zero-muted"]["ratio_to_zero"] = round(out["zero-muted"]["per_hop_ms_median"] / out["zero"]["per_hop_ms_median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--silent-frames", default=None, metavar="LEGS",
                    help="the silent-frames leg: a comma list of off / zero / zero-muted (see above)")
    ap.add_argument("--label", default=None, help="with --silent-frames: recorded as `build`, the commit that was measured")
    ap.add_argument("--rounds", type=int, default=3, help="with --silent-frames: rounds the legs take turns for")
    ap.add_argument("--feed", type=int, default=0, help="1: the feed leg (feed / tick of slots fed at their own pace)")
    ap.add_argument("--hold", type=int, default=0, metavar="K", help="the hold leg: pushes of one hop with K of the slots held")
    ap.add_argument("--migrate", type=int, default=0, help="1: the migrate leg (export_stream / import_stream per call)")
    ap.add_argument("--streams", default="1,8,64,256")
    ap.add_argument("--hops", default="1,4")
    ap.add_argument("--timed", type=int, default=60, help="pushes timed per case")
    ap.add_argument("--separate-max", type=int, default=64, help="largest S run as S separate repet.online handles")
    ap.add_argument("--only", choices=["all", "device"], default="all", help="device: the one-handle device-chunk cases only")
    ap.add_argument("--churn", type=int, default=0, metavar="K",
                    help="the churn leg: one finish_stream and one restart on every K-th push of one hop")
    ap.add_argument("--churn-separate", type=int, default=1, help="0: skip the separate-handles side of the churn leg")
    ap.add_argument("--which", default="background",
                    help="comma list of background / foreground / mixture / both: what the one-handle device pushes deliver")
    ap.add_argument("--start-length", type=float, default=None, metavar="SECONDS",
                    help="open the one-handle cases with this start_length and time pushes of young frames (see above)")
    ap.add_argument("--background-gain", type=float, default=None, metavar="G",
                    help="set this background gain on the one-handle cases right after the open (see above)")
    ap.add_argument("--gain-change-every", type=int, default=0, metavar="K",
                    help="with --background-gain: set a new gain before every K-th timed push")
    ap.add_argument("--levels", choices=["host", "device"], default=None,
                    help="a levels call after every timed push of the one-handle cases, inside the clock (see above)")
    ap.add_argument("--frames", choices=["frames", "bands"], default=None,
                    help="a last_frames call after every timed push of the one-handle cases, inside the clock (see above)")
    ap.add_argument("--matches", action="store_true",
                    help="a last_matches call after every timed push of the one-handle cases, inside the clock (see above)")
    ap.add_argument("--band-gains", type=int, default=0, metavar="N",
                    help="set_background_band_gains of N mel bands with distinct gains after the open (one-handle cases)")
    ap.add_argument("--band-gains-change-every", type=int, default=0, metavar="K",
                    help="with --band-gains: set the bands again before every K-th timed push")
    ap.add_argument("--out-dtype", choices=["float64", "float32", "int16", "float16", "bfloat16"], default=None,
                    help="the hop-sized one-handle device pushes fill out= tensors of this dtype (default: fresh float64 results)")
    args = ap.parse_args()
    fs, ch, warm_s = 44100, 2, 11
    streams = [int(s) for s in args.streams.split(",")]
    if args.silent_frames:
        legs = args.silent_frames.split(",")
        if not legs or any(leg not in ("off", "zero", "zero-muted") for leg in legs):
            ap.error("--silent-frames takes a comma list of off, zero, zero-muted")
        hop = repet.derive_params(fs).step_length
        result = {"fs": fs, "channels": ch, "rounds": args.rounds, "legs": legs, "cases": []}
        if args.label:
            result["build"] = args.label
        for S in streams:
            xs = stream_signals(S, warm_s + 1 + (args.rounds * args.timed + 8) * hop / fs, fs, ch)
            result["cases"].append(dict({"streams": S}, **silent_frames_legs(xs, fs, legs, args.timed, warm_s, args.rounds)))
        print(json.dumps(result, indent=1))
        return
    if args.feed > 0:
        hop = repet.derive_params(fs).step_length
        result = {"fs": fs, "channels": ch, "cases": []}
        for S in streams:
            xs = stream_signals(S, warm_s + 1 + (4 * args.timed + 24) * hop / fs, fs, ch)
            result["cases"].append(dict({"streams": S}, **feed_one_handle(xs, fs, args.timed, warm_s)))
        print(json.dumps(result, indent=1))
        return
    if args.hold > 0:
        hop = repet.derive_params(fs).step_length
        result = {"fs": fs, "channels": ch, "cases": []}
        for S in streams:
            xs = stream_signals(S, warm_s + 1 + (3 * args.timed + 16) * hop / fs, fs, ch)
            result["cases"].append(dict({"streams": S}, **hold_one_handle(xs, fs, min(args.hold, S), args.timed, warm_s)))
        print(json.dumps(result, indent=1))
        return
    if args.migrate > 0:
        hop = repet.derive_params(fs).step_length
        result = {"fs": fs, "channels": ch, "cases": []}
        for S in streams:
            xs = stream_signals(S, warm_s + 1 + (args.timed + 8) * hop / fs, fs, ch)
            result["cases"].append(dict({"streams": S}, **migrate_one_handle(xs, fs, args.timed, warm_s)))
        print(json.dumps(result, indent=1))
        return
    if args.churn > 0:
        hop = repet.derive_params(fs).step_length
        result = {"fs": fs, "channels": ch, "churn_every_pushes": args.churn, "cases": []}
        for S in streams:
            xs = stream_signals(S, warm_s + 1 + (args.timed + 8) * hop / fs, fs, ch)
            case = {"streams": S, "one_handle_slots": churn_one_handle(xs, fs, args.churn, args.timed, warm_s)}
            if args.churn_separate and S <= args.separate_max:
                case["separate_handles_host"] = churn_separate_handles(xs, fs, args.churn, args.timed, warm_s)
            result["cases"].append(case)
        print(json.dumps(result, indent=1))
        return
    hops_list = [int(h) for h in args.hops.split(",")]
    hop = repet.derive_params(fs).step_length
    seconds = warm_s + 1 + (args.timed + 4) * max(hops_list) * hop / fs
    result = {"fs": fs, "channels": ch, "cases": []}
    if args.start_length is not None:
        result["start_length_s"] = args.start_length
    if args.background_gain is not None:
        result["background_gain"] = args.background_gain
        result["gain_change_every"] = args.gain_change_every
    if args.levels is not None:
        result["levels"] = args.levels
    if args.out_dtype is not None:
        result["out_dtype"] = args.out_dtype
    if args.frames is not None:
        result["frames"] = args.frames
    if args.matches:
        result["matches"] = True
    if args.band_gains > 0:
        result["band_gains"] = args.band_gains
        result["band_gains_change_every"] = args.band_gains_change_every
    for S in streams:
        xs = stream_signals(S, seconds, fs, ch)
        for hops in hops_list:
            case = {"streams": S, "hops_per_push": hops}
            for which in args.which.split(","):
                key = "one_handle_device_chunks" + ("" if which == "background" else "_" + which)
                case[key] = one_handle(xs, fs, hops, True, args.timed, warm_s, which, args.start_length, args.background_gain,
                                       args.gain_change_every, args.levels, args.out_dtype, args.frames, args.band_gains,
                                       args.band_gains_change_every, args.matches)
            if args.only == "all":
                case["one_handle_host_chunks"] = one_handle(xs, fs, hops, False, args.timed, warm_s, start_length=args.start_length,
                                                            gain=args.background_gain, gain_every=args.gain_change_every,
                                                            levels=args.levels)
                if S <= args.separate_max:
                    case["separate_handles_host"] = separate_handles(xs, fs, hops, args.timed, warm_s)
            result["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
    one = {(c["streams"], c["hops_per_push"]): c["one_handle_device_chunks"]["latency_ms_median"] for c in result["cases"]
           if "one_handle_device_chunks" in c}
    result["device_push_ratio_to_S1"] = {f"S{S}_{h}hop": round(one[(S, h)] / one[(1, h)], 2)
                                         for (S, h) in one if (1, h) in one}
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
