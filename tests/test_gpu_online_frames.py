"""The spectra of a live handle's last frames (``last_frames`` of ``repet.online_streams`` / ``repet.online``; include/repet_hip.h:
repet_online_last_frames*, repet_online_last_band_energies*): for the frames a push completed, the fp32 magnitudes of the
mixture, of the masked spectrum (background) and their difference (foreground), whole or summed into bands.

Expected values come from the float64 statement of tests/frames_reference.py (tied to the oracle by
tests/test_frames_reference.py), on the signals of tests/test_gpu_online_start.py. Bars, none of them fitted:

  mix   2e-6 x max |want|      the STFT stage test's bar for X (tests/test_gpu_stft_stages.py): |X| is one rounded square, one fma
                               and a 1-ulp square root of it
  bg    2.5e-6 x max |want|    a median and a minimum pick values, they do not amplify their error; the mask's divide and the
                               two products add a few fp32 roundings of a value <= max
  fg    4.5e-6 x max |want|    the sum of the two
  (max |want| over the stream's whole statement of that signal, for bg and fg over its frames past the warm-up: only those are
  compared, and none is left out: the similar-frame lists of these signals are the reference's)
  bands F x 2**-53 relative, against the float64 sum of squares of the device's own ``last_frames`` output: a sum of F
        non-negative float64 terms (the squares of fp32 values are exact in float64) cannot be further off in any order
  everything else              exact: bit for bit

The largest error met per check is collected in PARITY and printed (and written to $REPET_FRAMES_PARITY_OUT) by the last test:
profiles/online_frames_parity.txt is that output from an MI355X."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from frames_reference import band_energies, frames_from
from oracle import repet_oracle as orc
from test_gpu_online_foreground import to_numpy
from test_gpu_online_start import signal
from test_gpu_online_streams import lockstep_sizes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 8000
W, H, B, F, CUT = 512, 256, 312, 257, 6
M_YOUNG = 33                                  # start_frames of the start_length cases: similarity_distance is 31 frames
N = (B + 20) * H + 77
BARS = {"mixture": 2e-6, "background": 2.5e-6, "foreground": 4.5e-6}
WHICH = ("mixture", "background", "foreground")
PARITY = {}


def note(check, err, bar, shape):
    ratio = err / bar if bar > 0 else 0.0
    if check not in PARITY or ratio > PARITY[check][0]:
        PARITY[check] = (ratio, err, bar, shape)


def bits(a):
    a = to_numpy(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    """Identical bits; a NaN matches a NaN (the payload of a NaN is not part of any promise)."""
    a, b = to_numpy(a), to_numpy(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    differ = (bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))
    assert not differ.any(), f"{int(differ.sum())} of {differ.size} values differ"


def geometry(fs):
    p = repet.derive_params(fs)
    return p.window_length, p.step_length, p.buffer_frames, p.window_length // 2 + 1, p.cutoff_bins


def open_streams(streams, channels, m=None, fs=FS):
    h = geometry(fs)[1]
    handle = repet.online_streams(fs, channels, streams, start_length=None if m is None else m * h / fs)
    assert handle.start_frames == (m or geometry(fs)[2])
    return handle


@functools.lru_cache(maxsize=None)
def statement(seed, m, n, fs, ch):
    """(mix, bg, fg), each (T, C, F) float64, of signal(seed, n, fs, ch) separated from frame m - 1 on: computed once, shared,
    left unchanged."""
    _, mix, bg, fg = frames_from(np.array(signal(seed, n, fs, ch)), fs, m)
    for a in (mix, bg, fg):
        a.setflags(write=False)
    return {"mixture": mix, "background": bg, "foreground": fg}


def frames_done(pushed, w, h):
    return (pushed - w) // h + 1 if pushed >= w else 0


def three(handle, **kw):
    """mixture, background and foreground of the last push from three separate calls, with the exact relations between them."""
    got = {which: to_numpy(handle.last_frames(which, **kw)) for which in WHICH}
    mix, bg, fg = (got[w] for w in WHICH)
    assert mix.dtype == bg.dtype == fg.dtype == np.float32 and mix.shape == bg.shape == fg.shape
    with np.errstate(invalid="ignore"):
        same_bits(fg, np.maximum(mix - bg, np.float32(0)))
    return got


def check_push(handle, got, first, seeds, m, n, fs, label):
    """One push's frames against the statement: parity past the warm-up, the exact rules everywhere."""
    w, h, b, f, cut = geometry(fs)
    mix, bg, fg = (got[k] for k in WHICH)
    count = mix.shape[1]
    assert mix.shape[3] == f
    for s, seed in enumerate(seeds):
        want = statement(seed, m, n, fs, mix.shape[2])
        warm = np.arange(first, first + count) < m - 1
        # warm-up frames: nothing removed; the high-pass bins of every other frame: the mask is 1
        assert not bg[s, warm].any()
        same_bits(fg[s, warm], mix[s, warm])
        same_bits(bg[s, ~warm][..., 1:cut + 1], mix[s, ~warm][..., 1:cut + 1])
        assert not fg[s, ~warm][..., 1:cut + 1].any()
        for which in WHICH:
            rows = slice(None) if which == "mixture" else ~warm
            ref = want[which][first:first + count][rows]
            if not ref.size:
                continue
            top = float(np.max(np.abs(want[which] if which == "mixture" else want[which][m - 1:])))
            err = float(np.max(np.abs(got[which][s][rows].astype(np.float64) - ref)))
            note(f"{which} fs={fs} C={mix.shape[2]} M={m}", err, BARS[which] * top, f"{label} stream {s}")
            assert err <= BARS[which] * top, (which, label, s, err, BARS[which] * top)


def run_parity(seeds, channels, m, n, fs, sizes):
    w, h, b, f, cut = geometry(fs)
    m_eff = m or b
    xs = np.stack([signal(seed, n, fs, channels) for seed in seeds])
    handle = open_streams(len(seeds), channels, m, fs)
    with pytest.raises(ValueError, match="stale"):
        handle.last_frame_range
    pos, seen_empty, seen_many, separated = 0, False, False, 0
    for size in sizes + [None]:
        before = frames_done(pos, w, h)
        if size is None:
            handle.finish()
            after = orc.online_frame_count(n, w, h)
        else:
            handle.push(xs[:, pos:pos + size])
            pos += size
            after = frames_done(pos, w, h)
        assert handle.last_frame_range == (before, after - before)
        got = three(handle)
        assert got["mixture"].shape == (len(seeds), after - before, channels, f)
        seen_empty |= after == before
        seen_many |= after - before > 2
        separated += max(0, after - max(before, m_eff - 1))
        check_push(handle, got, before, seeds, m_eff, n, fs, f"push of {size}")
    assert pos == n and seen_empty and seen_many and separated > 3
    again = three(handle)                                        # finish's zero-padded frame, a second time: identical bits
    for which in WHICH:
        same_bits(again[which], got[which])
    handle.close()


# ---- 1. parity with the float64 statement, push by push ------------------------------------------------------------------------
@pytest.mark.parametrize("streams,channels,m", [(3, 2, M_YOUNG), (1, 1, None), (3, 1, M_YOUNG), (1, 2, None)])
def test_parity_per_push(streams, channels, m):
    sizes = lockstep_sizes(N, FS, seed=FS + channels + streams)
    assert 0 in sizes and 3 * H in sizes and max(sizes) > B * H
    run_parity([31, 32, 33][:streams], channels, m, N, FS, sizes)


def test_parity_44k_mono_partial_last_group():
    fs = 44100
    w, h, b, f, cut = geometry(fs)
    assert (w, f) == (2048, 1025) and f % 4 == 1                 # a last 16-byte group of one bin
    n = 9 * h + 333
    run_parity([33, 34], 1, 2, n, fs, [h - 1, 1, 3 * h, 0, h + 7, 4 * h, n - (9 * h + 7)])


# ---- 2. forms: host and device, repeated, strided ----------------------------------------------------------------------------
def test_host_and_device_forms_and_strided_destinations():
    S, C, m = 3, 2, M_YOUNG
    n = (m + 6) * H + W
    xs = np.stack([signal(seed, N, FS, C)[:n] for seed in (31, 32, 33)])
    handle = open_streams(S, C, m)
    handle.push(xs)
    first, count = handle.last_frame_range
    assert (first, count) == (0, m + 7)
    host = three(handle)
    for which in WHICH:
        assert isinstance(handle.last_frames(which), np.ndarray)
        dense = torch.full((S, count, C, F), 7.0, dtype=torch.float32, device=DEV)
        assert handle.last_frames(which, out=dense) is dense
        same_bits(dense, host[which])
        same_bits(handle.last_frames(which, out=dense), host[which])                       # a repeated call
        # channels first, every other bin of a wider buffer: the gaps stay as they were
        wide = torch.full((S, C, count, 2 * F), 7.0, dtype=torch.float32, device=DEV)
        view = wide[..., ::2].permute(0, 2, 1, 3)
        assert view.shape == dense.shape and view.stride(3) == 2
        handle.last_frames(which, out=view)
        same_bits(view.contiguous(), host[which])
        assert bool((wide[..., 1::2] == 7.0).all())
        # bins side by side but rows that begin off a 16-byte boundary
        odd = torch.full((S * count * C * F + 1,), 7.0, dtype=torch.float32, device=DEV)
        handle.last_frames(which, out=odd[1:].view(S, count, C, F))
        same_bits(odd[1:].view(S, count, C, F), host[which])
        assert float(odd[0]) == 7.0
        into = np.full((S, count, C, F), 7.0, dtype=np.float32)
        assert handle.last_frames(which, out=into) is into
        same_bits(into, host[which])
    for bad in (torch.empty((S, count, C, F), dtype=torch.float64, device=DEV), torch.empty((S, count, C, F + 1), dtype=torch.float32, device=DEV),
                torch.empty((count, C, F), dtype=torch.float32, device=DEV).expand(S, count, C, F), np.empty((S, count, C, F)),
                torch.empty((S, count, C, F), dtype=torch.float32)):
        with pytest.raises(ValueError):
            handle.last_frames("mixture", out=bad)
    with pytest.raises(ValueError, match="one signal"):
        handle.last_frames("both")
    same_bits(handle.last_frames("mixture"), host["mixture"])                              # refusals change nothing
    # after a device chunk the result is a tensor, and equals the host chunk's
    twin = open_streams(S, C, m)
    twin.push(torch.from_numpy(xs).to(DEV))
    for which in WHICH:
        got = twin.last_frames(which)
        assert isinstance(got, torch.Tensor) and got.device == torch.device(DEV) and got.dtype == torch.float32
        same_bits(got, host[which])
    bands = twin.last_frames("background", bands=[0, 7, F])
    assert isinstance(bands, torch.Tensor) and bands.dtype == torch.float64
    same_bits(bands, handle.last_frames("background", bands=[0, 7, F]))
    handle.close()
    twin.close()


def test_one_stream_handle_has_no_stream_axis():
    C, m = 2, M_YOUNG
    n = (m + 3) * H + W
    x = signal(31, N, FS, C)[:n]
    one, many = repet.online(FS, C, start_length=m * H / FS), open_streams(1, C, m)
    assert one.start_frames == m
    with pytest.raises(ValueError, match="stale"):
        one.last_frames()
    one.push(x)
    many.push(x[None])
    assert one.last_frame_range == many.last_frame_range == (0, m + 4)
    for which in WHICH:
        got = one.last_frames(which)
        assert isinstance(got, np.ndarray) and got.shape == (m + 4, C, F)
        same_bits(got, many.last_frames(which)[0])
        out = torch.empty((m + 4, C, F), dtype=torch.float32, device=DEV)
        assert one.last_frames(which, out=out) is out
        same_bits(out, got)
    same_bits(one.last_frames("foreground", bands=[0, 10, 100, F]), many.last_frames("foreground", bands=[0, 10, 100, F])[0])
    one.close()
    many.close()


# ---- 3. slots that are not live, and NaN --------------------------------------------------------------------------------------
def test_idle_held_and_restarted_slots_are_zero_whatever_the_chunk_carried():
    S, C, m = 3, 2, M_YOUNG
    xs = np.stack([signal(seed, N, FS, C) for seed in (31, 32, 33)])
    handle = open_streams(S, C, m)
    handle.push(xs[:, :40 * H])
    handle.release([1])
    handle.hold([2])
    handle.restart([0])                                          # slot 0's stream begins at sample 40 H: its frame 0 is frame 40
    chunk = np.array(xs[:, 40 * H:43 * H])
    chunk[1:] = np.nan                                           # the idle and the held slot's share
    chunk[0, 5, 0] = np.nan                                      # ... and in frames 39 and 40 of slot 0, channel 0
    handle.push(chunk)
    assert handle.last_frame_range == (39, 3)
    got = three(handle)
    bands = to_numpy(handle.last_frames("mixture", bands=[0, 1, 100, F]))
    for which in WHICH:
        g = got[which]
        assert not bits(g[1:]).any()                             # idle, held: +0 in every bit
        assert not bits(g[0, 0]).any()                           # the frame that straddles the restart
    assert not bits(bands[1:]).any() and not bits(bands[0, 0]).any()
    mix, bg, fg = (got[k][0] for k in WHICH)
    assert np.isnan(mix[1, 0]).all() and not np.isnan(mix[1, 1]).any() and not np.isnan(mix[2]).any()
    assert mix[1, 1].any() and mix[2].any()
    assert not bg.any()                                          # frames 40 and 41 are the new stream's frames 0 and 1: warm-up
    same_bits(fg[1:], mix[1:])
    assert np.isnan(bands[0, 1, 0]).all() and np.isfinite(bands[0, 1, 1]).all() and (bands[0, 2] > 0).all()
    handle.close()


def test_a_nan_sample_shows_in_its_own_frames_and_channel_only():
    """The mixture is NaN in exactly the frames and the channel that hold the sample. The background and the foreground are
    the reference's own quantities, and the reference's mask of such a frame is NaN in BOTH channels (the similarity is formed
    from the channel mean) except on the high-pass bins, where it is 1 -- and in the next frames for as long as its lists are
    empty: their NaN positions must be the float64 statement's. The other slots are untouched."""
    S, C, m = 3, 2, M_YOUNG
    xs = np.stack([signal(seed, N, FS, C) for seed in (31, 32, 33)])
    handle, twin = open_streams(S, C, m), open_streams(S, C, m)
    for h in (handle, twin):
        h.push(xs[:, :50 * H])
    chunk = np.array(xs[:, 50 * H:54 * H])
    twin.push(chunk)
    clean = three(twin)
    chunk[1, H + 10, 1] = np.nan                                 # sample 51 H + 10 of slot 1, channel 1: frames 50 and 51
    handle.push(chunk)
    assert handle.last_frame_range == twin.last_frame_range == (49, 4)
    got = three(handle)
    heard = np.concatenate((xs[1, :50 * H], chunk[1]))
    with np.errstate(invalid="ignore"):
        statement_nan = [np.isnan(a[49:53]) for a in frames_from(heard, FS, m)[1:]]
    for which, want_nan in zip(WHICH, statement_nan):
        g = got[which]
        nan = np.isnan(g)
        print(which, "NaN bins per (slot, frame, channel):", nan.sum(axis=-1).tolist())
        assert not nan[[0, 2]].any() and np.array_equal(nan[1], want_nan), which
        same_bits(g[[0, 2]], clean[which][[0, 2]])                # the other slots: untouched
        same_bits(g[1, 0], clean[which][1, 0])                    # the frame before
    mix_nan = np.zeros(got["mixture"].shape, dtype=bool)
    mix_nan[1, 1:3, 1] = True
    assert np.array_equal(np.isnan(got["mixture"]), mix_nan)
    same_bits(got["mixture"][1, :, 0], clean["mixture"][1, :, 0])  # the other channel's magnitudes
    assert np.isnan(got["background"][1, 1:3]).any(axis=-1).all()  # NaN where the mixture or the mask is NaN ...
    same_bits(got["background"][1, 1:3, 0, 1:CUT + 1], got["mixture"][1, 1:3, 0, 1:CUT + 1])   # ... and the mixture where the mask is 1
    for which in WHICH:
        e = to_numpy(handle.last_frames(which, bands=[0, 1, CUT + 1, 50, F]))
        assert np.array_equal(np.isnan(e), np.isnan(band_energies(got[which], [0, 1, CUT + 1, 50, F]))), which
    handle.close()
    twin.close()


# ---- 4. bands ---------------------------------------------------------------------------------------------------------------------
def band_lists(fs, f):
    return {"mel 32": repet.band_edges(fs, 32),
            "mel 24 in 100..3000 Hz": repet.band_edges(fs, 24, 100.0, 3000.0),
            "empty and single-bin bands": [0, 1, 2, 2, 3, 3, f - 1, f],
            "one band": [0, f],
            "128 bands": [int(v) for v in np.round(np.linspace(0, f, 129))],
            "128 bands, most of them empty": [0] * 100 + list(range(29))}


@pytest.mark.parametrize("fs,channels,m", [(FS, 2, M_YOUNG), (44100, 1, 2)])
def test_band_energies(fs, channels, m):
    w, h, b, f, cut = geometry(fs)
    S = 3
    n = (m + 4) * h + w + 5
    xs = np.stack([signal(seed, n, fs, channels) for seed in (31, 32, 33)])
    handle = open_streams(S, channels, m, fs)
    handle.push(xs)
    count = handle.last_frame_range[1]
    assert count == m + 5
    for which in WHICH:
        frames = to_numpy(handle.last_frames(which))
        for name, edges in band_lists(fs, f).items():
            got = handle.last_frames(which, bands=edges)
            assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (S, count, channels, len(edges) - 1)
            want = band_energies(frames, edges)
            err = np.abs(got - want)
            bound = f * 2.0 ** -53 * want
            assert (err <= bound).all(), (which, name, float(np.max(err - bound)))
            with np.errstate(invalid="ignore", divide="ignore"):
                note(f"bands {which} fs={fs}", float(np.nanmax(np.where(want > 0, err / want, 0.0))), f * 2.0 ** -53, name)
            empty = [k for k in range(len(edges) - 1) if edges[k] == edges[k + 1]]
            assert not bits(got[..., empty]).any()
            same_bits(handle.last_frames(which, bands=edges), got)                             # a repeated call
            dev = torch.full(got.shape, 7.0, dtype=torch.float64, device=DEV)
            assert handle.last_frames(which, bands=edges, out=dev) is dev
            same_bits(dev, got)                                                               # the device form
            same_bits(handle.last_frames(which, bands=np.asarray(edges, dtype=np.int64)), got)
        assert want.any()
    handle.close()


def test_bad_bands_are_refused_and_change_nothing():
    S, C, m = 2, 1, 2
    xs = np.stack([signal(seed, N, FS, C)[:6 * H] for seed in (31, 32)])
    handle = open_streams(S, C, m)
    handle.push(xs)
    good = [0, 3, 50, F]
    want = handle.last_frames("foreground", bands=good)
    frames = handle.last_frames("foreground")
    for bad in ([0, 5, 3], [0, F + 1], [-1, 4], [4], [], [0.5, 3.0], [[0, 1]]):
        with pytest.raises(ValueError):
            handle.last_frames("foreground", bands=bad)
        with pytest.raises(ValueError):
            handle.last_frames("foreground", bands=bad, out=torch.empty((S, 5, C, 2), dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="128"):
        handle.last_frames("foreground", bands=list(range(130)))                            # 129 bands
    with pytest.raises(ValueError):
        handle.last_frames("foreground", bands=good, out=torch.empty((S, 5, C, 3), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        handle.last_frames("foreground", bands=good, out=torch.empty((S, 5, C, 6), dtype=torch.float64, device=DEV)[..., ::2])
    same_bits(handle.last_frames("foreground", bands=good), want)
    same_bits(handle.last_frames("foreground"), frames)
    assert handle.last_frame_range == (0, 5)
    handle.close()


# ---- 5. lifecycle -----------------------------------------------------------------------------------------------------------------
def stale(handle):
    with pytest.raises(ValueError, match="stale"):
        handle.last_frame_range
    for kw in ({}, {"bands": [0, F]}, {"out": torch.empty((2, 1, 1, F), dtype=torch.float32, device=DEV)}):
        with pytest.raises(ValueError, match="stale"):
            handle.last_frames("mixture", **kw)


def test_the_record_follows_the_pushes_and_goes_stale():
    S, C, m = 2, 1, 2
    xs = np.stack([signal(seed, N, FS, C) for seed in (31, 32)])
    handle = open_streams(S, C, m)
    stale(handle)
    pos = 0

    def push(hops):
        nonlocal pos
        before = frames_done(pos, W, H)
        handle.push(xs[:, pos:pos + hops * H])
        pos += hops * H
        assert handle.last_frame_range == (before, frames_done(pos, W, H) - before)
        assert handle.last_frames("mixture").shape == (S, frames_done(pos, W, H) - before, C, F)

    push(1)                                                      # no frame yet: an empty result, not an error
    assert handle.last_frame_range == (0, 0)
    assert handle.last_frames("mixture", bands=[0, F]).shape == (S, 0, C, 1)
    push(5)
    handle.restart([1])
    stale(handle)
    push(2)
    handle.release([1])
    stale(handle)
    push(1)
    handle.hold([0])
    stale(handle)
    push(2)
    assert not bits(handle.last_frames("mixture")).any()         # slot 0 held, slot 1 idle
    handle.resume([0])
    stale(handle)
    push(3)
    state = handle.export_stream(0)
    assert handle.last_frame_range[1] == 3                        # an export leaves the record alone
    handle.finish_stream(0)
    stale(handle)
    push(1)
    handle.import_stream(1, state)
    stale(handle)
    push(2)
    assert handle.last_frames("mixture")[1].any()
    handle.close()
    # an import of a stream older than the handle moves the handle's epoch: the range stays in the caller's pushes
    young = open_streams(S, C, m)
    young.push(xs[:, :2 * H])
    assert young.last_frame_range == (0, 1)
    young.import_stream(0, state)
    stale(young)
    young.push(xs[:, 2 * H:5 * H])
    assert young.last_frame_range == (1, 3)
    got = young.last_frames("mixture")
    assert got.shape == (S, 3, C, F) and got[0].any() and got[1].any()
    young.finish()
    assert young.last_frame_range == (4, orc.online_frame_count(5 * H, W, H) - 4)
    young.close()


# ---- 6. nothing changed for others -------------------------------------------------------------------------------------------
def test_asking_changes_nothing_of_the_time_domain_output():
    S, C, m = 3, 2, M_YOUNG
    n = (m + 12) * H + 77
    xs = np.stack([signal(seed, N, FS, C)[:n] for seed in (31, 32, 33)])
    sizes = [0, 100, 3 * H, (m + 2) * H, 1, H, 5 * H + 9]
    sizes.append(n - sum(sizes))
    asked, plain = open_streams(S, C, m), open_streams(S, C, m)
    pos = 0
    for size in sizes + [None]:
        outs = []
        for h in (asked, plain):
            outs.append(h.finish(which="both") if size is None else h.push(xs[:, pos:pos + size], which="both"))
            if h is asked:
                for which in WHICH:
                    h.last_frames(which)
                    h.last_frames(which, bands=repet.band_edges(FS, 20))
                    h.last_frames(which, out=torch.empty((S, h.last_frame_range[1], C, F), dtype=torch.float32, device=DEV))
        pos += size or 0
        for a, b in zip(*outs):
            assert a.dtype == np.float64 and np.array_equal(a, b)
        for which in ("background", "foreground", "mixture"):
            assert np.array_equal(asked.last_emission(which), plain.last_emission(which))
    asked.close()
    plain.close()


def test_zz_report_the_largest_errors():
    """Last in the module: the table profiles/online_frames_parity.txt is made of (check, max error, bar, where)."""
    lines = ["%-34s err %.3e  bar %.3e  (%.2f of the bar)  %s" % (check, err, bar, ratio, shape)
             for check, (ratio, err, bar, shape) in sorted(PARITY.items())]
    print("\n".join(lines))
    path = os.environ.get("REPET_FRAMES_PARITY_OUT")
    if path and lines:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
