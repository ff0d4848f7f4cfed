"""Band gains of the live handles (``set_background_band_gains`` of ``repet.online_streams`` / ``repet.online``; include/repet_hip.h:
repet_online_set_background_band_gains): a share of the background kept in the foreground bin by bin.

    a[k] = float32(1 - float64(float32(g[k])));   shaped_bg = overlap-add inverse of a_j[k] * Y_j[k];   fg = fma(-a_s, shaped_bg, x)

Signals and tables are those of tests/band_gains_cases.py (fp32-exact; ``signal`` of tests/test_gpu_online_start.py), the model is
tests/band_gains_reference.py, tied to the frames statement and held to its sensitivity conditions by
tests/test_band_gains_reference.py. The similar-frame lists of these signals are the reference's and no frame is left out.

Bars:
  bit for bit      whatever does not depend on the tables (background, mixture, last_frames, the MIX / BG levels, the exported
                   state, the foregrounds of slots without a table), ``g = 1`` everywhere (the input), the forms of one emission
  against the model  the shaped background is recovered as ``mixture - foreground`` (float64, scalar gain 0) and compared in rms
                   over the separated part of the stream with ``2 E + 2**-22 max |bg_model|``, where ``E = rms(bg_gpu -
                   bg_model)`` of the PLAIN background of the same run (code that does not know of the tables): shaping
                   multiplies every bin's error by a factor <= 1, adds one fp32 rounding per bin and goes through the same
                   inverse; the factor 2 covers that the overlap-add sum of per-frame errors need not shrink monotonically, the
                   second term streams whose E is tiny. Not fitted: the ratio met is printed and collected.
  RMS_TOL          the foreground against ``x - shaped_bg_model``, the project's tolerance for a separated signal

The error met, E and their ratio per check are collected in PARITY and printed (and written to $REPET_BAND_GAINS_PARITY_OUT) by
the last test: profiles/online_band_gains_parity.txt is that output from an MI355X."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from band_gains_cases import B, F, F44, FS, FS44, H, H44, M44, M_YOUNG, N8, N44, TABLES, USES, W, signal
from band_gains_reference import factor, masks_of, shaped_from, table
from emit_dtypes_reference import round_ref
from helpers import rms_err
from levels_reference import BG_ENERGY, BG_PEAK, FG_ENERGY, FG_PEAK, LIVE, MIX_ENERGY, MIX_PEAK, NONFINITE, check as check_levels, levels
from test_gpu_online_background_gain import fade
from test_gpu_online_foreground import to_numpy
from test_gpu_online_start import signal as start_signal
from test_gpu_online_streams import lockstep_sizes, same
from test_gpu_variants import RMS_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PARITY = {}
UNSHAPED = (MIX_ENERGY, BG_ENERGY, MIX_PEAK, BG_PEAK, LIVE, NONFINITE)


def geometry(fs):
    p = repet.derive_params(fs)
    return p.window_length, p.step_length, p.buffer_frames, p.window_length // 2 + 1


def frames_done(pushed, w, h):
    return (pushed - w) // h + 1 if pushed >= w else 0


def rms(a):
    return float(np.sqrt(np.mean(np.square(a)))) if a.size else 0.0


@functools.lru_cache(maxsize=None)
def state(seed, n, fs, ch, m):
    """The model's spectra and masks of signal(seed, n, fs, ch) separated from frame m - 1 on: computed once, shared."""
    return masks_of(np.array(signal(seed, n, fs, ch)), fs, m)


def factors(name, f):
    """The factor row a set of TABLES[name] leaves (None: no table)."""
    return np.ones(f) if name is None else factor(table(f, *TABLES[name]))


def set_table(handle, name, slots=None):
    edges, gains = TABLES[name]
    if slots is None:
        handle.set_background_band_gains(gains, edges)
    else:
        handle.set_background_band_gains(gains, edges, slots)


def open_streams(streams, channels, m, fs=FS):
    h = geometry(fs)[1]
    return repet.online_streams(fs, channels, streams, start_length=None if m is None else m * h / fs)


def drive(handle, xs, sizes, fs, sets=None, probe=None, finish=True, start=None):
    """Push xs (S, N, C) in ``sizes`` with which="both", making the sets of ``sets[k]`` -- (slots, table name or None for a clear)
    -- before call k (k = len(sizes): the finish); ``start``: the table names the slots were given before this call. Returns the concatenated background, foreground and mixture (S, n, C) and,
    per slot and frame, the factor row in force at the call that completed the frame (S, T, F)."""
    w, h, _, f = geometry(fs)
    S, n_total = xs.shape[0], xs.shape[1]
    t_all = state_frames(n_total, fs)
    current = np.stack([factors(name, f) for name in (start or [None] * S)])
    tabs = np.ones((S, t_all, f))
    out = {"background": [], "foreground": [], "mixture": []}
    pos = 0
    for k, n in enumerate(list(sizes) + ([None] if finish else [])):
        for slots, name in (sets or {}).get(k, []):
            if name is None:
                handle.clear_background_band_gains(slots)
            else:
                set_table(handle, name, slots)
            current[list(range(S)) if slots is None else list(slots)] = factors(name, f)
        before = frames_done(pos, w, h)
        if n is None:
            bg, fg = handle.finish(which="both")
            after = t_all
        else:
            bg, fg = handle.push(xs[:, pos:pos + n], which="both")
            pos += n
            after = frames_done(pos, w, h)
        tabs[:, before:after] = current[:, None, :]
        mix = to_numpy(handle.last_emission("mixture"))
        out["background"].append(to_numpy(bg)); out["foreground"].append(to_numpy(fg)); out["mixture"].append(mix)
        if probe:
            probe(k, n, pos, out)
    return {key: np.concatenate(v, axis=1) for key, v in out.items()}, tabs


def state_frames(n, fs):
    from oracle import repet_oracle as orc
    w, h = geometry(fs)[:2]
    return orc.online_frame_count(n, w, h)


def against_model(label, got, s, st, tabs, x, m, h, lo=0, hi=None, wrong=None):
    """Slot s of a run against the model of its stream under the per-frame factor rows ``tabs`` (T, F), over the emitted samples
    [lo, hi) of the stream that lie past the warm-up. Returns the bar (for the caller's own assertions on the model)."""
    bg_model, shaped_model = shaped_from(st, tabs)
    hi = x.shape[0] if hi is None else hi
    part = slice(max(lo, (m - 1) * h), hi)
    bg, fg, mix = (got[key][s] for key in ("background", "foreground", "mixture"))
    same(mix, np.asarray(x))
    shaped = mix - fg
    e_plain = rms((bg - bg_model)[part])
    err = rms((shaped - shaped_model)[part])
    bar = 2 * e_plain + 2.0 ** -22 * float(np.max(np.abs(bg_model)))
    ratio = err / e_plain if e_plain > 0 else float("inf")
    print(f"{label}: shaped background off by {err:.3e} rms, plain E {e_plain:.3e}, ratio {ratio:.3f}, bar {bar:.3e}")
    PARITY[label] = (err, e_plain, ratio, bar)
    assert np.any(shaped_model[part] != bg_model[part]), label
    assert err <= bar, (label, err, bar)
    tol = rms_err(fg[part], (np.asarray(x) - shaped_model)[part])
    assert tol <= RMS_TOL, (label, tol)
    if wrong is not None:
        # the same frames with the NEWEST table on every carried frame: the model must tell the two apart by more than the bar
        _, shaped_wrong = shaped_from(st, wrong)
        apart = rms((shaped_wrong - shaped_model)[part])
        print(f"{label}: the newest table on the carried frames would be off by {apart:.3e} rms")
        assert apart > bar, (label, apart, bar)
        assert rms((shaped - shaped_wrong)[part]) > bar
    return bar


def newest_on_carried(tabs):
    """The factor rows a handle would use that inverted every carried frame with the table of the frames behind it."""
    wrong = tabs.copy()
    changed = np.flatnonzero(np.any(tabs[1:] != tabs[:-1], axis=1))       # frame j + 1 has another row than frame j
    wrong[changed] = tabs[changed + 1]
    return wrong


def test_the_cases_are_the_start_tests_signals():
    assert np.array_equal(signal(31, N8, FS, 2), start_signal(31, N8, FS, 2))
    assert np.array_equal(signal(35, N44, FS44, 2), start_signal(35, N44, FS44, 2))
    assert geometry(FS) == (W, H, B, F) and geometry(FS44)[1:] == (H44, 431, F44)
    assert M44 * H44 / FS44 > 3 * repet.derive_params(FS44).sim_distance_frames * H44 / FS44 and N44 / FS44 < 3.6


# ---- 1 + 2 + 5. bit for bit, against the model, levels ---------------------------------------------------------------------------
CASES = {
    # name: (fs, channels, start_frames, n, [(seed, table)])
    "8k-stereo": (FS, 2, M_YOUNG, N8, [(31, "speech-only"), (32, None), (33, "all")]),
    "8k-mono-reference-start": (FS, 1, None, N8, [(31, "per-bin"), (32, None)]),
    "8k-three-channels": (FS, 3, M_YOUNG, N8, [(31, "duck"), (33, "all")]),
    "44k-mono": (FS44, 1, M44, N44, [(34, "mel44"), (36, None)]),
    "44k-stereo": (FS44, 2, M44, N44, [(35, "per-bin44"), (36, None), (35, "one-bin44")]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_bits_model_and_levels(case):
    fs, ch, m, n, slots = CASES[case]
    w, h, b, f = geometry(fs)
    m_eff = m or b
    S = len(slots)
    xs = np.stack([signal(seed, n, fs, ch) for seed, _ in slots])
    if fs == FS:
        sizes = lockstep_sizes(n, fs, seed=fs + ch + S)
        assert 0 in sizes and 3 * h in sizes and max(sizes) > b * h
    else:
        sizes = [h - 1, 1, (M44 - 1) * h, 0, 3 * h, h + 7, 5 * h]
        sizes.append(n - sum(sizes))
        assert n / fs <= 3.6 and frames_done(sum(sizes[:3]), w, h) >= M44 - 1
    handle, twin = open_streams(S, ch, m, fs), open_streams(S, ch, m, fs)
    for s, (_, name) in enumerate(slots):
        if name is not None:
            set_table(handle, name, [s])
            assert np.array_equal(handle.background_band_gains(s), table(f, *TABLES[name]))
        else:
            assert not handle.background_band_gains(s).any()
    records = {id(handle): [], id(twin): []}

    def probe_of(hd):
        def probe(k, size, pos, out):
            rec = to_numpy(hd.last_levels())
            want = levels(out["mixture"][-1], out["background"][-1], out["foreground"][-1])
            check_levels(rec, want, f"{case}: call {k}")                   # FG_* measure the foreground as emitted: the shaped one
            frames = {which: to_numpy(hd.last_frames(which)) for which in ("mixture", "background", "foreground")}
            again = to_numpy(hd.last_emission("foreground"))
            assert again.tobytes() == to_numpy(hd.last_emission("foreground")).tobytes() == out["foreground"][-1].tobytes()
            if out["foreground"][-1].size:
                dev = hd.last_emission("foreground", out=torch.empty(out["foreground"][-1].shape, dtype=torch.float64, device=DEV))
                assert to_numpy(dev).tobytes() == again.tobytes()
            records[id(hd)].append((rec, frames))
        return probe

    got, tabs = drive(handle, xs, sizes, fs, probe=probe_of(handle), start=[name for _, name in slots])
    plain, _ = drive(twin, xs, sizes, fs, probe=probe_of(twin))
    handle.close(); twin.close()
    # what does not depend on the tables: bit for bit
    assert got["background"].tobytes() == plain["background"].tobytes() and got["mixture"].tobytes() == plain["mixture"].tobytes()
    for (rec, frames), (rec0, frames0) in zip(records[id(handle)], records[id(twin)]):
        assert rec[..., UNSHAPED].tobytes() == rec0[..., UNSHAPED].tobytes()
        for which in frames:
            assert frames[which].tobytes() == frames0[which].tobytes()
    for s, (seed, name) in enumerate(slots):
        if name is None:
            assert got["foreground"][s].tobytes() == plain["foreground"][s].tobytes()
            for (rec, _), (rec0, _) in zip(records[id(handle)], records[id(twin)]):
                assert rec[s].tobytes() == rec0[s].tobytes()
        elif name == "all":
            same(got["foreground"][s], got["mixture"][s])                  # g = 1 on every bin: the input
            assert np.any(plain["foreground"][s] != plain["mixture"][s])
        else:
            assert (name, seed, n, fs, ch, m_eff) in USES
            assert np.any(got["foreground"][s] != plain["foreground"][s])
            against_model(f"{case} slot {s} {name}", got, s, state(seed, n, fs, ch, m_eff), tabs[s], xs[s], m_eff, h)


def test_float32_and_int16_destinations_round_the_float64_foreground_once():
    S, ch, m = 2, 2, M_YOUNG
    n = (m + 24) * H + 77
    xs = np.stack([signal(seed, N8, FS, ch)[:n] for seed in (32, 33)]) * 16384.0     # (a power of two: still fp32 values)
    sizes = [(m + 6) * H + 5, 3 * H, 100, 9 * H + 1]
    sizes.append(n - sum(sizes))
    full = torch.tensor(xs, dtype=torch.float32, device=DEV)
    runs = {}
    for name, dt in (("float64", None), ("float32", torch.float32), ("int16", torch.int16)):
        hd = open_streams(S, ch, m)
        set_table(hd, "duck", [0])
        set_table(hd, "one-bin", [1])
        pieces, pos = [], 0
        for size in sizes + [None]:
            if dt is None:
                piece = hd.finish(which="foreground") if size is None else hd.push(xs[:, pos:pos + size], which="foreground")
            else:
                count = hd.emit_count(0, True) if size is None else hd.emit_count(size)
                out = torch.full((S, count, ch), 7, dtype=dt, device=DEV)
                piece = hd.finish(which="foreground", out=out) if size is None else hd.push(full[:, pos:pos + size], which="foreground", out=out)
                assert piece is out
            pieces.append(to_numpy(piece))
            pos += size or 0
        hd.close()
        runs[name] = np.concatenate(pieces, axis=1)
    assert np.any(np.abs(runs["float64"]) > 100)
    same(runs["float32"], runs["float64"].astype(np.float32))
    assert np.array_equal(runs["int16"], round_ref(runs["float64"], "int16"))


# ---- 3. the frame rule -------------------------------------------------------------------------------------------------------------
def test_the_frame_rule():
    """Tables set between pushes of mixed sizes -- several hops, off the hop grid, a push that completes no frame (the table set in
    front of it and replaced behind it never shapes a frame) -- and in front of the finish. Every frame is shaped with the table in
    force at the call that completed it, the carried frame included: the model with the newest table on the carried frames is
    further from the device's result than the bar."""
    S, ch, m = 2, 2, M_YOUNG
    seeds = (32, 33)
    xs = np.stack([signal(seed, N8, FS, ch) for seed in seeds])
    sizes = [40 * H + 5, 3 * H, 100, 2 * H + 151, 5 * H, H, 2 * H + 3, 30 * H, 7, 90 * H - 10, 6 * H, 120 * H + 1]
    sizes.append(N8 - sum(sizes))
    assert sizes[-1] > H and sum(sizes[:4]) == 46 * H
    assert frames_done(sum(sizes[:2]), W, H) == frames_done(sum(sizes[:3]), W, H)          # the push of 100 completes no frame
    sets = {1: [([0], "bass")], 2: [([0], "one-bin"), ([1], "duck")], 3: [([0], "duck")], 5: [([0], "per-bin"), ([1], None)],
            7: [([1], "one-bin")], 8: [([0], "speech-only")], 10: [([1], "bass"), ([0], None)], 11: [([0], "bass")],
            12: [([0], "duck")], 13: [([1], "duck")]}
    handle, twin = open_streams(S, ch, m), open_streams(S, ch, m)
    exported = {}

    def probe_of(hd):
        def probe(k, size, pos, out):
            if k == 3:                                                     # on the hop grid: the exported state knows no table
                st = hd.export_stream(0)
                exported[id(hd)] = (st.header, bytes(to_numpy(st.payload)))
            if hd is handle and k == 6:
                before = to_numpy(hd.last_emission("foreground"))
                set_table(hd, "all", [0])                                  # a set leaves the emission that stands as it is
                assert to_numpy(hd.last_emission("foreground")).tobytes() == before.tobytes() == out["foreground"][-1].tobytes()
                set_table(hd, "per-bin", [0])                              # (and the table in force is the last one set)
        return probe

    got, tabs = drive(handle, xs, sizes, FS, sets, probe_of(handle))
    plain, _ = drive(twin, xs, sizes, FS, None, probe_of(twin))
    handle.close(); twin.close()
    assert exported[id(handle)] == exported[id(twin)]
    assert got["background"].tobytes() == plain["background"].tobytes()
    for s, seed in enumerate(seeds):
        assert not np.array_equal(tabs[s], newest_on_carried(tabs[s]))
        against_model(f"frame rule slot {s}", got, s, state(seed, N8, FS, ch, m), tabs[s], xs[s], m, H, wrong=newest_on_carried(tabs[s]))
    # the finish's own frames took the tables set in front of it
    assert np.array_equal(tabs[0, -1], factors("duck", F)) and np.array_equal(tabs[1, -1], factors("duck", F))


# ---- 1 (rest) + 6. clearing, errors, the single-stream handle ------------------------------------------------------------------------
def test_clear_errors_and_the_single_stream_handle():
    S, ch, m = 2, 2, M_YOUNG
    n = (m + 30) * H + 77
    xs = np.stack([signal(seed, N8, FS, ch)[:n] for seed in (32, 33)])
    sizes = [(m + 5) * H, 2 * H, 3 * H + 9, H - 9, 2 * H, 3 * H + 7, H, 4 * H]
    sizes.append(n - sum(sizes))
    handle, twin = open_streams(S, ch, m), open_streams(S, ch, m)
    set_table(handle, "duck")
    assert np.array_equal(handle.background_band_gains(1), table(F, *TABLES["duck"]))
    pos = 0
    for k, size in enumerate(sizes + [None]):
        if k == 2:
            handle.clear_background_band_gains()
            assert not handle.background_band_gains(0).any() and not handle.background_band_gains(1).any()
        if k == 6:
            # refusals: nothing is enqueued and nothing changes -- the pushes that follow are still the untouched handle's
            for bad in (lambda: handle.set_background_band_gains([0.5, 1.5], [0, 4, 9]),
                        lambda: handle.set_background_band_gains([0.5, float("nan")], [0, 4, 9], slots=[1]),
                        lambda: handle.set_background_band_gains([0.5, -0.01], [0, 4, 9]),
                        lambda: handle.set_background_band_gains([0.5, 0.5], [4, 0, 9]),
                        lambda: handle.set_background_band_gains([0.5, 0.5], [0, 4, F + 1]),
                        lambda: handle.set_background_band_gains(np.zeros(F - 1)),
                        lambda: handle.set_background_band_gains([0.5, 0.5], [0, 4, 9], slots=[2]),
                        lambda: handle.set_background_band_gains(np.zeros((3, 2)), [0, 4, 9], slots=[0, 1])):
                with pytest.raises(ValueError):
                    bad()
            lib, bad_gain, edges = repet._native.lib(), (repet._native.C.c_float * 2)(0.5, 2.0), (repet._native.C.c_int32 * 3)(0, 4, 9)
            assert lib.repet_online_set_background_band_gains(handle._handle(), None, 0, edges, 2, bad_gain, 1) == repet._native.ERR_BAD_ARG
            assert lib.repet_online_set_background_band_gains(handle._handle(), None, 0, edges, 2, bad_gain, 3) == repet._native.ERR_BAD_ARG
            assert not handle.background_band_gains(0).any()
        if size is None:
            a, b = handle.finish(which="both"), twin.finish(which="both")
        else:
            a, b = handle.push(xs[:, pos:pos + size], which="both"), twin.push(xs[:, pos:pos + size], which="both")
            pos += size
        assert a[0].tobytes() == b[0].tobytes()
        if k < 2:
            assert np.any(a[1] != b[1]) or not np.any(a[0])
        elif k >= 4:                                                       # two frame-completing pushes behind the clear
            assert a[1].tobytes() == b[1].tobytes(), k
    handle.close(); twin.close()

    # repet.online: the same three calls without slots, and the same bits as a handle of one slot
    x = np.array(signal(32, N8, FS, ch)[:n])
    single, one = repet.online(FS, ch, start_length=m * H / FS), open_streams(1, ch, m)
    assert not single.background_band_gains().any()
    set_table(single, "bass")
    set_table(one, "bass")
    assert np.array_equal(single.background_band_gains(), table(F, *TABLES["bass"]))
    with pytest.raises(ValueError):
        single.set_background_band_gains([2.0], [0, 4])
    pos = 0
    for k, size in enumerate(sizes + [None]):
        if k == 3:
            single.clear_background_band_gains()
            one.clear_background_band_gains()
            set_table(single, "one-bin")
            set_table(one, "one-bin", [0])
        if size is None:
            a, b = single.finish(which="both"), one.finish(which="both")
        else:
            a, b = single.push(x[pos:pos + size], which="both"), one.push(x[None, pos:pos + size], which="both")
            pos += size
        assert a[0].tobytes() == b[0][0].tobytes() and a[1].tobytes() == b[1][0].tobytes()
    single.close(); one.close()


# ---- 4. lifecycle --------------------------------------------------------------------------------------------------------------------
def test_hold_finish_stream_and_restart():
    """Slot 0 is held over one push with a set made during the hold: the frame it carries keeps its own table and the frames
    behind the resume take the new one. Its stream then ends with finish_stream on an odd tail; the slot is restarted, keeps its
    table, and is the slot of a fresh handle with that table bit for bit. Slot 1 runs through to an odd finish."""
    ch, m = 2, M_YOUNG
    sizes = [40 * H, 3 * H, 2 * H, 4 * H, 2 * H + 77, H - 77, 36 * H, 3 * H + 5]
    n1 = sum(sizes)
    n0 = sum(sizes[:5]) - sizes[2]                                         # slot 0: everything up to its end but the held push
    x0, x1 = np.array(signal(32, N8, FS, ch)[:n0]), np.array(signal(33, N8, FS, ch)[:n1])
    x2 = np.array(signal(31, N8, FS, ch)[:sizes[6] + sizes[7]])            # the stream that restarts in slot 0
    handle = open_streams(2, ch, m)
    t0, t1 = state_frames(n0, FS), state_frames(n1, FS)
    tabs0, tabs1 = np.ones((t0, F)), np.ones((t1, F))
    out0, out1, out2 = {k: [] for k in ("background", "foreground", "mixture")}, {k: [] for k in ("background", "foreground", "mixture")}, []
    cur0, cur1 = np.ones(F), np.ones(F)
    p0 = p1 = p2 = 0
    fresh = open_streams(1, ch, m)
    set_table(fresh, "duck")
    for k, size in enumerate(sizes):
        if k == 1:
            set_table(handle, "bass", [0]); cur0 = factors("bass", F)
            set_table(handle, "duck", [1]); cur1 = factors("duck", F)
        if k == 2:
            handle.hold([0])
            set_table(handle, "duck", [0]); cur0 = factors("duck", F)      # during the hold: from the frames behind the resume on
        if k == 3:
            handle.resume([0])
        if k == 6:
            handle.restart([0])
            assert np.array_equal(handle.background_band_gains(0), table(F, *TABLES["duck"]))
        chunk = np.zeros((2, size, ch))
        chunk[1] = x1[p1:p1 + size]
        if k == 2:
            chunk[0] = 0.5                                                 # a held slot's share of the chunk is not read
        elif k < 5:
            chunk[0] = x0[p0:p0 + size]
        elif k >= 6:
            chunk[0] = x2[p2:p2 + size]
        b1, b0 = frames_done(p1, W, H), frames_done(p0, W, H)
        bg, fg = handle.push(chunk, which="both")
        mix = to_numpy(handle.last_emission("mixture"))
        if k == 0:
            handle.last_levels()                                           # (asked once: finish_stream measures its tail from now on)
        p1 += size
        tabs1[b1:frames_done(p1, W, H)] = cur1
        for key, v in (("background", bg), ("foreground", fg), ("mixture", mix)):
            out1[key].append(v[1])
        if k == 2:
            assert not bg[0].any() and not fg[0].any() and not mix[0].any()
        elif k < 5:
            p0 += size
            tabs0[b0:frames_done(p0, W, H)] = cur0
            for key, v in (("background", bg), ("foreground", fg), ("mixture", mix)):
                out0[key].append(v[0])
        elif k >= 6:
            p2 += size
            want = fresh.push(x2[None, p2 - size:p2], which="both")
            out2.append((bg[0], fg[0], want[0][0], want[1][0]))
        else:
            assert not fg[0].any()                                         # idle between finish_stream and restart
        if k == 4:
            set_table(handle, "one-bin", [0]); cur0 = factors("one-bin", F)     # in front of finish_stream: its frames take it
            tail_bg, tail_fg = handle.finish_stream(0, which="both")
            assert tail_fg.shape[0] == H + 77 and p0 == n0
            tail_mix = x0[n0 - (H + 77):]                                  # (finish_stream has released the samples: the input itself)
            tabs0[frames_done(p0, W, H):] = cur0
            rec = to_numpy(handle.last_levels())
            check_levels(rec[None], levels(tail_mix[None], to_numpy(tail_bg)[None], to_numpy(tail_fg)[None]), "finish_stream tail")
            for key, v in (("background", tail_bg), ("foreground", tail_fg), ("mixture", tail_mix)):
                out0[key].append(to_numpy(v))
            set_table(handle, "duck", [0])                                 # the slot's table while it is idle: the next stream's
    bg, fg = handle.finish(which="both")
    mix = to_numpy(handle.last_emission("mixture"))
    want = fresh.finish(which="both")
    assert fg.shape[1] % 2 == 1
    # (the handle emits one hop behind what it was pushed: the slot's first emission begins a hop before its stream, zero there)
    restarted_bg, restarted_fg = (np.concatenate([o[j] for o in out2] + [v[0]]) for j, v in ((0, bg), (1, fg)))
    fresh_bg, fresh_fg = (np.concatenate([o[j] for o in out2] + [v[0]]) for j, v in ((2, want[0]), (3, want[1])))
    assert not restarted_bg[:H].any() and not restarted_fg[:H].any()
    restarted_bg, restarted_fg = restarted_bg[H:], restarted_fg[H:]
    assert restarted_bg.tobytes() == fresh_bg.tobytes() and restarted_fg.tobytes() == fresh_fg.tobytes()
    assert np.any(restarted_bg) and np.any(restarted_fg != x2 - restarted_bg)               # the table was kept
    tabs1[frames_done(p1, W, H):] = cur1
    for key, v in (("background", bg), ("foreground", fg), ("mixture", mix)):
        out1[key].append(v[1])
    handle.close(); fresh.close()
    got0 = {key: np.concatenate(v)[None] for key, v in out0.items()}
    got1 = {key: np.concatenate(v)[None] for key, v in out1.items()}
    against_model("hold + finish_stream slot 0", got0, 0, masks_of(x0, FS, m), tabs0, x0, m, H, wrong=newest_on_carried(tabs0))
    against_model("beside a held slot, slot 1", got1, 0, masks_of(x1, FS, m), tabs1, x1, m, H)


def test_import_stream_same_table_and_another():
    """A stream exported on the hop grid goes on, in a slot with the SAME table, bit for bit as the unmoved one; in a slot with
    ANOTHER table it follows the model with the frame it carried in under the importing slot's table."""
    ch, m = 2, M_YOUNG
    sizes = [45 * H, 6 * H + 3, 2 * H, 5 * H - 3, 4 * H + 1]
    n = sum(sizes)
    x = np.array(signal(32, N8, FS, ch)[:n])
    a = open_streams(1, ch, m)
    set_table(a, "duck")
    first = a.push(x[None, :sizes[0]], which="both")
    moved = a.export_stream(0)
    same_table, other = open_streams(2, ch, m), open_streams(2, ch, m)
    set_table(same_table, "duck", [1])
    set_table(other, "bass", [1])
    set_table(other, "one-bin", [1])                                       # (two sets, nothing committed yet: the import settles the slot)
    same_table.import_stream(1, moved)
    other.import_stream(1, moved)
    pieces = {"background": [to_numpy(first[0])[0]], "foreground": [to_numpy(first[1])[0]], "mixture": [x[:first[0].shape[1]]]}
    pos = sizes[0]
    for size in sizes[1:] + [None]:
        chunk = np.zeros((2, size or 0, ch))
        if size is None:
            want, got, far = a.finish(which="both"), same_table.finish_stream(1, which="both"), other.finish_stream(1, which="both")
            far_mix = x[n - far[0].shape[0]:]                              # (finish_stream has released the samples: the input itself)
            got, far = (got[0][None], got[1][None]), (far[0][None], far[1][None])
            want = (want[0], want[1])
        else:
            chunk[1] = x[pos:pos + size]
            want, got, far = a.push(x[None, pos:pos + size], which="both"), same_table.push(chunk, which="both"), other.push(chunk, which="both")
            far_mix = to_numpy(other.last_emission("mixture"))[1]
            got, far = (got[0][1:], got[1][1:]), (far[0][1:], far[1][1:])
            pos += size
        assert to_numpy(got[0]).tobytes() == to_numpy(want[0]).tobytes() and to_numpy(got[1]).tobytes() == to_numpy(want[1]).tobytes()
        assert to_numpy(far[0]).tobytes() == to_numpy(want[0]).tobytes()
        pieces["background"].append(to_numpy(far[0])[0]); pieces["foreground"].append(to_numpy(far[1])[0])
        pieces["mixture"].append(far_mix)
    a.close(); same_table.close(); other.close()
    t = state_frames(n, FS)
    done = frames_done(sizes[0], W, H)
    tabs = np.tile(factors("duck", F), (t, 1))
    tabs[:m - 1] = 1.0
    tabs[done - 1:] = factors("one-bin", F)                                # the carried frame and everything behind it
    got = {key: np.concatenate(v)[None] for key, v in pieces.items()}
    emitted = first[0].shape[1]
    wrong = tabs.copy()
    wrong[done - 1] = factors("duck", F)                                   # (the carried frame under the table it was completed with)
    bar = against_model("import into another table", got, 0, masks_of(x, FS, m), tabs, x, m, H, lo=emitted)
    _, shaped_wrong = shaped_from(masks_of(x, FS, m), wrong)
    assert rms(((got["mixture"][0] - got["foreground"][0]) - shaped_wrong)[emitted:emitted + H]) > bar


def test_a_scalar_gain_with_its_fade_on_top():
    """The two gains multiply: fma(-a_k, shaped_bg, x) with a_k the scalar gain's factor and fade, shaped_bg from a twin with the
    same tables and scalar gain 0, within the fade bound derived in tests/test_gpu_online_background_gain.py (which, with the
    two roundings of recovering shaped_bg as mixture - foreground, still has room: 12 of its 32 units)."""
    S, ch, m = 2, 2, M_YOUNG
    n = (m + 24) * H + 77
    xs = np.stack([signal(seed, N8, FS, ch)[:n] for seed in (32, 33)])
    sizes = [(m + 6) * H + 5, 3 * H, 3 * H, 2 * H + 1, 5 * H]
    sizes.append(n - sum(sizes))
    handle, twin = open_streams(S, ch, m), open_streams(S, ch, m)
    for hd in (handle, twin):
        set_table(hd, "duck", [0])
        set_table(hd, "one-bin", [1])
    g_old, g_new = [0.25, 0.0], [0.8, 0.5]
    handle.set_background_gain(g_old, slots=[0, 1])
    pos, faded = 0, 0
    for k, size in enumerate(sizes + [None]):
        if k == 2:
            handle.set_background_gain(g_new, slots=[0, 1])
        if k == 4:
            set_table(handle, "bass", [0]); set_table(twin, "bass", [0])            # a change of table under a settled gain
        if size is None:
            a, b = handle.finish(which="both"), twin.finish(which="both")
        else:
            a, b = handle.push(xs[:, pos:pos + size], which="both"), twin.push(xs[:, pos:pos + size], which="both")
            pos += size
        assert a[0].tobytes() == b[0].tobytes()
        mix = to_numpy(handle.last_emission("mixture"))
        shaped = mix - b[1]
        for s in range(S):
            old, new = (g_old[s], g_new[s]) if k == 2 else ((g_old[s],) * 2 if k < 2 else (g_new[s],) * 2)
            want, bound = fade(mix[s], shaped[s], old, new, H)
            err = np.abs(a[1][s] - want)
            assert (err <= bound).all(), (k, s, float(err.max()))
            if k == 2 and np.any(shaped[s, :H]):
                faded += 1
                assert np.any(a[1][s, :H] != fade(mix[s], shaped[s], new, new, H)[0][:H])
    assert faded == S
    handle.close(); twin.close()


def test_zz_parity_table():
    """Prints what the checks above met (run after them: pytest keeps file order)."""
    if not PARITY:
        return
    lines = ["check                                              error (rms)   plain E (rms)   error / E      bar"]
    for label in sorted(PARITY):
        err, e_plain, ratio, bar = PARITY[label]
        lines.append(f"{label:<50} {err:.3e}     {e_plain:.3e}       {ratio:7.3f}   {bar:.3e}")
    text = "\n".join(lines)
    print("\n" + text)
    path = os.environ.get("REPET_BAND_GAINS_PARITY_OUT")
    if path:
        with open(path, "w") as fh:
            fh.write(text + "\n")
