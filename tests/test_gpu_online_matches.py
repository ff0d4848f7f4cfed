"""The similar frames a live handle matched (``last_matches`` / ``match_capacity`` of ``repet.online_streams`` / ``repet.online``;
include/repet_hip.h: repet_online_last_matches*): for the frames a push completed, per slot, the length of each frame's
similar-frame list, the age of every entry in the stream's own frames and its cosine similarity.

Expected values come from the float64 statement of tests/matches_reference.py (tied to the oracle by
tests/test_matches_reference.py), on the signals of tests/test_gpu_online_start.py, whose lists that file already requires to be
the float64 statement's on every row.

  count, age       exact, on every row of every push: none is left out
  padding, order   exact: age -1 and similarity +0 behind the list, ages strictly ascending
  similarity       |fp32 band entry - float64 unit[i] . unit[j]| <= similarity_bar, derived from the bars of the two stage tests
                   the value passes through, none of it fitted. Both rows are unit vectors with non-negative components, so
                   sum_k a_k b_k <= 1 (Cauchy-Schwarz), and that sum is the scale of every term:
                     rows   the unit rows on the device are within 1e-6 relative of the float64 ones, component by component
                            (tests/test_gpu_stft_stages.py: "Vn rel", the STFT bar carried through the normalisation): the
                            product of two such rows moves by at most ((1 + 1e-6)**2 - 1) sum a b
                     band   the Gram stage against the float64 band of the rows it read (tests/test_gpu_gram_band_stages.py):
                            f16-split form 3 FS u sum |products| (sum |products| <= (1 + 2**-9) sum a' b') plus
                            gram_reference.split_band_bound, which for unit rows at the fixed scale 128 is at most
                            (2**-20 + 2**-22) sum a' b' + 2**-30 sum (a' + b') + terms of second order, sum a' <= sqrt(F);
                            fp32 form (REPET_GRAM=f32) FS u sum a' b'
                   with u = 2**-24 and FS the padded row length: 5.5e-5 at 8 kHz, 1.9e-4 at 44.1 kHz (1.9e-5 / 6.5e-5 for the
                   fp32 form). The bound is a worst case over FS accumulated roundings; what is met is far below it.

The largest error met per case is collected in PARITY and printed (and written to $REPET_MATCHES_PARITY_OUT) by the last test:
profiles/online_matches_parity.txt is that output from an MI355X."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from matches_reference import capacity, matches_from
from oracle import repet_oracle as orc
from test_gpu_online_foreground import to_numpy
from test_gpu_online_start import signal
from test_gpu_online_streams import lockstep_sizes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 8000
W, H, B, F = 512, 256, 312, 257
M_YOUNG = 33                                  # start_frames of the start_length cases: similarity_distance is 31 frames
N = (B + 20) * H + 77
K = 10                                        # min(similarity_number = 100, ceil(312 / 32)); also ceil(431 / 44) at 44.1 kHz
U = 2.0 ** -24
PARITY = {}


def split_form():
    return not os.environ.get("REPET_GRAM", "").startswith("f3")


def similarity_bar(f, split=None):
    """The bar of the module docstring for rows of f bins."""
    split = split_form() if split is None else split
    fs_pad = -(-f // 32) * 32
    s = (1 + 1e-6) ** 2                                           # sum a' b' of the device's rows, at most
    rows = s - 1
    if not split:
        return rows + fs_pad * U * s
    sa = np.sqrt(f) * (1 + 1e-6)                                  # sum a' of a unit row, at most
    rel, absolute = 2.0 ** -21, 2.0 ** -24 / 128                  # gram_reference.split_error at the unit rows' scale
    first = 2 * (rel * s + absolute * sa)
    second = rel * rel * s + 2 * rel * absolute * sa + f * absolute * absolute
    dropped = 2.0 ** -22 * (s + first + second)
    return rows + 3 * fs_pad * U * (1 + 2.0 ** -9) * s + first + second + dropped


def note(case, err, bar, where):
    ratio = err / bar
    if case not in PARITY or ratio > PARITY[case][0]:
        PARITY[case] = (ratio, err, bar, where)


def bits(a):
    a = to_numpy(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint64)


def same_bits(a, b):
    a, b = to_numpy(a), to_numpy(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(bits(a), bits(b)), f"{int((bits(a) != bits(b)).sum())} of {a.size} values differ"


def same_matches(a, b):
    for x, y in zip(a, b):
        same_bits(x, y)


def geometry(fs):
    p = repet.derive_params(fs)
    return p.window_length, p.step_length, p.buffer_frames, p.window_length // 2 + 1


def open_streams(streams, channels, m=None, fs=FS):
    h = geometry(fs)[1]
    handle = repet.online_streams(fs, channels, streams, start_length=None if m is None else m * h / fs)
    assert handle.start_frames == (m or geometry(fs)[2])
    return handle


def frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def statement(seed, m, n, fs, ch, number=100):
    """(count, age, similarity) of every frame of signal(seed, n, fs, ch) separated from frame m - 1 on: computed once, shared,
    left unchanged."""
    return frozen(matches_from(np.array(signal(seed, n, fs, ch)), fs, m, orc.Params(similarity_number=number)))


def frames_done(pushed, w, h):
    return (pushed - w) // h + 1 if pushed >= w else 0


def numpy_matches(m, lead=False):
    got = tuple(to_numpy(v) for v in m)
    return tuple(v[None] for v in got) if lead else got


def well_formed(got, k=K):
    """What holds of every result, whatever it is compared with."""
    count, age, sim = got
    assert count.dtype == np.int32 and age.dtype == np.int32 and sim.dtype == np.float32
    assert age.shape == sim.shape == count.shape + (k,)
    assert ((count >= 0) & (count <= k)).all()
    behind = np.arange(k) >= count[..., None]
    assert (age[behind] == -1).all() and not bits(sim)[behind].any()        # -1 and +0 behind the list
    assert (age[~behind] >= 0).all()
    rising = (np.diff(age, axis=-1) > 0) | behind[..., 1:]
    assert rising.all()                                                      # strictly ascending ages


def empty_rows(got, rows):
    count, age, sim = (v[rows] for v in got)
    assert not count.any() and (age == -1).all() and not bits(sim).any()


def check_stream(got, want, f, case, where, first=0):
    """One stream's rows (count (T,), age (T, K), similarity (T, K)) against rows [first, first + T) of the statement."""
    count, age, sim = got
    wc, wa, ws = (v[first:first + len(count)] for v in want)
    assert len(wc) == len(count), (where, len(wc), len(count))
    wrong = np.flatnonzero((count != wc) | (age != wa).any(axis=-1))
    assert not wrong.size, (where, "rows that differ", (first + wrong[:8]).tolist(), count[wrong[:4]].tolist(), wc[wrong[:4]].tolist(),
                            age[wrong[:2]].tolist(), wa[wrong[:2]].tolist())
    if count.any():
        bar = similarity_bar(f)
        err = float(np.max(np.abs(sim.astype(np.float64) - ws)))
        note(case, err, bar, where)
        print(f"{case}: {where}: rows {len(count)}, with a list {int((count > 0).sum())}, counts {int(count.min())}..{int(count.max())}, "
              f"similarity error {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (case, where, err, bar)


def collect(handle, xs, sizes, fs=FS, single=False, k=K):
    """Push xs (S, N, C) in lockstep chunks, then finish; after every call the matches of the frames it completed, checked for
    shape and form. Returns the rows of all frames (S, T, ...) and the frames each call completed."""
    w, h = geometry(fs)[:2]
    n = xs.shape[1]
    parts, counts, pos, done = [], [], 0, 0
    for size in list(sizes) + [None]:
        if size is None:
            handle.finish()
            after = orc.online_frame_count(n, w, h)
        else:
            handle.push(xs[0, pos:pos + size] if single else xs[:, pos:pos + size])
            pos += size
            after = frames_done(pos, w, h)
        assert handle.last_frame_range == (done, after - done)
        m = handle.last_matches()
        assert isinstance(m, repet.Matches) and all(isinstance(v, np.ndarray) for v in m)
        got = numpy_matches(m, single)
        assert got[0].shape == (xs.shape[0], after - done)
        well_formed(got, k)
        parts.append(got)
        counts.append(after - done)
        done = after
    assert pos == n
    return tuple(np.concatenate([p[i] for p in parts], axis=1) for i in range(3)), counts


def run_parity(seeds, channels, m, n, fs, sizes, single=False, case=None):
    w, h, b, f = geometry(fs)
    xs = np.stack([signal(seed, n, fs, channels) for seed in seeds])
    handle = repet.online(fs, channels, start_length=None if m is None else m * h / fs) if single else open_streams(len(seeds), channels, m, fs)
    assert handle.match_capacity == K == capacity(fs)
    with pytest.raises(ValueError, match="stale"):
        handle.last_matches()
    got, counts = collect(handle, xs, sizes, fs, single)
    assert 0 in counts and max(counts) > 2                       # some calls completed no frame, some more than two
    case = case or f"fs={fs} S={len(seeds)} C={channels} M={m or b}"
    for s, seed in enumerate(seeds):
        want = statement(seed, m or b, n, fs, channels)
        assert len(want[0]) == got[0].shape[1] == orc.online_frame_count(n, w, h)
        check_stream(tuple(v[s] for v in got), want, f, case, f"stream {s}")
        empty_rows(tuple(v[s] for v in got), slice(0, (m or b) - 1))
        assert (got[0][s, (m or b) - 1:] > 0).all()               # the frame itself, at least
        assert (got[1][s, (m or b) - 1:, 0] == 0).all()
    again = numpy_matches(handle.last_matches(), single)         # finish's frames, a second time: identical bits
    same_matches(again, tuple(v[:, -counts[-1]:] for v in got) if counts[-1] else again)
    handle.close()
    return got


# ---- 1. and 2. parity with the float64 statement, push by push ------------------------------------------------------------------
@pytest.mark.parametrize("streams,channels,m,single", [(3, 2, M_YOUNG, False), (1, 1, None, True), (3, 1, M_YOUNG, False)])
def test_parity_per_push(streams, channels, m, single):
    sizes = lockstep_sizes(N, FS, seed=FS + channels + streams)
    assert 0 in sizes and 3 * H in sizes and max(sizes) > B * H
    got = run_parity([31, 32, 33][:streams], channels, m, N, FS, sizes, single)
    if m == M_YOUNG:
        live = got[0][0, m - 1:]
        assert live.min() < live.max() < K                       # lists of several lengths, all short of the capacity: padding everywhere


def test_parity_44k_stereo_register_fft_path():
    fs = 44100
    w, h, b, f = geometry(fs)
    assert (w, h, b, f) == (2048, 1024, 431, 1025)
    n = (b + 10) * h
    run_parity([33], 2, 100, n, fs, lockstep_sizes(n, fs, seed=fs + 2 + 1))


# ---- 3. the top-K cut ---------------------------------------------------------------------------------------------------------
def test_similarity_number_cuts_the_lists():
    C, m = 2, M_YOUNG
    before = repet.similarity_number
    repet.similarity_number = 4
    try:
        handle = open_streams(1, C, m)
    finally:
        repet.similarity_number = before
    assert handle.match_capacity == 4
    xs = signal(31, N, FS, C)[None]
    got, _ = collect(handle, xs, [40 * H, 100 * H + 5, N - 140 * H - 5], k=4)
    want = statement(31, m, N, FS, C, 4)
    assert want[1].shape[1] == 4
    live = got[0][0, m - 1:]
    assert (live == 4).any() and (live < 4).any()
    assert (statement(31, m, N, FS, C)[0] > 4).any()              # without the cut some lists are longer
    check_stream(tuple(v[0] for v in got), want, F, "similarity_number=4", "stream 0")
    handle.close()


def test_lists_longer_than_a_wavefront():
    """With ``similarity_distance`` below a frame every frame of the buffer is a candidate and the ``similarity_number`` most
    similar are kept: a capacity of 100 and lists of 60 to 100 entries, so the ranking takes a second round of 64 entries and
    the padding begins beyond the first. Near the cut such lists depend on similarities that differ in the last bits, so they
    are not compared with the float64 statement's; what must hold whatever was picked: every place is written exactly once
    (the destination is pre-filled), ages ascend strictly from 0 and stay inside the stream, and every similarity is the float64
    product of the two unit spectra its age names, within the bar of the module docstring."""
    from matches_reference import unit_spectra
    C, m = 1, 60
    n = (m + 60) * H + W
    x = signal(31, N, FS, C)[:n]
    saved = repet.similarity_distance
    repet.similarity_distance = 0.005                             # 0 frames
    try:
        handle = open_streams(2, C, m)
    finally:
        repet.similarity_distance = saved
    assert handle.match_capacity == 100
    handle.push(np.stack([x, x]))
    T = m + 61
    assert handle.last_frame_range == (0, T)
    outs = fresh_outs(2, T, k=100)
    handle.last_matches(out=outs)
    got = numpy_matches(outs)
    well_formed(got, 100)
    same_matches(handle.last_matches(), got)                      # the host form
    same_matches(tuple(v[0] for v in got), tuple(v[1] for v in got))
    count, age, sim = (v[0] for v in got)
    frames = np.arange(T)
    assert not count[:m - 1].any() and np.array_equal(count[m - 1:], np.minimum(frames[m - 1:] + 1, 100))
    assert count.min() == 0 and 60 <= count[m - 1] < 64 < count.max() == 100
    unit = unit_spectra(np.array(x), FS)
    bar, worst = similarity_bar(F), 0.0
    for j in range(m - 1, T):
        a = age[j, :count[j]]
        assert a[0] == 0 and a[-1] <= j
        worst = max(worst, float(np.max(np.abs(sim[j, :count[j]].astype(np.float64) - unit[j - a] @ unit[j]))))
    note("similarity_distance=0 K=100", worst, bar, "stream 0")
    assert worst <= bar, (worst, bar)
    handle.close()


# ---- 4. slots -----------------------------------------------------------------------------------------------------------------
def test_idle_held_restarted_and_resumed_slots():
    S, C, m = 4, 2, M_YOUNG
    xs = np.stack([signal(seed, N, FS, C) for seed in (31, 32, 33, 31)])
    handle = open_streams(S, C, m)
    handle.push(xs[:, :40 * H])                                   # frames 0 .. 38
    handle.release([1])
    handle.hold([2])
    handle.restart([0])                                           # slot 0's stream begins at sample 40 H: its frame 0 is frame 40
    chunk = np.array(xs[:, 40 * H:43 * H])
    chunk[1:3] = np.nan                                           # the idle and the held slot's share
    chunk[0, 5, 0] = np.nan                                       # ... and in frames 39 and 40 of slot 0
    handle.push(chunk)
    assert handle.last_frame_range == (39, 3)
    got = numpy_matches(handle.last_matches())
    well_formed(got)
    empty_rows(got, np.s_[0:3])                                   # the straddling frame and two warm-up frames; idle; held
    whole = statement(31, m, N, FS, C)
    check_stream(tuple(v[3] for v in got), whole, F, "slots", "the untouched neighbour", first=39)
    assert (got[0][3] > 0).all()
    # after the resume the held slot's ages count its own frames: the model runs on what the slot was fed
    handle.resume([2])
    handle.push(xs[:, 43 * H:80 * H])                             # frames 42 .. 78: slot 2's own 39 .. 75, slot 0's own 2 .. 38
    assert handle.last_frame_range == (42, 37)
    got = numpy_matches(handle.last_matches())
    well_formed(got)
    empty_rows(got, np.s_[1])
    fed2 = np.concatenate((xs[2, :40 * H], xs[2, 43 * H:80 * H]))
    check_stream(tuple(v[2] for v in got), matches_from(fed2, FS, m), F, "slots", "the resumed slot", first=39)
    assert (got[0][2] > 0).all()
    assert (got[1][2].max(axis=-1) > np.arange(37)).any()         # ages that reach back over the hold
    # the restarted slot: warm-up rows while its neighbours are past theirs, then its own lists
    empty_rows(got, np.s_[0, :m - 1 - 2])
    check_stream(tuple(v[0] for v in got), matches_from(xs[0, 40 * H:80 * H], FS, m), F, "slots", "the restarted slot", first=2)
    assert (got[0][0, m - 1 - 2:] > 0).all() and got[1][0].max() <= 38
    check_stream(tuple(v[3] for v in got), whole, F, "slots", "the untouched neighbour", first=42)
    handle.close()


def test_a_moved_stream_reports_what_the_unmoved_one_does():
    S, C, m = 2, 2, M_YOUNG
    xs = np.stack([signal(seed, N, FS, C) for seed in (31, 32)])
    home = open_streams(S, C, m)
    home.push(xs[:, :60 * H])
    state = home.export_stream(1)
    away = open_streams(3, C, m)                                  # a younger handle with other neighbours
    away.push(np.stack([xs[0, :7 * H]] * 3))
    away.import_stream(2, state)
    chunk = xs[:, 60 * H:70 * H + 100]
    home.push(chunk)
    away.push(np.stack([chunk[0], chunk[0], chunk[1]]))
    assert home.last_frame_range[1] == away.last_frame_range[1] == 10
    a, b = numpy_matches(home.last_matches()), numpy_matches(away.last_matches())
    well_formed(b)
    same_matches(tuple(v[1] for v in a), tuple(v[2] for v in b))
    assert (a[0][1] > 0).all()
    check_stream(tuple(v[2] for v in b), statement(32, m, N, FS, C), F, "slots", "the moved stream", first=59)
    home.close()
    away.close()


# ---- 5. a NaN sample ----------------------------------------------------------------------------------------------------------
def test_a_nan_sample_empties_its_frames_lists_and_is_never_listed():
    S, C, m = 3, 2, M_YOUNG
    xs = np.stack([signal(seed, N, FS, C) for seed in (31, 32, 33)])
    handle, twin = open_streams(S, C, m), open_streams(S, C, m)
    for h in (handle, twin):
        h.push(xs[:, :50 * H])
    chunk = np.array(xs[:, 50 * H:54 * H])
    twin.push(chunk)
    clean = numpy_matches(twin.last_matches())
    chunk[1, H + 10, 1] = np.nan                                  # sample 51 H + 10 of slot 1, channel 1: frames 50 and 51
    handle.push(chunk)
    assert handle.last_frame_range == twin.last_frame_range == (49, 4)
    got = numpy_matches(handle.last_matches())
    well_formed(got)
    empty_rows(got, np.s_[1, 1:3])
    same_matches(tuple(v[[0, 2]] for v in got), tuple(v[[0, 2]] for v in clean))       # the other slots: untouched
    same_matches(tuple(v[1, 0] for v in got), tuple(v[1, 0] for v in clean))           # the frame before
    heard = np.concatenate((xs[1, :50 * H], chunk[1], xs[1, 54 * H:100 * H]))
    want = matches_from(heard, FS, m)
    assert not want[0][50:52].any()                               # the reference's lists of those frames are empty too
    check_stream(tuple(v[1] for v in got), want, F, "a NaN sample", "its push", first=49)
    for h in (handle, twin):
        h.push(xs[:, 54 * H:100 * H])
    got, clean = numpy_matches(handle.last_matches()), numpy_matches(twin.last_matches())
    well_formed(got)
    assert handle.last_frame_range == (53, 46)
    listed = np.arange(53, 99)[:, None] - got[1][1]               # the frames slot 1's rows list (behind the list: beyond the row)
    assert not np.isin(listed[got[1][1] >= 0], (50, 51)).any()
    assert not np.isnan(got[2]).any()
    check_stream(tuple(v[1] for v in got), want, F, "a NaN sample", "the pushes after", first=53)
    same_matches(tuple(v[[0, 2]] for v in got), tuple(v[[0, 2]] for v in clean))
    handle.close()
    twin.close()


# ---- 6. forms -----------------------------------------------------------------------------------------------------------------
def fresh_outs(s, t, k=K, fill=7):
    return (torch.full((s, t), fill, dtype=torch.int32, device=DEV), torch.full((s, t, k), fill, dtype=torch.int32, device=DEV),
            torch.full((s, t, k), float(fill), dtype=torch.float32, device=DEV))


def test_host_and_device_forms_give_identical_bits():
    S, C, m = 3, 2, M_YOUNG
    n = (m + 40) * H + W
    xs = np.stack([signal(seed, N, FS, C)[:n] for seed in (31, 32, 33)])
    handle = open_streams(S, C, m)
    handle.push(xs)
    T = m + 41
    assert handle.last_frame_range == (0, T)
    host = handle.last_matches()
    assert all(isinstance(v, np.ndarray) for v in host)
    well_formed(host)
    assert host.count[:, m - 1:].all() and not host.count[:, :m - 1].any()
    same_matches(handle.last_matches(), host)                     # a second call
    outs = fresh_outs(S, T)
    back = handle.last_matches(out=outs)
    assert isinstance(back, repet.Matches) and all(a is b for a, b in zip(back, outs))
    same_matches(outs, host)
    same_matches(handle.last_matches(out=list(outs)), host)       # ... and a second call of that form
    bad = [(outs[0].to(torch.int64), outs[1], outs[2]), (outs[0], outs[1].to(torch.float32), outs[2]), (outs[0], outs[1], outs[2].double()),
           (outs[0][:, :-1], outs[1], outs[2]), (outs[0], outs[1][..., :-1], outs[2]), (outs[0], outs[1], outs[2].cpu()),
           (outs[0], outs[1], torch.empty((S, T, 2 * K), dtype=torch.float32, device=DEV)[..., ::2]), (outs[0], outs[1]), outs[0],
           tuple(to_numpy(v) for v in outs)]
    marked = fresh_outs(S, T, fill=9)
    for k, wrong in enumerate(bad):
        with pytest.raises(ValueError):
            handle.last_matches(out=wrong)
    for k in range(3):                                            # one wrong tensor: the two right ones stay as they were
        trial = list(marked)
        trial[k] = trial[k].to(torch.float64)
        with pytest.raises(ValueError):
            handle.last_matches(out=trial)
    assert all(bool((v == 9).all()) for v in marked)
    same_matches(handle.last_matches(), host)                     # refusals change nothing
    # after a device chunk the result is tensors, and equals the host chunk's
    twin = open_streams(S, C, m)
    twin.push(torch.from_numpy(xs).to(DEV))
    got = twin.last_matches()
    assert all(isinstance(v, torch.Tensor) and v.device == torch.device(DEV) for v in got)
    assert (got.count.dtype, got.age.dtype, got.similarity.dtype) == (torch.int32, torch.int32, torch.float32)
    same_matches(got, host)
    handle.close()
    twin.close()


def test_one_stream_handle_has_no_stream_axis():
    C, m = 2, M_YOUNG
    n = (m + 3) * H + W
    x = signal(31, N, FS, C)[:n]
    one, many = repet.online(FS, C, start_length=m * H / FS), open_streams(1, C, m)
    one.push(x)
    many.push(x[None])
    got = one.last_matches()
    assert got.count.shape == (m + 4,) and got.age.shape == got.similarity.shape == (m + 4, K)
    same_matches(got, tuple(v[0] for v in many.last_matches()))
    outs = tuple(v[0] for v in fresh_outs(1, m + 4))
    assert one.last_matches(out=outs).age is outs[1]
    same_matches(outs, got)
    one.close()
    many.close()


# ---- 7. the stale rule --------------------------------------------------------------------------------------------------------
def stale(handle):
    for kw in ({}, {"out": fresh_outs(2, 1)}):
        with pytest.raises(ValueError, match="stale"):
            handle.last_matches(**kw)


def test_the_record_follows_the_pushes_and_goes_stale():
    S, C, m = 2, 1, 2
    xs = np.stack([signal(seed, N, FS, C) for seed in (31, 32)])
    handle = open_streams(S, C, m)
    stale(handle)                                                # before any push
    pos = 0

    def push(hops):
        nonlocal pos
        handle.push(xs[:, pos:pos + hops * H])
        before = frames_done(pos, W, H)
        pos += hops * H
        got = handle.last_matches()
        assert got.count.shape == (S, frames_done(pos, W, H) - before)
        well_formed(got)
        return got

    got = push(1)                                                 # no frame yet: empty arrays, not an error
    assert got.count.shape == (S, 0) and got.age.shape == got.similarity.shape == (S, 0, K)
    outs = fresh_outs(S, 0)
    assert handle.last_matches(out=outs).count is outs[0]
    assert push(5).count[:, 1:].all()
    handle.push(xs[:, pos:pos + H])                               # a push makes the record of the push before stale: it is replaced
    pos += H
    assert handle.last_matches().count.shape == (S, 1)
    handle.restart([1])
    stale(handle)
    push(2)
    handle.release([1])
    stale(handle)
    push(1)
    handle.hold([0])
    stale(handle)
    empty_rows(push(2), np.s_[:])                                 # slot 0 held, slot 1 idle
    handle.resume([0])
    stale(handle)
    push(3)
    state = handle.export_stream(0)
    assert handle.last_matches().count.shape == (S, 3)            # an export leaves the record alone
    handle.finish_stream(0)
    stale(handle)
    push(1)
    handle.import_stream(1, state)
    stale(handle)
    assert push(2).count[1].all()
    handle.close()
    with pytest.raises(ValueError):
        handle.last_matches()


# ---- 8. asking changes nothing ------------------------------------------------------------------------------------------------
def test_asking_changes_nothing():
    S, C, m = 3, 2, M_YOUNG
    n = (m + 12) * H
    xs = np.stack([signal(seed, N, FS, C)[:n] for seed in (31, 32, 33)])
    sizes = [0, 100, 3 * H, (m + 2) * H, 1, H, 5 * H + 9]
    sizes.append(n - sum(sizes))
    asked, plain = open_streams(S, C, m), open_streams(S, C, m)
    pos = 0
    for size in sizes + [None]:
        if size is None:                                         # on the hop grid: what a slot's state holds
            for s in range(S):
                a, b = asked.export_stream(s), plain.export_stream(s)
                assert a.header == b.header
                same_bits(a.payload, b.payload)
        outs = []
        for h in (asked, plain):
            outs.append(h.finish(which="both") if size is None else h.push(xs[:, pos:pos + size], which="both"))
            if h is asked:
                h.last_matches()
                h.last_matches(out=fresh_outs(S, h.last_frame_range[1]))
                h.last_matches()
        pos += size or 0
        for a, b in zip(*outs):
            assert a.dtype == np.float64 and np.array_equal(a, b)
        for which in ("background", "foreground", "mixture"):
            assert np.array_equal(asked.last_emission(which), plain.last_emission(which))
            same_bits(asked.last_frames(which), plain.last_frames(which))
        same_bits(asked.last_levels(), plain.last_levels())
        assert asked.last_frame_range == plain.last_frame_range
        same_matches(asked.last_matches(), plain.last_matches())  # after the levels and frames launches, too
    asked.close()
    plain.close()


# ---- 9. the other band layout -------------------------------------------------------------------------------------------------
def child_case(path):
    """(run in a child process under REPET_GRAM=f32) case 1 of the file, its rows saved for the parent."""
    sizes = lockstep_sizes(N, FS, seed=FS + 2 + 3)
    got = run_parity([31, 32, 33], 2, M_YOUNG, N, FS, sizes, case="fs=8000 S=3 C=2 M=33 REPET_GRAM=f32")
    ratio, err, bar, where = PARITY["fs=8000 S=3 C=2 M=33 REPET_GRAM=f32"]
    np.savez(path, count=got[0], age=got[1], similarity=got[2], err=err, bar=bar)


def test_the_diagonal_band_layout(tmp_path):
    """REPET_GRAM=f32 leaves the band as band[t][l] = sim(t, t + l), which the gather reads by another formula. The switch is
    read once, so the case runs in a process of its own: the import, the first use of the device and one live run of 332 hops,
    a few seconds; a child that meets the limit of 120 s has hung."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_online_matches as t; t.child_case(sys.argv[1])"
            % (os.path.join(root, "repet-python_amd"), root, os.path.join(root, "tests")))
    out = str(tmp_path / "matches_f32.npz")
    subprocess.check_call([sys.executable, "-c", code, out], env=dict(os.environ, REPET_GRAM="f32"), timeout=120)
    with np.load(out) as z:
        got = (z["count"], z["age"], z["similarity"])
        err, bar = float(z["err"]), float(z["bar"])
    assert bar == similarity_bar(F, split=False)
    note("fs=8000 S=3 C=2 M=33 REPET_GRAM=f32", err, bar, "child process")
    for s, seed in enumerate((31, 32, 33)):                       # the same rows as case 1: the lists do not depend on the layout
        want = statement(seed, M_YOUNG, N, FS, 2)
        assert np.array_equal(got[0][s], want[0]) and np.array_equal(got[1][s], want[1])
        assert np.max(np.abs(got[2][s] - want[2])) <= bar


def test_zz_report_the_largest_errors():
    """Last in the module: the table profiles/online_matches_parity.txt is made of (case, max similarity error, bar, where)."""
    lines = ["%-40s err %.3e  bar %.3e  (%.3f of the bar)  %s" % (case, err, bar, ratio, where)
             for case, (ratio, err, bar, where) in sorted(PARITY.items())]
    print("\n".join(lines))
    path = os.environ.get("REPET_MATCHES_PARITY_OUT")
    if path and lines:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
