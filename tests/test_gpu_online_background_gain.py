"""The background gain: a chosen share ``g`` in [0, 1] of the background kept in the FOREGROUND of live handles and tensor calls.

    foreground = x - a * bg,    a = float32(1 - float64(float32(g)))

Every input here is fp32-exact (float32 tensors, or float64 derived from 16-bit PCM), so ``x`` is exact, and every expectation
is computed in NumPy from the SAME run's background (``which="both"``) and its ``last_emission("mixture")`` (or the input, where
a ``finish_stream`` has released the samples), never from the foreground under test.

* Outside a fade ``a`` and ``bg`` are fp32 values, so ``float64(a) * bg`` is exact in float64 and the kernel's
  ``fma(-a, bg, x)`` is ``x - a * bg`` rounded once: NumPy's ``mix - float64(a) * bg`` reproduces it bit for bit.
* A change of gain is a fade over the first ``R = min(H, n_emit)`` samples of the next emission that covers the slot: sample
  ``k`` takes ``a_k = a_old + (a_new - a_old) * ((k + 1) / R)`` for ``k + 1 < R`` and ``a_new`` itself from there on. Inside the
  fade the bound is ``|fg - (x - a_k * bg)| <= 2**-48 * (|x| + |bg|)``, derived, not measured: the kernel forms ``a_k`` with three
  roundings (the difference, the quotient, the fma), NumPy with four (difference, quotient, product, sum), every one at most
  ``2**-53`` relative on a quantity of magnitude at most 1 (``0 <= a <= 1``), so the two ``a_k`` differ by at most ``7 * 2**-53``
  and ``a_k * bg`` by ``7 * 2**-53 |bg|``; NumPy rounds the product once more (``2**-53 |bg|``; the kernel's fma does not), and
  each side rounds its sum once (``2 * 2**-53 (|x| + |bg|)``). Together at most ``10 * 2**-53 (|x| + |bg|) < 2**-48 (|x| + |bg|)``.
* With ``W = 2 H`` every push emits whole hops and a finish (or ``finish_stream``) tail has between ``H`` and ``2 H - 1`` samples,
  so ``R = H`` in every emission a handle can make; the fade before a finish is checked on such a tail (odd, off the hop grid):
  its first ``H`` samples fade and everything behind them, the last sample included, is exactly at the new value.
* A float32 destination holds ``np.float32`` of the float64 result; a strided destination the values of a dense one.
* ``bg == repet.simonline(x, fs)`` bit for bit as ever, whatever the gains are."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet import _native
from test_gpu_online_streams import lockstep_sizes, same, signals
from test_gpu_online_foreground import pcm_exact, run_which, to_numpy

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 8000
GAINS = [0.0, 1.0, 0.25, 10 ** (-12 / 20), 0.5]


def factor(g):
    """What the library multiplies the background by for a gain g."""
    return np.float32(1.0 - np.float64(np.float32(g)))


def kept(mix, bg, g):
    """The foreground at a settled gain g: bit for bit."""
    return mix - np.float64(factor(g)) * bg


def fade(mix, bg, g_old, g_new, R):
    """(expected foreground, bound) of one stream's emission (n, C) that fades from g_old to g_new over its first R samples."""
    n = mix.shape[0]
    a_old, a_new = np.float64(factor(g_old)), np.float64(factor(g_new))
    k1 = np.arange(1, n + 1, dtype=np.float64)
    a = np.where(k1 >= R, a_new, a_old + (a_new - a_old) * (k1 / np.float64(R)))[:, None]
    return mix - a * bg, 2.0 ** -48 * (np.abs(mix) + np.abs(bg))


def check_fade(fg, mix, bg, g_old, g_new, R):
    want, bound = fade(mix, bg, g_old, g_new, R)
    err = np.abs(fg - want)
    print(f"fade {g_old} -> {g_new}: largest error {err[:R].max():.3e}, of its bound {np.max(err[:R] / np.maximum(bound[:R], 1e-300)):.3f}")
    assert (err[:R] <= bound[:R]).all(), f"inside the fade off by up to {err[:R].max():.3e}"
    same(fg[R - 1:], kept(mix[R - 1:], bg[R - 1:], g_new))                 # from sample R - 1 on: the new value itself
    assert np.any(fg[:R] != kept(mix[:R], bg[:R], g_new)) and np.any(fg[:R] != kept(mix[:R], bg[:R], g_old))


def streams_of(channels, seconds, seeds, odd=True):
    xs = pcm_exact(signals(FS, channels, seconds, seeds))
    return xs[:, :xs.shape[1] - (1 - xs.shape[1] % 2)] if odd else xs      # an odd length: the finish tail is odd


def hop_and_buffer():
    p = repet.derive_params(FS)
    assert (p.window_length, p.step_length) == (512, 256)
    return p.step_length, p.buffer_frames


# ---- 1. steady state, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,seconds", [(1, 13.0), (2, 12.5)])
def test_steady_state_bit_for_bit(channels, seconds):
    H, B = hop_and_buffer()
    xs = streams_of(channels, seconds, [3, 5, 7, 11, 13])
    S, N = xs.shape[0], xs.shape[1]
    sizes = lockstep_sizes(N, FS, seed=FS + channels)
    assert N % 2 == 1 and any(n > 2 * H and n % H for n in sizes) and any(n % H == 0 and n >= 2 * H for n in sizes)
    h = repet.online_streams(FS, channels, S)
    h.set_background_gain(GAINS, slots=range(S))
    assert [h.background_gain(s) for s in range(S)] == [float(np.float32(g)) for g in GAINS]
    got = run_which(h, xs, sizes, "both", mixture=True)
    twin = run_which(repet.online_streams(FS, channels, S), xs, sizes, "both")
    same(got["mixture"], xs)
    same(got["background"], twin["background"])
    for s, g in enumerate(GAINS):
        same(got["background"][s], repet.simonline(xs[s], FS))
        same(got["foreground"][s], kept(got["mixture"][s], got["background"][s], g))
        assert np.any(got["background"][s, (B - 1) * H:])
    same(got["foreground"][0], twin["foreground"][0])                      # g = 0: as if no gain had ever been set
    same(got["foreground"][1], got["mixture"][1])                          # g = 1: the input
    for s in (2, 3, 4):
        assert np.any(got["foreground"][s] != twin["foreground"][s]) and np.any(got["foreground"][s] != xs[s])

    # float32 destinations that are [:, :, ::2] views, fed float32 tensors on the device: np.float32 of the dense float64 result
    full = torch.tensor(xs, dtype=torch.float32, device=DEV)
    h = repet.online_streams(FS, channels, S)
    h.set_background_gain(GAINS, slots=range(S))
    pieces, pos = {"background": [], "foreground": []}, 0
    for n in sizes + [None]:
        m = h.emit_count(0, True) if n is None else h.emit_count(n)
        store = torch.full((2, S, m, 2 * channels), 7.0, dtype=torch.float32, device=DEV)
        out = (store[0, :, :, ::2], store[1, :, :, ::2])
        ret = h.finish(out=out, which="both") if n is None else h.push(full[:, pos:pos + n], out=out, which="both")
        assert ret[0] is out[0] and ret[1] is out[1] and torch.all(store[..., 1::2] == 7.0)
        pieces["background"].append(to_numpy(out[0]))
        pieces["foreground"].append(to_numpy(out[1]))
        pos += n or 0
    h.close()
    for k, v in pieces.items():
        same(np.concatenate(v, axis=1), got[k].astype(np.float32))


def test_dense_float32_and_strided_float64_destinations():
    """The destinations the test above leaves out, through a fade and a finish: a DENSE float32 ``out=`` (four elements per
    thread, one 16-byte store), alone as "foreground" and as the second destination of "both", and a strided float64 one. Mono
    with an odd tail, so a thread's run of four crosses from one stream into the next and the last thread's is short."""
    H, B = hop_and_buffer()
    S = 3
    xs = streams_of(1, 12.3, [14, 15, 16])
    N = xs.shape[1]
    full = torch.tensor(xs, dtype=torch.float32, device=DEV)
    sizes = [321 * H + 5, 3 * H - 5, 2 * H, 7 * H + 2]
    sizes.append(N - sum(sizes))
    g0, g1 = [0.25, 1.0, 10 ** (-12 / 20)], [0.75, 0.0, 10 ** (-12 / 20)]
    change_before = 2                                                      # the push of 2 H samples fades slots 0 and 1

    def run(make_out, which):
        h = repet.online_streams(FS, 1, S)
        h.set_background_gain(g0, slots=range(S))
        pieces, pos = [], 0
        for k, n in enumerate(sizes + [None]):
            if k == change_before:
                h.set_background_gain(g1, slots=range(S))
            m = h.emit_count(0, True) if n is None else h.emit_count(n)
            out, read = make_out(m)
            ret = h.finish(out=out, which=which) if n is None else h.push(full[:, pos:pos + n], out=out, which=which)
            pieces.append([to_numpy(t) for t in read(ret)])
            pos += n or 0
        h.close()
        return [np.concatenate(v, axis=1) for v in zip(*pieces)], [p[0].shape[1] for p in pieces]

    (bg, fg), emitted = run(lambda m: (None, lambda ret: ret), "both")          # dense float64, checked against NumPy here
    assert emitted[change_before] == 2 * H and emitted[-1] % 4 and (S * emitted[-1]) % 4
    a, b = sum(emitted[:change_before]), sum(emitted[:change_before + 1])
    assert np.any(bg[:, a:a + H])
    for s in range(S):
        same(bg[s], repet.simonline(xs[s], FS))
        same(fg[s, :a], kept(xs[s, :a], bg[s, :a], g0[s]))
        same(fg[s, b:], kept(xs[s, b:], bg[s, b:], g1[s]))
    for s in (0, 1):
        check_fade(fg[s, a:b], xs[s, a:b], bg[s, a:b], g0[s], g1[s], H)
    same(fg[2, a:b], kept(xs[2, a:b], bg[2, a:b], g1[2]))

    def dense32(m):
        out = torch.full((S, m, 1), 7.0, dtype=torch.float32, device=DEV)
        assert out.is_contiguous()
        return out, lambda ret: (ret,)

    (fg32,), _ = run(dense32, "foreground")
    same(fg32, fg.astype(np.float32))

    def dense32_pair(m):
        out = (torch.full((S, m, 1), 7.0, dtype=torch.float32, device=DEV), torch.full((S, m, 1), 7.0, dtype=torch.float32, device=DEV))
        return out, lambda ret: ret

    (bg32, fg32), _ = run(dense32_pair, "both")
    same(bg32, bg.astype(np.float32))
    same(fg32, fg.astype(np.float32))

    stores = []

    def strided64(m):
        store = torch.full((2, S, m, 2), 7.0, dtype=torch.float64, device=DEV)
        stores.append(store)
        return (store[0, :, :, ::2], store[1, :, :, ::2]), lambda ret: ret

    (bg64, fg64), _ = run(strided64, "both")
    assert all(torch.all(t[..., 1::2] == 7.0) for t in stores)
    same(bg64, bg)
    same(fg64, fg)


def test_the_single_stream_handle_and_the_run_device_entry():
    """``repet.online``'s own ``set_background_gain`` / ``background_gain`` through a fade, and ``repet_set_run_background_gain``
    with a value in range in front of ``repet_run_device``."""
    H, B = hop_and_buffer()
    x = streams_of(2, 12.1, [17])[0]
    N = x.shape[0]
    s = repet.online(FS, 2)
    assert s.background_gain() == 0.0
    s.set_background_gain(0.25)
    assert s.background_gain() == 0.25
    with pytest.raises(ValueError):
        s.set_background_gain(1.5)
    assert s.background_gain() == 0.25
    sizes = [322 * H + 9, 4 * H, 3 * H + 1, 5 * H]
    sizes.append(N - sum(sizes))
    pieces, pos = [], 0
    for k, n in enumerate(sizes):
        if k == 2:
            s.set_background_gain(0.8)
        pieces.append(s.push(x[pos:pos + n], which="both"))
        pos += n
    pieces.append(s.finish(which="both"))
    s.close()
    bg, fg = (np.concatenate([p[k] for p in pieces]) for k in (0, 1))
    same(bg, repet.simonline(x, FS))
    a, b = sum(p[0].shape[0] for p in pieces[:2]), sum(p[0].shape[0] for p in pieces[:3])
    assert b - a == 3 * H and np.any(bg[a:a + H])
    same(fg[:a], kept(x[:a], bg[:a], 0.25))
    check_fade(fg[a:b], x[a:b], bg[a:b], 0.25, 0.8, H)
    same(fg[b:], kept(x[b:], bg[b:], 0.8))

    g = 10 ** (-12 / 20)
    t = torch.tensor(signals(FS, 2, 6.0, [18])[0].astype(np.float32), device=DEV)
    n, c = t.shape
    lib, params = _native.lib(), repet.derive_params(FS)
    strides = (C.c_int64 * 3)(n * c, c, 1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream or None)
    fore, back = _native.which_codes("foreground")[0], _native.which_codes("background")[0]

    def run_device(out):
        _native.check(lib.repet_run_device(_native.SIM, C.c_void_p(t.data_ptr()), _native.F32, 1, n, c, strides,
                                           C.c_void_p(out.data_ptr()), _native.F64, strides, params, 0, stream))
        torch.cuda.synchronize()
        return to_numpy(out)

    out = torch.empty((n, c), dtype=torch.float64, device=DEV)
    want_bg = to_numpy(repet.separate("sim", t, FS))
    xt = to_numpy(t).astype(np.float64)
    try:
        _native.check(lib.repet_select_run_result(0, fore))
        _native.check(lib.repet_set_run_background_gain(0, g))
        same(run_device(out), kept(xt, want_bg, g))
        assert np.any(want_bg) and np.any(to_numpy(out) != xt - want_bg)
        same(run_device(out), kept(xt, want_bg, g))                        # the setting stays, as the selection does
        assert lib.repet_set_run_background_gain(0, 1.5) == _native.ERR_BAD_ARG
        same(run_device(out), kept(xt, want_bg, g))
        _native.check(lib.repet_set_run_background_gain(0, 0.0))
        same(run_device(out), xt - want_bg)
    finally:
        lib.repet_set_run_background_gain(0, 0.0)
        lib.repet_select_run_result(0, back)
    same(run_device(out), want_bg)


# ---- 2. never set means today -----------------------------------------------------------------------------------------------------
def test_a_gain_of_zero_is_the_handle_that_never_set_one():
    xs = streams_of(2, 12.0, [21, 22, 23])
    sizes = lockstep_sizes(xs.shape[1], FS, seed=4)
    never = run_which(repet.online_streams(FS, 2, 3), xs, sizes, "both")
    h = repet.online_streams(FS, 2, 3)
    h.set_background_gain(0.0)
    zero = run_which(h, xs, sizes, "both")
    for k in ("background", "foreground"):
        assert never[k].tobytes() == zero[k].tobytes()
    assert np.any(never["background"]) and np.any(never["foreground"] != xs)


# ---- 3. a change is a fade ------------------------------------------------------------------------------------------------------
def test_a_change_of_gain_fades_over_one_hop():
    H, B = hop_and_buffer()
    ch, S = 2, 4
    N = 390 * H + 77                                                      # the finish tail: H + 77 samples, odd
    xs = streams_of(ch, 12.6, [31, 32, 33, 34], odd=False)[:, :N]
    full = torch.tensor(xs, device=DEV)
    g = [0.0, 0.8, 0.3, 0.0]
    h = repet.online_streams(FS, ch, S)
    h.set_background_gain(g, slots=range(S))
    state = {"pos": 0}

    def push(n):
        bg, fg = h.push(full[:, state["pos"]:state["pos"] + n], which="both")
        state["pos"] += n
        return to_numpy(bg), to_numpy(fg), to_numpy(h.last_emission("mixture"))

    def settled(bg, fg, mix):
        for s in range(S):
            same(fg[s], kept(mix[s], bg[s], g[s]))

    for n in (320 * H, 2 * H, 5 * H + 3):                                  # past the warm-up, then steady
        bg, fg, mix = push(n)
        settled(bg, fg, mix)
    assert np.any(bg)
    old = list(g)
    h.set_background_gain([1.0, 0.2], slots=[0, 1])
    g[0], g[1] = 1.0, 0.2
    assert h.emit_count(3 * H) == 3 * H
    bg, fg, mix = push(3 * H)
    same(mix, xs[:, state["pos"] - 3 * H - (H + 3):state["pos"] - (H + 3)])
    for s in (0, 1):
        assert np.any(bg[s, :H])
        check_fade(fg[s], mix[s], bg[s], old[s], g[s], H)
    for s in (2, 3):
        same(fg[s], kept(mix[s], bg[s], g[s]))                             # the unchanged slots: bit for bit throughout
    # last_emission returns what that push's own gain and fade produced, whatever has been set since
    h.set_background_gain(0.6, slots=[3])
    same(h.last_emission("foreground"), fg)
    g[3] = 0.6
    bg, fg, mix = push(2 * H)                                              # slot 3 fades now, the others are settled
    check_fade(fg[3], mix[3], bg[3], 0.0, 0.6, H)
    for s in (0, 1, 2):
        same(fg[s], kept(mix[s], bg[s], g[s]))
    for n in (H, 4 * H + 9, 7 * H):
        settled(*push(n))
    settled(*push(N - state["pos"]))
    # a change before the finish: the tail has H + 77 samples, fades over its first H and ends exactly at the new value
    h.set_background_gain(0.9, slots=[2])
    n_rest = h.emit_count(0, True)
    assert n_rest == H + 77
    bg, fg = (to_numpy(t) for t in h.finish(which="both"))
    mix = to_numpy(h.last_emission("mixture"))
    h.close()
    same(mix, xs[:, N - n_rest:])
    check_fade(fg[2], mix[2], bg[2], 0.3, 0.9, H)
    same(fg[2, -1], kept(mix[2, -1], bg[2, -1], 0.9))
    for s in (0, 1, 3):
        same(fg[s], kept(mix[s], bg[s], g[s]))


# ---- 4. the gain is the slot's ----------------------------------------------------------------------------------------------------
def test_the_gain_survives_restart_and_import():
    H, B = hop_and_buffer()
    ch = 2
    P, N = 330 * H, 395 * H + 31
    xs = streams_of(ch, 12.7, [41, 42, 43, 44], odd=False)[:, :N]
    moved = xs[3]                                                          # lives in A's slot 1, then in B's slot 2
    a = repet.online_streams(FS, ch, 2)
    a.set_background_gain(0.3, slots=[1])
    first = a.push(np.stack([xs[0, :P], moved[:P]]))                       # (the background is what is checked of A)
    state = a.export_stream(1)
    assert a.background_gain(1) == float(np.float32(0.3)) and a.background_gain(0) == 0.0
    a.close()

    g = [0.5, 0.0, 0.7]
    b = repet.online_streams(FS, ch, 3)
    b.set_background_gain([0.5, 0.7], slots=[0, 2])
    R0 = 8 * H                                                             # slot 0 begins a new stream here
    new0 = xs[2, :N - R0]
    feed = np.stack([np.concatenate([xs[0, :R0], new0]), xs[1], np.concatenate([xs[0, :P], moved[P:]])])
    out = {k: [] for k in ("background", "foreground", "mixture")}
    pos = 0

    def push(n):
        nonlocal pos
        bg, fg = b.push(feed[:, pos:pos + n], which="both") if n is not None else b.finish(which="both")
        for k, v in (("background", bg), ("foreground", fg), ("mixture", b.last_emission("mixture"))):
            out[k].append(v)
        pos += n or 0

    push(R0)
    b.restart([0])
    for n in (100 * H, P - R0 - 100 * H):
        push(n)
    b.import_stream(2, state)
    assert [b.background_gain(s) for s in range(3)] == [float(np.float32(v)) for v in g]
    for n in (3 * H, 20 * H + 5, N - P - 23 * H - 5, None):
        push(n)
    b.close()
    got = {k: np.concatenate(v, axis=1) for k, v in out.items()}
    for s in range(3):
        same(got["foreground"][s], kept(got["mixture"][s], got["background"][s], g[s]))
    # the lives are what they always were: the restarted stream, and the moved one across its two handles
    same(got["background"][0, R0:], repet.simonline(new0, FS))
    same(got["mixture"][0, R0:], new0)
    emitted = first.shape[1]
    want = repet.simonline(moved, FS)
    same(first[1], want[:emitted])
    # (the importing handle emits in lockstep: the moved stream's samples from where A stopped emitting)
    same(got["background"][2, emitted:], want[emitted:])
    same(got["mixture"][2, emitted:], moved[emitted:])
    assert np.any(got["background"][0, R0:]) and np.any(got["background"][2, emitted:])
    assert np.any(got["foreground"][2, emitted:] != got["mixture"][2, emitted:] - got["background"][2, emitted:])


def test_finish_stream_fades_its_own_slot_and_idle_slots_stay_zero():
    H, B = hop_and_buffer()
    ch, S = 2, 4
    Q, N = 330 * H + 101, 350 * H
    xs = streams_of(ch, 11.3, [51, 52, 53, 54], odd=False)[:, :N]
    feed = xs.copy()
    feed[3] = np.nan                                                       # slot 3 is idle: its share of every chunk is NaN
    g0 = [0.2, 0.4, 0.6, 0.5]

    def run(with_finish_stream):
        h = repet.online_streams(FS, ch, S)
        h.release([3])
        h.set_background_gain(g0, slots=range(S))
        pieces = {"background": [], "foreground": []}

        def keep(pair):
            for k, v in zip(("background", "foreground"), pair):
                pieces[k].append(v)

        keep(h.push(feed[:, :Q], which="both"))
        h.set_background_gain([0.9, 0.1], slots=[1, 2])                    # both pending when slot 1 ends
        tail = h.finish_stream(1, which="both") if with_finish_stream else None
        assert h.background_gain(1) == float(np.float32(0.9))
        keep(h.push(feed[:, Q:], which="both"))
        keep(h.finish(which="both"))
        h.close()
        return {k: np.concatenate(v, axis=1) for k, v in pieces.items()}, tail

    got, tail = run(True)
    twin, _ = run(False)
    emitted = ((Q - 512) // H + 1) * H
    n_tail = Q - emitted
    assert tail[0].shape == (n_tail, ch) and H <= n_tail < 2 * H and n_tail % 2 == 1
    # the slot that ended: its own pending change fades over the first hop of its tail
    same(np.concatenate([got["background"][1, :emitted], tail[0]]), repet.simonline(xs[1, :Q], FS))
    assert np.any(tail[0][:H])
    check_fade(tail[1], xs[1, emitted:Q], tail[0], 0.4, 0.9, H)
    assert not got["background"][1, emitted:].any() and not got["foreground"][1, emitted:].any()     # idle from there on
    # the other slots: as if the call had not been made; slot 2's change fades in the push that follows
    for s in (0, 2, 3):
        for k in ("background", "foreground"):
            assert got[k][s].tobytes() == twin[k][s].tobytes()
    same(got["foreground"][0], kept(xs[0], got["background"][0], 0.2))
    same(got["foreground"][2, :emitted], kept(xs[2, :emitted], got["background"][2, :emitted], 0.6))
    n_next = ((N - 512) // H + 1) * H - emitted
    check_fade(got["foreground"][2, emitted:emitted + n_next], xs[2, emitted:emitted + n_next],
               got["background"][2, emitted:emitted + n_next], 0.6, 0.1, H)
    same(got["foreground"][2, emitted + n_next:], kept(xs[2, emitted + n_next:], got["background"][2, emitted + n_next:], 0.1))
    # the idle slot: zeros whatever its gain is and whatever the chunk carried
    assert not got["background"][3].any() and not got["foreground"][3].any()
    assert not np.isnan(got["foreground"]).any() and not np.isnan(got["background"]).any()


# ---- 5. host chunks and device chunks ---------------------------------------------------------------------------------------------
def test_host_chunks_give_the_bytes_of_device_chunks():
    H, B = hop_and_buffer()
    xs = streams_of(2, 12.2, [61, 62, 63])
    full = torch.tensor(xs, device=DEV)
    sizes = lockstep_sizes(xs.shape[1], FS, seed=15)

    def run(chunk_of):
        h = repet.online_streams(FS, 2, 3)
        h.set_background_gain([0.1, 0.35, 1.0], slots=range(3))
        bgs, fgs, pos = [], [], 0
        for k, n in enumerate(sizes):
            if pos > (B + 4) * H and k % 3 == 0:
                h.set_background_gain(((k * 37) % 100) / 100.0, slots=[k % 2])     # fades on both paths alike
            bg, fg = h.push(chunk_of(pos, pos + n), which="both")
            bgs.append(to_numpy(bg)); fgs.append(to_numpy(fg))
            pos += n
        bg, fg = h.finish(which="both")
        h.close()
        return np.concatenate(bgs + [to_numpy(bg)], axis=1), np.concatenate(fgs + [to_numpy(fg)], axis=1)

    host = run(lambda a, b: xs[:, a:b])
    dev = run(lambda a, b: full[:, a:b])
    assert host[0].tobytes() == dev[0].tobytes() and host[1].tobytes() == dev[1].tobytes()
    assert np.any(host[0]) and np.any(host[1][2] != xs[2] - host[0][2])


# ---- 6. tensor calls --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,batched,seconds", [("sim", False, 6.0), ("simonline", True, 12.0)])
def test_separate_with_a_background_gain(algo, batched, seconds):
    g = 10 ** (-12 / 20)
    xs = signals(FS, 2, seconds, [71, 72] if batched else [73]).astype(np.float32)
    t = torch.tensor(xs if batched else xs[0], device=DEV)
    x = to_numpy(t).astype(np.float64)
    bg, fg = repet.separate(algo, t, FS, which="both", background_gain=g)
    assert np.any(to_numpy(bg)) and tuple(fg.shape) == tuple(t.shape)
    same(fg, kept(x, to_numpy(bg), g))
    assert np.any(to_numpy(fg) != x - to_numpy(bg))
    same(repet.separate(algo, t, FS, which="foreground", background_gain=1.0), x)
    store = torch.full(tuple(t.shape) + (2,), 7.0, dtype=torch.float32, device=DEV)
    ret = repet.separate(algo, t, FS, out=store[..., 0], which="foreground", background_gain=g)
    assert ret.dtype == torch.float32 and torch.all(store[..., 1] == 7.0)
    same(ret, to_numpy(fg).astype(np.float32))
    aliasing = torch.empty((1,) * (t.dim() - 1) + (2,), dtype=torch.float64, device=DEV).expand(tuple(t.shape))
    with pytest.raises(ValueError, match="overlap"):                       # refused by the egress itself: the gain does not stick either
        repet.separate(algo, t, FS, out=aliasing, which="foreground", background_gain=g)
    plain = repet.separate(algo, t, FS, which="foreground")                # the following call: the foreground as ever
    same(plain, x - to_numpy(bg))
    same(repet.separate(algo, t, FS, which="foreground", background_gain=0.0), plain)
    same(repet.separate(algo, t, FS), bg)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    H, B = hop_and_buffer()
    ch, S = 2, 3
    xs = streams_of(ch, 12.0, [81, 82, 83])
    sizes = [320 * H, 3 * H, 5 * H + 1, xs.shape[1] - 328 * H - 1]
    lib = _native.lib()

    def run(abuse):
        h = repet.online_streams(FS, ch, S)
        h.set_background_gain([0.25, 0.5], slots=[0, 1])
        pieces, pos = [], 0
        for n in sizes:
            if abuse:
                for bad in (-0.1, 1.5, float("nan"), float("inf")):
                    one, two = (C.c_float * 1)(bad), (C.c_float * 2)(0.75, bad)
                    assert lib.repet_online_set_background_gain(h._h, None, 0, one) == _native.ERR_BAD_ARG
                    assert b"[0, 1]" in lib.repet_last_error()
                    assert lib.repet_online_set_background_gain(h._h, (C.c_int32 * 2)(2, 0), 2, two) == _native.ERR_BAD_ARG
                    assert lib.repet_ctx_set_background_gain(_native.tensor_context(0).handle, bad) == _native.ERR_BAD_ARG
                    with pytest.raises(ValueError):
                        h.set_background_gain(bad)
                    with pytest.raises(ValueError):
                        h.set_background_gain([0.75, bad], slots=[2, 0])
                assert lib.repet_online_set_background_gain(h._h, (C.c_int32 * 2)(2, S), 2, (C.c_float * 2)(0.75, 0.75)) == _native.ERR_BAD_ARG
                assert b"slot" in lib.repet_last_error()
                assert lib.repet_online_set_background_gain(h._h, (C.c_int32 * 1)(-1), 1, (C.c_float * 1)(0.75)) == _native.ERR_BAD_ARG
                assert lib.repet_online_background_gain(h._h, S, C.byref(C.c_float())) == _native.ERR_BAD_ARG
                with pytest.raises(ValueError):
                    h.set_background_gain(0.75, slots=[S])
                with pytest.raises(ValueError):
                    h.background_gain(S)
                assert [h.background_gain(s) for s in range(S)] == [0.25, 0.5, 0.0]
            pieces.append(h.push(xs[:, pos:pos + n], which="both"))
            pos += n
        pieces.append(h.finish(which="both"))
        h.close()
        return np.concatenate([p[0] for p in pieces], axis=1), np.concatenate([p[1] for p in pieces], axis=1)

    clean, abused = run(False), run(True)
    assert clean[0].tobytes() == abused[0].tobytes() and clean[1].tobytes() == abused[1].tobytes()
    for s, g in enumerate((0.25, 0.5, 0.0)):
        same(clean[1][s], kept(xs[s], clean[0][s], g))
    assert np.any(clean[0])
    t = torch.zeros((4 * FS, ch), device=DEV)
    for which in ("background", "mixture"):
        with pytest.raises(ValueError, match="background_gain"):
            repet.separate("sim", t, FS, which=which, background_gain=0.5)
    with pytest.raises(ValueError, match="background_gain"):
        repet.separate("sim", t, FS, background_gain=0.5)
    with pytest.raises(ValueError, match="background_gain"):
        repet.separate("sim", t, FS, which="both", background_gain=1.5)
