"""The foreground, aligned (``which=`` of the live handles and of ``repet.separate``).

For a stream with input ``x`` (as float64 values) and ``bg`` the background the same handle returns:

* input that is exactly fp32 + fp32 (float32 / float16 / bfloat16 / int16, float64 derived from PCM or fp32): foreground
  ``== x - bg`` and mixture ``== x``, bit for bit, NaN positions equal;
* any other float64 input: the engine holds ``hi = fp32(x)`` and ``lo = fp32(x - hi)``. Both casts round to nearest (the
  ingest kernels and the host conversion use plain C conversions: ``(float)x``, ``(float)(x - (double)hi)``), the subtraction
  in between is exact, so ``|x - (hi + lo)| <= 2**-24 * |x - hi| <= 2**-48 |x|`` as long as neither cast leaves fp32's normal
  range (asserted on the test data: ``x == 0`` or ``|x| >= 2**-100``). The foreground is ``fl(hi + lo - bg)`` against
  ``fl(x - bg)``: two roundings of at most ``2**-53 (|x| + |bg|)`` each on top, hence ``|fg - (x - bg)| <= 2**-47 *
  max(|x|, |bg|)`` elementwise, and ``|mixture - x| <= 2**-48 |x|``. Derived, not measured;
* a float32 destination holds ``np.float32`` of the float64 result, bit for bit;
* ``bg == repet.simonline(x, fs)`` bit for bit (the existing guarantee), asserted here as well."""
import ctypes as C
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet import _native
from repet_synth import synth
from test_gpu_online_streams import DEVICE_DTYPES, lockstep_sizes, same, signals, sleep_cycles
from test_gpu_online_slots import Drive, churn_scenario, plan_sizes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def to_numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def pcm_exact(xs):
    """float64 values derived from 16-bit PCM: every one is an fp32 value."""
    out = np.clip(np.round(xs * 20000), -32768, 32767) / 32768.0
    assert np.array_equal(out, out.astype(np.float32).astype(np.float64))
    return out


def check_rules(fg, mix, x, bg, exact):
    """The rules of the module docstring for one stream (or any block of samples)."""
    if exact:
        same(fg, x - bg)
        same(mix, x)
        return
    assert ((x == 0) | (np.abs(x) >= 2.0 ** -100)).all()
    err = np.abs(fg - (x - bg))
    assert (err <= 2.0 ** -47 * np.maximum(np.abs(x), np.abs(bg))).all(), f"foreground off by up to {err.max():.3e}"
    err = np.abs(mix - x)
    assert (err <= 2.0 ** -48 * np.abs(x)).all(), f"mixture off by up to {err.max():.3e}"


def run_which(h, xs, sizes, which="both", chunk_of=None, mixture=False, close=True):
    """Push xs (S, N, C) in the given sizes with ``which``; the concatenated signal(s), ``mixture`` adding what
    ``last_emission("mixture")`` returns after every emitting call. A dict name -> (S, N, C)."""
    chunk_of = chunk_of or (lambda a, b: xs[:, a:b])
    names = ("background", "foreground") if which == "both" else (which,)
    pieces = {k: [] for k in names + (("mixture",) if mixture else ())}
    pos = 0

    def keep(got):
        got = got if which == "both" else (got,)
        for k, g in zip(names, got):
            pieces[k].append(to_numpy(g))
        if mixture:
            m = to_numpy(h.last_emission("mixture"))
            assert m.shape == pieces[names[0]][-1].shape
            pieces["mixture"].append(m)

    for n in sizes:
        expect = h.emit_count(n)
        got = h.push(chunk_of(pos, pos + n), which=which)
        assert tuple((got[0] if which == "both" else got).shape) == (xs.shape[0], expect, xs.shape[2])
        keep(got)
        pos += n
    keep(h.finish(which=which))
    if close:
        h.close()
    out = {k: np.concatenate(v, axis=1) for k, v in pieces.items()}
    assert all(v.shape == xs.shape for v in out.values())
    return out


# ---- 1. lockstep parity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pcm", "raw"])
@pytest.mark.parametrize("fs,channels,seconds", [(8000, 1, 13.0), (8000, 2, 12.5), (44100, 1, 11.2), (44100, 2, 11.3)])
def test_lockstep_parity(fs, channels, seconds, kind):
    xs = signals(fs, channels, seconds, [3, 5, 7, 11, 13])
    if kind == "pcm":
        xs = pcm_exact(xs)
    sizes = lockstep_sizes(xs.shape[1], fs, seed=fs + channels)
    p = repet.derive_params(fs)
    assert any(n > p.buffer_frames * p.step_length for n in sizes) and any(n % p.step_length for n in sizes)
    got = run_which(repet.online_streams(fs, channels, len(xs)), xs, sizes, "both", mixture=True)
    for s, x in enumerate(xs):
        want_bg = repet.simonline(x, fs)
        same(got["background"][s], want_bg)
        check_rules(got["foreground"][s], got["mixture"][s], x, got["background"][s], kind == "pcm")
        check_rules(got["foreground"][s], got["mixture"][s], x, want_bg, kind == "pcm")
    assert np.any(got["foreground"]) and np.any(got["background"])


# ---- 2. one pass against two ----------------------------------------------------------------------------------------------
def test_both_equals_background_and_foreground_of_twin_handles():
    fs, ch = 8000, 2
    xs = signals(fs, ch, 12.0, [21, 22, 23])
    sizes = lockstep_sizes(xs.shape[1], fs, seed=4)
    both = run_which(repet.online_streams(fs, ch, 3), xs, sizes, "both")
    bg = run_which(repet.online_streams(fs, ch, 3), xs, sizes, "background")["background"]
    fg = run_which(repet.online_streams(fs, ch, 3), xs, sizes, "foreground")["foreground"]
    mix = run_which(repet.online_streams(fs, ch, 3), xs, sizes, "mixture")["mixture"]
    same(both["background"], bg)
    same(both["foreground"], fg)
    check_rules(fg, mix, xs, bg, False)
    # and the default is the background, as before
    h = repet.online_streams(fs, ch, 3)
    pieces = [h.push(xs[:, :9 * fs]), h.push(xs[:, 9 * fs:]), h.finish()]
    h.close()
    same(np.concatenate(pieces, axis=1), bg)


# ---- 3. no dead air ---------------------------------------------------------------------------------------------------------
def test_the_warm_up_foreground_is_the_input():
    fs, ch = 8000, 2
    p = repet.derive_params(fs)
    quiet = (p.buffer_frames - 1) * p.step_length
    xs = pcm_exact(signals(fs, ch, 12.0, [31, 32]))
    got = run_which(repet.online_streams(fs, ch, 2), xs, lockstep_sizes(xs.shape[1], fs, seed=8), "both")
    assert not got["background"][:, :quiet].any()
    same(got["foreground"][:, :quiet], xs[:, :quiet])
    assert np.any(got["foreground"][:, :quiet])
    assert np.any(got["background"][:, quiet:]) and not np.array_equal(got["foreground"][:, quiet:], xs[:, quiet:])


# ---- 4. slots ---------------------------------------------------------------------------------------------------------------
class Selected:
    """A handle whose emitting calls deliver one fixed signal (what ``Drive`` of the slot tests then records)."""

    def __init__(self, h, which):
        self.h, self.which = h, which

    def push(self, chunk, out=None):
        return self.h.push(chunk, out=out, which=self.which)

    def finish(self, out=None):
        return self.h.finish(out=out, which=self.which)

    def finish_stream(self, slot, out=None):
        return self.h.finish_stream(slot, out=out, which=self.which)

    def __getattr__(self, name):
        return getattr(self.h, name)


@pytest.mark.parametrize("which", ["foreground", "mixture"])
def test_lives_foreground_equals_input_minus_simonline(which):
    fs, ch = 8000, 2
    xs, sizes, actions, lives, (H, B, P3a) = churn_scenario(fs, ch, np.nan)
    fp32_exact = lambda a: a.astype(np.float32).astype(np.float64)         # float64 derived from fp32: the bit-for-bit rule
    xs, lives = fp32_exact(xs), [(slot, P, Q, fp32_exact(x), whole) for slot, P, Q, x, whole in lives]
    d = Drive(Selected(repet.online_streams(fs, ch, 5), which), xs).run(sizes, actions)
    assert not np.isnan(d.whole).any()
    assert not d.whole[4].any()                                            # idle and fed NaN: exactly zero
    assert not d.whole[1, :lives[1][1]].any()                              # idle (NaN) until its restart, its last hop included
    P2b = lives[3][1]
    assert np.isnan(xs[2, P2b - H:P2b]).all() and not d.whole[2, lives[2][2]:P2b].any()
    same(d.whole[3, :P3a - H], xs[3, :P3a - H])                            # a life that never left its warm-up: its input
    assert np.any(xs[3, P3a - H:P3a]) and not d.whole[3, P3a - H:P3a].any()   # the hop emitted behind a restart: zero
    P3b = lives[5][1]
    assert np.any(xs[3, P3b - H:P3b]) and not d.whole[3, P3b - H:P3b].any()
    for slot, P, Q, x, whole in lives:
        want = x - repet.simonline(x, fs) if which == "foreground" else x
        if whole:
            same(d.life(slot, P, Q), want)
        else:
            same(d.lockstep[slot, P:Q - H], want[:Q - P - H])
        assert np.any(want[(B - 1) * H:] != x[(B - 1) * H:]) == (which == "foreground")


def test_finish_stream_both_on_the_device_off_the_hop_grid():
    fs, ch, S = 8000, 2, 3
    p = repet.derive_params(fs)
    H, B = p.step_length, p.buffer_frames
    Q, total = 330 * H + 100, 340 * H
    xs = pcm_exact(np.stack([synth(total / fs + 0.01, fs, ch, s)[:total] for s in (91, 92, 93)])).astype(np.float32)
    full = torch.tensor(xs, device=DEV)
    h = repet.online_streams(fs, ch, S)
    fgs, pos = [], 0
    for n in plan_sizes(Q, [], H, B, 2):
        fgs.append(to_numpy(h.push(full[:, pos:pos + n], which="foreground")))
        pos += n
    n_rest = h.stream_emit_count(1)
    store = torch.full((2, n_rest, 2 * ch), 7.0, dtype=torch.float64, device=DEV)
    bg_tail, fg_tail = h.finish_stream(1, out=(store[0, :, ::2], store[1, :, ::2]), which="both")
    assert torch.all(store[:, :, 1::2] == 7.0)
    with pytest.raises(ValueError):
        h.last_emission("mixture")                                         # the slot was released: the samples are gone
    rest = to_numpy(h.push(full[:, Q:], which="foreground"))
    assert not rest[1].any()                                               # idle from its finish_stream on
    tail_all = to_numpy(h.finish(which="foreground"))
    h.close()
    x = xs[1, :Q].astype(np.float64)
    want_bg = repet.simonline(xs[1, :Q], fs)
    emitted = sum(f.shape[1] for f in fgs)
    same(to_numpy(bg_tail), want_bg[emitted:])
    same(np.concatenate([f[1] for f in fgs] + [to_numpy(fg_tail)]), x - want_bg)
    other = np.concatenate([f[0] for f in fgs] + [rest[0], tail_all[0]])
    same(other, xs[0].astype(np.float64) - repet.simonline(xs[0], fs))


# ---- 5. device chunks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", ["f32", "f64"])
@pytest.mark.parametrize("dtype", list(DEVICE_DTYPES))
def test_device_chunks_equal_host_chunks(dtype, out_dtype):
    fs, ch, S = 8000, 2, 3
    xs = signals(fs, ch, 11.4, [31, 32, 33])
    if dtype == "i16":
        xs = np.clip(np.round(xs * 20000), -32768, 32767)
    t = torch.tensor(xs, dtype=DEVICE_DTYPES[dtype])
    host = t.numpy() if dtype in ("f64", "f32", "i16") else t.to(torch.float32).numpy()
    full = t.to(DEV)
    sizes = lockstep_sizes(xs.shape[1], fs, seed=77)
    want = run_which(repet.online_streams(fs, ch, S), host, sizes, "both", mixture=True)
    check_rules(want["foreground"], want["mixture"], host.astype(np.float64), want["background"], dtype != "f64")
    tdt = torch.float32 if out_dtype == "f32" else torch.float64
    h = repet.online_streams(fs, ch, S)
    got = {"background": [], "foreground": [], "mixture": []}
    pos = 0

    def stores(m):
        # non-dense destinations: every other sample of a channels-first store, and a channel slice of a wider one
        a = torch.full((S, ch, 2 * m + 1), 7.0, dtype=tdt, device=DEV)
        b = torch.full((S, m, ch + 3), 7.0, dtype=tdt, device=DEV)
        return a, a[:, :, 1::2].permute(0, 2, 1), b, b[:, :, 2:2 + ch]

    def keep(a, bg, b, fg, ret):
        assert ret[0] is bg and ret[1] is fg
        assert torch.all(a[:, :, 0::2] == 7.0) and torch.all(b[:, :, :2] == 7.0) and torch.all(b[:, :, 2 + ch:] == 7.0)
        got["background"].append(to_numpy(bg))
        got["foreground"].append(to_numpy(fg))
        mix = torch.full((S, 2 * bg.shape[1], ch), 7.0, dtype=tdt, device=DEV)
        assert h.last_emission("mixture", out=mix[:, ::2]) is not None
        assert torch.all(mix[:, 1::2] == 7.0)
        got["mixture"].append(to_numpy(mix[:, ::2]))

    for n in sizes:
        a, bg, b, fg = stores(h.emit_count(n))
        keep(a, bg, b, fg, h.push(full[:, pos:pos + n], out=(bg, fg), which="both"))
        pos += n
    a, bg, b, fg = stores(h.emit_count(0, True))
    keep(a, bg, b, fg, h.finish(out=(bg, fg), which="both"))
    h.close()
    for k, v in got.items():
        w = want[k].astype(np.float32) if out_dtype == "f32" else want[k]
        same(np.concatenate(v, axis=1), w)


def test_device_push_of_both_does_not_wait_on_the_host():
    fs, ch, S = 8000, 2, 8
    p = repet.derive_params(fs)
    hop = p.step_length
    xs = signals(fs, ch, 12.0, range(40, 48)).astype(np.float32)
    full = torch.tensor(xs, device=DEV)
    h = repet.online_streams(fs, ch, S, max_push_samples=4 * hop)
    pieces, pos = [], 0

    def push(n):
        nonlocal pos
        pieces.append(h.push(full[:, pos:pos + n], which="both"))
        pos += n

    while pos < 11 * fs:
        push(fs // 2)
    push(2 * hop)                                    # the warm-up push of the timed size
    torch.cuda.synchronize()
    torch.cuda._sleep(sleep_cycles(100))
    t0 = time.perf_counter()
    push(2 * hop)
    mix = h.last_emission("mixture")
    elapsed = time.perf_counter() - t0
    assert elapsed < 0.05, f"the device push took {elapsed * 1e3:.1f} ms behind a 100-ms sleep: it waited on the host"
    torch.cuda.synchronize()
    end = ((pos - p.window_length) // hop + 1) * hop                       # the frames complete so far, in whole hops
    same(mix, xs[:, end - 2 * hop:end].astype(np.float64))
    while pos < xs.shape[1]:
        push(min(fs // 2, xs.shape[1] - pos))
    pieces.append(h.finish(which="both"))
    h.close()
    bg = torch.cat([p[0] for p in pieces], dim=1).cpu().numpy()
    fg = torch.cat([p[1] for p in pieces], dim=1).cpu().numpy()
    for s, x in enumerate(xs):
        same(bg[s], repet.simonline(x, fs))
        same(fg[s], x.astype(np.float64) - bg[s])


# ---- 6. samples that are not finite -----------------------------------------------------------------------------------------
def test_nan_and_infinite_samples_stay_in_their_stream():
    fs, ch = 8000, 2
    xs = pcm_exact(signals(fs, ch, 12.0, [51, 52, 53, 54]))
    xs[2, 40000:40003, 1] = np.nan
    xs[2, 70001, 0] = np.inf
    xs[2, 90500, 1] = -np.inf
    got = run_which(repet.online_streams(fs, ch, len(xs)), xs, lockstep_sizes(xs.shape[1], fs, seed=5), "both", mixture=True)
    for s, x in enumerate(xs):
        with np.errstate(invalid="ignore"):
            same(got["foreground"][s], x - got["background"][s])
        same(got["mixture"][s], x)
        if s == 2:
            assert np.isnan(got["foreground"][s]).sum() > 3 and np.isnan(got["background"][s]).any()
        else:
            same(got["background"][s], repet.simonline(x, fs))
            assert np.isfinite(got["foreground"][s]).all()


# ---- 7. the single-stream form; host and device pushes on one handle ----------------------------------------------------------
def test_single_stream_form():
    fs, ch = 8000, 2
    x = pcm_exact(synth(12.3, fs, ch, 61))
    sizes = lockstep_sizes(len(x), fs, seed=61)
    want = repet.simonline(x, fs)
    for which in ("foreground", "mixture", "both"):
        h = repet.online(fs, ch)
        pieces, pos = [], 0
        for n in sizes:
            pieces.append(h.push(x[pos:pos + n], which=which))
            pos += n
        pieces.append(h.finish(which=which))
        h.close()
        if which == "both":
            same(np.concatenate([p[0] for p in pieces]), want)
            same(np.concatenate([p[1] for p in pieces]), x - want)
        else:
            same(np.concatenate(pieces), x - want if which == "foreground" else x)


def test_host_and_device_pushes_mixed_on_one_handle():
    fs, ch, S = 8000, 2, 2
    xs = pcm_exact(signals(fs, ch, 12.0, [71, 72]))
    full = torch.tensor(xs, device=DEV)
    sizes = lockstep_sizes(xs.shape[1], fs, seed=12)
    h = repet.online_streams(fs, ch, S)
    fg, bg, pos = [], [], 0
    for k, n in enumerate(sizes):
        if k % 3 == 0:
            b, f = h.push(xs[:, pos:pos + n], which="both")
            assert isinstance(f, np.ndarray)
        elif k % 3 == 1:
            f = h.push(full[:, pos:pos + n], which="foreground")
            assert isinstance(f, torch.Tensor)
            b = h.last_emission("background")
        else:
            b = h.push(full[:, pos:pos + n].to(torch.float32))
            f = h.last_emission("foreground", out=torch.empty(tuple(b.shape), dtype=torch.float64, device=DEV))
        fg.append(to_numpy(f))
        bg.append(to_numpy(b))
        pos += n
    b, f = h.finish(which="both")
    h.close()
    bg, fg = np.concatenate(bg + [to_numpy(b)], axis=1), np.concatenate(fg + [to_numpy(f)], axis=1)
    for s, x in enumerate(xs):
        same(bg[s], repet.simonline(x, fs))
        same(fg[s], x - bg[s])


# ---- 8. offline tensors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f16"])
@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("algo", ["original", "extended", "adaptive", "sim", "simonline"])
def test_separate_which(algo, batched, dtype):
    fs, ch = 8000, 2
    xs = signals(fs, ch, 12.0, [81, 82] if batched else [83])
    t = torch.tensor(xs if batched else xs[0], dtype=DEVICE_DTYPES[dtype], device=DEV)
    x = t.to(torch.float64).cpu().numpy()
    bg = repet.separate(algo, t, fs)
    assert bg.dtype == torch.float64 and np.any(to_numpy(bg))
    fg = repet.separate(algo, t, fs, which="foreground")
    mix = repet.separate(algo, t, fs, which="mixture")
    assert fg.dtype == torch.float64 and tuple(fg.shape) == tuple(t.shape)
    check_rules(to_numpy(fg), to_numpy(mix), x, to_numpy(bg), dtype != "f64")
    if dtype == "f64":
        # the remainders were used: the float32 samples alone would be off by far more than the bound allows
        assert np.abs(x.astype(np.float32).astype(np.float64) - to_numpy(bg) - to_numpy(fg)).max() > 2.0 ** -40
    both = repet.separate(algo, t, fs, which="both")
    same(both[0], bg)
    same(both[1], fg)
    store = torch.full((2,) + tuple(t.shape) + (2,), 7.0, dtype=torch.float32, device=DEV)
    out = (store[0, ..., 0], store[1, ..., 0])
    ret = repet.separate(algo, t, fs, out=out, which="both")
    assert ret[0] is out[0] and ret[1] is out[1] and torch.all(store[..., 1] == 7.0)
    same(ret[0], to_numpy(bg).astype(np.float32))
    same(ret[1], to_numpy(fg).astype(np.float32))
    same(repet.separate(algo, t, fs), bg)                                   # the selection does not stick


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    fs, ch, S = 8000, 2, 3
    H = repet.derive_params(fs).step_length
    h = repet.online_streams(fs, ch, S)
    lib = _native.lib()
    for bad in (-1, 3):
        assert lib.repet_online_set_output(h._h, bad) == _native.ERR_BAD_ARG
        assert lib.repet_online_also_emit(h._h, bad, None, _native.F64, None) == _native.ERR_BAD_ARG
        assert lib.repet_online_last_emission(h._h, bad, None, 0, C.byref(C.c_int64())) == _native.ERR_BAD_ARG
        assert lib.repet_ctx_select_result(_native.tensor_context(0).handle, bad) == _native.ERR_BAD_ARG
    with pytest.raises(ValueError):
        h.last_emission("foreground")                                      # nothing was emitted yet
    x = torch.zeros((S, 4 * H, ch), device=DEV)
    m = h.emit_count(4 * H)
    assert m == 3 * H
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        h.push(x, out=f64(S, m, ch), which="both")                         # one tensor where a pair is due
    with pytest.raises(ValueError):
        h.push(x, out=(f64(S, m, ch), f64(S, m + 1, ch)), which="both")    # wrong shape
    with pytest.raises(ValueError):
        h.push(x, out=(f64(S, m, ch), torch.empty((S, m, ch), dtype=torch.float32, device=DEV)), which="both")
    with pytest.raises(ValueError):
        h.push(x, out=(f64(S, m, ch), f64(S, m, ch)), which="foreground")  # a pair where one tensor is due
    shared = f64(S, m + 1, ch)
    with pytest.raises(ValueError):
        h.push(x, out=(shared[:, :m], shared[:, 1:]), which="both")        # the pair overlaps
    # (the same through the C ABI alone: refused by the emitting call, before any launch, and nothing was pushed)
    strides = (C.c_int64 * 3)(*shared[:, :m].stride())
    n = C.c_int64()
    stream = _native._stream_handle(torch.cuda.current_stream())
    assert lib.repet_online_also_emit(h._h, 1, C.c_void_p(shared[:, 1:].data_ptr()), _native.F64, strides) == 0
    assert lib.repet_online_push_device(h._h, C.c_void_p(x.data_ptr()), _native.F32, 4 * H, (C.c_int64 * 3)(*x.stride()), stream,
                                        C.c_void_p(shared.data_ptr()), _native.F64, strides, stream, C.byref(n)) == _native.ERR_BAD_ARG
    assert b"overlap" in lib.repet_last_error()
    assert h.samples_pushed == 0 and h.emit_count(4 * H) == m
    got = h.push(x, which="foreground")
    assert tuple(got.shape) == (S, m, ch)
    assert tuple(h.last_emission("mixture").shape) == (S, m, ch)
    with pytest.raises(ValueError):
        h.last_emission("mixture", out=f64(S, m + 2, ch))                  # wrong shape
    with pytest.raises(ValueError):
        h.last_emission("both")
    h.restart([1])
    with pytest.raises(ValueError, match="stale"):
        h.last_emission("mixture")                                         # stale: a restart came after the emission
    h.push(x)
    assert tuple(h.last_emission("foreground").shape) == (S, 4 * H, ch)
    h.release([2])
    with pytest.raises(ValueError, match="stale"):
        h.last_emission("foreground")
    h.close()
    t = torch.zeros((12 * fs, ch), dtype=torch.float64, device=DEV)
    pair = torch.empty((12 * fs + 1, ch), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        repet.separate("sim", t, fs, out=(pair[:-1], pair[1:]), which="both")
    with pytest.raises(ValueError):
        repet.separate("sim", t, fs, out=pair[:-1], which="both")
    with pytest.raises(ValueError):
        repet.separate("sim", t, fs, which="vocals")
