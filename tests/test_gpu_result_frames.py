"""The spectra of a tensor call (``repet.separate(..., frames=, frame_bands=, frames_out=)``, ``Context.request_frames``;
include/repet_hip.h: repet_ctx_request_frames): the fp32 magnitudes of mixture, background and foreground of every frame of the
clip(s), whole or in bands, written behind the pass that decided them.

Expected values come from the float64 statement of tests/result_frames_reference.py (tied to the oracle by
tests/test_result_frames_reference.py). Every case first asserts that what the variant DECIDED -- the period, the periods, the
similar-frame lists -- is the statement's, so every frame of every case is compared and none is left out. Bars, the ones
tests/test_gpu_online_frames.py derives for the live frames (a median, a minimum and a period gather pick values, they do not
amplify their error), none of them fitted:

  mix   2e-6 x max |want|      bit for bit the V of ``repet._stft_stage`` on the same samples as well
  bg    2.5e-6 x max |want|    (max |want| over the case's whole statement of that signal, past the warm-up for bg and fg)
  fg    4.5e-6 x max |want|
  bands F x 2**-53 relative, against the float64 sum of squares of the call's own frames
  everything else              exact: bit for bit

Measured on an MI355X (profiles/result_frames_parity.txt, the output of the last test here): every case holds all three bars,
the worst ratio err / bar being 0.129 (foreground of ``sim``, 36 s at 8 kHz). The foreground of the W = 8192 case is zero in the
statement -- 1.5 s hold 72 frames and similarity_distance is 47, so every list is the frame alone -- and zero on the device: its
bar is 0 and it is held exactly.

The cases are the smallest that reach every path: 44.1 kHz stereo and mono (the register kernels, the model form of
``original``, the mask plane of ``adaptive``, ``sim`` and ``simonline``), 8 kHz ``sim`` with more than 1024 frames (the median on
rank codes, masked in place) and with fewer (the float median), W = 8192 (always in place), ``simonline`` with a start of 33
frames. Between them the three forms a pipeline leaves its masked spectrum in are all met: asserted."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from frames_reference import band_energies
from helpers import periodic_clip
from oracle import repet_oracle as orc
from repet import _native
from result_frames_reference import frame_count, statement
from test_gpu_online_foreground import to_numpy
from test_gpu_online_frames import BARS, WHICH, same_bits
from test_gpu_online_start import fp32_exact, signal
from test_gpu_stft_stages import window_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = {"mixture": "mix", "background": "bg", "foreground": "fg"}
PARITY = {}

# name: (algo, fs, samples, channels, start_frames, how the signal is made)
CASES = {
    "original-44k-stereo": ("original", 44100, 4 * 44100, 2, None, "periodic"),
    "original-44k-mono": ("original", 44100, 4 * 44100 + 333, 1, None, "periodic"),
    "adaptive-44k-stereo": ("adaptive", 44100, 12 * 44100, 2, None, "periodic"),
    "sim-44k-stereo": ("sim", 44100, 12 * 44100 + 7, 2, None, 31),
    "simonline-44k-mono": ("simonline", 44100, 12 * 44100, 1, None, 61),
    "simonline-44k-stereo-start33": ("simonline", 44100, 3 * 44100, 2, 33, 62),
    "sim-8k-36s-ranks": ("sim", 8000, 36 * 8000, 2, None, 31),
    "sim-8k-4s-float": ("sim", 8000, 4 * 8000 + 5, 2, None, 61),
    "sim-192k-w8192": ("sim", 192000, 288000, 1, None, 62),
}


def clip_of(name):
    algo, fs, n, ch, start, how = CASES[name]
    if how == "periodic":
        # a period of 50 hops lies inside the period range of a 4 s clip (43 .. 58 frames at 44.1 kHz); the noise breaks the ties
        x = fp32_exact(periodic_clip(fs, 50, n / fs + 0.01, ch, seed=3, jitter=1e-3)[:n])
    else:
        x = np.array(signal(how, n, fs, ch))
    assert x.shape == (n, ch)
    return x


@functools.lru_cache(maxsize=None)
def want_of(name):
    """The float64 statement of the case: computed once, shared, left unchanged."""
    algo, fs, n, ch, start, _ = CASES[name]
    with np.errstate(invalid="ignore", divide="ignore"):
        st = statement(algo, clip_of(name), fs, start_frames=start)
    for k in ("mix", "bg", "fg"):
        st[k].setflags(write=False)
    return st


class online_start:
    """``start_frames`` on this thread's tensor context for the calls inside (None: nothing set)."""

    def __init__(self, start):
        self.start = start

    def __enter__(self):
        if self.start is not None:
            _native.tensor_context(0).set_online_start(self.start)

    def __exit__(self, *exc):
        if self.start is not None:
            _native.tensor_context(0).set_online_start(0)


def decisions(name):
    """What the last run on the tensor context decided, in the statement's terms."""
    algo, fs, n, ch, start, _ = CASES[name]
    ctx = _native.tensor_context(0)
    p = repet.derive_params(fs)
    t = frame_count(algo, n, fs)
    if algo == "original":
        return {"period": int(ctx.last_periods(1)[0])}
    if algo == "adaptive":
        return {"periods": np.asarray(ctx.last_periods(t), dtype=np.int64)}
    first = 0 if algo == "sim" else (start or p.buffer_frames) - 1
    idx, cnt = ctx.last_sim_indices(t - first, p.sim_number)
    lists = [np.zeros(0, dtype=np.int64)] * first + [np.sort(idx[r, :cnt[r]].astype(np.int64)) for r in range(t - first)]
    return {"lists": lists}


@functools.lru_cache(maxsize=None)
def run_of(name):
    """The case through ``repet.separate``: the three signals from three calls, the waveform of each, the plain call's waveform,
    the decisions and the form of the masked spectrum. Run once, shared."""
    algo, fs, n, ch, start, _ = CASES[name]
    x = torch.from_numpy(clip_of(name)).to(DEV)
    out = {}
    with online_start(start):
        plain = to_numpy(repet.separate(algo, x, fs))
        for which in WHICH:
            wave, frames = repet.separate(algo, x, fs, frames=which)
            assert frames.dtype == torch.float32 and frames.device == x.device
            out[which] = to_numpy(frames)
            same_bits(to_numpy(wave), plain)                      # the waveform does not know it was asked
        out["decided"] = decisions(name)
        out["form"] = _native.tensor_context(0).last_spectrum_form
    out["plain"] = plain
    return out


def note(check, err, bar):
    ratio = err / bar if bar > 0 else 0.0
    if check not in PARITY or ratio > PARITY[check][0]:
        PARITY[check] = (ratio, err, bar)


@pytest.mark.parametrize("name", list(CASES))
def test_frames_against_the_statement(name):
    algo, fs, n, ch, start, _ = CASES[name]
    want, got = want_of(name), run_of(name)
    p = repet.derive_params(fs)
    t, f, cut = frame_count(algo, n, fs), p.window_length // 2 + 1, p.cutoff_bins
    assert t == repet.frame_count(algo, n, fs) and cut >= 1
    # the decisions first: they are the statement's, so no frame is left out below
    decided = got["decided"]
    if algo == "original":
        assert decided["period"] == want["period"]
    elif algo == "adaptive":
        assert np.array_equal(decided["periods"], want["periods"])
    else:
        assert len(decided["lists"]) == len(want["lists"]) == t
        differ = [j for j in range(t) if not np.array_equal(decided["lists"][j], want["lists"][j])]
        assert not differ, f"{len(differ)} of {t} lists differ from the statement's, first frame {differ[0]}"
    mix, bg, fg = (got[w] for w in WHICH)
    assert mix.shape == bg.shape == fg.shape == (t, ch, f)
    # the mixture is the forward kernel's V, bit for bit
    stage = repet._stft_stage(clip_of(name), window_of(p.window_length), p.step_length, centred=algo != "simonline")
    assert stage["T"] == t and stage["F"] == f
    same_bits(mix, np.ascontiguousarray(np.transpose(stage["V"][0, :, :t, :f], (1, 0, 2))))
    # the exact relations: foreground = max(mixture - background, 0); the high-pass bins; the warm-up
    with np.errstate(invalid="ignore"):
        same_bits(fg, np.maximum(mix - bg, np.float32(0)))
    warm = want["warm"]
    assert warm == ((start or p.buffer_frames) - 1 if algo == "simonline" else 0)
    assert not bg[:warm].any()
    same_bits(fg[:warm], mix[:warm])
    same_bits(bg[warm:, :, 1:cut + 1], mix[warm:, :, 1:cut + 1])
    assert not fg[warm:, :, 1:cut + 1].any()
    # parity, every frame
    for which in WHICH:
        ref = want[KEYS[which]]
        rows = slice(None) if which == "mixture" else slice(warm, None)
        top = float(np.max(np.abs(ref[rows])))
        err = float(np.max(np.abs(got[which][rows].astype(np.float64) - ref[rows])))
        note(f"{which:10s} {name}", err, BARS[which] * top)
        print(f"{name} {which}: err {err:.3e} bar {BARS[which] * top:.3e}")       # (a statement that is all zero has the bar 0)
    for which in WHICH:
        ratio, err, bar = PARITY[f"{which:10s} {name}"]
        assert err <= bar, (name, which, err, bar)


def test_all_three_forms_of_the_masked_spectrum_are_met():
    forms = {name: run_of(name)["form"] for name in CASES}
    assert set(forms.values()) == {0, 1, 2}, forms
    assert forms["sim-192k-w8192"] == 0 and forms["sim-8k-36s-ranks"] == 0          # W = 8192; rank codes without the register inverse
    assert forms["original-44k-stereo"] == forms["original-44k-mono"] == 2          # the model, on the register inverse STFT


@pytest.mark.parametrize("name", ["original-44k-stereo", "sim-8k-4s-float", "simonline-44k-stereo-start33", "sim-192k-w8192"])
def test_two_calls_return_the_same_bits_and_out_takes_any_strides(name):
    algo, fs, n, ch, start, _ = CASES[name]
    got = run_of(name)
    x = torch.from_numpy(clip_of(name)).to(DEV)
    t, c, f = got["background"].shape
    with online_start(start):
        for which in ("background", "foreground"):
            _, again = repet.separate(algo, x, fs, frames=which)
            same_bits(to_numpy(again), got[which])
        # a destination with permuted strides and a gap between rows: the same values, nothing written outside them
        base = torch.full((c, f + 3, t), -7.0, dtype=torch.float32, device=DEV)
        view = base.permute(2, 0, 1)[:, :, :f]
        assert view.shape == (t, c, f) and not view.is_contiguous()
        wave, ret = repet.separate(algo, x, fs, frames="background", frames_out=view)
        assert ret is view
        same_bits(to_numpy(view), got["background"])
        assert (to_numpy(base)[:, f:, :] == -7.0).all()
        same_bits(to_numpy(wave), got["plain"])
        # with the levels: result, levels, frames
        res = repet.separate(algo, x, fs, which="foreground", background_gain=0.5, levels=True, frames="background")
        assert len(res) == 3 and tuple(res[1].shape) == (c, len(repet.LEVELS))
        same_bits(to_numpy(res[2]), got["background"])                    # the gains do not change the spectra


@pytest.mark.parametrize("name", ["original-44k-mono", "adaptive-44k-stereo", "sim-8k-36s-ranks", "simonline-44k-stereo-start33"])
def test_band_energies(name):
    algo, fs, n, ch, start, _ = CASES[name]
    got = run_of(name)
    x = torch.from_numpy(clip_of(name)).to(DEV)
    f = got["mixture"].shape[2]
    edges = repet.band_edges(fs, 32)
    assert edges[0] == 0 and edges[-1] <= f and len(edges) == 33
    odd = [0, 1, 1, 7, 255, 256, 257, f] if f > 257 else [0, 1, 1, 7, f - 2, f]      # an empty band, bands across the 256-bin blocks
    with online_start(start):
        for bands in (edges, odd):
            for which in WHICH:
                _, e = repet.separate(algo, x, fs, frames=which, frame_bands=bands)
                assert e.dtype == torch.float64 and tuple(e.shape) == got[which].shape[:2] + (len(bands) - 1,)
                e = to_numpy(e)
                ref = band_energies(got[which], bands)
                with np.errstate(invalid="ignore"):
                    err = np.abs(e - ref)
                    bad = ~(err <= f * 2.0 ** -53 * ref) & ~(np.isnan(e) & np.isnan(ref))
                assert not bad.any(), (name, which, int(bad.sum()))
                _, e2 = repet.separate(algo, x, fs, frames=which, frame_bands=bands, frames_out=torch.empty_like(torch.from_numpy(e)).to(DEV))
                same_bits(to_numpy(e2), e)


FS8 = 8000
N8 = {"sim": 4 * FS8 + 5, "simonline": (312 + 20) * 256 + 77}


@functools.lru_cache(maxsize=None)
def batch_clips(algo):
    return np.stack([np.array(signal(seed, N8[algo], FS8, 2)) for seed in (31, 61, 62)])


def one_clip(algo, x, which):
    wave, frames = repet.separate(algo, torch.from_numpy(np.ascontiguousarray(x)).to(DEV), FS8, frames=which)
    return to_numpy(wave), to_numpy(frames)


@pytest.mark.parametrize("algo", ["sim", "simonline"])
def test_equal_batch_slices_are_the_one_clip_calls(algo):
    xs = batch_clips(algo)
    ctx = _native.tensor_context(0)
    for which in ("background", "foreground"):
        wave, frames = repet.separate(algo, torch.from_numpy(xs).to(DEV), FS8, frames=which)
        assert ctx.last_clip_passes == (3 if algo == "sim" else 1)
        assert tuple(frames.shape) == (3, repet.frame_count(algo, xs.shape[1], FS8), 2, 257)
        wave, frames = to_numpy(wave), to_numpy(frames)
        for b in range(3):
            w1, f1 = one_clip(algo, xs[b], which)
            same_bits(frames[b], f1)
            same_bits(wave[b], w1)
    edges = repet.band_edges(FS8, 8)
    _, e = repet.separate(algo, torch.from_numpy(xs).to(DEV), FS8, frames="background", frame_bands=edges)
    for b in range(3):
        _, e1 = repet.separate(algo, torch.from_numpy(xs[b]).to(DEV), FS8, frames="background", frame_bands=edges)
        same_bits(to_numpy(e)[b], to_numpy(e1))


@pytest.mark.parametrize("algo", ["sim", "simonline"])
def test_ragged_batch_slices_are_the_one_clip_calls_and_zero_behind(algo):
    xs = batch_clips(algo).copy()
    n = xs.shape[1]
    lengths = [n - 5 * 256 - 3, n, n - 1000]
    for b, length in enumerate(lengths):
        xs[b, length:] = np.nan                                        # the padding is never read
    ctx = _native.tensor_context(0)
    t = repet.frame_count(algo, n, FS8)
    for which in WHICH:
        wave, frames = repet.separate(algo, torch.from_numpy(xs).to(DEV), FS8, frames=which, lengths=lengths)
        assert ctx.last_clip_passes == (3 if algo == "sim" else 1)
        assert tuple(frames.shape) == (3, t, 2, 257)
        frames = to_numpy(frames)
        for b, length in enumerate(lengths):
            tb = repet.frame_count(algo, length, FS8)
            assert tb <= t and (b == 1) == (tb == t)
            _, f1 = one_clip(algo, xs[b, :length], which)
            assert f1.shape[0] == tb
            same_bits(frames[b, :tb], f1)
            assert not frames[b, tb:].any() and not np.isnan(frames[b]).any()
    edges = repet.band_edges(FS8, 8)
    _, e = repet.separate(algo, torch.from_numpy(xs).to(DEV), FS8, frames="mixture", frame_bands=edges, lengths=lengths)
    e = to_numpy(e)
    for b, length in enumerate(lengths):
        tb = repet.frame_count(algo, length, FS8)
        _, e1 = repet.separate(algo, torch.from_numpy(np.ascontiguousarray(xs[b, :length])).to(DEV), FS8, frames="mixture", frame_bands=edges)
        same_bits(e[b, :tb], to_numpy(e1))
        assert not e[b, tb:].any()


def test_a_request_serves_one_run_and_the_refusals_enqueue_nothing():
    fs = FS8
    x = torch.from_numpy(np.array(signal(31, N8["sim"], fs, 2))).to(DEV)
    p = repet.derive_params(fs)
    t, f = repet.frame_count("sim", x.shape[0], fs), p.window_length // 2 + 1
    ctx = _native.Context(0)
    try:
        ctx.upload_tensor(x)
        with pytest.raises(ValueError, match="no separation"):
            ctx.last_spectrum_form
        out = torch.full((t, 2, f), -1.0, dtype=torch.float32, device=DEV)
        # the stage list of a served run is the plain run's plus "result_frames" at its end: no stage is pushed out
        plain = [s["name"] for s in ctx.execute("sim", p, timing=True)["stages"]]
        ctx.request_frames("sim", p, "background", out)
        served = [s["name"] for s in ctx.execute("sim", p, timing=True)["stages"]]
        assert served == plain + ["result_frames"] and len(served) <= _native.MAX_STAGES
        first = to_numpy(out).copy()
        assert (first >= 0).all()
        # ... and serves that run alone: the next one writes nothing
        out.fill_(-1.0)
        assert [s["name"] for s in ctx.execute("sim", p, timing=True)["stages"]] == plain
        torch.cuda.synchronize()
        assert (to_numpy(out) == -1.0).all()
        # cleared before the run: nothing written
        ctx.request_frames("sim", p, "background", out)
        ctx.clear_requests()
        ctx.execute("sim", p)
        torch.cuda.synchronize()
        assert (to_numpy(out) == -1.0).all()
        # a run other than the one it was sized for refuses, drops the request and runs nothing
        ctx.request_frames("sim", p, "background", out)
        with pytest.raises(ValueError, match="another"):
            ctx.execute("adaptive", p)
        ctx.execute("sim", p)
        torch.cuda.synchronize()
        assert (to_numpy(out) == -1.0).all()
        # the library's own refusals (a C caller has no Python in front): extended, a window of a longer clip, edges beyond F
        lib = _native.lib()
        strides = (_native.C.c_int64 * 4)(0, 2 * f, f, 1)
        arm = lambda: _native.check(lib.repet_ctx_request_frames(ctx.handle, 0, None, 0, _native.C.c_void_p(out.data_ptr()), strides, None))
        arm()
        with pytest.raises(ValueError, match="extended"):
            ctx.execute("extended", p)
        assert [s["name"] for s in ctx.execute("sim", p, timing=True)["stages"]] == plain          # dropped with the failed execute
        arm()
        ctx.set_window(10 * x.shape[0], 0)
        with pytest.raises(ValueError, match="window of a longer clip"):
            ctx.execute("sim", p)
        ctx.set_window(0, 0)
        edges = (_native.C.c_int32 * 2)(0, f + 1)
        dst = torch.zeros((t, 2, 1), dtype=torch.float64, device=DEV)
        _native.check(lib.repet_ctx_request_frames(ctx.handle, 0, edges, 1, _native.C.c_void_p(dst.data_ptr()), None, None))
        with pytest.raises(ValueError, match="band edges"):
            ctx.execute("sim", p)
        overlap = (_native.C.c_int64 * 4)(0, f, f, 1)                      # two channels on top of each other
        _native.check(lib.repet_ctx_request_frames(ctx.handle, 0, None, 0, _native.C.c_void_p(out.data_ptr()), overlap, None))
        with pytest.raises(ValueError, match="overlap"):
            ctx.execute("sim", p)
        torch.cuda.synchronize()
        assert (to_numpy(out) == -1.0).all()
        # and the context still serves
        ctx.request_frames("sim", p, "background", out)
        ctx.execute("sim", p)
        same_bits(to_numpy(out), first)
    finally:
        ctx.close()


def test_zz_parity_report():
    """Prints the largest error met per check (and writes it to $REPET_RESULT_FRAMES_PARITY_OUT): profiles/
    result_frames_parity.txt is this output from an MI355X."""
    for name in CASES:
        if not any(k.endswith(name) for k in PARITY):
            test_frames_against_the_statement(name)
    lines = ["check                                              err / bar   err         bar"]
    for check in sorted(PARITY):
        ratio, err, bar = PARITY[check]
        lines.append(f"{check:50s} {ratio:9.3f}   {err:.3e}   {bar:.3e}")
    forms = {name: run_of(name)["form"] for name in CASES}
    lines.append("form of the masked spectrum (0 in place, 1 plane, 2 model): " + ", ".join(f"{k}={v}" for k, v in forms.items()))
    text = "\n".join(lines)
    print(text)
    path = os.environ.get("REPET_RESULT_FRAMES_PARITY_OUT")
    if path:
        with open(path, "w") as fh:
            fh.write(text + "\n")
    assert all(r <= 1.0 for r, _, _ in PARITY.values())
