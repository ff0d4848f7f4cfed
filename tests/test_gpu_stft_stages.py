"""The production STFT and fused inverse STFT kernels, stage by stage: launch_stft and launch_istft_ola (through
repet._stft_stage / repet._istft_stage) against the float64 references of tests/stft_reference.py, element by element, for
every kernel family (block, wave, reg) at the shapes, offsets, batches and edges the pipelines give them. Every case asserts
which kernel ran; a family that does not take a shape must refuse it (RuntimeError), never hand it to another family.

Bars (none of them fitted to the kernels):
  X                 2e-6 x max |want| of the spectrum compared (test_stft_matches_oracle)
  time signals      2e-6 x the larger of max |want| over the span compared and max |overlap-add of the whole clip|
                    (test_istft_roundtrip_and_oracle's 2e-6 at unit scale): the clip's scale, not the span's -- a span of one
                    sample out of the zero padding has no scale of its own, so for short spans this is looser than a bar
                    from the span alone
  V vs |own X|      2 ulp (one rounded square, one fma, a 1-ulp square root); Vm: 2 ulp per operation (C - 1 sums and the
                    division), P: 2 ulp; Vn: 1e-6 relative (an fp32 norm over F <= 4097 terms)
  f16 planes        2^-21 |v| + 2^-24 / scale (hi = f16(v), lo = f16(v - hi)); Ph_inv an exact power of two
  pad, untouched samples, Hermitian bins, NaN placement, plane form = model form: exact
The largest error met per family and check is collected in PARITY and printed (and written to $REPET_STAGE_PARITY_OUT) by
the last test of the module: profiles/stft_stage_parity.txt is that output from an MI355X."""
import os

import numpy as np
import pytest

import repet
import stft_reference as ref
from repet_synth import synth

pytestmark = pytest.mark.gpu

FAMILIES = ("block", "wave", "reg")
WINDOWS = (64, 128, 256, 512, 1024, 2048, 4096, 8192)
CHANNELS = (1, 2, 3, 4, 5, 8, 16)
ALL_WANT = ("Vm", "Vn", "P", "Vh")
PARITY = {}          # (direction, family, check) -> (error / bar, error, bar, shape)
TINY = float(np.finfo(np.float32).tiny)


# ---- what each family takes: the documented rules of reg_fft_supported, launch_stft and launch_istft_ola ------------------
def forward_takes(family, w, c):
    # the wave kernel's LDS: W + W / 2 + 2 W complex values and (4 / C, at least one) frames of C rows of FS floats, in 160 KB
    fs = -(-(w // 2 + 1) // 32) * 32
    wave_lds = (w + w // 2 + 2 * w) * 8 + (1 if c >= 4 else 4 // c) * c * fs * 4
    return {"block": True, "wave": w <= 4096 and c <= 8 and wave_lds <= 160 * 1024, "reg": w == 2048}[family]


def inverse_takes(family, w, c, form="none"):
    if form == "model":
        return family == "reg" and w == 2048 and c in (1, 2)
    if family == "block":
        return not (form == "plane" and w > 4096)
    return w <= 4096 and c in (1, 2, 4) if family == "wave" else (w == 2048 and c in (1, 2))


def forward_kernel(family, w, c):
    if family == "reg":
        return "stft_reg_kernel<%d>" % (c if c <= 2 else 0)
    if family == "wave":
        return "stft_wave_kernel"
    return "stft_pair_kernel" if c % 2 == 0 and w <= 2048 else "stft_kernel"


def inverse_kernel(family, w, c, form):
    if family == "reg":
        return "istft_ola_reg_kernel<%d, %d>" % (c, {"none": 0, "plane": 1, "model": 2}[form])
    if family == "wave":
        return "istft_ola_wave_kernel"
    return "istft_ola_kernel<masked>" if form == "plane" else "istft_ola_kernel<plain>"


def production_family(w, c, inverse):
    """What launch_stft(a, s) / launch_istft_ola(a, s) pick, by REPET_FFT_PATH as reg_fft_supported and use_wave_kernels read
    it: unset, the register kernels for mono and stereo at W = 2048; r(eg): both register kernels for whatever they take;
    f(wd): the forward one only; w(ave): the wave kernels where they fit; anything else: the block kernels."""
    env = os.environ.get("REPET_FFT_PATH", "")[:1]
    if env == "":
        reg = w == 2048 and c in (1, 2)
    elif env == "r":
        reg = forward_takes("reg", w, c) if not inverse else inverse_takes("reg", w, c)
    else:
        reg = env == "f" and not inverse and forward_takes("reg", w, c)
    if reg:
        return "reg"
    if env == "w" and (inverse_takes("wave", w, c) if inverse else forward_takes("wave", w, c)):
        return "wave"
    return "block"


def note(direction, family, check, err, bar, shape):
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else np.inf)
    key = (direction, family, check)
    if key not in PARITY or ratio > PARITY[key][0]:
        PARITY[key] = (ratio, err, bar, shape)


def window_of(w):
    return np.hamming(w + 1)[:w].astype(np.float32)        # periodic Hamming, as the pipelines' tables hold it


def noise(n, c, seed, scale=0.5):
    return (np.random.default_rng(seed).standard_normal((n, c)) * scale).astype(np.float32)


def ulps(got, want64):
    """|got - want| in units of the spacing of fp32 at |want| (want in float64)."""
    sp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want64) / sp


# ---- forward ---------------------------------------------------------------------------------------------------------------
def check_forward(family, w, audio, centred=True, sample_offset=0, n_samples=None, n_batch=1, stride=0, want=ALL_WANT, prefill=0,
                  tag=""):
    h = w // 2
    audio = np.asarray(audio, dtype=np.float32)
    c = audio.shape[1]
    window = window_of(w)
    n = audio.shape[0] - sample_offset if n_samples is None else n_samples
    shape = "W=%d C=%d n=%d B=%d off=%d centred=%d %s" % (w, c, n, n_batch, sample_offset, centred, tag)
    kw = dict(centred=centred, sample_offset=sample_offset, n_samples=n, n_batch=n_batch, batch_sample_stride=stride)
    if not forward_takes(family, w, c) and ref.frame_count(n, w, h, centred) > 0:        # (no frame: nothing is asked of any family)
        with pytest.raises(RuntimeError, match="does not take this shape"):
            repet._stft_stage(audio, window, h, path=family, want=want, **kw)
        return None
    if family == "reg" and w == 2048 and "Ph" not in want:
        want = tuple(want) + ("Ph",)
    r = repet._stft_stage(audio, window, h, path=family, want=want, prefill=prefill, **kw)
    t, f, fs, tpad = r["T"], r["F"], r["FS"], r["Tpad"]
    assert t == ref.frame_count(n, w, h, centred) and f == w // 2 + 1 and fs % 32 == 0 and fs >= f and tpad % 128 == 0
    launch = r["launch"]
    print("forward", family, shape, launch)
    fill32 = np.frombuffer(bytes([prefill]) * 4, dtype=np.uint32)[0]
    untouched = lambda a: np.all(np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize != 2 else np.uint16) ==
                                 (fill32 if a.dtype.itemsize != 2 else (fill32 & 0xFFFF)))
    if t == 0:
        assert launch["family"] is None and launch["launches"] == 0 and untouched(r["X"]) and untouched(r["V"])
        return r
    assert launch["family"] == family and launch["kernel"] == forward_kernel(family, w, c) and launch["launches"] == 1, launch
    if family == "block":
        assert launch["workgroups"] == -(-t // launch["run"]) * n_batch and launch["run"] >= 4 and launch["slots"] >= 1, launch
    want64 = ref.forward(audio, window, h, centred, sample_offset, n, n_batch, stride)
    X, V = r["X"], r["V"]
    # the pad: bins [F, FS) of the frame rows are written as zero, the rows behind the frames are not written at all
    assert np.all(X[:, :, :t, f:] == 0) and np.all(V[:, :, :t, f:] == 0), shape
    assert untouched(X[:, :, t:]) and untouched(V[:, :, t:]), shape
    for key in want:
        assert untouched(r[key][:, t:]), (shape, key)
    if "Ph" in want:
        assert untouched(r["Ph_inv"][:, t:]), shape
    Xg = X[:, :, :t, :f].astype(np.complex128)
    finite = np.isfinite(want64["X"])
    assert np.array_equal(np.isfinite(Xg), finite), shape
    for b in range(n_batch):
        for ch in range(c):
            top = float(np.max(np.abs(want64["X"][b, ch])))
            err = float(np.max(np.abs(Xg[b, ch] - want64["X"][b, ch])))
            note("forward", family, "X", err, 2e-6 * top, shape)
            assert err <= 2e-6 * top, (shape, b, ch, err, top, np.unravel_index(np.argmax(np.abs(Xg[b, ch] - want64["X"][b, ch])), Xg[b, ch].shape))
    # a real signal: DC and Nyquist have no imaginary part
    assert np.all(X[:, :, :t, 0].imag == 0) and np.all(X[:, :, :t, f - 1].imag == 0), shape
    Vg = V[:, :, :t, :f]
    u = ulps(Vg, np.abs(Xg))
    note("forward", family, "V ulp", float(u.max()), 2.0, shape)
    assert u.max() <= 2.0, (shape, float(u.max()), np.unravel_index(np.argmax(u), u.shape))
    silent = ~np.any(want64["Vm"] > 0, axis=2)                   # (B, T): frames without any sample
    assert np.all(Vg.transpose(0, 2, 1, 3)[silent] == 0), shape
    Vg64 = Vg.astype(np.float64)
    if "Vm" in want:
        Vm = r["Vm"][:, :t]
        assert np.all(Vm[:, :, f:] == 0), shape
        u = ulps(Vm[:, :, :f], Vg64.mean(axis=1))
        note("forward", family, "Vm ulp", float(u.max()), 2.0 * c, shape)
        assert u.max() <= 2.0 * c, (shape, float(u.max()))
        Vm64 = Vm[:, :, :f].astype(np.float64)
    else:
        Vm64 = Vg64.mean(axis=1)
    if "P" in want and "Vm" in want:
        P = r["P"][:, :t]
        assert np.all(P[:, :, f:] == 0), shape
        u = ulps(P[:, :, :f], Vm64 * Vm64)
        note("forward", family, "P ulp", float(u.max()), 2.0, shape)
        assert u.max() <= 2.0, (shape, float(u.max()))
    if "Vn" in want and "Vm" in want:
        Vn = r["Vn"][:, :t]
        assert np.all(Vn[:, :, f:][~silent] == 0), shape
        with np.errstate(invalid="ignore", divide="ignore"):
            unit = Vm64 / np.sqrt(np.sum(Vm64 * Vm64, axis=2, keepdims=True))
        # a silent frame: 0 / 0, a NaN row (the similarity of such a frame is NaN downstream, as repet.py:1220 makes it)
        assert np.all(np.isnan(Vn[:, :, :f][silent])) and not np.any(np.isnan(Vn[:, :, :f][~silent])), shape
        live = ~silent
        if live.any():
            rel = np.abs(Vn[:, :, :f][live] - unit[live]) / (1e-6 * np.abs(unit[live]) + TINY)
            note("forward", family, "Vn rel", float(rel.max()) * 1e-6, 1e-6, shape)
            assert rel.max() <= 1.0, (shape, float(rel.max()))
        if "Vh" in want:
            back = ref.decode_planes(r["Vh"][:, :t], 1.0 / 128)
            v = Vn.astype(np.float64)
            assert np.array_equal(np.isnan(back[:, :, :f]), np.isnan(v[:, :, :f])), shape
            ok = ~np.isnan(v)
            err = np.abs(back - v)[ok] / (2.0 ** -21 * np.abs(v[ok]) + 2.0 ** -24 / 128)
            note("forward", family, "Vh decode", float(err.max()), 1.0, shape)
            assert err.max() <= 1.0, (shape, float(err.max()))
    if "Ph" in want and "Vm" in want:
        p32 = r["Vm"][:, :t] * r["Vm"][:, :t]                         # the fp32 squares the planes are made of
        scale = np.array([[ref.row_scale(float(row.max())) for row in clip] for clip in p32])
        assert np.array_equal(r["Ph_inv"][:, :t].astype(np.float64), 1.0 / scale), shape
        back = ref.decode_planes(r["Ph"][:, :t], r["Ph_inv"][:, :t])
        err = np.abs(back - p32) / (2.0 ** -21 * np.abs(p32) + 2.0 ** -24 / scale[..., None])
        note("forward", family, "Ph decode", float(err.max()), 1.0, shape)
        assert err.max() <= 1.0, (shape, float(err.max()))
    return r


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("family", FAMILIES)
def test_forward_every_window_and_channel_count(family, w):
    h = w // 2
    for c in CHANNELS:
        check_forward(family, w, noise(5 * h + 3, c, 100 + c), tag="noise")


def test_production_pick_reports_its_kernel():
    for w, c in ((2048, 1), (2048, 2), (2048, 3), (2048, 4), (256, 2), (256, 3), (4096, 2), (8192, 1)):
        fam = production_family(w, c, False)
        window = window_of(w)
        r = repet._stft_stage(noise(3 * w, c, 5), window, w // 2)
        assert r["launch"]["family"] == fam and r["launch"]["kernel"] == forward_kernel(fam, w, c), r["launch"]
        spectra = r["X"][:, :, :r["T"], :r["F"]]
        _, launch = repet._istft_stage(spectra, w, np.zeros((3 * w, c), np.float32), w // 2, 3 * w)
        fam = production_family(w, c, True)
        assert launch["family"] == fam and launch["kernel"] == inverse_kernel(fam, w, c, "none"), launch


@pytest.mark.parametrize("centred", [True, False])
@pytest.mark.parametrize("w,c", [(64, 1), (64, 2), (256, 3), (2048, 1), (2048, 2), (2048, 3)])
@pytest.mark.parametrize("family", FAMILIES)
def test_forward_clip_lengths(family, w, c, centred):
    h = w // 2
    for n in (1, h - 1, h, h + 1, w - 1, w, w + 1, 997, 4099, 10007):
        check_forward(family, w, synth(1.0, 16000, c, 3)[:n] if n > 4000 else noise(n, c, n), centred=centred)


@pytest.mark.parametrize("w,c", [(256, 1), (256, 2), (256, 3), (2048, 1), (2048, 2), (2048, 5)])
@pytest.mark.parametrize("family", FAMILIES)
def test_forward_offsets_and_batches_do_not_leak(family, w, c):
    """Clips inside a longer buffer whose samples before, between and behind them are fifty times as loud."""
    n = 5 * w + 11
    for n_batch in (1, 2, 7):
        for gap in (0, 53):
            stride = n + gap
            off = 37
            audio = noise(off + stride * n_batch + 29, c, 7 * n_batch + gap, scale=25.0)
            for b in range(n_batch):
                audio[off + b * stride:off + b * stride + n] = noise(n, c, 1000 + b)
            for centred in (True, False):
                check_forward(family, w, audio, centred, off, n, n_batch, stride if n_batch > 1 else 0, tag="gap=%d" % gap)


@pytest.mark.parametrize("family", FAMILIES)
def test_forward_launch_geometry_boundaries(family):
    """Frame counts each side of the places where the launch geometry changes, read back from the launch itself."""
    if family == "reg":
        w = 2048
        probe = repet._stft_stage(noise(w, 2, 1), window_of(w), w // 2, centred=False, path="reg")["launch"]
        assert probe["units"] == 1 and probe["run"] == 12
        cus = probe["slots"]
        for units in (1, 11, 12, 13, 12 * cus, 12 * cus + 1):
            r = check_forward("reg", w, noise(w + (units - 1) * (w // 2), 2, units), centred=False, tag="units=%d" % units)
            assert r["launch"]["units"] == units and r["launch"]["workgroups"] == min(-(-units // 12), cus)
        for n_batch, t in ((2, 6), (7, 2), (7, 13)):          # the units of a batch cross the clips inside one workgroup
            n = w + (t - 1) * (w // 2)
            r = check_forward("reg", w, noise(n * n_batch, 1, t), False, 0, n, n_batch, n, tag="units=%d" % (t * n_batch))
            assert r["launch"]["units"] == t * n_batch
        return
    for w, c in ((64, 1), (64, 2), (256, 2)):
        h = w // 2
        first = check_forward(family, w, noise(w + 2 * h, c, 1), centred=False)["launch"]
        run, slots = first["run"], first["slots"]

        def at(t):
            r = check_forward(family, w, noise(w + (t - 1) * h, c, t), centred=False, want=("Vm", "Vn"), tag="T=%d" % t)
            assert r["T"] == t and r["launch"]["workgroups"] == -(-t // r["launch"]["run"])
            return r["launch"]["run"]

        for t in (run - 1, run, run + 1, 2 * run, 2 * run + 1):
            at(t)
        if family != "block":
            continue
        # T = run x slots fills the resident slots exactly with the run the launch ITSELF reports; one frame more and
        # frames_per_workgroup takes a second round or a longer run. Each side of that edge, then of the edge of whatever run
        # the launch past it reports, and so on up to the longest run it may pick (8 x the least).
        pending, done, runs = [run * slots], [], set()
        while pending and len(done) < 5:
            edge = pending.pop(0)
            if edge in done or edge > 8 * run * slots:
                continue
            done.append(edge)
            for t in (edge - 1, edge, edge + 1):
                chosen = at(t)
                runs.add(chosen)
                assert run <= chosen <= 8 * run
                pending.append(chosen * slots)
        print("block forward W=%d C=%d: slots %d, edges %s, runs met %s" % (w, c, slots, done, sorted(runs)))


@pytest.mark.parametrize("w,c", [(256, 2), (2048, 2), (2048, 3), (8192, 1)])
@pytest.mark.parametrize("family", FAMILIES)
def test_forward_special_signals(family, w, c):
    h = w // 2
    n = 9 * h + 5
    seam = np.zeros((n, c), np.float32)
    seam[3 * h] = 1.0                                      # an impulse on a frame seam, and one just before the next
    seam[4 * h - 1, 0] = -0.5
    check_forward(family, w, seam, tag="impulse")
    check_forward(family, w, np.full((n, c), 0.25, np.float32), tag="constant")
    gap = noise(n + 4 * w, c, 9)
    gap[2 * h + 3:2 * h + 3 + 3 * w] = 0                   # digital silence: whole frames of zeros
    r = check_forward(family, w, gap, tag="silent stretch")
    if r is not None:
        assert np.isnan(r["Vn"][0, :r["T"], 0]).any()
    check_forward(family, w, synth(0.5, 44100, c, 2), prefill=255, tag="synth")     # every cell of the frame rows is written


@pytest.mark.parametrize("w,c", [(256, 2), (2048, 1), (2048, 2), (2048, 3)])
@pytest.mark.parametrize("family", FAMILIES)
def test_forward_nan_and_infinite_samples_stay_in_their_frames(family, w, c):
    h = w // 2
    n = 12 * h
    if not forward_takes(family, w, c):
        with pytest.raises(RuntimeError, match="does not take this shape"):
            repet._stft_stage(noise(n, c, 4), window_of(w), h, path=family)
        return
    for bad, fix in ((np.nan, False), (np.inf, True), (-np.inf, True)):
        audio = noise(n, c, 4)
        at = 5 * h + 17
        audio[at, c - 1] = bad
        r = repet._stft_stage(audio, window_of(w), h, path=family, want=("Vm", "Vn"), fix_infinite=fix)
        t, f = r["T"], r["F"]
        frames = np.arange(t)
        holds = (frames * h - h <= at) & (at < frames * h - h + w)            # centred: frame k covers [k h - W / 2, k h + W / 2)
        assert holds.sum() == 2
        X, V = r["X"][0, :, :t, :f], r["V"][0, :, :t, :f]
        for ch in range(c):
            expect = holds if ch == c - 1 else np.zeros(t, bool)
            nan_bin = np.isnan(X[ch].real) | np.isnan(X[ch].imag)         # (DC and Nyquist may keep an exact zero imaginary part)
            assert np.array_equal(np.all(nan_bin, axis=1), expect) and np.array_equal(np.any(nan_bin, axis=1), expect), (bad, ch)
            assert np.array_equal(np.all(np.isnan(V[ch]), axis=1), expect) and np.array_equal(np.any(np.isnan(V[ch]), axis=1), expect)
        assert np.array_equal(np.any(np.isnan(r["Vm"][0, :t, :f]), axis=1), holds)


# ---- inverse ---------------------------------------------------------------------------------------------------------------
def spectra_of(w, c, t, seed, n_spec=1):
    """Half spectra of real noise, (n_spec, C, T, F) complex64: what a forward transform hands the inverse."""
    h = w // 2
    out = []
    for s in range(n_spec):
        x = noise((t - 1) * h, c, seed + 31 * s)
        out.append([ref.stft_half(x[:, ch], window_of(w), h)[:t] for ch in range(c)])
    y = np.array(out).astype(np.complex64)
    assert y.shape == (n_spec, c, t, w // 2 + 1)
    return y


def random_mask(shape, seed):
    rng = np.random.default_rng(seed)
    m = rng.random(shape).astype(np.float32)
    m[rng.random(shape) < 0.15] = 0
    m[rng.random(shape) < 0.15] = 1
    return m


def check_inverse(family, w, Y, trim, n_out, out_offset=0, out_len=None, mask=None, model=None, periods=None, cutoff=0, mode=0,
                  fade_in=0, tag="", mask64=None):
    """One clip (n_batch = 0) through the fused inverse against the float64 overlap-add; returns (out, launch) or None."""
    n_spec, c, t, f = Y.shape
    n = w // 2
    form = "model" if model is not None else "plane" if mask is not None else "none"
    shape = "W=%d C=%d T=%d trim=%d n_out=%d off=%d %s mode=%d %s" % (w, c, t, trim, n_out, out_offset, form, mode, tag)
    scale = 1.0 / float(np.sum(window_of(w)[::n].astype(np.float64)))
    out_len = out_offset + n_out + 9 if out_len is None else out_len
    before = noise(out_len, c, 77, scale=0.1)
    kw = dict(out_offset=out_offset, scale=scale, mask=mask, model=model, periods=periods, cutoff=cutoff, accumulate_weighted=mode,
              fade_in=fade_in, path=family)
    if not inverse_takes(family, w, c, form):
        with pytest.raises(RuntimeError, match="does not take this shape"):
            repet._istft_stage(Y, w, before, trim, n_out, **kw)
        return None
    got, launch = repet._istft_stage(Y, w, before, trim, n_out, **kw)
    print("inverse", family, shape, launch)
    written = max(min(n_out, (t + 1) * n - trim), 0)
    if written == 0:
        assert launch["launches"] == 0 and np.array_equal(got.view(np.uint32), before.view(np.uint32))
        return got, launch
    assert launch["family"] == family and launch["kernel"] == inverse_kernel(family, w, c, form), (shape, launch)
    if family == "block":
        per = (96 * 1024 - (n * 4 if mode else 0)) // (n * 8)
        assert launch["launches"] == (-(-c // per) if c * n * 8 + (n * 4 if mode else 0) > 96 * 1024 else 1), (shape, launch)
    else:
        assert launch["launches"] == 1
    m64 = mask64 if mask64 is not None else (None if mask is None else mask[0].astype(np.float64))
    piece = ref.inverse_piece(Y[0].astype(np.complex128), w, trim, n_out, np.float32(scale).astype(np.float64), mask=m64)
    assert len(piece) == written
    wts = ref.single_fade_weights(n_out, fade_in) if mode else None
    want = ref.inverse(before, [(out_offset, piece, wts)], mode=mode)
    span = slice(out_offset, out_offset + written)
    # nothing outside the span is touched, bit for bit
    assert np.array_equal(got[:out_offset].view(np.uint32), before[:out_offset].view(np.uint32)), shape
    assert np.array_equal(got[span.stop:].view(np.uint32), before[span.stop:].view(np.uint32)), shape
    # the scale of the bar is the clip's, not the span's: a span of one sample out of the zero padding is no "unit scale"
    whole = ref.inverse_piece(Y[0].astype(np.complex128), w, 0, (t + 1) * n, np.float32(scale).astype(np.float64), mask=m64)
    top = max(float(np.max(np.abs(whole))), float(np.max(np.abs(want[span]))))
    diff = np.abs(got[span].astype(np.float64) - want[span])
    err = float(diff.max())
    note("inverse", family, form + (" weighted" if mode else ""), err, 2e-6 * top, shape)
    assert err <= 2e-6 * top, (shape, err, top, np.unravel_index(np.argmax(diff), diff.shape))
    return got, launch


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("family", FAMILIES)
def test_inverse_every_window_and_channel_count(family, w):
    """C = 16 at W = 2048 and C = 26 at W = 1024 (and most counts at the two longest windows) go through the channel groups of
    launch_istft_ola: every channel carries its own signal, so one landing in another's place of the interleaved output fails."""
    h = w // 2
    t = 6
    for c in CHANNELS + ((26,) if w == 1024 else ()):
        Y = spectra_of(w, c, t, 10 * c)
        check_inverse(family, w, Y, w - h, (t - 1) * h - 3, out_offset=5)
        check_inverse(family, w, Y, w - h, (t - 1) * h - 3, out_offset=5, mask=random_mask(Y.shape, c))


@pytest.mark.parametrize("w,c", [(128, 1), (2048, 1), (2048, 2), (2048, 3), (4096, 4)])
@pytest.mark.parametrize("family", FAMILIES)
def test_inverse_trim_and_span(family, w, c):
    n = w // 2
    t = 9
    Y = spectra_of(w, c, t, 3)
    M = random_mask(Y.shape, 8)
    whole = (t + 1) * n
    for trim in (0, n, 3 * n, 5, n + 1, 2 * n - 1):            # W - H, k H as the online handle trims, and off the hop grid
        for n_out in (1, n - 1, n, n + 1, whole - trim, whole - trim - 1, whole - trim + 4):
            check_inverse(family, w, Y, trim, n_out, out_offset=3, out_len=3 + n_out + 2)
        check_inverse(family, w, Y, trim, (t - 1) * n, out_offset=0, mask=M)


@pytest.mark.parametrize("family", FAMILIES)
def test_inverse_hop_counts_each_side_of_the_workgroup_runs(family):
    """The register kernel emits 12 R - 1 hops per workgroup and picks R by a cost loop; the block kernels fit a run to the
    resident slots. Hop counts each side of those edges, with the run read back."""
    w, n = 2048, 1024
    probe = repet._istft_stage(spectra_of(w, 1, 2, 1), w, np.zeros((n, 1), np.float32), 0, n, path="reg")[1]
    cus = probe["slots"]
    seen = set()
    for hops in (1, 10, 11, 12, 22, 23, 24, 11 * cus - 1, 11 * cus, 11 * cus + 1):
        t = max(hops, 2) if hops < 100 else hops
        Y = spectra_of(w, 1, t, hops) if hops < 100 else np.tile(spectra_of(w, 1, 64, hops), (1, 1, -(-t // 64), 1))[:, :, :t]
        res = check_inverse(family, w, Y, 0, hops * n, out_offset=1, tag="hops=%d" % hops)
        launch = res[1]
        assert launch["units"] == hops and launch["workgroups"] == -(-hops // launch["run"]), launch
        seen.add(launch["run"])
        if family == "reg":
            assert launch["run"] == 12 * launch["rounds"] - 1
    if family == "reg":
        assert 11 in seen and len(seen) > 1, seen            # the cost loop did flip to a longer run somewhere in the list


@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("family", FAMILIES)
def test_inverse_model_form(family, c):
    """The repeating-segment model applied by the inverse itself (register kernel only): soft_mask(|Y|, model[t mod period]) with
    bins 1 .. cutoff forced to 1; periods 1, 2 and longer than the clip."""
    w, t = 2048, 30
    Y = spectra_of(w, c, t, 21)
    mag = np.abs(Y[0].astype(np.complex128))
    rng = np.random.default_rng(4)
    for period, cutoff in ((1, 0), (2, 5), (7, 5), (t + 3, 2)):
        rows = period
        model = (np.median(mag, axis=1, keepdims=True) * rng.random((1, c, rows, w // 2 + 1)) * 2).astype(np.float32)
        m64 = np.stack([ref.model_mask(mag[ch], model[0, ch], period, cutoff) for ch in range(c)])
        check_inverse(family, w, Y, w // 2, (t - 1) * 1024, out_offset=2, model=model, periods=[period], cutoff=cutoff, mask64=m64,
                      tag="period=%d" % period)


def test_inverse_model_form_with_a_period_per_clip_of_a_batch():
    w, t, c, n = 2048, 14, 2, 1024
    n_spec = 3
    Y = spectra_of(w, c, t, 5, n_spec)
    periods = [3, 1, 20]
    rows = 20
    rng = np.random.default_rng(6)
    model = (rng.random((n_spec, c, rows, n + 1)) * 40).astype(np.float32)
    n_out = (t - 1) * n
    before = noise(n_spec * n_out + 10, c, 2)
    batch = dict(n_batch=n_spec, batch_first=0, batch_step=1, batch_total=n_spec, batch_local0=0, batch_out_stride=n_out, overlap=0)
    scale = 0.5
    got, launch = repet._istft_stage(Y, w, before, n, n_out, out_offset=4, scale=scale, model=model, periods=periods, cutoff=3,
                                     batch=batch, path="reg")
    assert launch["kernel"] == "istft_ola_reg_kernel<2, 2>"
    pieces = []
    for s in range(n_spec):
        mag = np.abs(Y[s].astype(np.complex128))
        m64 = np.stack([ref.model_mask(mag[ch], model[s, ch], periods[s], 3) for ch in range(c)])
        pieces.append((4 + s * n_out, ref.inverse_piece(Y[s].astype(np.complex128), w, n, n_out, scale, mask=m64), None))
    want = ref.inverse(before, pieces)
    assert np.array_equal(got[:4], before[:4]) and np.array_equal(got[4 + n_spec * n_out:], before[4 + n_spec * n_out:])
    err, top = float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))
    note("inverse", "reg", "model batch", err, 2e-6 * top, "W=2048 C=2 T=14 periods=3,1,20")
    assert err <= 2e-6 * top, (err, top)
    with pytest.raises(RuntimeError, match="does not take this shape"):
        repet._istft_stage(Y, w, before, n, n_out, out_offset=4, model=model, periods=periods, batch=batch, path="block")


@pytest.mark.parametrize("c", [1, 2])
def test_plane_form_and_model_form_give_the_same_bits(c):
    """On a mask both forms can hold exactly: every |Y| a power of two (real bins), every model value a dyadic fraction of it, so
    soft_mask's quotient is exact and the plane holds the very mask the kernel derives from the model."""
    w, t, n = 2048, 25, 1024
    f = n + 1
    rng = np.random.default_rng(12)
    level = np.ldexp(1.0, rng.integers(-3, 6, size=(c, 1, f)))
    Y = (level * rng.choice([-1.0, 1.0], size=(c, t, f))).astype(np.complex64)[None]
    for period in (1, 4, t + 2):
        frac = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0, 2.0], size=(c, period, f))
        model = (frac * level).astype(np.float32)[None]
        mask = np.minimum(frac, 1.0)[:, np.arange(t) % period].astype(np.float32)[None]
        mask[0][:, :, 1:4] = 1
        mask[mask == 0] = np.float32(ref.EPS) / np.broadcast_to(level, (c, t, f))[mask[0] == 0].astype(np.float32)   # (0 + eps) / v
        before = np.zeros(((t - 1) * n, c), np.float32)
        a, la = repet._istft_stage(Y, w, before, n, (t - 1) * n, scale=0.37, mask=mask, path="reg")
        b, lb = repet._istft_stage(Y, w, before, n, (t - 1) * n, scale=0.37, model=model, periods=[period], cutoff=3, path="reg")
        assert la["kernel"] == "istft_ola_reg_kernel<%d, 1>" % c and lb["kernel"] == "istft_ola_reg_kernel<%d, 2>" % c
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (period, int(np.sum(a != b)))
        blk, _ = repet._istft_stage(Y, w, before, n, (t - 1) * n, scale=0.37, mask=mask, path="block")
        want = ref.inverse_piece(Y[0].astype(np.complex128), w, n, (t - 1) * n, np.float64(np.float32(0.37)), mask=mask[0].astype(np.float64))
        for got in (a, blk):
            assert np.max(np.abs(got - want)) <= 2e-6 * np.max(np.abs(want))


@pytest.mark.parametrize("c", [1, 2])
def test_plane_form_and_model_form_round_the_same_products_on_general_data(c):
    """The promise of mul_rounded (common.h): on a general complex spectrum the inverse that derives the mask from the model
    multiplies in the very products the mask kernel's plane gives. The plane is the period-mask kernel's own output
    (repet._mask on the forward kernel's V, the same soft_mask on the same magnitudes); the model is the median over an ODD
    number of whole repetitions, so it is one of the fp32 values themselves and NumPy's median is the kernel's, bit for bit."""
    w, n, period, reps = 2048, 1024, 5, 5
    t, f = period * reps, n + 1
    x = noise((t - 1) * n, c, 41)
    x[3 * n:4 * n] *= 0.05                                            # a quiet stretch: masks well below 1 around it
    r = repet._stft_stage(x, window_of(w), n, path="reg")
    assert r["T"] == t
    Y = r["X"][:, :, :t, :f]
    V = r["V"][0, :, :t, :f]
    model = np.median(V.reshape(c, reps, period, f), axis=1)
    assert model.dtype == np.float32 and np.all(np.any(model[:, None] == V.reshape(c, reps, period, f), axis=1))
    mask = np.stack([repet._mask(V[ch].T, period).T for ch in range(c)]).astype(np.float32)
    v64, m64 = V.astype(np.float64), np.tile(model.astype(np.float64), (1, reps, 1))
    want_mask = (np.minimum(v64, m64) + ref.EPS) / (v64 + ref.EPS)
    assert np.max(np.abs(mask - want_mask)) <= 4 * 2.0 ** -24 and 0.05 < np.mean(mask < 0.9) < 0.95      # the plane IS this model's mask
    before = np.zeros(((t - 1) * n, c), np.float32)
    a, la = repet._istft_stage(Y, w, before, n, (t - 1) * n, scale=0.37, mask=mask[None], path="reg")
    b, lb = repet._istft_stage(Y, w, before, n, (t - 1) * n, scale=0.37, model=model[None], periods=[period], cutoff=0, path="reg")
    assert la["kernel"] == "istft_ola_reg_kernel<%d, 1>" % c and lb["kernel"] == "istft_ola_reg_kernel<%d, 2>" % c
    differ = a.view(np.uint32) != b.view(np.uint32)
    assert not differ.any(), (int(differ.sum()), float(np.max(np.abs(a - b))))
    want = ref.inverse_piece(Y[0].astype(np.complex128), w, n, (t - 1) * n, np.float64(np.float32(0.37)), mask=want_mask)
    assert np.max(np.abs(b - want)) <= 2e-6 * np.max(np.abs(want))


@pytest.mark.parametrize("w,c", [(256, 1), (256, 3), (2048, 2), (4096, 2)])
@pytest.mark.parametrize("family", FAMILIES)
def test_inverse_weighted_segments(family, w, c):
    """The cross-fade of `extended`: one faded-in segment added to what is there, and a batch of nine segments whose step is
    shorter than their overlap (several later segments fade one sample), launched class by class as run_original does."""
    n = w // 2
    t = 7
    Y = spectra_of(w, c, t, 17)
    n_out = (t - 1) * n - 5
    if check_inverse(family, w, Y, n, n_out, out_offset=6, mode=1, fade_in=2 * n + 3, tag="single") is None:
        return
    check_inverse(family, w, Y, n, n_out, out_offset=6, mode=2, fade_in=n - 1, mask=random_mask(Y.shape, 3), tag="single")
    total, step = 9, n + 7
    overlap = n_out - step
    assert step < overlap
    Yb = spectra_of(w, c, t, 40, total)
    scale = 1.0 / float(np.sum(window_of(w)[::n].astype(np.float64)))
    out_len = 11 + (total - 1) * step + n_out + 13
    before = noise(out_len, c, 9, scale=0.1)
    classes = -(-n_out // step)
    got = before
    for k in range(min(classes, total)):
        batch = dict(n_batch=(total - k + classes - 1) // classes, batch_first=k, batch_step=classes, batch_total=total, batch_local0=k,
                     batch_out_stride=step, overlap=overlap)
        got, launch = repet._istft_stage(Yb, w, got, n, n_out, out_offset=11, scale=scale, accumulate_weighted=1, batch=batch, path=family)
        assert launch["family"] == family and launch["kernel"] == inverse_kernel(family, w, c, "none"), launch
    pieces = [(11 + j * step, ref.inverse_piece(Yb[j].astype(np.complex128), w, n, n_out, np.float64(np.float32(scale))),
               ref.fade_weights(n_out, j, total, step, overlap)) for j in range(total)]
    want = ref.inverse(before, pieces, mode=1)
    lo, hi = 11, 11 + (total - 1) * step + n_out
    assert np.array_equal(got[:lo].view(np.uint32), before[:lo].view(np.uint32))
    assert np.array_equal(got[hi:].view(np.uint32), before[hi:].view(np.uint32))
    err, top = float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))
    note("inverse", family, "weighted batch", err, 2e-6 * top, "W=%d C=%d T=%d segments=%d step=%d overlap=%d" % (w, c, t, total, step, overlap))
    assert err <= 2e-6 * top, (err, top, np.unravel_index(np.argmax(np.abs(got - want)), got.shape))


@pytest.mark.parametrize("w,c", [(256, 2), (2048, 1), (2048, 2), (2048, 3)])
@pytest.mark.parametrize("family", FAMILIES)
def test_inverse_spreads_a_nan_frame_over_its_own_samples_only(family, w, c):
    n = w // 2
    t, bad = 12, 5
    Y = spectra_of(w, c, t, 2)
    if not inverse_takes(family, w, c):
        with pytest.raises(RuntimeError, match="does not take this shape"):
            repet._istft_stage(Y, w, np.zeros(((t + 1) * n, c), np.float32), 0, (t + 1) * n, path=family)
        return
    Y[0, c - 1, bad, :] = np.nan
    got, _ = repet._istft_stage(Y, w, np.zeros(((t + 1) * n, c), np.float32), 0, (t + 1) * n, path=family)
    expect = np.zeros(((t + 1) * n, c), bool)
    expect[bad * n:bad * n + w, c - 1] = True
    assert np.array_equal(np.isnan(got), expect), (int(np.isnan(got).sum()), int(expect.sum()))


@pytest.mark.parametrize("w,c", [(64, 1), (256, 3), (1024, 2), (2048, 1), (2048, 2), (2048, 4), (4096, 2), (8192, 1)])
@pytest.mark.parametrize("family", FAMILIES)
def test_round_trip_reproduces_the_input(family, w, c):
    h = w // 2
    if not forward_takes(family, w, c) or not inverse_takes(family, w, c):
        with pytest.raises(RuntimeError, match="does not take this shape"):
            r = repet._stft_stage(noise(3 * w, c, 1), window_of(w), h, path=family)
            repet._istft_stage(r["X"][:, :, :r["T"], :r["F"]], w, np.zeros((w, c), np.float32), h, w, path=family)
        return
    for n in (7 * h + 13, 997):
        x = synth(1.0, 16000, c, 6)[:n].astype(np.float32) if n <= 16000 else noise(n, c, 1)
        window = window_of(w)
        r = repet._stft_stage(x, window, h, path=family)
        spectra = r["X"][:, :, :r["T"], :r["F"]]
        scale = 1.0 / float(np.sum(window[::h].astype(np.float64)))
        got, _ = repet._istft_stage(spectra, w, np.full((n + 2, c), 9.0, np.float32), w - h, n, out_offset=1, scale=scale, path=family)
        assert np.all(got[0] == 9.0) and np.all(got[-1] == 9.0)
        err, top = float(np.max(np.abs(got[1:-1] - x))), float(np.max(np.abs(x)))
        note("round trip", family, "x", err, 2e-6 * top, "W=%d C=%d n=%d" % (w, c, n))
        assert err <= 2e-6 * top, (w, c, n, err, top)


def test_refusals_over_the_grid_are_the_documented_ones():
    """Every (family, window, channel count) pair of the grid, forward, inverse with a mask plane and inverse with a model: a
    pair is refused exactly when the rules of reg_fft_supported / launch_stft / launch_istft_ola say the family does not take it."""
    expected = refused = 0
    for family in FAMILIES:
        for w in WINDOWS:
            h = w // 2
            window = window_of(w)
            for c in CHANNELS:
                x = noise(2 * w, c, 1)
                Y = spectra_of(w, c, 3, 2)
                calls = [
                    (forward_takes(family, w, c), lambda: repet._stft_stage(x, window, h, path=family)),
                    (inverse_takes(family, w, c, "none"), lambda: repet._istft_stage(Y, w, np.zeros((w, c), np.float32), h, w, path=family)),
                    (inverse_takes(family, w, c, "plane"),
                     lambda: repet._istft_stage(Y, w, np.zeros((w, c), np.float32), h, w, mask=np.ones(Y.shape, np.float32), path=family)),
                    (inverse_takes(family, w, c, "model"),
                     lambda: repet._istft_stage(Y, w, np.zeros((w, c), np.float32), h, w, model=np.ones((1, c, 1, h + 1), np.float32),
                                                periods=[1], path=family)),
                ]
                for takes, call in calls:
                    expected += not takes
                    try:
                        res = call()
                        launch = res["launch"] if isinstance(res, dict) else res[1]
                        assert takes and launch["family"] == family, (family, w, c, launch)
                    except RuntimeError as e:
                        assert not takes and "does not take this shape" in str(e), (family, w, c, str(e))
                        refused += 1
    print("refused (family, shape) pairs: %d of %d asked, %d expected by the rules" % (refused, 4 * len(FAMILIES) * len(WINDOWS) * len(CHANNELS), expected))
    assert refused == expected


def test_zz_report_the_largest_errors():
    """Last in the module: the table profiles/stft_stage_parity.txt is made of (family, check, shape, max error, bar)."""
    lines = ["%-10s %-5s %-16s err %.3e  bar %.3e  (%.2f of the bar)  %s" % (d, fam, check, err, bar, ratio, shape)
             for (d, fam, check), (ratio, err, bar, shape) in sorted(PARITY.items())]
    print("\n".join(lines))
    path = os.environ.get("REPET_STAGE_PARITY_OUT")
    if path and lines:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
