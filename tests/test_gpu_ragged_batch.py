"""A ragged batch in one tensor call (``repet.separate(..., lengths=...)``, ``Context.upload_tensor(x, lengths=...)``;
include/repet_hip.h: repet_ctx_upload_device_ragged): clips of unequal lengths, padded to one pitch.

The bar throughout is the one-clip call: clip ``b`` of the batch against ``separate(algo, x[b, :lengths[b]], fs, ...)`` AS VALUES
(``torch.equal``: NaN at the same positions, -0 equals +0) below the length, exactly zero behind it. The padding of every input is
NaN (or, for int16, full scale): a kernel that read it would show it. 8 kHz throughout: window 512, hop 256, a 10-s buffer of 312
frames. One-clip results are computed once per (variant, input, keywords) and shared."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet import _native
from helpers import periodic_clip, rms_err
from repet_synth import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 8000
H = 256
N = 98304
LENGTHS = (98304, 97280, 91137, 88001)        # full; a multiple of the hop; odd (splits a 16-byte store, a partial last frame); odd
ALGOS = ("original", "extended", "adaptive", "sim", "simonline")
LIVE, NONFINITE = 6, 7                        # fields of a level record (repet.LEVELS)
_cache = {}


def clips(channels):
    """The B = 4 clips, float64 (B, N, C) on the host, each a different mixture."""
    key = ("clips", channels)
    if key not in _cache:
        x = np.stack([synth(N / FS, FS, channels, 11 + b) for b in range(len(LENGTHS))])
        assert x.shape == (len(LENGTHS), N, channels)
        _cache[key] = x
    return _cache[key]


def padded(x, lengths, dtype=torch.float64, scale=1.0, fill=float("nan")):
    """The clips on the device in `dtype`, everything behind each length overwritten with `fill`."""
    t = torch.tensor(np.asarray(x) * scale, dtype=torch.float64, device=DEV)
    t = t.round().clamp(-32768, 32767).to(dtype) if dtype == torch.int16 else t.to(dtype)
    for b, n in enumerate(lengths):
        t[b, n:] = fill
    return t


def one_clip(key, algo, t, b, n, **kw):
    """separate() of clip b alone, trimmed to its n samples; cached under `key`."""
    key = (key, algo, b, n)
    if key not in _cache:
        _cache[key] = repet.separate(algo, t[b, :n], FS, **kw)
    return _cache[key]


def same_values(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.is_floating_point():
        nan_g, nan_w = torch.isnan(got), torch.isnan(want)
        assert torch.equal(nan_g, nan_w), f"NaN positions differ: {int(nan_g.sum())} against {int(nan_w.sum())}"
        got, want = got[~nan_g], want[~nan_w]
    differ = got != want
    assert not bool(differ.any()), f"{int(differ.sum())} of {differ.numel()} values differ"


def check_batch(results, lengths, reference):
    """results: the tensors of a which="both" call on the batch; reference(b) the pair of the one-clip call."""
    for b, n in enumerate(lengths):
        want = reference(b)
        for got, w in zip(results, want):
            same_values(got[b, :n], w)
            tail = got[b, n:]
            assert int(torch.count_nonzero(tail != 0)) == 0 and not bool(torch.isnan(tail.double()).any()), \
                f"clip {b}: {int(torch.count_nonzero(tail != 0))} values behind the length are not zero"


# ---- 1. parity with the one-clip call ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [2, 1], ids=["stereo", "mono"])
@pytest.mark.parametrize("algo", ALGOS)
def test_every_clip_is_the_one_clip_call(algo, channels):
    t = padded(clips(channels), LENGTHS)
    bg, fg = repet.separate(algo, t, FS, which="both", lengths=list(LENGTHS))
    assert bg.shape == fg.shape == t.shape and bg.dtype == fg.dtype == torch.float64
    check_batch((bg, fg), LENGTHS, lambda b: one_clip(("f64", channels), algo, t, b, LENGTHS[b], which="both"))
    assert bool(torch.isnan(t[1, LENGTHS[1]:]).all())             # the input is untouched


@pytest.mark.parametrize("dtype, fill", [(torch.float64, float("nan")), (torch.int16, 32767), (torch.bfloat16, float("nan"))],
                         ids=["float64", "int16", "bfloat16"])
@pytest.mark.parametrize("algo", ALGOS)
def test_other_inputs_into_a_strided_int16_out(algo, dtype, fill):
    """PCM-scale input of three dtypes, lengths as a NumPy array, and a pair of int16 destinations that are every other column
    of wider, longer buffers: the ragged ingest of each dtype and the ragged emission's element-wise stores."""
    t = padded(clips(2), LENGTHS, dtype=dtype, scale=20000.0, fill=fill)
    outs = tuple(torch.full((len(LENGTHS), N + 3, 4), 77, dtype=torch.int16, device=DEV) for _ in range(2))
    views = tuple(o[:, :N, ::2] for o in outs)
    got = repet.separate(algo, t, FS, which="both", out=views, lengths=np.array(LENGTHS))
    assert got[0].data_ptr() == views[0].data_ptr() and got[1].data_ptr() == views[1].data_ptr()
    check_batch(views, LENGTHS, lambda b: one_clip(("pcm", str(dtype)), algo, t, b, LENGTHS[b], which="both", dtype=torch.int16))
    for o in outs:                                                # nothing outside the views was written
        assert bool((o[:, N:] == 77).all()) and bool((o[:, :, 1::2] == 77).all())
    assert bool((views[0] != 0).any())


# ---- 2. padding is never read ------------------------------------------------------------------------------------------------------
def test_padding_does_not_trip_the_refusal_mode_and_a_nan_inside_a_clip_does(monkeypatch):
    monkeypatch.setattr(repet, "strict_reference", False)
    x = clips(2)
    for fill in (float("nan"), float("inf"), float("-inf")):
        t = padded(x, LENGTHS, fill=fill)
        bg = repet.separate("simonline", t, FS, lengths=LENGTHS)
        assert not bool(torch.isnan(bg).any()) and bool(torch.isfinite(bg).all())
    for algo in ("simonline", "sim"):
        t = padded(x, LENGTHS, dtype=torch.float32)
        t[2, LENGTHS[2] - 1, 1] = float("nan")                    # the last live sample of clip 2
        with pytest.raises(ValueError, match="NaN or infinite"):
            repet.separate(algo, t, FS, lengths=LENGTHS)
        t[2, LENGTHS[2] - 1, 1] = 0.0
        t[2, LENGTHS[2], 0] = float("inf")                        # the first padded one
        repet.separate(algo, t, FS, lengths=LENGTHS)


# ---- 3. simonline stays batched ----------------------------------------------------------------------------------------------------
def test_simonline_keeps_one_launch_per_stage_and_the_others_loop():
    t = padded(clips(2), LENGTHS)
    p = repet.derive_params(FS)
    ctx = repet.Context(0)
    try:
        ctx.upload_tensor(t, lengths=LENGTHS)
        assert ctx.shape == (len(LENGTHS), N, 2) and ctx.clip_lengths() == LENGTHS
        stages = [s["name"] for s in ctx.execute("simonline", p, timing=True)["stages"]]
        assert "clips" not in stages, stages
        for name in ("stft", "local_maxima", "mask_sim", "tail_clear", "istft_ola"):
            assert stages.count(name) == 1, stages
        assert stages.index("mask_sim") < stages.index("tail_clear") < stages.index("istft_ola")
        bg = ctx.download_tensor()
        for b, n in enumerate(LENGTHS):
            same_values(bg[b, :n], one_clip(("f64", 2), "simonline", t, b, n, which="both")[0])
        for algo in ("sim", "original"):
            assert [s["name"] for s in ctx.execute(algo, p, timing=True)["stages"]] == ["clips"]
        # an equal batch on the same context: the lengths are gone with the upload, and so is the extra launch
        ctx.upload_tensor(torch.nan_to_num(t))
        assert ctx.clip_lengths() == (N,) * len(LENGTHS)
        stages = [s["name"] for s in ctx.execute("simonline", p, timing=True)["stages"]]
        assert "tail_clear" not in stages and "clips" not in stages, stages
        # lengths that all equal N are that path
        ctx.upload_tensor(torch.nan_to_num(t), lengths=[N] * len(LENGTHS))
        assert "tail_clear" not in [s["name"] for s in ctx.execute("simonline", p, timing=True)["stages"]]
    finally:
        ctx.close()


# ---- 4. the tail -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("silent_frames", ["reference", "zero"])
def test_the_last_hop_takes_nothing_from_the_frames_behind_the_clip(silent_frames):
    """One clip ends one sample into a new hop, one on the hop grid, one a window short of the pitch; the frames behind each are
    zeros and the clip's own end -- digital silence under the reference rule, NaN masks. Their share of the overlap-add is the
    clip's last 512 samples."""
    lengths = (352 * H + 1, 352 * H, N - 512, N)
    t = padded(clips(2), lengths)
    bg, fg = repet.separate("simonline", t, FS, which="both", silent_frames=silent_frames, lengths=lengths)
    for b, n in enumerate(lengths):
        want = one_clip(("tail", silent_frames), "simonline", t, b, n, which="both", silent_frames=silent_frames)
        for got, w in zip((bg, fg), want):
            assert not bool(torch.isnan(w[-512:]).any())
            same_values(got[b, n - 512:n], w[-512:])
            same_values(got[b, :n], w)
            assert int(torch.count_nonzero(got[b, n:])) == 0 and not bool(torch.isnan(got[b, n:]).any())


# ---- 5. levels and gains -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["simonline", "sim", "extended"])
def test_levels_are_the_one_clip_records(algo):
    t = padded(clips(2), LENGTHS)
    (bg, fg), record = repet.separate(algo, t, FS, which="both", levels=True, lengths=LENGTHS)
    assert record.shape == (len(LENGTHS), 2, 8) and record.dtype == torch.float64
    for b, n in enumerate(LENGTHS):
        _, want = one_clip(("levels", 2), algo, t, b, n, which="both", levels=True)
        assert torch.equal(record[b], want), (b, record[b].tolist(), want.tolist())          # bit for bit (no NaN in these)
        assert record[b, :, LIVE].tolist() == [float(n)] * 2 and record[b, :, NONFINITE].tolist() == [0.0] * 2


@pytest.mark.parametrize("algo", ["simonline", "sim", "original"])
def test_gains_give_the_one_clip_foregrounds(algo):
    t = padded(clips(2), LENGTHS)
    edges = [0, 12, 90, 257]
    table = np.array([[1.0, 0.5, 0.0], [0.25, 0.0, 0.75], [0.0, 1.0, 0.125], [0.5, 0.5, 0.5]])
    bg, fg = repet.separate(algo, t, FS, which="both", background_gain=0.25, lengths=LENGTHS)
    check_batch((bg, fg), LENGTHS, lambda b: one_clip(("gain", 2), algo, t, b, LENGTHS[b], which="both", background_gain=0.25))
    (bg, fg), record = repet.separate(algo, t, FS, which="both", background_band_gains=table, band_edges=edges, levels=True,
                                      lengths=LENGTHS)
    for b, n in enumerate(LENGTHS):
        want, want_record = one_clip(("bands", 2), algo, t, b, n, which="both", background_band_gains=table[b], band_edges=edges,
                                     levels=True)
        same_values(bg[b, :n], want[0])
        same_values(fg[b, :n], want[1])
        assert torch.equal(record[b], want_record)
        assert int(torch.count_nonzero(fg[b, n:])) == 0 and int(torch.count_nonzero(bg[b, n:])) == 0
    plain = one_clip(("f64", 2), algo, t, 1, LENGTHS[1], which="both")[1]
    assert not torch.equal(fg[1, :LENGTHS[1]], plain)             # the table did shape the foreground


# ---- 6. against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sim", "simonline"])
def test_against_the_oracle(algo):
    from oracle import repet_oracle as orc
    lengths = (88001, 81920)
    pitch = 90112
    x = np.stack([periodic_clip(FS, 9 + b, pitch / FS, 2, seed=3 + b, jitter=1e-7) for b in range(2)])
    t = padded(x, lengths)
    bg = repet.separate(algo, t, FS, lengths=lengths)
    for b, n in enumerate(lengths):
        want = orc.ALGORITHMS[algo](np.array(x[b, :n]), FS)
        got = bg[b, :n].cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        err = rms_err(got[ok], want[ok])
        print(f"ragged {algo} clip {b} ({n} samples): rms error against the oracle {err:.3e}")
        assert err <= 1e-4, (b, err)


# ---- 7. errors on the device path --------------------------------------------------------------------------------------------------
def test_a_clip_too_short_is_refused_by_name_and_the_next_call_is_right():
    p = repet.derive_params(FS)
    least = (p.buffer_frames - 2) * p.step_length + p.window_length
    t = padded(clips(2), LENGTHS)
    with pytest.raises(ValueError, match="operands could not be broadcast together") as one:
        repet.separate("simonline", t[0, :least - 1], FS)
    with pytest.raises(ValueError, match=r"clip 2 of the batch .*operands could not be broadcast together") as batch:
        repet.separate("simonline", t, FS, lengths=[N, least, least - 1, N])
    assert str(one.value) in str(batch.value)
    bg, fg = repet.separate("simonline", t, FS, which="both", lengths=LENGTHS)
    check_batch((bg, fg), LENGTHS, lambda b: one_clip(("f64", 2), "simonline", t, b, LENGTHS[b], which="both"))
    # the low-level call makes the same refusal at execute, before anything is enqueued, and the context goes on
    ctx = repet.Context(0)
    try:
        ctx.upload_tensor(t, lengths=[N, least, least - 1, N])
        with pytest.raises(ValueError, match="clip 2 of the batch"):
            ctx.execute_async("simonline", p)
        ctx.upload_tensor(t, lengths=LENGTHS)
        ctx.execute_async("simonline", p)
        same_values(ctx.download_tensor()[3, :LENGTHS[3]], one_clip(("f64", 2), "simonline", t, 3, LENGTHS[3], which="both")[0])
        with pytest.raises(ValueError, match="outside"):
            ctx.upload_tensor(t, lengths=[N, N, N + 1, N])
    finally:
        ctx.close()


def test_lengths_on_the_device_are_a_type_error():
    t = padded(clips(2), LENGTHS)
    with pytest.raises(TypeError, match="host"):
        repet.separate("simonline", t, FS, lengths=torch.tensor(LENGTHS, device=DEV))
    with pytest.raises(ValueError, match="batch"):
        repet.separate("simonline", t[0], FS, lengths=[N])
