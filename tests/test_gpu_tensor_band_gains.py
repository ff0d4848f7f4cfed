"""Band gains of the tensor calls (``repet.separate(..., background_band_gains=, band_edges=)``, ``Context.set_background_band_gains``;
include/repet_hip.h: repet_ctx_set_background_band_gains): a share of the background kept in the foreground bin by bin, one table
for the whole clip.

    a[k] = float32(1 - float64(float32(g[k])));   shaped_bg = the variant's inverse of a[k] * Y_j[k];   fg = fma(-a_s, shaped_bg, x)

Signals, tables and the float64 model are those of tests/band_gains_offline_reference.py, held to the sensitivity condition by
tests/test_band_gains_offline_reference.py (a library that ignored the table would be off by ten times RMS_TOL or more).

Bars:
  bit for bit      whatever does not depend on the table (background, mixture, the MIX / BG / LIVE / NONFINITE levels, the similar
                   frames and the periods), an all-zero table (the plain foreground), ``g = 1`` everywhere (the input), the
                   destination dtypes, the live handles' foreground for ``simonline``, a batch against its clips
  against the model  the shaped background is recovered as ``mixture - foreground`` (float64, scalar gain 0) and compared in rms
                   with ``2 E + 2**-22 max |bg_model|``, ``E = rms(bg_gpu - bg_model)`` of the PLAIN background of the same call:
                   the bar of tests/test_gpu_online_band_gains.py, for the reason given there. ``simonline``: over the samples from
                   ``(B - 1) H`` on. Not fitted: the ratio met is printed and collected.
  RMS_TOL          the foreground against ``x - shaped_model``

The error met, E and their ratio per case are collected in PARITY and printed (and written to
$REPET_TENSOR_BAND_GAINS_PARITY_OUT) by the last test: profiles/tensor_band_gains_parity.txt is that output from an MI355X."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet import _native
import band_gains_offline_reference as model
from band_gains_cases import FS, FS44, H, H44, N8, signal
from band_gains_reference import factor
from emit_dtypes_reference import round_ref
from helpers import rms_err
from levels_reference import BG_ENERGY, BG_PEAK, FG_ENERGY, FG_PEAK, LIVE, MIX_ENERGY, MIX_PEAK, NONFINITE, check as check_levels, levels
from test_gpu_online_foreground import to_numpy
from test_gpu_online_streams import same
from test_gpu_variants import RMS_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PARITY = {}
UNSHAPED = (MIX_ENERGY, BG_ENERGY, MIX_PEAK, BG_PEAK, LIVE, NONFINITE)


def dev(x, dtype=torch.float64):
    return torch.tensor(np.asarray(x), dtype=dtype, device=DEV)


def table_args(name):
    edges, gains = model.TABLES[name]
    return {"background_band_gains": gains, "band_edges": edges}


def both(algo, x, fs, **kw):
    bg, fg = repet.separate(algo, dev(x), fs, which="both", **kw)
    return to_numpy(bg), to_numpy(fg)


# ---- 1. against the model, per case ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,algo,table", model.USES, ids=["-".join(u) for u in model.USES])
def test_against_the_model(name, algo, table):
    x, fs = model.row_signal(name)
    x = np.asarray(x)
    bg, fg = both(algo, x, fs, **table_args(table))
    assert bg.shape == fg.shape == x.shape and bg.dtype == fg.dtype == np.float64
    if table == "all":
        same(fg, x)                                           # g = 1 on every bin: the input
        assert np.any(bg != 0)
        return
    p = repet.derive_params(fs)
    first = (p.buffer_frames - 1) * p.step_length if algo == "simonline" else 0
    part = slice(first, None)
    bg_model, shaped_model = model.plain_of(name, algo), model.shaped_of(name, algo, table)
    shaped = x - fg                                           # (the mixture of an fp32-exact float64 tensor is the tensor)
    e_plain = model.rms((bg - bg_model)[part])
    err = model.rms((shaped - shaped_model)[part])
    bar = 2 * e_plain + 2.0 ** -22 * float(np.max(np.abs(bg_model)))
    ratio = err / e_plain if e_plain > 0 else float("inf")
    label = f"{name} {algo} {table}"
    print(f"{label}: shaped background off by {err:.3e} rms, plain E {e_plain:.3e}, ratio {ratio:.3f}, bar {bar:.3e}")
    PARITY[label] = (err, e_plain, ratio, bar)
    assert err <= bar, (label, err, bar)
    tol = rms_err(fg[part], (x - shaped_model)[part])
    assert tol <= RMS_TOL, (label, tol)


# ---- 2. bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,algo,table", [("8k-stereo", "sim", "speech-only"), ("8k-stereo", "extended", "per-bin"),
                                             ("8k-stereo", "simonline", "duck"), ("44k-stereo", "original", "mel44"),
                                             ("44k-stereo", "adaptive", "per-bin44"), ("8k-three", "sim", "duck")])
def test_what_the_table_does_not_touch_keeps_its_bits(name, algo, table):
    x, fs = model.row_signal(name)
    xt = dev(x)
    ctx = _native.tensor_context(0)
    p = repet.derive_params(fs)

    def lists():
        if algo in ("sim", "simonline"):
            t = _native.lib().repet_frame_count(len(x), p.window_length, p.step_length, 1 if algo == "sim" else 0)
            rows = t if algo == "sim" else t - p.buffer_frames + 1
            idx, cnt = ctx.last_sim_indices(rows, p.sim_number)
            return idx.tobytes() + cnt.tobytes()
        return ctx.last_periods(4096).tobytes()

    (bg0, fg0), rec0 = repet.separate(algo, xt, fs, which="both", levels=True)
    lists0 = lists()
    mix0 = repet.separate(algo, xt, fs, which="mixture")
    (bg1, fg1), rec1 = repet.separate(algo, xt, fs, which="both", levels=True, **table_args(table))
    lists1 = lists()
    assert ctx.background_band_gains() is None                # for that call alone
    bg0, fg0, bg1, fg1, rec0, rec1 = (to_numpy(a) for a in (bg0, fg0, bg1, fg1, rec0, rec1))
    assert bg1.tobytes() == bg0.tobytes() and lists1 == lists0
    assert rec1[..., UNSHAPED].tobytes() == rec0[..., UNSHAPED].tobytes()
    assert np.any(fg1 != fg0) and np.any(rec1[..., FG_ENERGY] != rec0[..., FG_ENERGY])
    # FG_* measure the foreground as emitted: the shaped one
    mix = to_numpy(mix0)
    same(mix, np.asarray(x))
    check_levels(rec1[None], levels(mix[None], bg1[None], fg1[None]), f"{name} {algo} {table}")
    assert np.array_equal(rec1[..., FG_PEAK], np.max(np.abs(fg1), axis=0))
    # an all-zero table is no table; the call after a table is the plain one again
    edges, gains = model.TABLES[table]
    bgz, fgz = both(algo, x, fs, background_band_gains=np.zeros_like(np.asarray(gains, dtype=np.float64)), band_edges=edges)
    assert bgz.tobytes() == bg0.tobytes() and fgz.tobytes() == fg0.tobytes()
    bgp, fgp = both(algo, x, fs)
    assert bgp.tobytes() == bg0.tobytes() and fgp.tobytes() == fg0.tobytes()
    # "foreground" alone is the second half of "both"
    assert to_numpy(repet.separate(algo, xt, fs, which="foreground", **table_args(table))).tobytes() == fg1.tobytes()


def test_a_scalar_gain_multiplies_on_top():
    """fg = fma(-a_s, shaped, x) with ``shaped`` recovered as ``x - fg`` of the same table at scalar gain 0. Where that recovered
    value is an fp32 value (x - shaped was exact in float64: all but samples whose background is 2**29 times smaller than the
    input) the product a_s * shaped is exact in float64 and the fma is the float64 sum: bit for bit. Elsewhere the recovery is
    off by at most one rounding of x - shaped, 2**-53 max(|x|, |shaped|), twice through: 2**-51 of it bounds the difference."""
    x, fs = model.row_signal("8k-stereo")
    x = np.asarray(x)
    for algo, table in (("sim", "duck"), ("extended", "per-bin")):
        fg0 = both(algo, x, fs, **table_args(table))[1]
        fg_half = both(algo, x, fs, background_gain=0.5, **table_args(table))[1]
        shaped = x - fg0
        a_s = float(factor(0.5))
        want = x + (-a_s * shaped)
        exact = shaped.astype(np.float32).astype(np.float64) == shaped
        assert np.mean(exact) > 0.99
        assert np.array_equal(fg_half[exact], want[exact])
        assert np.all(np.abs(fg_half - want) <= 2.0 ** -51 * np.maximum(np.abs(x), np.abs(shaped)))
        assert np.any(fg_half != fg0)


def test_float32_and_int16_destinations_round_the_float64_foreground_once():
    x, fs = model.row_signal("8k-three")
    xs = np.asarray(x) * 16384.0                                   # (a power of two: still fp32 values)
    xt = dev(xs)
    kw = table_args("duck")
    fg64 = to_numpy(repet.separate("sim", xt, fs, which="foreground", **kw))
    assert np.any(np.abs(fg64) > 100)
    out32 = torch.full(xs.shape, 7, dtype=torch.float32, device=DEV)
    assert repet.separate("sim", xt, fs, which="foreground", out=out32, **kw) is out32
    same(to_numpy(out32), fg64.astype(np.float32))
    got16 = to_numpy(repet.separate("sim", xt, fs, which="foreground", dtype=torch.int16, **kw))
    assert np.array_equal(got16, round_ref(fg64, "int16"))
    unit = dev(x)                                                  # (the 16-bit floats: at the signal's own scale)
    unit64 = to_numpy(repet.separate("sim", unit, fs, which="foreground", **kw))
    for dt, name in ((torch.float16, "float16"), (torch.bfloat16, "bfloat16")):
        got = repet.separate("sim", unit, fs, which="foreground", dtype=dt, **kw)
        bits = to_numpy(got.view(torch.int16)).view(np.uint16)
        want = round_ref(unit64, name)
        assert np.array_equal(bits, want if want.dtype == np.uint16 else want.view(np.uint16))


# ---- 3. the live handles' definition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,seed,n,ch,table", [(FS, 32, N8, 2, "speech-only"), (FS44, 35, model.samples(16, FS44), 2, "mel44")])
def test_simonline_is_the_live_handles_foreground(fs, seed, n, ch, table):
    x = np.asarray(signal(seed, n, fs, ch))
    h = repet.derive_params(fs).step_length
    offline = to_numpy(repet.separate("simonline", dev(x), fs, which="foreground", **table_args(table)))
    plain = to_numpy(repet.separate("simonline", dev(x), fs, which="foreground"))
    handle = repet.online_streams(fs, ch, 1)
    edges, gains = model.TABLES[table]
    handle.set_background_band_gains(gains, edges)
    xt = dev(x[None])
    pieces = [handle.push(xt[:, pos:pos + h], which="foreground") for pos in range(0, n, h)]
    pieces.append(handle.finish(which="foreground"))
    handle.close()
    live = np.concatenate([to_numpy(p) for p in pieces], axis=1)[0]
    assert live.shape == offline.shape
    assert live.tobytes() == offline.tobytes()
    assert np.any(offline != plain)


# ---- 4. batches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sim", "simonline", "original"])
def test_a_batch_is_its_clips(algo):
    xs = np.stack([np.asarray(signal(seed, N8, FS, 2)) for seed in (31, 32, 33)])
    xt = dev(xs)
    edges = [0, 7, 19, 218, model.bins(FS)]
    rows = np.array([[1.0, 0.0, 0.5, 0.25], [0.0, 0.75, 0.0, 1.0], [0.5, 0.5, 1.0, 0.0]])
    one = to_numpy(repet.separate(algo, xt, FS, which="foreground", background_band_gains=rows[1], band_edges=edges))
    per = to_numpy(repet.separate(algo, xt, FS, which="foreground", background_band_gains=rows, band_edges=edges))
    plain = to_numpy(repet.separate(algo, xt, FS, which="foreground"))
    for b in range(3):
        single = to_numpy(repet.separate(algo, xt[b], FS, which="foreground", background_band_gains=rows[1], band_edges=edges))
        assert one[b].tobytes() == single.tobytes(), b
        own = to_numpy(repet.separate(algo, xt[b], FS, which="foreground", background_band_gains=rows[b], band_edges=edges))
        assert per[b].tobytes() == own.tobytes(), b
        assert np.any(own != plain[b])
    assert per[1].tobytes() == one[1].tobytes() and np.any(per[0] != one[0])
    with pytest.raises(ValueError, match="band gains"):
        repet.separate(algo, xt, FS, which="foreground", background_band_gains=rows[:2], band_edges=edges)     # two rows, three clips


# ---- 5. rule of time and refusals ------------------------------------------------------------------------------------------------------
def test_the_table_of_the_execute_shapes_the_result():
    x, fs = model.row_signal("8k-stereo")
    xt = dev(x)
    p = repet.derive_params(fs)
    w = p.window_length
    want = to_numpy(repet.separate("sim", xt, fs, which="foreground", **table_args("duck")))
    plain = to_numpy(repet.separate("sim", xt, fs, which="foreground"))
    ctx = _native.Context(0)
    try:
        edges, gains = model.TABLES["duck"]
        ctx.upload_tensor(xt)
        ctx.set_background_band_gains(gains, edges, window_length=w)
        assert np.array_equal(ctx.background_band_gains(), model.table_gains("duck", fs))
        ctx.execute_async("sim", p)
        ctx.set_background_band_gains(*reversed(model.TABLES["bass"]), window_length=w)      # a set behind the execute
        assert to_numpy(ctx.download_tensor(which="foreground")).tobytes() == want.tobytes()
        ctx.clear_background_band_gains()                                                     # and a clear
        assert ctx.background_band_gains() is None
        assert to_numpy(ctx.download_tensor(which="foreground")).tobytes() == want.tobytes()
        assert to_numpy(ctx.result_levels())[..., FG_PEAK].tolist() == np.max(np.abs(want), axis=0).tolist()
        ctx.execute_async("sim", p)                                                           # the next run: no table
        assert to_numpy(ctx.download_tensor(which="foreground")).tobytes() == plain.tobytes()
        # refusals of an execute, before anything is enqueued: the resident result stays the plain one
        ctx.set_background_band_gains(np.full(1024 // 2 + 1, 0.5), window_length=1024)
        with pytest.raises(ValueError, match="window_length"):
            ctx.execute_async("sim", p)
        with pytest.raises(ValueError, match="window_length"):
            ctx.execute("sim", p)
        ctx.set_background_band_gains(np.full((2, w // 2 + 1), 0.5), window_length=w)        # two rows, one clip
        with pytest.raises(ValueError, match="band gains"):
            ctx.execute_async("sim", p)
        ctx.set_background_band_gains(gains, edges, window_length=w)
        for call in (lambda: ctx.execute_extended_range(p, 0, 1), lambda: ctx.execute_extended_range_async(p, 0, 1)):
            with pytest.raises(ValueError, match="band gains"):
                call()
        assert to_numpy(ctx.download_tensor(which="foreground")).tobytes() == plain.tobytes()
        assert to_numpy(ctx.download_tensor(which="background")).tobytes() == to_numpy(repet.separate("sim", xt, fs)).tobytes()
        # an all-zero table is no table: segment ranges run
        ctx.set_background_band_gains(np.zeros(w // 2 + 1), window_length=w)
        ctx.execute_extended_range(p, 0, 1)
        ctx.clear_background_band_gains()
        ctx.execute_async("sim", p)
        assert to_numpy(ctx.download_tensor(which="foreground")).tobytes() == plain.tobytes()
    finally:
        ctx.close()


def test_refusals_leave_the_plain_call_as_it_was():
    x, fs = model.row_signal("8k-three")
    xt = dev(x)
    f = model.bins(fs)
    plain = to_numpy(repet.separate("sim", xt, fs, which="foreground"))
    bad = [dict(background_band_gains=[0.5, 1.5], band_edges=[0, 4, 9]),
           dict(background_band_gains=[0.5, -0.1], band_edges=[0, 4, 9]),
           dict(background_band_gains=[0.5, float("nan")], band_edges=[0, 4, 9]),
           dict(background_band_gains=[0.5, 0.5], band_edges=[4, 0, 9]),                    # edges that descend
           dict(background_band_gains=[0.5, 0.5], band_edges=[0, 4, f + 1]),                # an edge past the last bin
           dict(background_band_gains=[0.5], band_edges=[0, 4, 9]),                         # one gain for two bands
           dict(background_band_gains=np.zeros(f - 1)),                                     # per bin, one short
           dict(background_band_gains=np.zeros((2, f))),                                    # rows without a batch
           dict(band_edges=[0, 4, 9])]                                                      # edges without gains
    for kw in bad:
        with pytest.raises(ValueError):
            repet.separate("sim", xt, fs, which="foreground", **kw)
    for which in ("background", "mixture"):
        with pytest.raises(ValueError, match="which"):
            repet.separate("sim", xt, fs, which=which, background_band_gains=[0.5, 0.5], band_edges=[0, 4, 9])
    assert to_numpy(repet.separate("sim", xt, fs, which="foreground")).tobytes() == plain.tobytes()
    # a window of 8192 samples has no masked inverse kernel: REPET_ERR_LIMIT, as on the live handles
    fs_hi = 192000
    assert repet.derive_params(fs_hi).window_length == 8192
    short = dev(np.asarray(signal(39, fs_hi // 2, fs_hi, 1)))
    with pytest.raises(RuntimeError, match=str(_native.ERR_LIMIT)):
        repet.separate("sim", short, fs_hi, which="foreground", background_band_gains=np.full(4097, 0.5))
    lib = _native.lib()
    gains = np.full(4097, 0.5, dtype=np.float32)
    assert lib.repet_set_run_background_band_gains(0, 8192, None, 4097, _native.ptr(gains), 1) == _native.ERR_LIMIT
    assert lib.repet_set_run_background_band_gains(0, 4096, None, 4097, _native.ptr(gains), 1) == _native.ERR_BAD_ARG
    assert lib.repet_set_run_background_band_gains(0, 8192, None, 0, None, 0) == 0
    assert _native.tensor_context(0).background_band_gains() is None
    assert to_numpy(repet.separate("sim", xt, fs, which="foreground")).tobytes() == plain.tobytes()


def test_the_per_thread_run_context_takes_the_table():
    """repet_run_device under repet_set_run_background_band_gains is the call of repet.separate, bit for bit."""
    import ctypes as C
    x, fs = model.row_signal("8k-stereo")
    xt = dev(x)
    want = to_numpy(repet.separate("sim", xt, fs, which="foreground", **table_args("duck")))
    lib = _native.lib()
    p = repet.derive_params(fs)
    edges, gains = _native.band_gain_rows(model.TABLES["duck"][1], model.TABLES["duck"][0], model.bins(fs))
    out = torch.empty_like(xt)
    n, ch = x.shape
    strides = (C.c_int64 * 3)(n * ch, ch, 1)
    stream = C.c_void_p(torch.cuda.current_stream(xt.device).cuda_stream)
    _native.check(lib.repet_set_run_background_band_gains(0, p.window_length, _native.ptr(edges), gains.shape[1], _native.ptr(gains), 1))
    try:
        _native.check(lib.repet_select_run_result(0, _native.OUT_FOREGROUND))
        _native.check(lib.repet_run_device(_native.ALGO_IDS["sim"], C.c_void_p(xt.data_ptr()), _native.F64, 1, n, ch, strides,
                                           C.c_void_p(out.data_ptr()), _native.F64, strides, C.byref(p), 0, stream))
    finally:
        lib.repet_select_run_result(0, _native.OUT_BACKGROUND)
        lib.repet_set_run_background_band_gains(0, 0, None, 0, None, 0)
    assert to_numpy(out).tobytes() == want.tobytes()


def test_zz_parity_table():
    """Prints what the checks above met (run after them: pytest keeps file order)."""
    if not PARITY:
        return
    lines = ["case                                               error (rms)   plain E (rms)   error / E      bar"]
    for label in sorted(PARITY):
        err, e_plain, ratio, bar = PARITY[label]
        lines.append(f"{label:<50} {err:.3e}     {e_plain:.3e}       {ratio:7.3f}   {bar:.3e}")
    text = "\n".join(lines)
    print("\n" + text)
    path = os.environ.get("REPET_TENSOR_BAND_GAINS_PARITY_OUT")
    if path:
        with open(path, "w") as fh:
            fh.write(text + "\n")
