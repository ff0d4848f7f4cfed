"""ROCm torch tensors through the drop-in functions and ``repet.separate``: the device-side ingest and egress (devio.hip)
replace the host round trip, and every result is the NumPy call's result bit for bit (NaN positions equal, every other value
identical). The calls are ordered on the caller's current stream by events and do not wait on the host."""
import ctypes
import threading
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet import _native
from helpers import golden_input
from repet_synth import synth

pytestmark = pytest.mark.gpu

ALGOS = ["original", "extended", "adaptive", "sim", "simonline"]


def same(got, want):
    """NaN positions equal and every other value identical (as values: -0.0 equals 0.0)."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), f"NaN positions differ: {int(nan_g.sum())} against {int(nan_w.sum())}"
    ok = ~nan_g
    diff = got[ok] != want[ok]
    assert not diff.any(), (f"{int(diff.sum())} of {diff.size} values differ, largest by "
                            f"{float(np.max(np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)))):.3e}")


def clip(name):
    if name == "synth44k":
        return synth(12.0, 44100, 2, 5), 44100
    return golden_input(name)


def as_dtype(x, dtype):
    """The host array a tensor of `dtype` holds (int16: the raw PCM values the NumPy path casts without scaling)."""
    if dtype == "i16":
        return np.clip(np.round(np.asarray(x) * 20000), -32768, 32767).astype(np.int16)
    return np.ascontiguousarray(x, dtype={"f64": np.float64, "f32": np.float32}[dtype])


def sleep_cycles(ms):
    """torch.cuda._sleep cycles worth about `ms` milliseconds on this device (calibrated once)."""
    if not hasattr(sleep_cycles, "rate"):
        torch.cuda._sleep(1000)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(int(2e7))
        b.record()
        b.synchronize()
        sleep_cycles.rate = 2e7 / max(a.elapsed_time(b), 1e-3)
    return int(ms * sleep_cycles.rate)


@pytest.mark.parametrize("dtype", ["f64", "f32", "i16"])
@pytest.mark.parametrize("name", ["small_stereo", "synth44k"])
@pytest.mark.parametrize("algo", ALGOS)
def test_tensor_equals_numpy_call(algo, name, dtype):
    x, fs = clip(name)
    xn = as_dtype(x, dtype)
    want = getattr(repet, algo)(xn, fs)
    got = getattr(repet, algo)(torch.from_numpy(xn).cuda(), fs)
    assert got.is_cuda and got.device.index == 0 and got.dtype == torch.float64
    same(got, want)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("algo", ALGOS)
def test_half_precision_tensor_equals_host_call_on_its_values(algo, dtype):
    x, fs = golden_input("small_stereo")
    t = torch.from_numpy(np.ascontiguousarray(x)).to(getattr(torch, dtype)).cuda()
    want = getattr(repet, algo)(t.float().cpu().numpy(), fs)
    same(getattr(repet, algo)(t, fs), want)


def test_other_real_dtypes_go_through_float64():
    x, fs = golden_input("small_stereo")
    xi = np.round(np.asarray(x) * 1e6).astype(np.int32)
    same(repet.sim(torch.from_numpy(xi).cuda(), fs), repet.sim(xi, fs))


def jittered_periodic_clip(fs, period_hops, seconds, channels, seed=3, jitter=1e-7):
    """Copies of one period of the synth() mixture tiled bit for bit, plus white noise far below fp32 resolution: the
    similarities of the copies differ by ~1e-13, which only the float64 second level of the peak picking resolves."""
    hop = repet.derive_params(fs).step_length
    period = period_hops * hop
    base = synth(period / fs, fs, channels, seed)
    n = int(round(seconds * fs))
    x = np.tile(base, (-(-n // period), 1))[:n].copy()
    x += jitter * np.random.RandomState(seed + 1).standard_normal(x.shape)
    return x


@pytest.mark.parametrize("algo", ["sim", "simonline"])
def test_float64_remainders_survive(algo):
    fs = 8000
    x = jittered_periodic_clip(fs, 12, 24.0, 2)
    same(getattr(repet, algo)(torch.from_numpy(x).cuda(), fs), getattr(repet, algo)(x, fs))
    p = repet.derive_params(fs)
    host = repet.Context(0)
    host.upload(x)
    host.execute(algo, p)
    t = host.last_frame_count()
    if algo == "simonline":
        t = t - p.buffer_frames + 1                          # rows of the frames past the buffer's warm-up
    want_idx, want_cnt = host.last_sim_indices(t, p.sim_number)
    want = host.download()
    host.close()
    ctx = repet.Context(0)
    ctx.upload_tensor(torch.from_numpy(x).cuda())
    ctx.execute(algo, p)
    assert ctx.last_exact_stats()["input_has_remainders"]
    idx, cnt = ctx.last_sim_indices(t, p.sim_number)
    got = ctx.download_tensor()
    torch.cuda.synchronize()
    ctx.close()
    assert np.array_equal(cnt, want_cnt)
    for r in range(t):
        assert np.array_equal(idx[r, :cnt[r]], want_idx[r, :want_cnt[r]]), r
    same(got, want)


def test_layouts():
    x, fs = golden_input("small_stereo")
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    want = repet.sim(xd, fs)
    # channels-first storage read through its .T view
    cf = xd.T.contiguous()
    same(repet.sim(cf.T, fs), want)
    # a step slice
    wide = torch.zeros(2 * xd.shape[0], 2, dtype=torch.float64, device="cuda")
    wide[::2] = xd
    same(repet.sim(wide[::2], fs), want)
    # a batch slice
    xb = torch.stack([torch.zeros_like(xd), xd, xd * 0.5])
    same(repet.sim(xb[1], fs), want)


@pytest.mark.parametrize("algo", ["sim", "simonline"])
def test_separate_batch_equals_single_calls(algo):
    fs = 16000
    clips = [synth(13.0, fs, 2, seed) for seed in (1, 2, 3)]    # (simonline: longer than its 10-s buffer)
    xb = torch.from_numpy(np.stack(clips)).cuda()
    got = repet.separate(algo, xb, fs)
    assert got.shape == xb.shape and got.dtype == torch.float64
    for b in range(3):
        same(got[b], getattr(repet, algo)(clips[b], fs))


def test_separate_into_strided_float32_out():
    x, fs = golden_input("small_stereo")
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    want = repet.sim(x, fs)
    store = torch.full((2, x.shape[0]), 7.0, dtype=torch.float32, device="cuda")
    out = store.T                                            # (N, 2) with strides (1, N)
    ret = repet.separate("sim", xd, fs, out=out)
    assert ret is out
    same(store.T, want.astype(np.float32))


def test_stream_ordering_without_host_sync():
    x, fs = golden_input("small_stereo")
    want = repet.sim(x, fs)
    src = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    xd = torch.zeros_like(src)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(sleep_cycles(100))
        xd.copy_(src)
        y = repet.sim(xd, fs)
        z = y.clone()
    torch.cuda.synchronize()
    same(z, want)


def test_calls_do_not_wait_for_the_device():
    x, fs = golden_input("small_stereo")
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    wants = {a: getattr(repet, a)(x, fs) for a in ALGOS}
    warm = [getattr(repet, a)(xd, fs) for a in ALGOS]           # workspaces of this shape, result blocks in the cache
    torch.cuda.synchronize()
    del warm
    cycles = sleep_cycles(200)
    torch.cuda._sleep(cycles)
    got, times = {}, {}
    for a in ALGOS:
        t0 = time.perf_counter()
        got[a] = getattr(repet, a)(xd, fs)
        times[a] = time.perf_counter() - t0
    torch.cuda.synchronize()
    assert all(t < 0.05 for t in times.values()), times
    for a in ALGOS:
        same(got[a], wants[a])


def test_non_finite_samples():
    x, fs = golden_input("small_stereo")
    x = np.array(x)
    x[40000, 1] = np.nan
    xd = torch.from_numpy(x).cuda()
    same(repet.sim(xd, fs), repet.sim(x, fs))
    saved = repet.strict_reference
    try:
        repet.strict_reference = False
        with pytest.raises(ValueError) as host:
            repet.sim(x, fs)
        with pytest.raises(ValueError) as dev:
            repet.sim(xd, fs)
        assert str(dev.value) == str(host.value)
        clean = torch.from_numpy(np.ascontiguousarray(golden_input("small_stereo")[0])).cuda()
        same(repet.sim(clean, fs), repet.sim(golden_input("small_stereo")[0], fs))
    finally:
        repet.strict_reference = saved


def test_threads_on_their_own_streams():
    fs = 16000
    clips = [synth(6.0, fs, 2, 11), synth(6.0, fs, 2, 12)]
    wants = [repet.sim(c, fs) for c in clips]
    results, errors = [[], []], []

    def work(k):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                xd = torch.from_numpy(clips[k]).cuda()
                for _ in range(3):
                    results[k].append(repet.sim(xd, fs))
            s.synchronize()
            repet.release_workspaces()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        assert len(results[k]) == 3
        for r in results[k]:
            same(r, wants[k])


def test_run_device_entry():
    """repet_run_device, the entry a C++ host with its own stream uses, through ctypes."""
    x, fs = golden_input("small_stereo")
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = torch.empty_like(xd)
    s = torch.cuda.current_stream()
    n, c = xd.shape
    rc = _native.lib().repet_run_device(_native.SIM, ctypes.c_void_p(xd.data_ptr()), _native.F64, 1, n, c,
                                        (ctypes.c_int64 * 3)(n * c, c, 1), ctypes.c_void_p(out.data_ptr()), _native.F64,
                                        (ctypes.c_int64 * 3)(n * c, c, 1), repet.derive_params(fs), 0,
                                        ctypes.c_void_p(s.cuda_stream or None))
    _native.check(rc)
    torch.cuda.synchronize()
    same(out, repet.sim(x, fs))


def test_context_round_trip_and_cpu_tensors_unchanged():
    x, fs = golden_input("small_stereo")
    want = repet.original(x, fs)
    same(torch.from_numpy(repet.original(torch.from_numpy(np.ascontiguousarray(x)), fs)), want)   # CPU tensor: NumPy path
    ctx = repet.Context(0)
    ctx.upload_tensor(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    ctx.execute_async("original", repet.derive_params(fs))
    got = ctx.download_tensor()
    torch.cuda.synchronize()
    same(got, want)
    same(torch.from_numpy(ctx.download()), want)
    ctx.close()


def test_second_gpu_follows_the_tensor():
    if _native.lib().repet_device_count() < 2:
        pytest.skip("needs two GPUs")
    x, fs = golden_input("small_stereo")
    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:1")
    repet.set_device(0)
    got = repet.sim(xd, fs)
    assert got.device == torch.device("cuda", 1)
    torch.cuda.synchronize(1)
    same(got, repet.sim(x, fs))


def test_egress_is_ordered_behind_the_callers_stream():
    """What the caller enqueues on its stream between upload and download (here a long sleep, then a write into `out`) comes
    before the egress writes `out`: the result is not overwritten by the fill."""
    x, fs = golden_input("small_stereo")
    want = repet.sim(x, fs)
    ctx = repet.Context(0)
    ctx.upload_tensor(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    ctx.execute_async("sim", repet.derive_params(fs))
    out = torch.empty(x.shape, dtype=torch.float64, device="cuda")
    torch.cuda._sleep(sleep_cycles(100))
    out.fill_(7.0)
    ctx.download_tensor(out)
    torch.cuda.synchronize()
    ctx.close()
    same(out, want)


@pytest.mark.parametrize("dtype", ["f64", "f32", "i16", "float16", "bfloat16"])
@pytest.mark.parametrize("channels", [1, 2])
def test_odd_lengths_and_channels_first_views(dtype, channels):
    """n_samples * n_channels not a multiple of four (the kernels' tail), for every source dtype, read contiguous and through a
    channels-first .T view, and written into float64 and float32 destinations, dense and channels-first."""
    x, fs = golden_input("small_stereo")
    x = np.ascontiguousarray(np.asarray(x)[:127999, :channels])
    if dtype in ("float16", "bfloat16"):
        t = torch.from_numpy(x).to(getattr(torch, dtype))
        xn = t.float().numpy()
    else:
        xn = as_dtype(x, dtype)
        t = torch.from_numpy(xn)
    t = t.cuda()
    for algo in ("sim", "original"):
        want = getattr(repet, algo)(xn, fs)
        same(getattr(repet, algo)(t, fs), want)
        same(getattr(repet, algo)(t.T.contiguous().T, fs), want)
        dense32 = torch.empty(x.shape, dtype=torch.float32, device="cuda")
        same(repet.separate(algo, t, fs, out=dense32), want.astype(np.float32))
        cf64 = torch.empty(x.shape[::-1], dtype=torch.float64, device="cuda")
        repet.separate(algo, t, fs, out=cf64.T)
        same(cf64.T, want)


def test_overlapping_destination_is_refused():
    x, fs = golden_input("small_stereo")
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    with pytest.raises(ValueError):
        repet.separate("sim", xd, fs, out=torch.empty(1, 2, dtype=torch.float64, device="cuda").expand(x.shape[0], 2))
    wide = torch.empty(x.shape[0] + 1, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):                                  # rows that share an element: strides (1, 1)
        repet.separate("sim", xd, fs, out=wide.as_strided(x.shape, (1, 1)))
    same(repet.separate("sim", xd, fs), repet.sim(x, fs))            # and the context is fine afterwards
