"""Many live streams in one streaming handle (``repet.online_streams``): S streams pushed in lockstep through one sequence of
batched launches per push. Every stream's concatenated output is ``repet.simonline`` of its concatenated input and what a
``repet.online`` handle of its own returns -- bit for bit, NaN positions equal -- from host chunks and from ROCm tensors of
every device dtype and layout, with no host wait on device pushes."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet_synth import synth

pytestmark = pytest.mark.gpu


def same(got, want):
    """NaN positions equal and every other value identical."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), f"NaN positions differ: {int(nan_g.sum())} against {int(nan_w.sum())}"
    ok = ~nan_g
    diff = got[ok] != want[ok]
    assert not diff.any(), (f"{int(diff.sum())} of {diff.size} values differ, largest by "
                            f"{float(np.max(np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)))):.3e}")


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


def lockstep_sizes(total, fs, seed):
    """Seeded chunk sizes covering 0, 1, less than a hop, a hop, several hops and more than a buffer."""
    p = repet.derive_params(fs)
    h, b = p.step_length, p.buffer_frames
    rs = np.random.RandomState(seed)
    kinds = [lambda: 0, lambda: 1, lambda: int(rs.randint(2, h)), lambda: h, lambda: h * int(rs.randint(2, 7)),
             lambda: int(rs.randint(h, 6 * h)), lambda: b * h + int(rs.randint(1, 4 * h))]
    sizes = [0, 1, int(rs.randint(2, h)), h, 3 * h, b * h + int(rs.randint(1, 4 * h))]
    while sum(sizes) < total:
        sizes.append(kinds[rs.randint(len(kinds) - 1)]())
    out, pos = [], 0
    for n in sizes:
        n = min(n, total - pos)
        out.append(n)
        pos += n
        if pos == total:
            break
    return out


def run_streams(h, xs, sizes, chunk_of=None):
    """Push xs (S, N, C) in lockstep chunks; check emit_count and that no output runs ahead; the (S, N, C) concatenation."""
    chunk_of = chunk_of or (lambda a, b: xs[:, a:b])
    pieces, pos, emitted = [], 0, 0
    for n in sizes:
        expect = h.emit_count(n)
        got = h.push(chunk_of(pos, pos + n))
        assert tuple(got.shape) == (xs.shape[0], expect, xs.shape[2])
        pos += n
        emitted += expect
        assert emitted <= pos                    # a hop is emitted only once its frame is complete
        pieces.append(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got)
    expect = h.emit_count(0, finishing=True)
    got = h.finish()
    assert got.shape[1] == expect and emitted + expect == pos
    pieces.append(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got)
    h.close()
    return np.concatenate(pieces, axis=1)


def run_single(x, fs, sizes):
    h = repet.online(fs, x.shape[1])
    pieces, pos = [], 0
    for n in sizes:
        pieces.append(h.push(x[pos:pos + n]))
        pos += n
    pieces.append(h.finish())
    h.close()
    return np.concatenate(pieces, axis=0)


def signals(fs, channels, seconds, seeds):
    return np.stack([synth(seconds, fs, channels, s) for s in seeds])


@pytest.mark.parametrize("fs,channels,seconds", [(8000, 1, 13.0), (8000, 2, 12.5), (8000, 3, 11.5), (44100, 2, 11.3)])
def test_lockstep_parity(fs, channels, seconds):
    xs = signals(fs, channels, seconds, [3, 5, 7, 11, 13])
    sizes = lockstep_sizes(xs.shape[1], fs, seed=fs + channels)
    got = run_streams(repet.online_streams(fs, channels, len(xs)), xs, sizes)
    assert got.shape == xs.shape
    for s, x in enumerate(xs):
        same(got[s], repet.simonline(x, fs))
        same(got[s], run_single(x, fs, sizes))


def test_second_level_reads_each_streams_own_samples():
    """float64 streams whose samples are not fp32-exact: one that loops an exact period (ties the fp32 spectra cannot
    settle), and a pair that differ only below the fp32 rounding of the other. A batch-stride error in the second level's
    sample source (it computes float64 spectra from the waveform) would hand one stream another's samples."""
    fs, ch = 8000, 2
    n = int(12.2 * fs)
    base = synth(12.2, fs, ch, 21)
    period = base[:int(1.5 * fs)]
    rs = np.random.RandomState(4)
    centre = np.tile(period, (n // len(period) + 1, 1))[:n].astype(np.float32)
    ulp = np.spacing(np.abs(centre)).astype(np.float64)
    # both round to `centre` in fp32 (a fifth of an ulp either way); only their fp32 remainders differ
    looped = centre.astype(np.float64) + 0.2 * ulp * rs.uniform(-1, 1, size=centre.shape)
    nudged = centre.astype(np.float64) + 0.2 * ulp * rs.uniform(-1, 1, size=centre.shape)
    assert np.array_equal(looped.astype(np.float32), nudged.astype(np.float32)) and not np.array_equal(looped, nudged)
    noisy = base + 1e-7 * rs.standard_normal(base.shape)
    xs = np.stack([noisy, looped, nudged, synth(12.2, fs, ch, 22) * (1 + 1e-8)])
    got = run_streams(repet.online_streams(fs, ch, len(xs)), xs, lockstep_sizes(n, fs, seed=9))
    for s, x in enumerate(xs):
        same(got[s], repet.simonline(x, fs))


DEVICE_DTYPES = {"f64": torch.float64, "f32": torch.float32, "i16": torch.int16, "f16": torch.float16, "bf16": torch.bfloat16}


@pytest.mark.parametrize("dtype", list(DEVICE_DTYPES))
@pytest.mark.parametrize("layout", ["contiguous", "channels_first", "sliced"])
def test_device_chunks_equal_host_chunks(dtype, layout):
    fs, ch, S = 8000, 2, 3
    xs = signals(fs, ch, 11.4, [31, 32, 33])
    if dtype == "i16":
        xs = np.clip(np.round(xs * 20000), -32768, 32767)
    t = torch.tensor(xs, dtype=DEVICE_DTYPES[dtype])
    host = t.numpy() if dtype in ("f64", "f32", "i16") else t.to(torch.float32).numpy()   # f16 / bf16: the exact fp32 values
    dev = torch.device("cuda", 0)
    if layout == "contiguous":
        full = t.to(dev)
    elif layout == "channels_first":
        full = t.permute(0, 2, 1).contiguous().to(dev).permute(0, 2, 1)
    else:                                  # a view into a bigger tensor: every other sample, a stream and a channel off
        big = torch.zeros((S + 1, 2 * xs.shape[1], ch + 1), dtype=t.dtype)
        big[1:, ::2, 1:] = t
        full = big.to(dev)[1:, ::2, 1:]
    sizes = lockstep_sizes(xs.shape[1], fs, seed=77)
    want = run_streams(repet.online_streams(fs, ch, S), host, sizes)
    got = run_streams(repet.online_streams(fs, ch, S), xs, sizes, chunk_of=lambda a, b: full[:, a:b])
    same(got, want)
    if dtype == "f64" and layout == "sliced":
        # a strided float32 destination: the float32 of the same values
        h = repet.online_streams(fs, ch, S)
        pieces, pos = [], 0
        for n in sizes:
            m = h.emit_count(n)
            store = torch.full((S, ch, 2 * m + 1), 7.0, dtype=torch.float32, device=dev)
            out = store[:, :, 1::2].permute(0, 2, 1)
            assert h.push(full[:, pos:pos + n], out=out) is out
            pieces.append(out.cpu().numpy())
            assert torch.all(store[:, :, 0::2] == 7.0)
            pos += n
        out = torch.empty((ch, S, h.emit_count(0, True)), dtype=torch.float32, device=dev).permute(1, 2, 0)
        pieces.append(h.finish(out=out).cpu().numpy())
        h.close()
        same(np.concatenate(pieces, axis=1), want.astype(np.float32))


def test_device_push_does_not_wait_on_the_host():
    fs, ch, S = 8000, 2, 8
    p = repet.derive_params(fs)
    hop = p.step_length
    xs = signals(fs, ch, 12.0, range(40, 48))
    dev = torch.device("cuda", 0)
    full = torch.tensor(xs, device=dev)
    h = repet.online_streams(fs, ch, S, max_push_samples=4 * hop)
    pieces, pos = [], 0

    def push(n):
        nonlocal pos
        pieces.append(h.push(full[:, pos:pos + n]))
        pos += n

    while pos < 11 * fs:                             # past the warm-up: the window is full, every frame is active
        push(fs // 2)
    push(2 * hop)                                    # the warm-up push of the timed size
    torch.cuda.synchronize()
    torch.cuda._sleep(sleep_cycles(100))
    t0 = time.perf_counter()
    push(2 * hop)
    elapsed = time.perf_counter() - t0
    assert elapsed < 0.05, f"the device push took {elapsed * 1e3:.1f} ms behind a 100-ms sleep: it waited on the host"
    torch.cuda.synchronize()
    while pos < xs.shape[1]:
        push(min(fs // 2, xs.shape[1] - pos))
    pieces.append(h.finish())
    h.close()
    got = torch.cat(pieces, dim=1).cpu().numpy()
    for s, x in enumerate(xs):
        same(got[s], repet.simonline(x, fs))


def test_nan_samples_stay_in_their_stream():
    fs, ch = 8000, 2
    xs = signals(fs, ch, 12.0, [51, 52, 53, 54])
    xs[2, 40000:40003, 1] = np.nan
    xs[2, 70001, 0] = np.nan
    sizes = lockstep_sizes(xs.shape[1], fs, seed=5)
    got = run_streams(repet.online_streams(fs, ch, len(xs)), xs, sizes)
    for s, x in enumerate(xs):
        if s == 2:
            assert np.isnan(got[s]).any()
            same(got[s], run_single(x, fs, sizes))
        else:
            same(got[s], repet.simonline(x, fs))


def test_one_stream_equals_online():
    fs, ch = 44100, 2
    x = synth(11.2, fs, ch, 61)
    sizes = lockstep_sizes(len(x), fs, seed=61)
    want = run_single(x, fs, sizes)
    same(run_streams(repet.online_streams(fs, ch, 1), x[None], sizes)[0], want)
    full = torch.tensor(x[None], device="cuda:0")
    same(run_streams(repet.online_streams(fs, ch, 1), x[None], sizes, chunk_of=lambda a, b: full[:, a:b])[0], want)


def test_errors():
    fs = 8000
    h = repet.online_streams(fs, 2, 3)
    dev = torch.device("cuda", 0)
    with pytest.raises(ValueError):
        h.push(np.zeros((100, 2)))                   # rank
    with pytest.raises(ValueError):
        h.push(np.zeros((2, 100, 2)))                # stream count
    with pytest.raises(ValueError):
        h.push(np.zeros((3, 100, 1)))                # channel count
    with pytest.raises(ValueError):
        h.push(torch.zeros((3, 100), device=dev))
    with pytest.raises(ValueError):
        h.push(torch.zeros((4, 100, 2), device=dev))
    with pytest.raises(ValueError):
        h.push(torch.zeros((3, 100, 3), device=dev))
    n = 3000
    m = h.emit_count(n)
    with pytest.raises(ValueError):
        h.push(torch.zeros((3, n, 2), device=dev), out=torch.empty((3, m + 1, 2), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        h.push(torch.zeros((3, n, 2), device=dev), out=torch.empty((3, m, 2), dtype=torch.float64))   # host out
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            h.push(torch.zeros((3, n, 2), device="cuda:1"))
    h.push(np.zeros((3, 5 * fs, 2)))                 # shorter than the 10-s buffer
    with pytest.raises(ValueError):
        h.finish()                                   # as repet.online raises (repet.py:802)
    h.close()


def test_emit_count_arithmetic():
    fs, ch, S = 8000, 1, 2
    p = repet.derive_params(fs)
    W, H, B = p.window_length, p.step_length, p.buffer_frames
    h = repet.online_streams(fs, ch, S)
    total, frames_done = 0, 0
    rs = np.random.RandomState(2)
    for n in [0, 1, W - 2, 1, 1, H - 1, H, 5 * H + 3, B * H, 17, 3 * H]:
        full = (total + n - W) // H + 1 if total + n >= W else 0
        assert h.emit_count(n) == (max(full, frames_done) - frames_done) * H
        got = h.push(rs.standard_normal((S, n, ch)))
        frames_done = max(full, frames_done)
        total += n
    emitted = frames_done * H
    assert h.emit_count(0, finishing=True) == total - emitted
    assert h.finish().shape == (S, total - emitted, ch)
    h.close()


def test_scale_64_stereo_streams_one_hop_at_a_time():
    fs, ch, S = 44100, 2, 64
    hop = repet.derive_params(fs).step_length
    dev = torch.device("cuda", 0)
    clips = torch.stack([torch.tensor(synth(15.0, fs, ch, 100 + s)) for s in range(S)]).to(dev)
    h = repet.online_streams(fs, ch, S, max_push_samples=hop)
    pieces, pos, N = [], 0, clips.shape[1]
    while pos < N:
        n = min(hop, N - pos)
        pieces.append(h.push(clips[:, pos:pos + n]))
        pos += n
    pieces.append(h.finish())
    h.close()
    got = torch.cat(pieces, dim=1)
    same(got, repet.separate("simonline", clips, fs))
