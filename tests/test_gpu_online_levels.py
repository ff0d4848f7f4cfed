"""The level records: per stream and channel the energies and peaks of mixture, background and foreground of an emission, its
live samples and those whose mixture is not finite (``repet.LEVELS``), reduced on the device by one kernel.

Expected values are never taken from the code under test: they are ``levels_reference.levels`` of the SAME run's float64
``which="both"`` outputs and its ``last_emission("mixture")`` (or the input itself, which is fp32-exact here, where a
``finish_stream`` has released the samples) -- the emission kernel's values bit for bit, by the foreground and gain tests.

* Peaks and the two counts must be identical.
* Energies must lie within ``4 * n * 2**-53 * E_want``, ``n`` the live samples of that stream and channel: each side squares
  with one rounding and sums ``n`` non-negative terms in some order, at most about ``n * 2**-53`` relative per side and
  ``2 n * 2**-53`` between them to first order; the factor 4 covers the second-order terms and an fma on one side. Derived,
  not measured; every test prints the largest observed ratio to the bound.
* Every test sees at least one emission with background energy > 0 and foreground energy > 0: none passes on silence.

All at 8 kHz (W = 512, H = 256)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet import _native
from levels_reference import check, levels
from test_gpu_online_streams import lockstep_sizes, same, signals
from test_gpu_online_foreground import pcm_exact, to_numpy

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 8000
GAINS = [0.0, 1.0, 0.25, 10 ** (-12 / 20), 0.5]
CHUNK = _native.LEVEL_CHUNK          # samples of one stream per workgroup of the reduction (REPET_LEVEL_CHUNK)
MIX_E, BG_E, FG_E, MIX_P, BG_P, FG_P, LIVE, BAD = range(8)


def streams_of(channels, seconds, seeds):
    xs = pcm_exact(signals(FS, channels, seconds, seeds))
    return xs[:, :xs.shape[1] - (1 - xs.shape[1] % 2)]                      # an odd length: the finish tail is odd


def hop_and_buffer():
    p = repet.derive_params(FS)
    assert (p.window_length, p.step_length) == (512, 256)
    return p.step_length, p.buffer_frames


class Seen:
    """What a test has checked so far: the largest ratio of an energy's error to its bound, and whether an emission had
    background and foreground energy."""

    def __init__(self):
        self.ratio, self.background, self.foreground, self.records = 0.0, False, False, 0

    def emission(self, h, got, live=None, label="", mixture=None):
        """After an emitting call that returned ``got`` = (background, foreground): its record against the reference."""
        bg, fg = (to_numpy(g) for g in got)
        mix = to_numpy(h.last_emission("mixture")) if mixture is None else mixture
        rec = to_numpy(h.last_levels())
        assert rec.dtype == np.float64 and rec.shape == (bg.shape[0], bg.shape[2], 8)
        want = levels(mix, bg, fg, live)
        self.ratio = max(self.ratio, check(rec, want, label))
        self.background |= bool(np.any(want[..., BG_E] > 0))
        self.foreground |= bool(np.any(want[..., FG_E] > 0))
        self.records += 1
        return rec, want

    def done(self, name):
        print(f"{name}: {self.records} records, largest energy error {self.ratio:.3f} of its bound")
        assert self.background and self.foreground, "no emission with background and foreground energy: the test saw silence"


# ---- 1. every kind of emission ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,seconds", [(1, 13.0), (2, 12.5), (3, 12.2)])
def test_every_kind_of_emission(channels, seconds):
    H, B = hop_and_buffer()
    xs = streams_of(channels, seconds, [3, 5, 7, 11, 13])
    S, N = xs.shape[0], xs.shape[1]
    sizes = lockstep_sizes(N, FS, seed=FS + channels)
    assert N % 2 == 1 and 0 in sizes and 1 in sizes and H in sizes and 3 * H in sizes and max(sizes) > B * H
    h = repet.online_streams(FS, channels, S)
    seen, pos, longest = Seen(), 0, 0
    for n in sizes:
        n_emit = h.emit_count(n)
        got = h.push(xs[:, pos:pos + n], which="both")
        pos += n
        rec, want = seen.emission(h, got, label=f"push of {n}")
        assert (want[..., LIVE] == n_emit).all()
        if n_emit == 0:
            assert rec.shape == (S, channels, 8) and (rec == 0).all()     # a push that emits nothing: all zeros
        longest = max(longest, n_emit)
    # the long chunk: at least three chunks of the kernel with a ragged last one, folded by the second launch
    assert longest >= 3 * CHUNK and longest % CHUNK, (longest, CHUNK)
    tail = h.finish(which="both")
    assert tail[0].shape[1] % 2 == 1 or N % 2 == 0
    rec, want = seen.emission(h, tail, label="finish")
    assert tail[0].shape[1] % 4 and (want[..., LIVE] == tail[0].shape[1]).all()
    again = to_numpy(h.last_levels())
    assert again.tobytes() == rec.tobytes()                                 # a second call: identical bits
    h.close()
    seen.done(f"every kind of emission, C = {channels}")


# ---- 2. gain and fade --------------------------------------------------------------------------------------------------------------
def test_gain_and_fade():
    H, B = hop_and_buffer()
    xs = streams_of(2, 12.3, [14, 15, 16, 17, 18])
    S, N = xs.shape[0], xs.shape[1]
    sizes = [(B + 9) * H + 5, 3 * H - 5, 2 * H, 7 * H + 2]
    sizes.append(N - sum(sizes))
    g1 = [0.5, 1.0, 0.75, 0.0, 10 ** (-12 / 20)]
    change_before = 2                                                      # the push of 2 H samples fades slots 0, 2, 3 and 4
    h, twin = repet.online_streams(FS, 2, S), repet.online_streams(FS, 2, S)
    h.set_background_gain(GAINS, slots=range(S))
    seen, pos, faded = Seen(), 0, None
    for k, n in enumerate(sizes + [None]):
        if k == change_before:
            h.set_background_gain(g1, slots=range(S))
        got = h.finish(which="both") if n is None else h.push(xs[:, pos:pos + n], which="both")
        plain = twin.finish(which="both") if n is None else twin.push(xs[:, pos:pos + n], which="both")
        pos += n or 0
        rec, want = seen.emission(h, got, label=f"call {k}")                # fields 2 and 5 follow the (faded) foreground returned
        rec_twin, _ = Seen().emission(twin, plain, label=f"twin call {k}")
        # background and mixture fields, the counts: those of a handle that never set a gain, bit for bit
        for f in (MIX_E, BG_E, MIX_P, BG_P, LIVE, BAD):
            same(rec[..., f], rec_twin[..., f])
        same(rec[1][..., [FG_E, FG_P]], rec[1][..., [MIX_E, MIX_P]])        # g = 1: the foreground is the mixture
        if k == change_before:
            assert got[0].shape[1] == 2 * H
            faded = (rec, rec_twin, to_numpy(got[0]))
    rec, rec_twin, bg = faded
    assert np.any(bg[:, :H])                                                # the fade had a background to weigh
    assert np.any(rec[2][..., FG_E] != rec_twin[2][..., FG_E])              # 0.25 -> 0.75: not the plain foreground's energy
    h.close()
    twin.close()
    seen.done("gain and fade")


# ---- 3. slots ----------------------------------------------------------------------------------------------------------------------
def test_slots_idle_restarted_and_finished():
    H, B = hop_and_buffer()
    C, S = 2, 4
    xs = streams_of(C, 12.1, [21, 22, 23, 24])
    xs[1] = np.nan                                                          # slot 1 stays idle: its share of every chunk is NaN
    h = repet.online_streams(FS, C, S, start_length=1.0)
    M = h.start_frames
    assert 2 < M < B
    h.release(range(S))
    begun = {}                                                             # slot -> handle sample of its restart
    seen, pos, emitted = Seen(), 0, 0
    hops = [4, 1, 1, 3, 1, 1, 2, M + 40, 5]
    restart_before = {1: 0, 4: 2}                                          # push index -> slot restarted in front of it
    per_push = []
    for k, nh in enumerate(hops):
        if k in restart_before:
            h.restart([restart_before[k]])
            begun[restart_before[k]] = pos
        n = nh * H
        got = h.push(xs[:, pos:pos + n], which="both")
        pos += n
        n_emit = got[0].shape[1]
        at = emitted + np.arange(n_emit)
        live = np.stack([at >= begun[s] if s in begun else np.zeros(n_emit, dtype=bool) for s in range(S)])
        rec, want = seen.emission(h, got, live, label=f"push {k}")
        per_push.append(rec)
        emitted += n_emit
        for s in range(S):
            if s not in begun:
                assert (rec[s] == 0).all()                                  # an idle slot: eight zeros, NaN in its share or not
    assert np.isnan(xs[1]).all()
    # the first hop after a restart lies before the slot's own stream: zeros, nothing live; from the next hop on, all of it
    assert (per_push[1][0] == 0).all() and (per_push[2][0][:, LIVE] == H).all() and (per_push[3][0][:, LIVE] == 3 * H).all()
    assert (per_push[4][2] == 0).all() and (per_push[5][2][:, LIVE] == H).all()
    # slot 0 warms up for M - 1 frames: no background yet, the foreground is the mixture
    assert (per_push[2][0][:, BG_E] == 0).all() and (per_push[2][0][:, MIX_E] > 0).all()
    same(per_push[2][0][:, [FG_E, FG_P]], per_push[2][0][:, [MIX_E, MIX_P]])
    # finish_stream: the record of that one slot's tail, (C, 8); the mixture is the slot's own input (fp32-exact: bit for bit)
    n_rest = h.stream_emit_count(0)
    tail = h.finish_stream(0, which="both")
    rec = h.last_levels()
    assert rec.shape == (C, 8) and rec.dtype == np.float64
    mix = xs[0, pos - n_rest:pos]
    want = levels(mix[None], tail[0][None], tail[1][None])[0]
    seen.ratio = max(seen.ratio, check(rec, want, "finish_stream"))
    assert (want[:, LIVE] == n_rest).all() and (want[:, BG_E] > 0).all()
    assert h.last_levels().tobytes() == rec.tobytes()
    h.restart([3])
    with pytest.raises(ValueError, match="stale"):
        h.last_levels()
    h.close()
    seen.done("slots")


# ---- 4. NaN and inf ----------------------------------------------------------------------------------------------------------------
def test_a_nan_sample_and_an_inf_sample_in_one_live_slot():
    H, B = hop_and_buffer()
    C, S = 2, 3
    xs = streams_of(C, 12.4, [31, 32, 33]).copy()
    first = (B + 6) * H
    bad_at = first + 2 * H + 7                       # inside the push that follows the first one, and inside what that push emits
    xs[1, bad_at, 0] = np.nan
    xs[1, bad_at + 3, 1] = np.inf
    assert repet.strict_reference
    h = repet.online_streams(FS, C, S)
    seen, pos, emitted, found = Seen(), 0, 0, 0
    for n in (first, 4 * H, 3 * H):
        got = h.push(xs[:, pos:pos + n], which="both")
        pos += n
        rec, want = seen.emission(h, got, label=f"push of {n}")
        n_emit = got[0].shape[1]
        mix = to_numpy(h.last_emission("mixture"))
        inside = emitted <= bad_at < emitted + n_emit
        emitted += n_emit
        bad = ~np.isfinite(mix)
        same(rec[..., BAD], bad.sum(axis=1).astype(np.float64))             # exactly the bad mixture samples of this emission
        assert (rec[[0, 2]][..., BAD] == 0).all() and np.isfinite(rec[[0, 2]]).all()      # the other slots: unaffected
        assert (rec[[0, 2]][..., BG_E] > 0).all() or not inside
        if inside:
            found += 1
            assert n == 4 * H and rec[1, :, BAD].tolist() == [1, 1]
            assert np.isnan(rec[1, 0, MIX_E]) and np.isnan(rec[1, 0, FG_E])
            assert rec[1, 1, MIX_E] == np.inf and not np.isfinite(rec[1, 1, FG_E])
            finite = np.where(np.isfinite(mix[1, :, 0]), np.abs(mix[1, :, 0]), 0.0)
            assert rec[1, 0, MIX_P] == finite.max() > 0                     # the largest finite |mix|
            assert rec[1, 1, MIX_P] == np.inf
        else:
            assert (rec[1][:, BAD] == 0).all()
    assert found == 1
    h.close()
    seen.done("NaN and inf")


# ---- 5. the device path ------------------------------------------------------------------------------------------------------------
def test_device_chunks_float32_views_and_a_young_stream():
    H, B = hop_and_buffer()
    C, S = 2, 3
    xs = streams_of(C, 12.2, [41, 42, 43])[:, :80 * H + 77]
    full = torch.tensor(xs, dtype=torch.float32, device=DEV)
    assert np.array_equal(to_numpy(full).astype(np.float64), xs)            # the same values, so the same float64 signals
    h = repet.online_streams(FS, C, S, start_length=1.0)
    twin = repet.online_streams(FS, C, S, start_length=1.0)
    M = h.start_frames
    sizes = [3 * H + 1, 20 * H - 1, 5 * H, 26 * H + 9, 2 * H]
    assert M == 31 and sum(sizes) < xs.shape[1]
    sizes.append(xs.shape[1] - sum(sizes))
    seen, pos, emitted, young = Seen(), 0, 0, 0
    for n in sizes + [None]:
        m = h.emit_count(0, True) if n is None else h.emit_count(n)
        store = torch.full((2, S, m, 2 * C), 7.0, dtype=torch.float32, device=DEV)
        out = (store[0, :, :, ::2], store[1, :, :, ::2])
        if n is None:
            h.finish(out=out, which="both")
            got = twin.finish(which="both")
        else:
            h.push(full[:, pos:pos + n], out=out, which="both")
            got = twin.push(xs[:, pos:pos + n], which="both")
            pos += n
        rec = h.last_levels()
        assert isinstance(rec, torch.Tensor) and rec.dtype == torch.float64 and rec.device == torch.device(DEV)
        assert tuple(rec.shape) == (S, C, 8) and rec.is_contiguous()
        rec_twin, want = seen.emission(twin, got, label=f"call of {n}")
        assert isinstance(rec_twin, np.ndarray)
        # the record does not depend on the destination dtype, nor on the form that returns it
        assert to_numpy(rec).tobytes() == rec_twin.tobytes()
        filled = torch.full((S, C, 8), 7.0, dtype=torch.float64, device=DEV)
        assert h.last_levels(out=filled) is filled and to_numpy(filled).tobytes() == rec_twin.tobytes()
        same(to_numpy(out[0]), to_numpy(got[0]).astype(np.float32))
        if m > 0 and emitted + m <= (M - 1) * H:
            # every emitted sample belongs to a frame younger than start_frames: no background, the foreground is the mixture
            young += 1
            assert (rec_twin[..., BG_E] == 0).all() and (rec_twin[..., MIX_E] > 0).all()
            same(rec_twin[..., [FG_E, FG_P]], rec_twin[..., [MIX_E, MIX_P]])
        emitted += m
        if n == 5 * H:
            for bad in (torch.empty((S, C, 8), dtype=torch.float32, device=DEV), torch.empty((S, C, 4), dtype=torch.float64, device=DEV),
                        torch.empty((C, 8), dtype=torch.float64, device=DEV), torch.empty((S, C, 8), dtype=torch.float64),
                        torch.empty((S, C, 16), dtype=torch.float64, device=DEV)[:, :, ::2]):
                with pytest.raises(ValueError):
                    h.last_levels(out=bad)
    assert young >= 2
    h.close()
    twin.close()
    seen.done("device path")


# ---- 6. tensor calls ---------------------------------------------------------------------------------------------------------------
def tensor_case(x, name):
    both, rec = repet.separate("sim", x, FS, which="both", background_gain=0.25, levels=True)
    assert isinstance(both, tuple) and len(both) == 2
    batch = x.dim() == 3
    assert rec.dtype == torch.float64 and rec.device == x.device and tuple(rec.shape) == tuple(x.shape[:-2]) + (x.shape[-1], 8)
    mix, rec_mix = repet.separate("sim", x, FS, which="mixture", levels=True)
    plain = repet.separate("sim", x, FS, which="both", background_gain=0.25)
    assert isinstance(plain, tuple) and len(plain) == 2 and isinstance(plain[0], torch.Tensor)      # levels=False: as ever
    same(plain[0], both[0])
    same(plain[1], both[1])
    as3 = (lambda t: to_numpy(t)) if batch else (lambda t: to_numpy(t)[None])
    want = levels(as3(mix), as3(both[0]), as3(both[1]))
    ratio = check(as3(rec), want, name)
    # the second call set no gain: its foreground is the plain one, everything else the same record
    want_plain = levels(as3(mix), as3(both[0]), as3(mix) - as3(both[0]))
    ratio = max(ratio, check(as3(rec_mix), want_plain, name + " (mixture call)"))
    for f in (MIX_E, BG_E, MIX_P, BG_P, LIVE, BAD):
        same(as3(rec)[..., f], as3(rec_mix)[..., f])
    assert (want[..., LIVE] == x.shape[-2]).all() and (want[..., BAD] == 0).all()
    assert (want[..., BG_E] > 0).all() and (want[..., FG_E] > 0).all()
    again = repet.separate("sim", x, FS, which="both", background_gain=0.25, levels=True)[1]
    assert to_numpy(again).tobytes() == to_numpy(rec).tobytes()
    print(f"{name}: largest energy error {ratio:.3f} of its bound")


def test_tensor_calls():
    N = 4 * FS - 1
    assert N % 2 == 1 and N >= 3 * CHUNK and N % CHUNK
    x = pcm_exact(signals(FS, 2, 4.0, [51]))[0][:N]
    tensor_case(torch.tensor(x, dtype=torch.float64, device=DEV), "(N, 2)")
    xb = pcm_exact(signals(FS, 1, 4.0, [52, 53]))[:, :N]
    tensor_case(torch.tensor(xb, dtype=torch.float32, device=DEV), "(2, N, 1)")
    short = pcm_exact(signals(FS, 2, 1.0, [54]))[0][:CHUNK - 1]
    assert short.shape[0] == CHUNK - 1
    tensor_case(torch.tensor(short, dtype=torch.float64, device=DEV), "a clip shorter than one chunk")
