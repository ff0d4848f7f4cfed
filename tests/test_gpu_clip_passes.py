"""Which way a batch went through a variant (``Context.last_clip_passes``; include/repet_hip.h: repet_ctx_last_clip_passes) and
the lists of any clip of a batch whose run kept them (``Context.last_sim_indices(..., clip=)``).

``simonline`` (and ``original`` over equal clips) runs every stage once over all clips of a batch: one pass. ``adaptive``,
``extended`` and every ragged batch but ``simonline``'s work through the clips one after the other: as many passes as clips. The
counter reports it, so that a caller can tell the two apart without a profiler. What ``sim`` does with a batch of EQUAL clips is
not asserted here. 8 kHz throughout (window 512, hop 256); the clips of a batch are different mixtures at different levels."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet import _native
from repet_synth import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 8000
N = 98304                # 385 frames for sim; 73 rows behind simonline's buffer of 312 frames
LEVELS = (1.0, 0.5, 0.8)
_cache = {}


def batch(channels=2):
    if channels not in _cache:
        x = np.stack([LEVELS[b] * synth(N / FS, FS, channels, 21 + b) for b in range(3)])
        _cache[channels] = torch.from_numpy(x).to(DEV)
    return _cache[channels]


def ctx():
    torch.cuda.synchronize()                                     # (the tensor calls do not wait on the host)
    return _native.tensor_context(0)


def test_passes_of_every_variant_over_a_batch():
    x = batch()
    for algo, want in (("simonline", 1), ("original", 1), ("adaptive", 3), ("extended", 3)):
        repet.separate(algo, x, FS)
        assert ctx().last_clip_passes == want, algo
        repet.separate(algo, x[1], FS)                           # a (N, C) call
        assert ctx().last_clip_passes == 1, algo
    repet.separate("sim", x[1], FS)
    assert ctx().last_clip_passes == 1


def test_a_ragged_batch_keeps_the_loop_except_for_simonline():
    x = batch()
    lengths = [N, N - 700, N - 1301]
    for algo, want in (("simonline", 1), ("original", 3), ("sim", 3), ("adaptive", 3)):
        repet.separate(algo, x, FS, lengths=lengths)
        assert ctx().last_clip_passes == want, algo


def test_a_single_clip_has_the_lists_of_clip_0_only():
    x = batch()
    p = repet.derive_params(FS)
    repet.separate("sim", x[2], FS)
    c = ctx()
    t = c.last_frame_count()
    idx, cnt = c.last_sim_indices(t, p.sim_number)
    idx0, cnt0 = c.last_sim_indices(t, p.sim_number, clip=0)
    assert np.array_equal(idx, idx0) and np.array_equal(cnt, cnt0) and int(cnt.max()) > 0
    with pytest.raises(ValueError, match="no lists of that clip"):
        c.last_sim_indices(t, p.sim_number, clip=1)


@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo"])
def test_any_clips_lists_of_a_simonline_batch(channels):
    x = batch(channels)
    p = repet.derive_params(FS)
    repet.separate("simonline", x, FS)
    c = ctx()
    assert c.last_clip_passes == 1
    rows = c.last_frame_count() - p.buffer_frames + 1
    assert rows > 0
    all_idx, all_cnt = c.last_sim_indices(3 * rows, p.sim_number)    # every clip's, back to back (clip 0 takes that too)
    per_clip = [c.last_sim_indices(rows, p.sim_number, clip=b) for b in range(3)]
    for bad in (3, -1):
        with pytest.raises(ValueError, match="no lists of that clip"):
            c.last_sim_indices(rows, p.sim_number, clip=bad)
    with pytest.raises(ValueError, match="shape"):
        c.last_sim_indices(3 * rows, p.sim_number, clip=1)           # with a clip, n_rows is one clip's
    for b in range(3):
        idx, cnt = per_clip[b]
        assert np.array_equal(idx, all_idx[b * rows:(b + 1) * rows]) and np.array_equal(cnt, all_cnt[b * rows:(b + 1) * rows])
        repet.separate("simonline", x[b], FS)
        one_idx, one_cnt = ctx().last_sim_indices(rows, p.sim_number)
        assert np.array_equal(cnt, one_cnt)
        for r in range(rows):
            assert np.array_equal(idx[r, :cnt[r]], one_idx[r, :one_cnt[r]]), (b, r)
    assert not np.array_equal(per_clip[0][0], per_clip[1][0])        # different clips, different lists


def test_context_calls_count_too():
    x = batch()
    p = repet.derive_params(FS)
    c = repet.Context(0)
    try:
        assert c.last_clip_passes == 0                           # nothing has run
        c.upload_tensor(x)
        c.execute("adaptive", p)
        assert c.last_clip_passes == 3
        c.execute_async("simonline", p)
        c.synchronize()
        assert c.last_clip_passes == 1
        c.upload(x[0].cpu().numpy())
        c.execute("sim", p)
        assert c.last_clip_passes == 1
    finally:
        c.close()
