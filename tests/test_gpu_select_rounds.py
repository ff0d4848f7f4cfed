"""The last round of the bit-sliced selection (csrc/mask_bits.hip: the descent's round on plane 0, which fetches no further plane)
through repet._mask_stage, in every instantiation of mask_sim_bits_kernel: 11 .. 15 planes x lists of at most 100 (H = 25) and 128
(H = 32) entries, stereo F = 129 (four blocks of 64 bins, the smallest layout the path takes). The launch, its report, the mask
bars and the untouched cells are checked by the helpers of tests/test_gpu_mask_stages.py against tests/mask_reference.py; on top:
  code words  lower code, upper code and flag bit equal to what np.sort / np.searchsorted give, for every row of the window
  mask        the bit-sliced path's plane equal to the float kernel's on the same input, bit for bit
Inputs in which plane 0 decides: the even bins of a channel hold one increasing function of the frame index (so a frame's rank
code there is its index) and a list is a run of consecutive frames placed so that its lower median is the frame's neighbour
t ^ 1; the odd bins hold shuffled values. Before anything runs on the GPU, NumPy counts on the checked window itself the cells
  a  whose lower and upper median codes differ in bit 0 only,
  b  whose lower median code is the frame's own code with bit 0 cleared (the borrow of `need` starts at plane 0 and stays),
  c  whose lower median code is the frame's own code with bit 0 set (no borrow),
and each class must hold at least one cell in fifty. T above 2 050: a window of 48 frames; the rows outside keep the prefill."""
import numpy as np
import pytest

import mask_reference as ref
import test_gpu_mask_stages as stages

pytestmark = pytest.mark.gpu

F, CHANNELS, WINDOW = 129, 2, 48
FRAMES = (1100, 2050, 4100, 8200, 16400)           # 11, 12, 13, 14, 15 planes
COUNTS = (100, 128)                                # H = 25, H = 32
_inputs = {}


def magnitudes(t, seed):
    """(1, 2, T, F) fp32, every value exact: bin f at a level 2^e(f); even bins below the Nyquist bin level * (1 + t / 2^15),
    increasing with the frame; the others level * (1 + j / 2^15) with j a permutation of the frames (all distinct: T <= 2^15)."""
    assert t <= 1 << 15
    rs = np.random.RandomState(seed)
    out = np.empty((1, CHANNELS, t, F), dtype=np.float64)
    ramp = 1.0 + np.arange(t) / 32768.0
    for ch in range(CHANNELS):
        level = np.exp2(rs.permutation(np.round(np.linspace(-40, 40, F))))
        for k in range(F):
            out[0, ch, :, k] = level[k] * (ramp if k % 2 == 0 and k < F - 1 else ramp[rs.permutation(t)])
    v = out.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), out)
    return v


def rank_codes(v):
    """v (T, n_cols) -> the codes of rank.hip: the number of smaller values of the column."""
    return np.stack([np.searchsorted(np.sort(v[:, k]), v[:, k], side="left") for k in range(v.shape[1])], axis=1)


def case_input(t):
    if t not in _inputs:
        V = magnitudes(t, 7000 + t)
        _inputs[t] = (V, [rank_codes(V[0, ch, :, :F - 1]) for ch in range(CHANNELS)])
    return _inputs[t]


def lists_for(t, max_count, frame0, frame_end, seed):
    """idx (1, T, max_count), cnt (1, T). Row r of the window: cnt[r] consecutive frames whose lower median is frame r ^ 1 (moved
    inside [0, T) at the clip's ends); the entries past the list's end are valid frames far from it. The lengths: 0, 1, 2, the
    odd and the even length below the longest, the longest, then random ones. Rows outside the window: their own frame."""
    rs = np.random.RandomState(seed)
    rows = np.arange(frame0, frame_end)
    lengths = np.concatenate(([0, 1, 2, max_count - 1, max_count - 2, max_count], rs.randint(1, max_count + 1, size=len(rows) - 6)))
    lengths[6:] += (lengths[6:] < max_count) & (rs.rand(len(rows) - 6) < 0.5) & (lengths[6:] % 2 == 1)     # (more even lists than odd ones)
    cnt = np.ones((1, t), dtype=np.int32)
    idx = np.tile(np.arange(t, dtype=np.int32)[None, :, None], (1, 1, max_count))
    for r, n in zip(rows[rs.permutation(len(rows))], lengths):
        n = int(n)
        first = min(max((r ^ 1) - (n - 1) // 2, 0), t - max_count)
        cnt[0, r] = n
        idx[0, r] = (first + np.arange(max_count)) % t
        idx[0, r, n:] = (r + t // 2 + np.arange(max_count - n)) % t
        idx[0, r, :n] = rs.permutation(idx[0, r, :n])
    return idx, cnt


def plane0_shares(ranks, idx, cnt, frame0, frame_end):
    """The shares of the window's cells in the classes a, b, c of the module's docstring."""
    a = b = c = total = 0
    for codes in ranks:
        for r in range(frame0, frame_end):
            n = int(cnt[0, r])
            total += codes.shape[1]
            if n == 0:
                continue
            s = np.sort(codes[idx[0, r, :n]], axis=0)
            lower, upper, own = s[(n - 1) // 2], s[n // 2], codes[r]
            a += np.count_nonzero((lower ^ upper) == 1)
            b += np.count_nonzero(((lower ^ own) == 1) & (lower < own))
            c += np.count_nonzero(((lower ^ own) == 1) & (lower > own))
    return a / total, b / total, c / total


def window_refs(V, idx, cnt, frame0, frame_end):
    """(mask float64, exactly one) per channel as ref.reference_sim gives them, for the rows of the window only (NaN elsewhere)."""
    t = V.shape[2]
    refs = []
    for ch in range(CHANNELS):
        v = V[0, ch]
        model = ref.model_sim(v, ref.lists_of(idx[0, frame0:frame_end], cnt[0, frame0:frame_end]))
        m, one = np.full((t, F), np.nan), np.zeros((t, F), dtype=bool)
        m[frame0:frame_end], one[frame0:frame_end] = ref.mask_of(v[frame0:frame_end], model)
        refs.append((m, one))
    return [refs]


@pytest.mark.parametrize("max_count", COUNTS)
@pytest.mark.parametrize("t", FRAMES)
def test_last_round_every_instantiation(t, max_count):
    frame0, frame_end = (0, t) if t <= 2050 else (t // 2 - 23, t // 2 - 23 + WINDOW)
    V, ranks = case_input(t)
    idx, cnt = lists_for(t, max_count, frame0, frame_end, 7100 + t + max_count)
    window = cnt[0, frame0:frame_end]
    assert {0, 1, 2, max_count - 2, max_count - 1, max_count} <= set(window.tolist())
    shares = plane0_shares(ranks, idx, cnt, frame0, frame_end)
    print("T=%d n<=%d rows [%d, %d): bit 0 alone parts the medians in %.3f of the cells, the lower median from the frame's own "
          "code in %.3f (below it) and %.3f (above it)" % ((t, max_count, frame0, frame_end) + shares))
    assert min(shares) >= 1 / 50, shares
    refs = window_refs(V, idx, cnt, frame0, frame_end)
    kw = dict(frame0=frame0, frame_end=0 if frame_end == t else frame_end)
    flt, _ = stages.run_sim(V, idx, cnt, max_count, refs, **kw)
    got, _ = stages.run_sim(V, idx, cnt, max_count, refs, path="bits", **kw)
    planes = max(11, int(t - 1).bit_length())
    assert got["launch"]["kernel"] == "mask_sim_bits_kernel<%d, %d>" % (25 if max_count <= 100 else 32, planes)
    assert np.array_equal(stages.bits(got["mask"]), stages.bits(flt["mask"])), "the mask is not the float kernel's bit for bit"
    for ch in range(CHANNELS):
        codes = got["codes"][ch].astype(np.int64)
        for r in range(frame0, frame_end):
            n = int(cnt[0, r])
            if n == 0:
                continue
            s = np.sort(ranks[ch][idx[0, r, :n]], axis=0)
            lower, upper = s[(n - 1) // 2], s[n // 2]
            word = codes[r, :F - 1]
            assert np.array_equal(word & 0x7fff, lower) and np.array_equal(word >> 16, upper), (ch, r, n)
            assert np.array_equal((word >> 15) & 1, (lower < ranks[ch][r]).astype(np.int64)), (ch, r, n)
        assert np.all(got["codes"][ch, :frame0] == stages.FILL) and np.all(got["codes"][ch, frame_end:] == stages.FILL)
        assert np.all(got["codes"][ch, :, F - 1:] == stages.FILL)
