"""The Nyquist bin in the ranked column of bin 1 (csrc/engine_sim.hip: nyquist_column_enabled; RankArgs / MaskArgs::swap_col): on
the bit-sliced path with a cutoff of at least one bin, `sim` builds column 1 of the rank chain from the magnitudes of bin F - 1 --
bin 1's own median is never read, soft_mask is 1 in bins 1 .. cutoff --, the sort, the code planes and the selection carry them
unchanged, mask_from_codes_kernel finishes the Nyquist cell beside bin 1's, and mask_sim_nyquist_kernel is not launched. A median is
a selection and equal magnitudes share a code, so every bar here is equality, bit for bit.

Stage level (repet._mask_stage, median_path "bits+nyquist" against "bits" with parts = 3, which launches the float Nyquist kernel),
stereo and mono F = 129, T = 1100 (11 planes, vs_pitch 1120), a window of 48 frames over the prefill byte, lists of at most 100 and
128 entries with the lengths 0, 1, 2, the odd and even ones below the longest and the longest, cutoff 1 and 5, the mask as a plane
and X in place:
  report      mask_sim_bits_kernel<H, 11>, no Nyquist kernel, the lookups behind the selection
  window      every cell, bins 1 and F - 1 included, equal to the unfolded run's
  elsewhere   rows outside the window, bins F .. FS - 1 and the rows past T hold the prefill (X: the caller's value)
  code words  at bin 1 what np.sort / np.searchsorted give for the NYQUIST column (lower code, upper code, flag); at every other bin
              the unfolded run's
Inputs: the exact-valued ones of tests/test_gpu_select_rounds.py with bin 1 at the level 2^-20 and bin F - 1 at 2^20, each in a
frame order of its own -- the lane that finishes both cells mixing up own value, flag or table is 2^40 off; a second one with
ties (three frames a value) and exact zeros in the Nyquist column.
Pipeline level: repet.sim by default against REPET_NYQUIST_COLUMN=0, each in one child process, on three short clips."""
import os
import subprocess
import sys

import numpy as np
import pytest

import repet
import test_gpu_mask_stages as stages
import test_gpu_select_rounds as rounds

pytestmark = pytest.mark.gpu

F, T, WINDOW = 129, 1100, 48
FRAME0 = T // 2 - 23
FRAME_END = FRAME0 + WINDOW
_inputs = {}
_spectra = {}


def case_input(channels, kind):
    """(1, channels, T, F) fp32, every value exact: rounds.magnitudes with bins 1 and F - 1 replaced."""
    if (channels, kind) not in _inputs:
        V = rounds.magnitudes(T, 9100)[:, :channels].copy()
        rs = np.random.RandomState(9200 + channels + (7 if kind == "ties" else 0))
        for ch in range(channels):
            V[0, ch, :, 1] = np.float32(2.0 ** -20) * (1.0 + rs.permutation(T) / 32768.0)
            j = rs.permutation(T)
            if kind == "ties":
                nyquist = 1.0 + (j // 3) / 32768.0
                nyquist[j % 7 == 0] = 0.0
            else:
                nyquist = 1.0 + j / 32768.0
            V[0, ch, :, F - 1] = np.float32(2.0 ** 20) * nyquist
        assert V.dtype == np.float32
        _inputs[channels, kind] = V
    return _inputs[channels, kind]


def run(V, idx, cnt, max_count, cutoff, want, X, path, parts):
    return repet._mask_stage("sim", V, X, want=want, cutoff=cutoff, prefill=stages.PREFILL, idx=idx, cnt=cnt, max_count=max_count,
                             frame0=FRAME0, frame_end=FRAME_END, parts=parts, median_path=path)


@pytest.mark.parametrize("cutoff", [1, 5])
@pytest.mark.parametrize("max_count", [100, 128])
@pytest.mark.parametrize("channels", [2, 1])
def test_stage_nyquist_column_equals_the_float_kernel(channels, max_count, cutoff):
    idx, cnt = rounds.lists_for(T, max_count, FRAME0, FRAME_END, 9300 + max_count)
    assert {0, 1, 2, max_count - 2, max_count - 1, max_count} <= set(cnt[0, FRAME0:FRAME_END].tolist())
    kernel = "mask_sim_bits_kernel<%d, 11>" % (25 if max_count <= 100 else 32)
    for kind in ("levels", "ties"):
        V = case_input(channels, kind)
        if channels not in _spectra:
            _spectra[channels] = stages.ref.spectra(V.shape, 9400 + channels)
        X = _spectra[channels]
        for want in (("mask",), ("X",)):
            tag = "C=%d n<=%d cutoff=%d %s %s" % (channels, max_count, cutoff, kind, want[0])
            x_in = X if want == ("X",) else None
            got = run(V, idx, cnt, max_count, cutoff, want, x_in, "bits+nyquist", 1)
            old = run(V, idx, cnt, max_count, cutoff, want, x_in, "bits", 3)
            rep = got["launch"]
            assert (rep["kernel"], rep["nyquist"], rep["nyquist_grid"], rep["lookups"]) == (kernel, "", (0, 0, 0), True), (rep, tag)
            assert old["launch"]["kernel"] == kernel and old["launch"]["nyquist"].startswith("mask_sim_nyquist_kernel<"), (old["launch"], tag)
            # every cell the two launches own, and every cell they do not
            if want == ("mask",):
                g, o = stages.bits(got["mask"][0]), stages.bits(old["mask"][0])                  # (channels, rows, FS)
                assert np.array_equal(g, o), "the mask is not the unfolded run's bit for bit: " + tag
                assert np.all(g[:, :FRAME0] == stages.FILL) and np.all(g[:, FRAME_END:] == stages.FILL), "a row outside the window: " + tag
                assert np.all(g[:, :, F:] == stages.FILL), "a pad bin: " + tag
                m = got["mask"][0, :, FRAME0:FRAME_END, :F]
                assert np.all(m[:, :, 1:cutoff + 1] == 1.0), tag
                live = cnt[0, FRAME0:FRAME_END] > 0
                empty = m[:, ~live]                          # np.median of an empty list: NaN outside the high-pass bins
                assert np.all(np.isnan(empty[:, :, 0])) and np.all(np.isnan(empty[:, :, cutoff + 1:])), tag
                assert not np.any(np.isnan(m[:, live][:, :, [0, F - 1]])), tag
                assert np.any(m[:, live, F - 1] < 1.0) and np.any(m[:, live, F - 1] == 1.0), "the Nyquist cells show both cases of the flag: " + tag
                if cutoff == 1:
                    assert np.any(m[:, live, 2] < 1.0), "bin 2 lies outside the cutoff and keeps its median: " + tag
            else:
                g = stages.bits(got["X"][0].view(np.float32))
                assert np.array_equal(g, stages.bits(old["X"][0].view(np.float32))), "X is not the unfolded run's bit for bit: " + tag
                x_before = np.full(got["X"][0].shape, 0, dtype=np.complex64)
                x_before.view(np.uint32)[...] = stages.FILL
                x_before[:, :T, :F] = X[0]
                outside = np.ones(got["X"][0].shape, dtype=bool)
                outside[:, FRAME0:FRAME_END, :F] = False
                assert np.array_equal(g.reshape(got["X"][0].shape + (2,))[outside], stages.bits(x_before.view(np.float32)).reshape(x_before.shape + (2,))[outside]), \
                    "X outside the launch was changed: " + tag
            # the words the selection left
            for ch in range(channels):
                words, unfolded = got["codes"][ch].astype(np.int64), old["codes"][ch].astype(np.int64)
                others = np.r_[0, 2:F - 1]
                assert np.array_equal(words[FRAME0:FRAME_END][:, others], unfolded[FRAME0:FRAME_END][:, others]), "a code word off bin 1: " + tag
                assert np.all(got["codes"][ch, :FRAME0] == stages.FILL) and np.all(got["codes"][ch, FRAME_END:] == stages.FILL), tag
                assert np.all(got["codes"][ch, :, F - 1:] == stages.FILL), tag
                nyquist = V[0, ch, :, F - 1]
                ranks = np.searchsorted(np.sort(nyquist), nyquist, side="left")
                differ = 0
                for r in range(FRAME0, FRAME_END):
                    n = int(cnt[0, r])
                    if n == 0:
                        continue
                    s = np.sort(ranks[idx[0, r, :n]])
                    lower, upper, word = s[(n - 1) // 2], s[n // 2], words[r, 1]
                    assert (word & 0x7fff, word >> 16, (word >> 15) & 1) == (lower, upper, int(lower < ranks[r])), (tag, ch, r, n)
                    differ += word != unfolded[r, 1]
                assert differ > 0, "bin 1's words are its own column's: the Nyquist column was not taken: " + tag


def test_stage_refuses_the_column_without_a_cutoff_or_beside_the_float_kernel():
    V = case_input(1, "levels")
    idx, cnt = rounds.lists_for(T, 100, FRAME0, FRAME_END, 9400)
    with pytest.raises(ValueError):
        run(V, idx, cnt, 100, 0, ("mask",), None, "bits+nyquist", 1)
    with pytest.raises(ValueError):
        run(V, idx, cnt, 100, 1, ("mask",), None, "bits+nyquist", 3)
    with pytest.raises(ValueError):
        run(V, idx, cnt, 100, 1, ("mask",), None, "bits+nyquist", 2)


# ---- repet.sim, default against REPET_NYQUIST_COLUMN=0 ---------------------------------------------------------------------------
CLIPS = ("synth", "groove", "mono8k", "nocut")
CHILD = """
import sys
import numpy as np
sys.path[:0] = [%r, %r]
import repet
from repet_synth import synth, synth_groove
out = {}
def run(name, x, fs):
    p = repet.derive_params(fs)
    c = repet.Context(0)
    c.upload(x)
    c.execute('sim', p)
    out[name + '_y'] = c.download()
    out[name + '_path'] = np.array(c.last_median_path())
    out[name + '_codes'] = c.last_median_codes(p.window_length // 2)[:, :, :3]
    out[name + '_cutoff'] = np.array(p.cutoff_bins)
run('synth', synth(26, 44100, 2, 41), 44100)            # T about 1 120, W = 2048: the mask leaves the lookups as a plane
run('groove', synth_groove(26, 44100, 2, 42), 44100)    # a silent bar: frames without similar frames, NaN
run('mono8k', synth(35, 8000, 1, 43), 8000)             # W = 512, F = 257: X masked in place
repet.cutoff_frequency = 0
run('nocut', synth(26, 44100, 2, 41), 44100)            # no high-pass bins: the column is not taken
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def pipeline_runs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = CHILD % (os.path.join(root, "repet-python_amd"), root)
    runs = {}
    for switch in ("1", "0"):
        out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "repet_nyquist_column_%s_%d.npz" % (switch, os.getpid()))
        subprocess.check_call([sys.executable, "-c", code, out], env=dict(os.environ, REPET_NYQUIST_COLUMN=switch))
        with np.load(out) as z:
            runs[switch] = {k: z[k] for k in z.files}
        os.remove(out)
    return runs


@pytest.mark.parametrize("clip", CLIPS)
def test_sim_with_the_nyquist_column_equals_sim_with_the_float_kernel(pipeline_runs, clip):
    new, old = pipeline_runs["1"], pipeline_runs["0"]
    assert str(new[clip + "_path"]) == "bits" and str(old[clip + "_path"]) == "bits"
    assert new[clip + "_y"].shape == old[clip + "_y"].shape
    assert np.array_equal(new[clip + "_y"], old[clip + "_y"], equal_nan=True), "the backgrounds differ: " + clip
    assert np.array_equal(np.isnan(new[clip + "_y"]), np.isnan(old[clip + "_y"]))
    codes_new, codes_old = new[clip + "_codes"], old[clip + "_codes"]
    assert np.array_equal(codes_new[:, :, [0, 2]], codes_old[:, :, [0, 2]])
    if clip == "nocut":
        assert int(new[clip + "_cutoff"]) == 0
        assert np.array_equal(codes_new[:, :, 1], codes_old[:, :, 1]), "without a cutoff bin 1 keeps its column"
    else:
        assert int(new[clip + "_cutoff"]) >= 1
        assert not np.array_equal(codes_new[:, :, 1], codes_old[:, :, 1]), "bin 1's words did not change: the column was not taken"
