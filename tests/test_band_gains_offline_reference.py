"""CPU tier of the tensor calls' band gains: the float64 model of tests/band_gains_offline_reference.py against the oracle, and
the sensitivity condition of every case tests/test_gpu_tensor_band_gains.py compares with it.

Sensitivity: for every (variant, signal, table) bar the table ``all`` the shaped background differs from the plain one by at
least 1e-3 rms -- ten times RMS_TOL, so a library that ignored the table could not pass the GPU comparison. The condition is the
issue's; a case that missed it would get another table, never another condition."""
import numpy as np
import pytest

from oracle import repet_oracle as orc

import band_gains_offline_reference as model
import band_gains_reference as bgr

SENSITIVITY = 1e-3


@pytest.mark.parametrize("algo", model.ALGOS)
def test_factor_one_is_the_oracles_background_bit_for_bit(algo):
    x, fs = model.row_signal("8k-stereo")
    got = model.shaped_background(algo, x, fs, np.ones(model.bins(fs)))
    assert np.array_equal(got, model.plain_of("8k-stereo", algo))
    assert orc.resynthesize.__module__ == orc.__name__ and orc.resynthesize.__name__ == "resynthesize"      # put back


def test_the_simonline_models_plain_background_is_the_oracles():
    x, fs = model.row_signal("8k-stereo")
    t = bgr.frame_count(len(x), fs)
    bg, shaped = bgr.band_gains_from(x, fs, model.buffer_frames(fs), np.ones((t, model.bins(fs))))
    assert np.array_equal(bg, orc.simonline(x, fs)) and np.array_equal(shaped, bg)


def test_the_rows_are_what_the_issue_lists():
    assert len(model.USES) == 30 + 4 + 10 + 2 + 2 + 1
    for name, fs, seconds, ch, _, _, _ in model.ROWS:
        x, _ = model.row_signal(name)
        assert x.shape == (round(seconds * fs) + 77, ch)
        assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    x, fs = model.row_signal("8k-stereo")
    assert len(orc.extended_plan(len(x), fs, orc.Params())[0]) == 3
    x, fs = model.row_signal("44k-stereo")
    assert len(orc.extended_plan(len(x), fs, orc.Params())[0]) == 2
    assert [orc.stft_geometry(row[1])[0] for row in model.ROWS] == [512, 512, 2048, 1024, 4096, 2048]
    assert "one-bin44" not in {u[2] for u in model.USES}


@pytest.mark.parametrize("name,algo,table", model.USES, ids=["-".join(u) for u in model.USES])
def test_every_use_moves_the_background(name, algo, table):
    _, fs = model.row_signal(name)
    g = model.table_gains(table, fs)
    assert g.shape == (model.bins(fs),) and np.all((g >= 0) & (g <= 1)) and np.any(g != 0)
    plain, shaped = model.plain_of(name, algo), model.shaped_of(name, algo, table)
    assert shaped.shape == plain.shape and np.all(np.isfinite(shaped))
    moved = model.rms(shaped - plain)
    print(f"{name} {algo} {table}: rms(shaped - plain) = {moved:.3e}")
    if table == "all":
        assert model.rms(shaped) == 0.0             # a = 0 on every bin: nothing of the background is taken away
    else:
        assert moved >= SENSITIVITY
