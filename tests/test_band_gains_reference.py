"""tests/band_gains_reference.py against tests/frames_reference.py, its own algebra, and the sensitivity conditions of the GPU
test (tests/test_gpu_online_band_gains.py): every table that file uses must, on the signal it is used on, move the shaped
background far enough from the plain one -- and far enough from the same table one bin off -- that the GPU test's bar tells a
right kernel from a wrong one. The bar's floor term is ``2**-22 * max |bg|``; the conditions are 100 x and 10 x that, in rms over
the separated part of the stream, on the float64 model alone."""
import functools

import numpy as np
import pytest

from band_gains_cases import B, F, FS, FS44, H, M_YOUNG, N8, TABLES, USES, signal
from band_gains_reference import band_gains_from, factor, masks_of, shaped_from, table
from frames_reference import frames_from

N_SHORT = (M_YOUNG + 24) * H + 77


@functools.lru_cache(maxsize=None)
def state(seed, n, fs, ch, m):
    return masks_of(np.array(signal(seed, n, fs, ch)), fs, m)


def rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


def test_factor_is_the_scalar_gains_rule():
    g = np.array([0.0, 1.0, 0.25, 10 ** (-12 / 20), 0.5, 1e-9])
    a = factor(g)
    assert a.dtype == np.float64 and np.array_equal(a, a.astype(np.float32).astype(np.float64))
    assert a[0] == 1.0 and a[1] == 0.0 and a[2] == 0.75
    assert np.array_equal(a, [float(np.float32(1.0 - np.float64(np.float32(v)))) for v in g])


def test_ones_are_the_plain_background_and_the_frames_statement():
    x = np.array(signal(31, N_SHORT, FS, 2))
    t = state(31, N_SHORT, FS, 2, M_YOUNG)["t"]
    bg, shaped = band_gains_from(x, FS, M_YOUNG, np.ones((t, F)))
    assert bg.tobytes() == shaped.tobytes()
    want = frames_from(x, FS, M_YOUNG)[0]
    assert bg.tobytes() == want.tobytes() and np.any(bg)
    assert not bg[:(M_YOUNG - 1) * H].any()


def test_zeros_remove_everything():
    st = state(31, N_SHORT, FS, 2, M_YOUNG)
    bg, shaped = shaped_from(st, np.zeros((st["t"], F)))
    assert np.any(bg) and not shaped.any()


def test_complementary_tables_add_up():
    st = state(31, N_SHORT, FS, 2, M_YOUNG)
    rs = np.random.RandomState(3)
    a = rs.uniform(0, 1, size=(st["t"], F))
    bg, one = shaped_from(st, a)
    _, other = shaped_from(st, 1.0 - a)
    assert np.max(np.abs(one + other - bg)) <= 1e-12 * np.max(np.abs(bg))


def test_table_restates_the_edges_rule():
    g = table(F, *TABLES["one-bin"])
    assert g.dtype == np.float32 and g[12] == 1.0 and g[13] == 0.25 and not g[:12].any() and not g[14:].any()
    g = table(F, *TABLES["speech-only"])
    assert g[:19].all() and not g[19:218].any() and g[218:].all()
    assert np.array_equal(table(F, *TABLES["per-bin"]), np.float32(TABLES["per-bin"][1]))
    edges = TABLES["mel44"][0]
    assert len(edges) == 25 and edges[0] == 0 and edges[-1] == 1025 and list(edges) == sorted(edges)


@pytest.mark.parametrize("use", USES, ids=lambda u: f"{u[0]}-seed{u[1]}-{u[3]}Hz-C{u[4]}")
def test_sensitivity(use):
    name, seed, n, fs, ch, m = use
    st = state(seed, n, fs, ch, m)
    f, t, h = st["f"], st["t"], st["h"]
    g = table(f, *TABLES[name])
    a = factor(g)
    bg, shaped = shaped_from(st, np.tile(a, (t, 1)))
    part = slice((m - 1) * h, None)
    floor = 2.0 ** -22 * float(np.max(np.abs(bg)))
    moved = rms((shaped - bg)[part])
    shifted = np.concatenate(([a[0]], a[:-1]))                 # the same table one bin up
    _, off = shaped_from(st, np.tile(shifted, (t, 1)))
    told = rms((off - shaped)[part])
    print(f"{name}: rms(shaped - bg) = {moved / floor:.0f} floors, one bin off = {told / floor:.0f} floors")
    assert moved >= 100 * floor, (moved, floor)
    assert told >= 10 * floor, (told, floor)
