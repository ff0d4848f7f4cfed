"""CPU checks of tests/peaks_reference.py: the float64 statement of the peak picking against the oracle (mode 0: ``orc.indices``
on ``orc.selfsimilaritymatrix``; modes 1 and 2: the ``similarity_vectors`` trace of ``orc.simonline``; filling rows:
tests/simonline_start_reference.py), ``unit64`` against a direct DFT in np.longdouble at the bar the kernels are held to, and
EVERY case of tests/test_gpu_peaks_stages.py built with its premises asserted, so that the GPU test never runs on an input
for which equality with the float64 lists is not a theorem."""
from types import SimpleNamespace

import numpy as np
import pytest

import peaks_reference as pr
import simonline_start_reference as start_ref
from oracle import repet_oracle as orc


def _clip(n, ch, seed):
    rng = np.random.RandomState(seed)
    t = np.arange(n)[:, None]
    x = 0.2 * rng.standard_normal((n, ch))
    for _ in range(12):
        x += rng.uniform(0.02, 0.1) * np.sin(2 * np.pi * rng.uniform(0.002, 0.4) * t + rng.uniform(0, 6.28, (1, ch))) * (1 + np.sin(t * rng.uniform(1e-4, 3e-3)))
    return x / np.max(np.abs(x)) * 0.9


@pytest.mark.parametrize("W, C", [(256, 1), (256, 3), (2048, 2), (4096, 2)])
def test_unit64_is_inside_the_bar_of_a_longdouble_dft(W, C):
    """A handful of frames per W -- the first and the last partly outside the signal, one silent -- against the direct DFT in
    np.longdouble: 2-norm and per-component error <= 16 log2(W) 2^-53, the bar of the kernels' float64 spectra."""
    H, n_frames = W // 2, 7
    hi = pr.make_audio(n_frames, W, C, 5, frame_sample0=-H)
    lo = pr.Planter.twin_plane(hi, 9)
    hi[2 * H:4 * H] = 0.0
    lo[2 * H:4 * H] = 0.0                                             # frame 3 (samples 2 H .. 4 H) is silent
    got = pr.unit64(hi, lo, W, H, -H, n_frames)
    frames = pr.frame_samples(hi, lo, W, H, -H, n_frames)
    assert np.all(frames[0, :H] == 0) and np.all(frames[-1, H:] == 0) and np.any(frames[0, H:] != 0)
    assert np.all(np.isnan(got[3])) and not np.any(np.isnan(np.delete(got, 3, axis=0)))
    pick = [0, 1, 4, n_frames - 1]
    want = pr.unit_longdouble(frames[pick], W)
    err = got[pick].astype(np.longdouble) - want
    bar = pr.fft_bar(W)
    assert float(np.max(np.sqrt(np.sum(err * err, axis=1)))) <= bar, (float(np.max(np.sqrt(np.sum(err * err, axis=1)))), bar)
    assert float(np.max(np.abs(err))) <= bar


def test_identical_frames_are_one_class_and_get_one_value():
    W, H = 256, 128
    hi = pr.make_audio(40, W, 2, 3)
    pl = pr.Planter(hi, W, 0, True)
    pl.copy(20, 5)
    pl.copy(30, 5, twin=4)
    sp = pr.Spectra(hi, pl.lo, W, 0, 40)
    assert sp.cls2[20] == sp.cls2[5] != sp.cls2[30] and sp.cls1[20] == sp.cls1[5] == sp.cls1[30]
    assert np.array_equal(sp.unit32[30], sp.unit32[5]) and not np.array_equal(sp.unit64[30], sp.unit64[5])
    e2 = sp.e2(9, np.arange(40))
    e1 = sp.e1(9, np.arange(40))
    assert e2[20] == e2[5] and e1[30] == e1[5] and e2[30] != e2[5] and abs(e2[30] - e2[5]) < 1e-7


def test_mode_0_against_the_oracles_indices():
    """e2 rows and their lists against orc.sim's similarity matrix and orc.indices (centred frames, two channels)."""
    fs = 8000
    x = _clip(9000, 2, 1)
    p = orc.Params(similarity_distance=0.16, similarity_number=7, similarity_threshold=0.6)
    tr = orc.Trace()
    orc.sim(x, fs, p, tr)
    w, _, h = orc.stft_geometry(fs)
    s, want = tr.items["similarity_matrix"], tr.items["similarity_indices"]
    t = s.shape[0]
    d = int(round(p.similarity_distance * fs / h))
    sp = pr.Spectra(x, None, w, -(w // 2), t)
    assert d == 5 and t == orc.centred_frame_count(len(x), w, h)
    for j in range(t):
        geo = pr.row_elements(0, j, t)
        e2 = sp.e2(geo.self_row, geo.rows)
        assert np.max(np.abs(e2 - s[j])) < 1e-13
        _, cols = pr.expected_list(e2, p.similarity_threshold, d, p.similarity_number)
        assert np.array_equal(geo.written[cols], want[j]), j
    full = orc.indices(orc.selfsimilaritymatrix(sp.unit64.T), p.similarity_threshold, d, p.similarity_number)
    assert all(np.array_equal(a, b) for a, b in zip(full, want))


@pytest.fixture(scope="module")
def online_clip():
    fs = 8000
    x = _clip(20000, 2, 2)
    w, _, h = orc.stft_geometry(fs)
    p = orc.Params(buffer_length=24 * h / fs, similarity_distance=0.1, similarity_number=4, similarity_threshold=0.5)
    return fs, x, w, h, p


def test_modes_1_and_2_against_the_simonline_trace(online_clip):
    fs, x, w, h, p = online_clip
    tr = orc.Trace()
    orc.simonline(x, fs, p, tr)
    b = tr.items["buffer_frames"]
    t = orc.online_frame_count(len(x), w, h)
    d = int(round(p.similarity_distance * fs / h))
    sp = pr.Spectra(x, None, w, 0, t)
    assert b == 24 and len(tr.items["similarity_vectors"]) == t - b + 1
    for r, (in_col, simvec) in enumerate(tr.items["similarity_vectors"]):
        j = b - 1 + r
        g1, g2 = pr.row_elements(1, j, b), pr.row_elements(2, j, b)
        assert np.array_equal(g1.rows, in_col) and np.array_equal(g2.rows, in_col) and g1.n == b
        assert np.array_equal(g1.band[0] + g1.band[1], np.full(b, j)) and np.all(g2.band[0] == j) and np.array_equal(g1.lag, g2.lag)
        assert np.array_equal(g1.lag, j - in_col)
        e2 = sp.e2(g1.self_row, g1.rows)
        assert np.max(np.abs(e2 - simvec)) < 1e-13
        _, cols = pr.expected_list(e2, p.similarity_threshold, d, p.similarity_number)
        assert np.array_equal(g1.written[cols], tr.items["similarity_indices"][r]), j


@pytest.mark.parametrize("start", [1, 9, 24])
def test_filling_rows_against_the_start_reference(online_clip, start):
    """Rows decided on min(B, j + 1) columns; the same rows of a stream that began at `origin` in a band shifted by `shift`."""
    fs, x, w, h, p = online_clip
    tr = orc.Trace()
    start_ref.simonline_from(x, fs, start, p, tr)
    b = tr.items["buffer_frames"]
    t = orc.online_frame_count(len(x), w, h)
    d = int(round(p.similarity_distance * fs / h))
    sp = pr.Spectra(x, None, w, 0, t)
    origin, shift = 1000, 983
    for r, want in enumerate(tr.items["similarity_indices"]):
        j = start - 1 + r
        geo = pr.row_elements(1, j, b, start=start)
        assert geo.n == min(b, j + 1)
        e2 = sp.e2(geo.self_row, geo.rows)
        _, cols = pr.expected_list(e2, p.similarity_threshold, d, p.similarity_number)
        assert np.array_equal(geo.written[cols], want), j
        moved = pr.row_elements(2, j + origin, b, start=start, origin=origin, shift=shift)
        assert moved.n == geo.n and np.array_equal(moved.written, geo.written + origin - shift) and moved.self_row == j + origin - shift
        assert np.array_equal(moved.lag, geo.lag)
    assert pr.row_elements(1, origin + start - 2, b, start=start, origin=origin, shift=shift) is None or start == 1
    assert pr.row_elements(1, 5, b, start=start, origin=1 << 60, shift=shift) is None


def _fp32_list(case, row):
    return pr.expected_list(row.m.astype(np.float64), case.spec.min_value, case.spec.d, case.spec.number)[1]


@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_every_gpu_case_meets_its_premises(name):
    """The case as the GPU test will run it (delta, delta2 of the design; the GPU test builds with the launch's own and checks
    again): the three premises, no more than a tenth of the rows tied across the cut, and the property the case is there for."""
    spec = pr.CASES[name]
    delta, delta2 = pr.design_deltas(spec.W // 2 + 1)
    case = pr.built(name, delta, delta2)
    assert max(pr.premises(case)) <= 1.0, pr.premises(case)
    assert case.tied_rows <= 0.1 * len(case.active)
    rows = [case.rows[k] for k in case.active]
    assert rows and all(check is None for check in (pr.check_row(np.concatenate([r.geo.written[r.cols2], np.full(spec.number, -1)]), len(r.cols2),
                                                                 r, 2, spec.number, spec.d) for r in rows))
    if 1 in spec.levels:                                         # level 1 alone: the e1 rows must give the e2 lists
        assert all(np.array_equal(r.cols1, r.cols2) for r in rows)
    if spec.planted:                                             # the planted perturbations flip fp32 decisions
        assert sum(not np.array_equal(_fp32_list(case, r), r.cols2) for r in rows) > 0
    if name.startswith(("twins", "reversed", "W", "band_level2")):   # level 1 and level 2 disagree: only float64 spectra give the lists
        assert sum(not np.array_equal(r.cols1, r.cols2) for r in rows) >= (len(rows) // 4 if spec.mode == 0 else 3)
        for r in rows:
            assert np.max(np.abs(r.e1 - r.e2)) <= 0.4 * delta2
    if spec.origin is not None and len(spec.origin) > 1:
        inactive = [k for k, v in case.rows.items() if v is None]
        assert inactive and any(k[0] == len(spec.origin) - 1 for k in inactive) == (spec.origin[-1] == 1 << 60)
    if spec.mode != 0:
        # every band cell outside the rows' own columns is absent (NaN), in both layouts; the two hold the same values
        for b in range(case.n_batch):
            cells = sum(case.rows[(b, r)].geo.n for r in range(spec.n_rows) if case.rows[(b, r)] is not None)
            assert np.sum(~np.isnan(case.band1[b])) == cells == np.sum(~np.isnan(case.band2[b]))
        assert any(v is not None and v.geo.n < spec.n_cols for v in case.rows.values()) == (0 < spec.start < spec.n_cols)


def test_the_stress_rows_are_sized_to_the_caps():
    delta, delta2 = pr.design_deltas(129)
    for name, copies in (("stress_amb_cap", pr.K_AMB_CAP), ("stress_amb_cap_plus_1", pr.K_AMB_CAP + 1), ("stress_rival_cap", 3 * (pr.K_RIVAL_CAP // 6 + 4))):
        row = pr.built(name, delta, delta2).rows[(0, 0)]
        tied = np.flatnonzero(row.e2 == row.e2[0])
        assert len(tied) == copies + 1 and row.cls2[tied].tolist() == [row.cls2[0]] * (copies + 1)      # + the row's own frame
        assert len(row.cols2) > 0 and row.cols2[0] == 0 and not set(tied[1:].tolist()) & set(row.cols2.tolist())
    row = pr.built("stress_hand_on", delta, delta2).rows[(0, 0)]
    low = np.flatnonzero(np.abs((1.0 - row.e2) - 2 * delta) < 0.05 * delta)
    assert len(low) == 106 and len(set(row.cls2[low].tolist())) == 1 and len(np.flatnonzero(row.e2 == row.e2[0])) == 54
    assert set(np.flatnonzero(row.e2 == row.e2[0]).tolist()) <= set(row.cols2.tolist()) and not set(low.tolist()) & set(row.cols2.tolist())


def test_check_row_refuses_a_wrong_list():
    delta, delta2 = pr.design_deltas(129)
    case = pr.built("wave_d7_T200", delta, delta2)
    spec = case.spec
    row = next(case.rows[k] for k in case.active if len(case.rows[k].cols2) >= 3)
    good = np.concatenate([row.geo.written[row.cols2], np.full(spec.number, -1)])[:spec.number]
    assert pr.check_row(good, len(row.cols2), row, 2, spec.number, spec.d) is None
    swapped = good.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert pr.check_row(swapped, len(row.cols2), row, 2, spec.number, spec.d)
    assert pr.check_row(good, len(row.cols2) - 1, row, 2, spec.number, spec.d)
    stale = good.copy()
    stale[len(row.cols2)] = 7
    assert pr.check_row(stale, len(row.cols2), row, 2, spec.number, spec.d)
    tied = pr.built("loop_far", *pr.design_deltas(129))
    row = tied.rows[(0, 75)]
    assert len(np.unique(row.vals2)) < len(row.vals2)
    back = np.concatenate([row.geo.written[row.cols2][::-1], np.full(100, -1)])[:100]
    assert pr.check_row(back, len(row.cols2), row, 2, 100, tied.spec.d) is None        # equal values in any order
    back[0] = back[1]
    assert pr.check_row(back, len(row.cols2), row, 2, 100, tied.spec.d)
