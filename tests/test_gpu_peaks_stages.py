"""Stage tests of the peak-picking kernels of ``sim``, ``simonline`` and the live handles, driven as the pipelines drive them:
``launch_segment_maxima`` -> ``make_refine`` -> ``launch_local_maxima`` -> ``run_exact_rows`` through ``repet._peaks_stage``
(repet_debug_peaks_stage, engine_stages.hip), at the smallest shapes that reach each path -- the four instantiations of the
wavefront kernel, its segment records, the workgroup kernel at every QMAX and in two stages, the diagonal walk and the
look-back row of modes 1 and 2 with ``row_columns`` / ``apply_origin`` / ``shift``, level 1, the record hand-over to
``local_maxima_lite_kernel``, ``unit_rows_f64_wg_kernel<1|4>`` and ``local_maxima_exact_kernel``.

The reference is tests/peaks_reference.py (checked on the CPU by tests/test_peaks_reference.py, which also builds every case
below and asserts its premises): the lists are ``orc.localmaxima`` of the float64 row. The fp32 matrix handed to the stage
is fp32(e1) plus perturbations of 0.35 delta whose sign flips every fp32 decision it can reach (window ties, threshold
crossings, pairs across the top-``number`` cut): a kernel that trusts fp32 where it should not gets a wrong list. delta and
delta2 come from the stage's report; the case is built with them and its premises are asserted again here.

Asserted for every launch: count and list of every active row (equal ordered sequences; equal sorted values, valid distinct
indices and -- below ``number`` survivors -- equal sets where frame classes tie exactly), -1 in cells count .. number-1, the
byte prefill in cells number .. KP-1 and in the guard row no launch owns, count 0 for inactive rows; at level 2 every stamped
float64 unit row against ``unit64`` (2-norm and per component <= 16 log2(W) 2^-53), the prefill in the unstamped ones, counter
[9] == stamped rows; and the launch report (family, QMAX, lite relaunch, general kernel, unit-row variant).

Three limits the kernels state themselves (peaks.h, peaks.hip), and what the cases do about them:
  * a row with more than kAmbCap near-tied elements or kRivalCap (element, rival) pairs ("flat", counter [3]) keeps its fp32
    decisions at level 1 and is decided by the second level only: the near-tie stress rows run with both levels;
  * ``refine`` 1 leaves level-1 verdicts closer than delta2 as they are: the level-1 cases are built so that the e1 row and the
    e2 row give the same lists;
  * the refinement re-takes VERDICTS (window maximum, threshold, top-``number`` cut); the ranking inside the kept set is by fp32
    value, a refined winner entering it with its level-1 value. FINDING of this module's first run on an MI355X: with a refined
    winner 0.25 delta above another kept entry that carried the planted -0.35 delta, the two came out in the wrong ORDER (same
    set; case two_stage, rows 1, 2, 4). The median that consumes the lists does not depend on their order and the kernels
    promise none inside delta, so no kernel was changed; ``peaks_reference.order_margin`` keeps such pairs out of every case
    (asserted by ``build``), which is what makes the ordered comparison below a theorem too.

The largest error / bar per (kernel, check) is collected in PARITY; the last test prints it and writes it to
$REPET_PEAKS_STAGE_PARITY_OUT: profiles/peaks_stage_parity.txt is that output from an MI355X (documentation; the asserts use
the bars)."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import peaks_reference as pr

pytestmark = pytest.mark.gpu

PARITY = {}          # (kernel, check) -> (error / bar, error, bar, case)
SEEN = set()         # launch facts the reports have shown
COUNTED = {3: 0, 14: 0}
TRANSFORMS = {}       # case -> (float64 transforms counted, rows stamped) of the launches that used the general kernel
FILL_A, FILL_B = 0xFF, 0x40      # NaN in the float cells and -1 in the lists; 3.0039 in the float cells and 0x40404040 in the lists


HIP_ERRORS = []


def _stage(*args, **kwargs):
    """repet._peaks_stage; after a HIP error nothing more is launched by this module (every later test fails at once)."""
    import repet
    if HIP_ERRORS:
        pytest.fail("not run: an earlier launch of this module ended in a HIP error: %s" % HIP_ERRORS[0])
    try:
        return repet._peaks_stage(*args, **kwargs)
    except RuntimeError as e:
        if "hip" in str(e).lower():
            HIP_ERRORS.append(str(e))
        raise


def _note(kernel, check, err, bar, case):
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else np.inf)
    key = (kernel, check)
    if key not in PARITY or ratio > PARITY[key][0]:
        PARITY[key] = (float(ratio), float(err), float(bar), case)


@functools.lru_cache(maxsize=None)
def _deltas(W):
    """delta and delta2 as a launch with this window's unit rows reports them (never a constant of the test)."""
    H, F = W // 2, W // 2 + 1
    hi = pr.make_audio(8, W, 1, 1)
    unit = pr.unit64(hi, None, W, H, 0, 8).astype(np.float32)
    m = (unit.astype(np.float64) @ unit.astype(np.float64).T).astype(np.float32)
    out = _stage(m, d=5, number=3, refine=2, unit=unit[None], hi=hi[None], W=W)
    assert out["delta"] > 4 * out["delta2"] > 0
    return out["delta"], out["delta2"]


def _case(name):
    spec = pr.CASES[name]
    delta, delta2 = _deltas(spec.W)
    case = pr.built(name, delta, delta2)
    assert max(pr.premises(case)) <= 1.0 <= case.order_margin, (pr.premises(case), case.order_margin)
    for k, what in enumerate(("|M - e1| / 0.4 delta", "|e1 - e2| / 0.4 delta2", "separation / closest pair")):
        _note("premises", what, pr.premises(case)[k], 1.0, name)
    return case


def _word(fill):
    return int(np.frombuffer(bytes([fill]) * 4, dtype=np.int32)[0])


def _run(name, level, mode=None, fill=FILL_B, absent=None):
    """One launch of case `name` at refinement `level`; every assert of the module's docstring. Returns (case, stage output)."""
    case = _case(name)
    s = case.spec
    mode = s.mode if mode is None else mode
    if mode == 0:
        m = case.M
    else:
        m = (case.band1 if mode == 1 else case.band2).copy()
        if absent is not None:
            m[np.isnan(m)] = absent
    out = _stage(m, pitch=s.pitch, mode=mode, row0=s.row0, n_rows=s.n_rows, min_value=s.min_value, d=s.d, number=s.number,
                             shift=s.shift, origin=s.origin, start=s.start, with_scratch=s.with_scratch, refine=level,
                             unit=case.unit32 if level else None, hi=case.hi if level == 2 else None, lo=case.lo if level == 2 else None,
                             W=s.W, frame_sample0=s.frame_sample0, prefill=fill)
    launch, cnt = out["launch"], out["counters"]
    kernel = "first pass: %s, mode %d, level %d" % (launch["family"], mode, level)
    if level:
        assert out["delta"] == case.delta and (level < 2 or out["delta2"] == case.delta2)
    assert launch["family"] == s.expect, (name, launch)
    if s.qmax is not None:
        assert launch["qmax"] == s.qmax, (name, launch)
    if s.expect == "wave":
        assert launch["rd"] == s.d & 3
    SEEN.add(launch["family"] + ("<%d>" % launch["qmax"] if launch["family"].startswith("block") else ""))
    SEEN.add("mode %d" % mode)
    # ---- the lists ---------------------------------------------------------------------------------------------------
    word = _word(fill)
    idx, count = out["idx"], out["count"]
    assert idx.shape == (case.n_batch, s.n_rows + 1, case.KP) and count.shape == idx.shape[:2]
    assert np.all(idx[:, s.n_rows] == word) and np.all(count[:, s.n_rows] == word), "%s: the row behind the launch was written" % name
    assert np.all(idx[:, :, s.number:] == word), "%s: cells behind `number` were written" % name
    bad = []
    for (b, r), row in case.rows.items():
        if row is None:
            if count[b, r] != 0:
                bad.append(((b, r), "inactive row with count %d" % count[b, r]))
            continue
        if level == 0:                                  # no refinement: the fp32 matrix itself decides
            v = row.m.astype(np.float64)
            vals, cols = pr.expected_list(v, s.min_value, s.d, s.number)
            row = SimpleNamespace(geo=row.geo, e1=v, vals1=vals, cols1=cols)
        why = pr.check_row(idx[b, r, :s.number], int(count[b, r]), row, 2 if level == 2 else 1, s.number, s.d)
        if why:
            bad.append(((b, r, "global row %d" % (s.row0 + r)), why))
    _note(kernel, "rows whose list differs", len(bad), 0.0, name)
    assert not bad, "%s (%s): %d of %d rows differ from the reference; (clip, row): %s" % (name, kernel, len(bad), len(case.rows), bad[:4])
    # ---- level 2: the float64 unit rows and the counters --------------------------------------------------------------------
    if level == 2:
        stamped, u64 = out["stamped"], out["u64"]
        bar = pr.fft_bar(s.W)
        fs = u64.shape[2]
        unit_kernel = "unit rows: %s" % ("unit_rows_f64_wg_kernel<%d>" % launch["unit_rows_variant"] if launch["lite"] else
                                         "local_maxima_exact_kernel, FFT plan %d" % launch["exact_fft"])
        raw = u64.view(np.uint8).reshape(case.n_batch, case.n_frames, fs * 8)
        assert np.all(raw[~stamped] == fill), "%s: a float64 unit row without a stamp was written" % name
        for b in range(case.n_batch):
            if case.clips[b] is None:
                assert not np.any(stamped[b])
                continue
            want = case.clips[b].sp.unit64
            for f in np.flatnonzero(stamped[b]):
                got = u64[b, f]
                assert np.all(got[case.F:] == 0), "%s: pad bins of float64 unit row %d" % (name, f)
                if np.any(np.isnan(want[f])):
                    assert np.all(np.isnan(got[:case.F])), "%s: the silent frame %d is a NaN row" % (name, f)
                    continue
                err = got[:case.F] - want[f]
                _note(unit_kernel, "2-norm error", float(np.sqrt(err @ err)), bar, name)
                _note(unit_kernel, "component error", float(np.max(np.abs(err))), bar, name)
                assert np.sqrt(err @ err) <= bar and np.max(np.abs(err)) <= bar, (name, b, int(f), float(np.sqrt(err @ err)), bar)
        # A frame QUEUED for level 2 (the fast path: frame_list, unit_rows_f64_wg_kernel) is computed exactly once. The general
        # kernel transforms on demand and, by its own statement, "a frame another workgroup is transforming right now is
        # transformed twice: same bits, no waiting" (peaks_exact.hip, level2) -- FINDING: with every row of a launch on that path
        # this is the rule, not the exception (loop_block: 675 and 830 transforms for 120 frames in two runs on an MI355X; harmless to the lists,
        # wasted work on a path that is rare in production). So equality is asserted where the queue alone computed, and the
        # general kernel is held to "every stamped row was counted"; the ratio goes into the PARITY table's documentation.
        n_stamped = int(np.sum(stamped))
        if cnt["rows_to_level2"] == 0:
            assert cnt["unit_rows_f64"] == n_stamped == cnt["frames_queued"], (name, cnt, n_stamped)
        else:
            assert cnt["unit_rows_f64"] >= n_stamped >= cnt["frames_queued"], (name, cnt, n_stamped)
            TRANSFORMS[name] = (cnt["unit_rows_f64"], n_stamped)
        assert launch["exact_fft"] > 0, "the general kernel is launched behind every first pass"
        SEEN.add("exact fft %d" % launch["exact_fft"])
        if launch["lite"]:
            SEEN.add("lite")
            SEEN.add("unit rows <%d>" % launch["unit_rows_variant"])
        if cnt["rows_to_level2"]:
            SEEN.add("general rows")
        _note("level 2", "largest |level 1 - level 2| / 0.4 delta2", cnt["level2_max_diff_1e12"] * 1e-12, 0.4 * out["delta2"], name)
        assert cnt["level2_max_diff_1e12"] * 1e-12 < 0.4 * out["delta2"]
    for k, key in ((3, "flat_rows"), (14, "rows_handed_on")):
        COUNTED[k] += cnt[key]
    return case, out


WAVE = sorted(n for n in pr.CASES if n.startswith("wave_"))
RECORDS = sorted(n for n in pr.CASES if n.startswith("records_"))
BLOCK = sorted(n for n in pr.CASES if n.startswith("block_"))
BAND = sorted(n for n in pr.CASES if n.startswith("band_") and pr.CASES[n].levels == (1,))


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("name", WAVE + RECORDS + BLOCK + ["two_stage"])
def test_first_pass_and_level_1(name, level):
    """Mode 0. Level 0 against orc.localmaxima of the fp32 matrix itself; level 1 -- the planted perturbations undone by the
    float64 similarities of the fp32 unit rows -- against the float64 reference: near-tied elements were found ([1]) and
    decisions changed ([2])."""
    case, out = _run(name, level)
    cnt = out["counters"]
    if level == 1 and case.spec.planted:
        assert cnt["near_tied"] > 0 and cnt["decisions_changed"] > 0, (name, cnt)
        assert cnt["rows_to_level2"] == 0 and cnt["rows_recorded"] == 0, "no second level was asked for"
    if level == 0:
        assert not any(out["stats"])


@pytest.mark.parametrize("fill, absent", [(FILL_A, None), (FILL_B, 2.0)])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", BAND)
def test_band_rows_of_filling_and_shifted_streams(name, mode, fill, absent):
    """Modes 1 and 2 from the same values: rows of min(B, j + 1) columns (start < B), a shifted band, one origin per clip, an idle
    clip and a clip that began mid-buffer. Every band cell and column the row rules call absent holds NaN, then + 2.0 (the pad
    cells 3.0039): a kernel that reads one gets a wrong list either way."""
    case, out = _run(name, 1, mode=mode, fill=fill, absent=absent)
    assert out["counters"]["near_tied"] > 0


def test_both_band_layouts_give_the_same_lists():
    for name in BAND:
        a = _run(name, 1, mode=1)[1]
        b = _run(name, 1, mode=2)[1]
        n = pr.CASES[name].number
        for key, v in _case(name).rows.items():
            if v is not None:           # (an inactive row's list cells are not part of the contract)
                assert a["count"][key] == b["count"][key] and np.array_equal(a["idx"][key][:n], b["idx"][key][:n])


LEVEL2 = sorted(n for n in pr.CASES if pr.CASES[n].levels == (2,))


@pytest.mark.parametrize("name", LEVEL2)
def test_level_2(name):
    """Twin frames (same hi, different lo: an exact level-1 tie that the float64 spectra decide against index order), pairs
    whose e1 order is the opposite of their e2 order, looped exact periods, rows at and past the caps of the first pass, a row
    the fast path hands on, a silent frame; lo absent, centred frames, W = 2048 and 4096; the band with origins."""
    case, out = _run(name, 2)
    s, cnt, launch = case.spec, out["counters"], out["launch"]
    if s.level2 is not None:
        assert cnt["rows_to_level2"] + cnt["rows_recorded"] > 0 and cnt["elements_level2"] > 0, (name, cnt)
    if s.level2 == "lite":
        assert launch["lite"] and cnt["rows_recorded"] > 0 and launch["unit_rows_variant"] == (1 if s.W <= 2048 else 4), (name, launch, cnt)
    if s.level2 == "general":
        assert cnt["rows_to_level2"] > 0, (name, cnt)
    if name.startswith(("twins", "reversed", "W", "band_level2")):
        assert cnt["rows_changed_level2"] > 0, (name, cnt)
    if s.flat_rows:
        assert cnt["flat_rows"] >= s.flat_rows, (name, cnt)
    if s.hands_on:
        assert cnt["rows_handed_on"] > 0, (name, cnt)
    if name == "stress_amb_cap":            # exactly kAmbCap near-tied elements: refined, not flat
        assert cnt["flat_rows"] == 0 and cnt["near_tied"] >= pr.K_AMB_CAP, (name, cnt)
    if s.mode != 0:
        _run(name, 2, mode=2, fill=FILL_A)


def test_level_1_leaves_flat_rows_to_the_second_level():
    """The same stress rows without the second level: the counter says which rows were flat; their lists are then fp32's (peaks.h)
    and not asserted. Everything else of the contract -- the other rows, the cells behind the lists -- is."""
    for name, flat in (("stress_amb_cap", 0), ("stress_amb_cap_plus_1", 1), ("stress_rival_cap", 1)):
        case = _case(name)
        s = case.spec
        out = _stage(case.M, d=s.d, number=s.number, refine=1, unit=case.unit32, prefill=FILL_B)
        assert out["counters"]["flat_rows"] == flat, (name, out["counters"])
        COUNTED[3] += out["counters"]["flat_rows"]
        word = _word(FILL_B)
        assert np.all(out["idx"][:, :, s.number:] == word) and np.all(out["idx"][:, s.n_rows] == word)
        for (b, r), row in case.rows.items():
            if r > 0 or not flat:
                assert pr.check_row(out["idx"][b, r, :s.number], int(out["count"][b, r]), row, 1, s.number, s.d) is None, (name, r)


def test_stage_entry_refuses_what_would_index_out_of_range():
    m = np.zeros((1, 20, 16), dtype=np.float32)
    unit = np.ones((1, 20, 129), dtype=np.float32)
    with pytest.raises(ValueError):
        _stage(m, mode=0, n_rows=21, d=4, number=3)                       # rows outside the matrix
    with pytest.raises(ValueError):
        _stage(m, mode=0, d=4, number=3, refine=1, unit=unit[:, :10])    # a column without a unit row
    with pytest.raises(ValueError):
        _stage(m, mode=1, row0=5, n_rows=4, d=4, number=3, shift=3)      # row 5 has 6 columns: band rows 2 .. -3
    with pytest.raises(ValueError):
        _stage(m, mode=2, row0=15, n_rows=8, d=4, number=3)              # band row 20 and later
    with pytest.raises(ValueError):
        _stage(m, mode=1, row0=30, n_rows=4, d=4, number=3, shift=10, origin=[5], start=4)   # frames before the band
    with pytest.raises(ValueError):
        _stage(m, mode=0, d=4, number=3, origin=[0])
    ok = _stage(m, mode=1, row0=15, n_rows=5, d=4, number=3)
    assert ok["launch"]["family"] == "wave" and np.all(ok["count"][0, :5] == 0)


def test_zz_parity_record():
    """Every path the issue names was shown by a launch report of this module; then the PARITY table, printed and written to
    $REPET_PEAKS_STAGE_PARITY_OUT."""
    want = {"wave", "wave+records", "block two-stage<8>", "lite", "general rows", "unit rows <1>", "unit rows <4>", "mode 0", "mode 1", "mode 2"}
    want |= {"block<%d>" % q for q in (1, 2, 4, 8, 16, 32)}
    assert want <= SEEN, sorted(want - SEEN)
    assert len({k for k in SEEN if k.startswith("exact fft")}) == 2, sorted(SEEN)       # both FFT plans of the exact kernel
    assert COUNTED[3] > 0 and COUNTED[14] > 0, COUNTED
    lines = ["%-62s %-44s %10s %12s %12s  %s" % ("kernel", "check", "err/bar", "err", "bar", "worst case")]
    for (kernel, check), (ratio, err, bar, case) in sorted(PARITY.items()):
        lines.append("%-62s %-44s %10.4f %12.4e %12.4e  %s" % (kernel, check, ratio, err, bar, case))
    lines.append("launch facts seen: " + ", ".join(sorted(SEEN)))
    lines.append("float64 transforms / stamped rows where the general kernel ran: " + ", ".join("%s %d / %d" % (k, a, b) for k, (a, b) in sorted(TRANSFORMS.items())))
    lines.append("flat rows (counter [3]): %d, rows handed on by the fast path (counter [14]): %d" % (COUNTED[3], COUNTED[14]))
    text = "\n".join(lines)
    print(text)
    out = os.environ.get("REPET_PEAKS_STAGE_PARITY_OUT")
    if out:
        with open(out, "w") as fh:
            fh.write(text + "\n")
    assert all(ratio <= 1.0 for ratio, _, _, _ in PARITY.values())
