"""tests/mask_reference.py against the float64 oracle, on the CPU: the reference the GPU stage tests hold the mask kernels to
(tests/test_gpu_mask_stages.py) restates which frames a median is taken over and rounds the mean of the two middle values of an
even count to fp32, as the kernels do; on fp32-exact inputs it may therefore differ from orc.mask / orc.adaptivemask / orc.simmask
by that one rounding (2^-24 relative) and by nothing else, and not at all where the count is odd. The conditions the input
generators promise (every list length present, a quarter of the cells below 1, exact values, distinct values in a bin) are
checked here for the cases the GPU module runs."""
import numpy as np
import pytest

import mask_reference as ref
import stft_reference
from oracle import repet_oracle as orc

U = ref.U


def same_or_both_nan(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@np.errstate(all="ignore")
def close_to_oracle(mine, oracle, exact_rows=None):
    mine, oracle = np.asarray(mine, dtype=np.float64), np.asarray(oracle, dtype=np.float64)
    assert np.array_equal(np.isnan(mine), np.isnan(oracle))
    ok = ~np.isnan(oracle)
    assert np.all(np.abs(mine - oracle)[ok] <= U * np.abs(oracle)[ok])
    if exact_rows is not None:
        assert same_or_both_nan(mine[exact_rows], oracle[exact_rows])


@pytest.mark.filterwarnings("ignore:Mean of empty slice")
@pytest.mark.parametrize("t,period", [(3, 2), (9, 2), (17, 2), (40, 5), (40, 13), (64, 2), (31, 11), (12, 3), (7, 7)])
def test_period_reference_against_the_oracle(t, period):
    v = ref.magnitudes((t, 37), 100 + t)
    model, (m, one) = ref.mask_period(v, period)
    counts = np.array([len(ref.period_frames(t, period, q)) for q in range(period)])
    want_model = np.stack([np.median(v[q::period].astype(np.float64), axis=0) for q in range(period)])
    close_to_oracle(model, want_model, exact_rows=counts % 2 == 1)
    close_to_oracle(m, orc.mask(v.T.astype(np.float64), period).T, exact_rows=(counts % 2 == 1)[np.arange(t) % period])
    assert np.all(m[one] == 1.0) and np.all(m[~one & ~np.isnan(m)] < 1.0)
    # the model applied by the inverse STFT (stft_reference.model_mask) is the same mask, cutoff included
    for cutoff in (0, 1, 7, 36, 42):
        _, (mc, _) = ref.mask_period(v, period, cutoff)
        assert same_or_both_nan(mc, stft_reference.model_mask(v, model, period, cutoff))
    ref.input_conditions(None, 0, m, np.ones(m.shape, dtype=bool)) if t >= 9 else None


@pytest.mark.parametrize("order", ref.ADAPTIVE_ORDERS)
def test_adaptive_reference_against_the_oracle(order):
    t = 150
    v = ref.magnitudes((t, 33), 200 + order)
    per = ref.adaptive_periods(t, order)
    assert {1, t - 1, t}.issubset(set(per.tolist())) and per.max() > t
    model = ref.model_adaptive(v, per, order)
    m, one = ref.mask_of(v, model)
    counts = np.array([len(ref.adaptive_frames(t, i, per[i], order)) for i in range(t)])
    assert counts.min() == 1                     # only the frame itself in range
    close_to_oracle(m, orc.adaptivemask(v.T.astype(np.float64), per, order).T, exact_rows=counts % 2 == 1)
    if order >= 3:
        first_tap = 1 - (order + 1) // 2
        off_front = np.arange(t) + first_tap * per < 0
        off_back = np.arange(t) + (first_tap + order - 1) * per >= t
        assert (off_front & ~off_back).any() and (off_back & ~off_front).any() and (off_front & off_back).any()
        ref.input_conditions(None, 0, m, np.ones(m.shape, dtype=bool))


@pytest.mark.parametrize("max_count", ref.SIM_COUNTS)
@pytest.mark.parametrize("f", ref.SIM_FLOAT_F)
def test_sim_reference_and_inputs(f, max_count):
    t = ref.sim_frames(max_count)
    V, idx, cnt = ref.build_sim(1, 2, t, f, max_count, 1000 * f + max_count)
    assert np.all(np.diff(cnt[0]) != 0)          # neighbouring lists differ in length ...
    assert all(not np.array_equal(idx[0, r, :3], idx[0, r + 1, :3]) for r in range(t - 1)) or max_count < 3      # ... and content
    for c in range(2):
        v = V[0, c]
        m, one, model = ref.reference_sim(v, idx[0], cnt[0])
        close_to_oracle(m, orc.simmask(v.T.astype(np.float64), ref.lists_of(idx[0], cnt[0])).T, exact_rows=cnt[0] % 2 == 1)
        assert np.all(np.isnan(m[cnt[0] == 0])) and not np.isnan(m[cnt[0] > 0]).any()
        ref.input_conditions(cnt, max_count, m, np.ones(m.shape, dtype=bool))


def test_generated_magnitudes_keep_their_promises():
    v = ref.magnitudes((2, 150, 257), 7)
    assert v.dtype == np.float32 and np.all(v >= 0)
    levels = np.log2(np.max(v[0], axis=0)[np.max(v[0], axis=0) > 0])
    assert levels.min() < -37 and levels.max() > 40
    assert np.count_nonzero(v[0, :, ref.ZERO_BIN] == 0) == 50
    assert len(np.unique(v[0, :, ref.CONST_BIN])) == 1 and len(np.unique(v[1, :, ref.TIE_BIN])) <= 5
    regular = np.ones(257, dtype=bool)
    regular[[ref.ZERO_BIN, ref.CONST_BIN, ref.TIE_BIN]] = False
    s = np.sort(v[0][:, regular].astype(np.float64), axis=0)
    assert np.all(np.diff(s, axis=0) > 2.0 ** -16 * s[1:])           # what can meet in one median differs by more than 2^-16 relative
    raised = ref.raise_absent(v[0], np.arange(150) % 2 == 0)
    s = np.sort(raised[:, regular].astype(np.float64), axis=0)
    assert np.all(np.diff(s, axis=0) > 2.0 ** -16 * s[1:])


@np.errstate(all="ignore")
def test_the_nan_rule_and_infinities():
    t, period = 21, 4
    v = ref.magnitudes((t, 40), 11)
    v[6] = np.nan
    v[9, 4] = np.nan
    v[3, 8] = v[7, 8] = v[11, 8] = np.inf
    v[1, 9] = np.inf
    model, (m, one) = ref.mask_period(v, period)
    assert np.all(np.isnan(model[6 % period])) and np.isnan(model[9 % period, 4]) and np.isnan(model[:, 10]).sum() == 1
    assert np.all(np.isnan(m[6 % period::period])) and np.isnan(m[np.arange(t) % period == 1, 4]).all()
    want = orc.mask(v.T.astype(np.float64), period).T
    assert np.array_equal(np.isnan(m) | (np.isinf(v) & one), np.isnan(want))       # (inf / inf is NaN in the oracle and 1 in the kernels)
    assert model[3, 8] == np.inf and np.all(m[3::4, 8] == 1.0) and m[1, 9] == 0.0
    # np.median of an empty list, and no NaN rule in `sim` (its lists never hold a NaN frame)
    assert np.isnan(ref.median32(np.empty((0, 3), dtype=np.float32), False)).all()
    assert ref.net_for(1) == 2 and ref.net_for(10) == 10 and ref.net_for(11) == 12 and ref.net_for(128) == 128 and ref.net_for(129) == 0
