"""The float64 kNN yardstick (tests/_knn_reference.py) held to the oracle's deterministic lists, and check_lists held to
what it must refuse.  No GPU."""
import numpy as np
import pytest

from oracle import oscillink_oracle as orc
from tests._knn_reference import check_lists, lists_f64


def _bad_rows_array(N, D, seed):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((N, D), dtype=np.float32)
    nonfinite, zero = [5, 70, 111, N - 1], [0, 64, 200]
    Y[5, 3] = np.nan
    Y[70] = np.nan
    Y[111, 0] = np.inf
    Y[N - 1, D - 1] = -np.inf
    Y[zero] = 0.0
    return Y, nonfinite, zero


def test_yardstick_agrees_with_the_oracle_on_finite_anchors():
    """An odd size, chunks that do not divide it: same lists in the same order (similarity desc, index asc) wherever the
    float64 gap at rank k is above the fp32 noise of the oracle's sgemm, near-ties only elsewhere."""
    N, D, k = 777, 40, 9
    Y = np.random.default_rng(3).standard_normal((N, D), dtype=np.float32)
    idx_o, val_o = orc.knn_topk(Y, k, deterministic=True)
    ref = lists_f64(Y, k, chunk=100)
    assert check_lists(Y, idx_o, val_o, k, 1e-6, ref=ref) <= int((ref[2] < 1e-6).sum())
    clear = np.abs(np.diff(ref[1], axis=1)).min(axis=1) > 1e-6  # no two of the row's k similarities within fp32 noise ...
    clear &= ref[2] > 1e-6                                       # ... and neither the k-th and the one behind it
    assert clear.sum() > N // 2
    assert np.array_equal(idx_o[clear], ref[0][clear])
    whole = lists_f64(Y, k, chunk=N)  # the chunking is invisible (up to the last bits of a float64 dot product)
    assert np.array_equal(ref[0][clear], whole[0][clear])
    assert np.allclose(ref[1], whole[1], rtol=0, atol=1e-14) and np.allclose(ref[2], whole[2], rtol=0, atol=1e-14)
    assert (ref[2] >= 0).all() and (np.diff(ref[1], axis=1) <= 0).all()


def test_yardstick_agrees_with_the_oracle_on_non_finite_and_zero_rows():
    """NaN / Inf rows are nobody's neighbour (their similarities rank last); a zero row's similarities are all exactly 0
    and tie by index, and no finite row's list reaches down to a zero column's 0 before its positive ones."""
    N, D, k = 300, 16, 12
    Y, nonfinite, zero = _bad_rows_array(N, D, 11)
    with np.errstate(invalid="ignore"):
        idx_o, val_o = orc.knn_topk(Y, k, deterministic=True)
    ref = lists_f64(Y, k, chunk=128)
    good = np.setdiff1d(np.arange(N), nonfinite)
    assert not np.isin(ref[0][good], nonfinite).any()
    check_lists(Y, idx_o, val_o, k, 1e-6, rows=good, ref=ref)
    first = [c for c in range(N) if c not in nonfinite]
    for r in zero:  # every similarity 0: the k smallest indices other than the row itself
        want = [c for c in first if c != r][:k]
        assert ref[0][r].tolist() == want and idx_o[r].tolist() == want
        assert (ref[1][r] == 0).all() and ref[2][r] == 0
    assert np.isinf(ref[2][nonfinite]).all() and (ref[1][nonfinite] == 0).all()


def test_check_lists_refuses_a_wrong_member_and_accepts_a_true_tie():
    N, D, k = 400, 24, 8
    Y = np.random.default_rng(5).standard_normal((N, D), dtype=np.float32)
    idx, val, gap = lists_f64(Y, k)
    r = int(np.argmax(gap))  # as far from a near-tie as this array gets
    assert gap[r] > 1e-3
    assert check_lists(Y, idx, val, k, 1e-6) == 0
    nxt = np.setdiff1d(np.arange(N), np.append(idx[r], r))[0]
    for wrong in (nxt, r, N, -1, int(idx[r, 0])):  # another column, the row itself, out of range, the fill pattern, a repeat
        bad = idx.copy()
        bad[r, k - 1] = wrong
        with pytest.raises(AssertionError):
            check_lists(Y, bad, val, k, 1e-6)
        with pytest.raises(AssertionError):
            check_lists(Y, bad, val, k, 1e-6, rows=[r])
        assert check_lists(Y, bad, val, k, 1e-6, rows=[q for q in range(N) if q != r]) == 0
    off = val.copy()
    off[r, 2] += 1e-5
    with pytest.raises(AssertionError):
        check_lists(Y, idx, off, k, 1e-6)
    # a true tie at rank k: the column behind the k-th is a copy of it -- either may stand in the list, nothing else
    j = int(idx[r, k - 1])
    m = int(np.setdiff1d(np.arange(j + 1, N), np.append(idx[r], r))[0])
    Y2 = Y.copy()
    Y2[m] = Y2[j]
    idx2, val2, gap2 = lists_f64(Y2, k)
    assert gap2[r] < 1e-12 and idx2[r, k - 1] == j  # the smaller index wins the tie
    swapped = idx2.copy()
    swapped[r, k - 1] = m
    assert check_lists(Y2, swapped, val2, k, 1e-6, rows=[r]) == 1
    swapped[r, k - 1] = np.setdiff1d(np.arange(N), np.concatenate([idx2[r], [r, m]]))[0]
    with pytest.raises(AssertionError):
        check_lists(Y2, swapped, val2, k, 1e-6, rows=[r])
