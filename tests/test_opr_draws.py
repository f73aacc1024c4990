"""CPU: rtx_opr_draw, the host half of the one-plus-random device route, draws what the reference's loop draws.

The reference (rectorch/evaluation.py:113-178) calls random.sample(negatives, r) for every held-out positive, row-major, the
positives of a row ascending; `negatives` is the sorted list of the items that are not positives of that row.  random.sample reads
len(population) and the generator only, so its draws are random.sample(range(len(negatives)), r) mapped through `negatives`.  These
tests compare the library's reproduction with the running Python's random module: the drawn items, and random.getstate()
afterwards -- across both branches of sample() (pool swap for n <= setsize, set with re-draws above), thousands of consecutive
contests per call, the ValueError point, and held-out rows with stored zeros, unsorted indices, duplicates and empty rows.
"""
import random

import numpy as np
import pytest
from scipy.sparse import csr_matrix

from rectorch_amd.engine import opr_draw


def _held(m):
    m = m.tocsr()
    return (np.ascontiguousarray(m.indptr, dtype=np.int64), np.ascontiguousarray(m.indices, dtype=np.int32),
            np.ascontiguousarray(m.data, dtype=np.float32))


def _python_draws(dense, rows, r):
    """the reference's loop on a dense held-out matrix: (row, positive, draws) per contest; raises ValueError as it does"""
    out = []
    n_items = dense.shape[1]
    for b, u in enumerate(rows):
        pos = np.flatnonzero(dense[u]).tolist()
        negatives = sorted(set(range(n_items)) - set(pos))
        for i in pos:
            out.append((b, i, random.sample(negatives, r)))
    return out


def _rows_with_positives(n_users, n_items, per_user, seed):
    rng = np.random.RandomState(seed)
    dense = np.zeros((n_users, n_items), np.float32)
    for u in range(n_users):
        k = min(per_user if per_user >= 0 else rng.randint(0, 4), n_items)
        dense[u, rng.choice(n_items, size=k, replace=False)] = 1.0
    return dense


def _check(dense, r, seed, rows=None, held=None):
    rows = np.arange(dense.shape[0]) if rows is None else np.asarray(rows)
    held = _held(csr_matrix(dense)) if held is None else held
    random.seed(seed)
    random.random()                                 # (a state position that is not at a block boundary)
    before = random.getstate()
    crow, citem, draws, short = opr_draw(held, rows, dense.shape[1], r)
    after = random.getstate()
    random.setstate(before)
    want = _python_draws(dense, rows, r)
    assert short == -1
    assert random.getstate() == after
    assert len(crow) == len(want)
    assert crow.numpy().tolist() == [w[0] for w in want]
    assert citem.numpy().tolist() == [w[1] for w in want]
    assert draws.shape == (len(want), r)
    assert np.array_equal(draws.numpy(), np.array([w[2] for w in want], np.int64).reshape(len(want), r))
    return len(want)


# r in {1, 5, 6, 7, 20, 100, 1000}; n = #negatives from 1 up to 20108: setsize is 21 for r <= 5, 21 + 4 ** ceil(log(3 r, 4)) above
# (r = 6: 85, 7: 85, 20: 85, 100: 1045, 1000: 4117).  Each (n_items, r) pair with n on one side of it or the other, or at it.
CASES = [(2, 1), (30, 1), (22, 5), (5000, 5), (7, 6), (86, 6), (87, 6), (200, 7), (21, 20), (86, 20), (300, 20),
         (1046, 100), (1047, 100), (1100, 100), (1001, 1000), (4118, 1000), (4119, 1000), (20108, 1000)]


@pytest.mark.parametrize("n_items,r", CASES, ids=["I%d-r%d" % c for c in CASES])
def test_draws_equal_random_sample(n_items, r):
    """one positive per user, so n = n_items - 1 negatives: the branch is decided by n against setsize"""
    users = max(2, min(400, 200000 // max(r, 1) // 10))
    dense = _rows_with_positives(users, n_items, 1, seed=n_items + r)
    assert _check(dense, r, seed=r) == users


@pytest.mark.parametrize("seed", [0, 1, 2, 12345])
def test_thousands_of_consecutive_contests(seed):
    """several thousand contests through one call: the MT19937 block regeneration is crossed many times, rows have 0 .. 3
    positives (a row without positives draws nothing)"""
    dense = _rows_with_positives(3000, 120, -1, seed=seed)
    assert _check(dense, 20, seed=seed) > 3000
    dense = _rows_with_positives(1500, 3000, -1, seed=seed + 1)
    assert _check(dense, 6, seed=seed) > 1500


def test_n_equal_to_r():
    """every non-positive item is drawn: a permutation of them, through the pool branch"""
    for n_items, r in [(8, 7), (1001, 1000), (21, 20)]:
        dense = _rows_with_positives(5, n_items, 1, seed=3)
        _check(dense, r, seed=7)


def test_r_zero_draws_nothing():
    dense = _rows_with_positives(4, 10, 2, seed=1)
    _check(dense, 0, seed=1)


def test_value_error_point():
    """a row with fewer than r negatives stops the draws at its first contest, with the state where random.sample raises"""
    dense = np.zeros((5, 30), np.float32)
    dense[0, [1, 4]] = 1
    dense[1, 7] = 1
    dense[2, :12] = 1                       # 18 negatives < r = 20
    dense[3, 0] = 1
    rows = np.arange(5)
    random.seed(99)
    before = random.getstate()
    crow, citem, draws, short = opr_draw(_held(csr_matrix(dense)), rows, 30, 20)
    after = random.getstate()
    assert short == 2
    assert crow.numpy().tolist() == [0, 0, 1] and citem.numpy().tolist() == [1, 4, 7]
    random.setstate(before)
    with pytest.raises(ValueError):
        _python_draws(dense, rows, 20)
    assert random.getstate() == after
    random.setstate(before)
    want = [random.sample(sorted(set(range(30)) - {1, 4}), 20) for _ in range(2)] + [random.sample(sorted(set(range(30)) - {7}), 20)]
    assert np.array_equal(draws.numpy(), np.array(want))


def test_short_first_row_consumes_nothing():
    dense = np.zeros((2, 10), np.float32)
    dense[0, :5] = 1
    random.seed(5)
    before = random.getstate()
    crow, _, _, short = opr_draw(_held(csr_matrix(dense)), np.arange(2), 10, 6)
    assert short == 0 and len(crow) == 0 and random.getstate() == before


def test_item_mapping_with_stored_zeros_unsorted_indices_and_empty_rows():
    """The held-out rows as stored: explicit zeros (not positives: dense.nonzero() skips them), column ids out of order, duplicate
    entries, empty rows, a row order that is not the matrix's.  Against a dense numpy restatement of the mapping: the j-th
    negative is the j-th column, ascending, that is not a nonzero of the row."""
    rng = np.random.RandomState(4)
    n_users, n_items, r = 60, 500, 30
    indptr, indices, values = [0], [], []
    for u in range(n_users):
        k = 0 if u % 7 == 0 else rng.randint(1, 40)
        cols = rng.choice(n_items, size=k, replace=False)
        vals = rng.choice([0.0, 1.0, 2.5, -1.0], size=k, p=[0.3, 0.4, 0.2, 0.1]).astype(np.float32)
        if k > 3:                                        # a duplicate of a positive entry
            cols, vals = np.append(cols, cols[0]), np.append(vals, np.float32(1.0) if vals[0] != 0 else np.float32(0.0))
        indices += cols.tolist()
        values += vals.tolist()
        indptr.append(len(indices))
    held = (np.array(indptr, np.int64), np.array(indices, np.int32), np.array(values, np.float32))
    assert any(np.any(np.diff(held[1][a:b]) < 0) for a, b in zip(indptr[:-1], indptr[1:]))     # unsorted rows exist
    assert (held[2] == 0).sum() > 0
    dense = np.zeros((n_users, n_items), np.float32)
    for u in range(n_users):
        for e in range(indptr[u], indptr[u + 1]):
            if held[2][e] != 0:
                dense[u, held[1][e]] = held[2][e]
    rows = rng.permutation(n_users)[:45]
    n = _check(dense, r, seed=8, rows=rows, held=held)
    assert n > 200
    # and the mapping on its own: the items are exactly the negatives of the ordinals random.sample(range(n_neg), r) drew
    random.seed(8)
    crow, citem, draws, _ = opr_draw(held, rows, n_items, r)
    random.seed(8)
    for c in range(len(crow)):
        u = rows[int(crow[c])]
        neg = np.flatnonzero(dense[u] == 0)
        assert dense[u, int(citem[c])] != 0
        assert np.array_equal(draws[c].numpy(), neg[random.sample(range(len(neg)), r)])


def test_bad_arguments_are_errors():
    from rectorch_amd._lib import RtxError
    held = _held(csr_matrix(np.eye(3, dtype=np.float32)))
    with pytest.raises(RtxError):
        opr_draw((held[0], np.array([0, 1, 5], np.int32), None), np.arange(3), 3, 1)    # a column outside [0, n_items)
