"""CPU: the numpy half of ``evaluation.metrics_from_lists`` against ``Metrics.compute``.

The lists are the ``(score descending, item id ascending)`` lexsort of random tie-free float64 scores at [37, 300]; with full-length
lists a cut-off means the same in both (``min(k, n_items)``), so the two must agree to 1e-12 (the project's metric bound: the only
difference is the order of a few hundred float64 additions) and ``hit`` exactly.  Held-out rows: binary and ratings 1..5, with an empty
row, a one-item row and a full row.  This half is the oracle of the kernel test (tests/test_list_metrics_kernel.py).
"""
import numpy as np
import pytest
from scipy.sparse import csr_matrix

U, I = 37, 300
KS = (1, 5, 64, 299, 300, 1000)
METRICS = ["%s@%d" % (name, k) for k in KS for name in ("ndcg", "recall", "hit", "mrr")]


def _scores(seed=0):
    rng = np.random.RandomState(seed)
    s = rng.standard_normal((U, I))
    assert all(len(np.unique(row)) == I for row in s), "argpartition's order among ties is unspecified: the scores must be distinct"
    return s


def _heldout(ratings, seed=1):
    rng = np.random.RandomState(seed)
    te = (rng.rand(U, I) < 0.06).astype(np.float64)
    te[2] = 0.0                                    # a user without held-out items
    te[5] = 0.0
    te[5, 123] = 1.0                               # exactly one
    te[7] = 1.0                                    # every item
    if ratings:
        te *= rng.randint(1, 6, size=te.shape)
    return te


def _lists(scores):
    ids = np.broadcast_to(np.arange(scores.shape[1]), scores.shape)
    return np.lexsort((ids, -scores), axis=1).astype(np.int32)


def _close(got, want, tag):
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if want.dtype == bool:
        assert np.array_equal(got, want), tag
        return
    assert np.array_equal(np.isnan(got), np.isnan(want)), tag
    ok = ~np.isnan(want)
    assert float(np.max(np.abs(got[ok] - want[ok]))) <= 1e-12, tag


@pytest.mark.parametrize("ratings", [False, True])
def test_numpy_half_equals_metrics_compute(ratings):
    from rectorch_amd.evaluation import metrics_from_lists
    from rectorch_amd.metrics import Metrics
    scores, te = _scores(), _heldout(ratings)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = Metrics.compute(scores, te, METRICS)
    got = metrics_from_lists(_lists(scores), csr_matrix(te), METRICS)
    assert set(got) == set(METRICS)
    for m in METRICS:
        _close(got[m], want[m], (ratings, m))
    assert np.isnan(got["ndcg@5"][2]) and np.isnan(got["recall@5"][2]) and not got["hit@5"][2] and got["mrr@5"][2] == 0.0


def test_rows_short_lists_and_errors():
    from rectorch_amd.evaluation import metrics_from_lists
    scores, te = _scores(3), _heldout(True, 4)
    lists = _lists(scores)
    full = metrics_from_lists(lists, csr_matrix(te), ["ndcg@10", "mrr@300"])
    # `rows`: list b belongs to held-out row rows[b]
    perm = np.random.RandomState(5).permutation(U)
    got = metrics_from_lists(lists[perm], csr_matrix(te), ["ndcg@10", "mrr@300"], rows=perm)
    for m in full:
        assert np.array_equal(got[m], full[m][perm], equal_nan=True), m
    # lists of K = 10 items: a cut-off above K counts the K ranked items
    short = metrics_from_lists(lists[:, :10], csr_matrix(te), ["ndcg@10", "ndcg@50", "hit@50", "hit@10"])
    assert np.array_equal(short["ndcg@10"], full["ndcg@10"], equal_nan=True)
    assert np.array_equal(short["ndcg@50"], short["ndcg@10"], equal_nan=True) and np.array_equal(short["hit@50"], short["hit@10"])
    # an id outside the matrix has relevance 0
    odd = lists[:, :10].copy()
    odd[:, 0] = -1
    odd[:, 1] = I + 7
    assert (metrics_from_lists(odd, csr_matrix(te), ["mrr@2"])["mrr@2"] == 0).all()
    with pytest.raises(ValueError):
        metrics_from_lists(lists, csr_matrix(te), ["ndcg"])
    with pytest.raises(ValueError):
        metrics_from_lists(lists, csr_matrix(te), ["precision@5"])
    with pytest.raises(ValueError):
        metrics_from_lists(lists, csr_matrix(te[:5]), ["ndcg@5"])
