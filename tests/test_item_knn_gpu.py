"""GPU: ItemKNN fitted, scored, ranked, evaluated, saved and loaded on the device, against the float64 restatement of knn_ref64.

Training matrices: 300 users x 257 items, binary (columns 0, 128 and 256 identical: exact ties across ids; column 1 and user 5 empty)
and half-star ratings (every Gram entry exact in float64, so numpy's G is the device's).  COS_ULPS is the native driver's bound for a
cosine against the host (tests/native/test_knn.cpp derives it: 13 units in the last place on an exact Gram matrix).
"""
import os
import random
import subprocess

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

from conftest import ROOT
import knn_ref64 as R

pytestmark = pytest.mark.gpu

U, N, K = 300, 257, 10
N_TEST = 23
COS_ULPS = 13
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _data(kind):
    if kind not in _CACHE:
        rng = np.random.RandomState(11 if kind == "binary" else 12)
        d = (rng.rand(U, N) < 0.08).astype(np.float64)
        if kind == "rated":
            d *= rng.randint(1, 11, size=d.shape) * 0.5
        else:
            d[:, 1] = 0
            d[:, N // 2] = d[:, 0]
            d[:, N - 1] = d[:, 0]
            d[5] = 0
        _CACHE[kind] = csr_matrix(d)
    return _CACHE[kind]


def _fitted(kind, similarity="cosine", normalize=False, shrink=0.0, k=K):
    """a model fitted once per setting and shared: no test changes it"""
    key = (kind, similarity, normalize, shrink, k)
    if key not in _CACHE:
        from rectorch_amd.models import ItemKNN
        m = ItemKNN(k=k, shrink=shrink, similarity=similarity, normalize=normalize)
        m.train(_data(kind))
        _CACHE[key] = m
    return _CACHE[key]


def _split(kind, seed=3):
    X = _data(kind)
    rng = np.random.RandomState(seed)
    ids = rng.choice(X.shape[0], N_TEST, replace=False)
    tr = X[ids]
    dense = tr.toarray()
    te = ((rng.rand(*dense.shape) < 0.06) & (dense == 0)).astype(np.float64)
    for u in np.flatnonzero(te.sum(axis=1) == 0):
        te[u, np.flatnonzero(dense[u] == 0)[0]] = 1.0
    return ids, tr, csr_matrix(te)


def _lexsort(scores, k):
    ids = np.broadcast_to(np.arange(scores.shape[1]), scores.shape)
    return np.lexsort((ids, -scores), axis=1)[:, :k]


def _same_w(got, want, tag):
    assert got.shape == want.shape and got.dtype == np.float64, tag
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), tag
    assert np.array_equal(_bits(got.data), _bits(want.data)), tag


# ---- the native driver ------------------------------------------------------------------------------------------------------------
def test_native_driver():
    path = os.path.join(ROOT, "build", "native", "test_knn")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-s", "-f", "knn.mk"])
    out = subprocess.run(["timeout", "-k", "10", "300", path], capture_output=True, text=True)
    print("\n".join(line for line in out.stdout.splitlines() if "largest cosine distance" in line))
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "KNN TESTS PASSED" in out.stdout and "host reference only" not in out.stdout


# ---- training -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True])
def test_jaccard_w_is_bit_equal_to_the_restatement(normalize):
    for shrink in (0.0, 2.5):
        m = _fitted("binary", "jaccard", normalize, shrink)
        _same_w(m.W, R.fit(_data("binary"), K, shrink, "jaccard", normalize), (normalize, shrink))
    assert m.W is m.W and "nnz=%d" % m.W.nnz in str(m)


@pytest.mark.parametrize("kind", ["binary", "rated"])
@pytest.mark.parametrize("normalize", [False, True])
def test_cosine_w_is_the_selection_of_the_device_similarity(kind, normalize):
    from rectorch_amd import engine
    X = _data(kind)
    for shrink in (0.0, 10.0):
        S = engine.knn_similarity(X, shrink, "cosine")
        assert S.is_cuda and S.dtype == torch.float64 and S.shape == (N, N)
        S = S.cpu().numpy()
        ref = R.similarity(R.gram(X), shrink, "cosine")
        assert np.array_equal(np.isneginf(S), np.isneginf(ref)) and np.isneginf(np.diag(S)).all()
        fin = np.isfinite(ref)
        assert np.isfinite(S[fin]).all()
        dist = int(R.ulp_distance(S[fin], ref[fin]).max())
        print("cosine %s shrink=%g: %d ulps from numpy (bound %d)" % (kind, shrink, dist, COS_ULPS))
        assert dist <= COS_ULPS
        assert np.array_equal(_bits(S), _bits(S.T))
        m = _fitted(kind, "cosine", normalize, shrink)
        _same_w(m.W, R.weights(S, K, normalize), (kind, normalize, shrink))
        assert (np.diff(m.W.tocsc().indptr) <= K).all()
    t = m._solver.timings()
    assert t["fit_ms"] > 0 and t["gram_ms"] + t["sim_ms"] + t["select_ms"] <= t["fit_ms"] * 1.001 + 1e-3
    iptr, idx, val = m._solver.weights()
    assert iptr.dtype == torch.int64 and idx.dtype == torch.int32 and val.dtype == torch.float64 and int(iptr[-1]) == m.W.nnz == m._solver.nnz


def test_jaccard_similarity_is_bit_equal():
    from rectorch_amd import engine
    X = _data("binary")
    for shrink in (0.0, 0.3):
        S = engine.knn_similarity(X, shrink, "jaccard").cpu().numpy()
        assert np.array_equal(_bits(S), _bits(R.similarity(R.gram(X), shrink, "jaccard")))


# ---- scoring and lists ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["binary", "rated"])
def test_predict_equals_score_rows_and_the_restatement(kind):
    m = _fitted(kind, "cosine", kind == "rated")
    ids, tr, _ = _split(kind)
    for remove_train in (True, False):
        want = m.predict(ids, tr, remove_train=remove_train, as_tensor=True)[0]
        got = m.score_rows(tr, remove_train=remove_train, as_tensor=True)
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == (N_TEST, N)
        assert torch.equal(got.cpu().view(torch.int64), want.cpu().view(torch.int64)), (kind, remove_train)
        host = m.predict(ids, tr, remove_train=remove_train)[0]
        assert isinstance(host, np.ndarray) and np.array_equal(_bits(host), _bits(got.cpu().numpy()))
        assert np.array_equal(np.isneginf(host), (tr.toarray() != 0) & remove_train)
        assert np.array_equal(_bits(host), _bits(R.scores(tr, m.W, mask=tr if remove_train else None))), (kind, remove_train)


@pytest.mark.parametrize("kind", ["binary", "rated"])
def test_recommend_equals_the_lexsort_of_predict(kind):
    m = _fitted(kind, "cosine", False)
    ids, tr, _ = _split(kind)
    for remove_train in (True, False):
        pred = m.predict(ids, tr, remove_train=remove_train)[0]
        for k in (10, N - 1):
            items, vals = m.recommend(ids, tr, k=k, remove_train=remove_train)
            assert items.is_cuda and items.dtype == torch.int32 and vals.dtype == torch.float64 and items.shape == (N_TEST, k)
            want = _lexsort(pred, k)
            assert np.array_equal(items.cpu().numpy(), want), (kind, remove_train, k)
            assert np.array_equal(_bits(vals.cpu().numpy()), _bits(np.take_along_axis(pred, want, axis=1)))


def test_recommend_rows_on_users_the_fit_never_saw():
    m = _fitted("rated", "cosine", True)
    rng = np.random.RandomState(17)
    new = (rng.rand(19, N) < 0.07) * (rng.randint(1, 11, size=(19, N)) * 0.5)
    new[4] = 0.0                                   # a user without history
    known = {row.tobytes() for row in _data("rated").toarray()}
    assert all(row.tobytes() not in known for row in new[np.arange(19) != 4]), "the rows must not be training rows"
    rows = csr_matrix(new)
    pred = m.score_rows(rows, remove_train=False)
    assert np.array_equal(_bits(pred), _bits(R.scores(rows, m.W))) and (pred[4] == 0).all()
    masked = m.score_rows(rows)
    assert np.array_equal(np.isneginf(masked), new != 0)
    for remove_train, sc in ((True, masked), (False, pred)):
        items, vals = m.recommend_rows(rows, k=10, remove_train=remove_train)
        want = _lexsort(sc, 10)
        assert np.array_equal(items.cpu().numpy(), want), remove_train
        assert np.array_equal(_bits(vals.cpu().numpy()), _bits(np.take_along_axis(sc, want, axis=1)))


# ---- evaluation -------------------------------------------------------------------------------------------------------------------
METRICS = ["ndcg@10", "recall@20", "hit@5", "mrr@10"]


def _device_and_host_metrics():
    """(evaluate() on a resident DataSampler, Metrics.compute on the host copy of the scores), computed once"""
    if "eval" not in _CACHE:
        from rectorch_amd.evaluation import _item_item_plan, evaluate
        from rectorch_amd.metrics import Metrics
        from rectorch_amd.samplers import DataSampler
        m = _fitted("rated", "cosine", True)
        _, tr, te = _split("rated")
        scores = m.score_rows(tr)
        for row in scores:                         # Metrics' order among equal scores is unspecified: the 21 best must be distinct
            top = np.sort(row[np.isfinite(row)])[::-1][:21]
            assert len(np.unique(top)) == len(top), "the fixture's best scores tie"
        want = Metrics.compute(scores, te.toarray(), METRICS)
        smp = DataSampler(tr, te, batch_size=7, shuffle=False)
        assert smp.resident and _item_item_plan(m, smp, METRICS) is not None
        got = evaluate(m, smp, METRICS)
        assert set(got) == set(want)
        _CACHE["eval"] = (got, want)
    return _CACHE["eval"]


@pytest.mark.parametrize("name", METRICS)
def test_evaluate_on_the_device_equals_metrics_on_the_host_scores(name):
    """Exact equality, metric by metric.  nDCG can be exact because k_list_metrics takes log2 of the first 1 024 ranks from a table
    the host writes with the log2 numpy calls, and adds the discounts of the ideal DCG in rank order, as Metrics' cumsum does (with
    the device's own log2 and a lane butterfly ndcg@10 was 2.78e-17, one ulp, off); and no list of this fixture holds more than two
    hits in its first ten places, so the gain's sum has one order."""
    got, want = _device_and_host_metrics()
    g, w = np.asarray(got[name]), np.asarray(want[name])
    assert g.shape == w.shape and g.dtype == w.dtype, name
    if w.dtype != bool:
        print("%s: max |device - host| = %.3g" % (name, float(np.nanmax(np.abs(g.astype(np.float64) - w.astype(np.float64))))))
    assert np.array_equal(g, w, equal_nan=w.dtype != bool), name


def test_evaluate_within_the_list_kernel_bound_and_from_lists():
    """every metric within 1e-12 of Metrics (the bound of tests/test_item_item_eval.py for the shared list-metrics kernel), from
    evaluate() and from metrics_from_lists on the model's own lists"""
    from rectorch_amd.evaluation import metrics_from_lists
    got, want = _device_and_host_metrics()
    for name in METRICS:
        g, w = np.asarray(got[name], dtype=np.float64), np.asarray(want[name], dtype=np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(w)), name
        ok = ~np.isnan(w)
        assert float(np.max(np.abs(g[ok] - w[ok]))) <= 1e-12, name
    m = _fitted("rated", "cosine", True)
    _, tr, te = _split("rated")
    lists = m.recommend_rows(tr, k=20)[0]
    again = metrics_from_lists(lists, te, METRICS)
    for name in METRICS:
        a, w = np.asarray(again[name]), np.asarray(want[name])
        assert a.shape == w.shape and a.dtype == w.dtype, name
        if w.dtype == bool:
            assert np.array_equal(a, w), name
        else:
            ok = ~np.isnan(w)
            assert np.array_equal(np.isnan(a), np.isnan(w)) and float(np.max(np.abs(a[ok] - w[ok]))) <= 1e-12, name


def test_one_plus_random_device_equals_the_host_route():
    """The device route ranks the positive first among equal scores; the host route ranks with numpy's argpartition, whose order among
    equal scores is unspecified (evaluation.one_plus_random's own words).  A neighbourhood model scores every item none of whose
    neighbours the user holds exactly 0, so the two routes are compared on a model with every neighbour kept (k = n - 1), whose scores
    are distinct -- which is asserted, not assumed."""
    from rectorch_amd.evaluation import _item_item_plan, one_plus_random
    from rectorch_amd.samplers import DataSampler
    m = _fitted("rated", "cosine", True, k=N - 1)
    _, tr, te = _split("rated")
    for row in m.score_rows(tr):
        fin = row[np.isfinite(row)]
        assert len(np.unique(fin)) == len(fin), "the fixture's scores tie"
    mets = ["ndcg@10", "recall@5", "hit@1", "mrr@20"]
    smp = DataSampler(tr, te, batch_size=7, shuffle=False)
    assert _item_item_plan(m, smp, mets) is not None
    random.seed(5)
    dev = one_plus_random(m, smp, mets, r=50)
    state_dev = random.getstate()
    m.device_metrics = False
    try:
        assert _item_item_plan(m, smp, mets) is None
        random.seed(5)
        host = one_plus_random(m, smp, mets, r=50)
        state_host = random.getstate()
    finally:
        del m.device_metrics
    assert state_dev == state_host
    n_contests = int((te.toarray() != 0).sum())
    for name in mets:
        assert dev[name].shape == host[name].shape == (n_contests, ) and dev[name].dtype == host[name].dtype, name
        assert np.array_equal(dev[name], host[name]), name


# ---- save and load ------------------------------------------------------------------------------------------------------------------
def test_save_and_load_give_the_same_bits(tmp_path):
    from rectorch_amd.evaluation import evaluate
    from rectorch_amd.models import ItemKNN
    from rectorch_amd.samplers import DataSampler
    m = _fitted("rated", "cosine", True)
    ids, tr, te = _split("rated")
    path = str(tmp_path / "knn.npy")
    m.save_model(path)
    back = ItemKNN()
    state = back.load_model(path)
    assert sorted(state) == ["W", "k", "normalize", "shrink", "similarity"]
    assert (back.k, back.shrink, back.similarity, back.normalize) == (K, 0.0, "cosine", True)
    _same_w(back.W, m.W, "loaded W")
    for remove_train in (True, False):
        assert np.array_equal(_bits(back.score_rows(tr, remove_train=remove_train)), _bits(m.score_rows(tr, remove_train=remove_train)))
    assert torch.equal(back.recommend_rows(tr, k=10)[0].cpu(), m.recommend_rows(tr, k=10)[0].cpu())
    smp = DataSampler(tr, te, batch_size=7, shuffle=False)
    a, b = evaluate(back, smp, METRICS), evaluate(m, smp, METRICS)
    for name in METRICS:
        assert np.array_equal(np.asarray(a[name]), np.asarray(b[name]), equal_nan=np.asarray(b[name]).dtype != bool), name
    for call in (lambda: back.predict(ids, tr), lambda: back.recommend(ids, tr)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "score_rows" in str(e.value)
    assert "nnz=%d" % m.W.nnz in str(back)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_carry_the_documented_messages():
    from rectorch_amd import _lib, engine
    from rectorch_amd.models import ItemKNN
    with pytest.raises(ValueError) as e:
        ItemKNN(k=1025)
    assert "[1, 1024]" in str(e.value)
    X = engine.CsrMatrix(_data("binary"))
    for k in (1025, 0):
        with pytest.raises(_lib.RtxError) as e:
            engine.KnnSolver(X, k)
        assert "k must be in [1, 1024]" in str(e.value)
    with pytest.raises(_lib.RtxError) as e:
        engine.KnnSolver(X, 3, shrink=-1.0)
    assert "shrink must be finite and >= 0" in str(e.value)
    m = ItemKNN(k=K, similarity="jaccard")
    with pytest.raises(_lib.RtxError) as e:
        m.train(_data("rated"))
    assert "binarise it first" in str(e.value) and m._solver is None
    with pytest.raises(_lib.RtxError) as e:
        engine.knn_similarity(_data("rated"), 0.0, "jaccard")
    assert "binarise it first" in str(e.value)
    with pytest.raises(ValueError):
        engine.knn_similarity(X, 0.0, "dice")
    # a stored value other than 1 that numpy calls binary-looking: 2.0 everywhere
    with pytest.raises(_lib.RtxError):
        engine.KnnSolver(_data("binary") * 2.0, 3, similarity="jaccard")
