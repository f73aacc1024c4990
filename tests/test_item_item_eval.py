"""GPU: EASE and ADMM_Slim scored, ranked and evaluated by fold-in (``score_rows``, ``recommend_rows``, ``evaluate``,
``one_plus_random``).

Families: ``ease`` on g10_ease_binary; ``admm`` on g14_admm_slim with ``item_bias=True``, ``num_iter=7`` (as test_recommend_models.py).
The device route of ``evaluate`` is compared with ``Metrics.compute`` on ``score_rows``' host copy at 1e-12 (the project's bound for
these metrics); everything that goes through the same kernel twice is compared bitwise.
"""
import os
import random
import tempfile

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

from conftest import load_golden

pytestmark = pytest.mark.gpu

N_TEST = 23
METRICS = ["ndcg@10", "recall@10", "hit@5", "mrr@20", "ndcg@100"]
_FITTED = {}


def _fitted(family):
    """(model, X) fitted once per family and shared: no test changes either"""
    if family not in _FITTED:
        from rectorch_amd.models import ADMM_Slim, EASE
        if family == "ease":
            g = load_golden("g10_ease_binary")
            X = csr_matrix(g["X"].astype(np.float64))
            model = EASE(lam=float(g["lam"]))
            model.train(X)
        else:
            g = load_golden("g14_admm_slim")
            X = csr_matrix(g["Xa"].astype(np.float64))
            model = ADMM_Slim(lambda1=float(g["hp"][0]), lambda2=float(g["hp"][1]), rho=float(g["hp"][2]), item_bias=True)
            model.train(X, num_iter=7)
        _FITTED[family] = (model, X)
    return _FITTED[family]


def _split(family, seed=3):
    """23 users of the training matrix: (ids, their rows, held-out rows disjoint from them with at least one item each)"""
    _, X = _fitted(family)
    rng = np.random.RandomState(seed)
    ids = rng.choice(X.shape[0], N_TEST, replace=False)
    tr = X[ids]
    dense = tr.toarray()
    te = ((rng.rand(*dense.shape) < 0.06) & (dense == 0)).astype(np.float64)
    for u in np.flatnonzero(te.sum(axis=1) == 0):
        te[u, np.flatnonzero(dense[u] == 0)[0]] = 1.0
    return ids, tr, csr_matrix(te)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _lexsort(scores, k):
    ids = np.broadcast_to(np.arange(scores.shape[1]), scores.shape)
    return np.lexsort((ids, -scores), axis=1)[:, :k]


def _distinct_rows(scores):
    """argpartition's order among equal scores is unspecified: the finite scores of every row must be distinct"""
    for row in scores:
        fin = row[np.isfinite(row)]
        if len(np.unique(fin)) != len(fin):
            return False
    return True


def _close(got, want, tag):
    assert set(got) == set(want), tag
    for m in want:
        g, w = np.asarray(got[m]), np.asarray(want[m])
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, m, g.shape, w.shape, g.dtype, w.dtype)
        if w.dtype == bool:
            assert np.array_equal(g, w), (tag, m)
        else:
            assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, m)
            ok = ~np.isnan(w)
            assert float(np.max(np.abs(g[ok] - w[ok]))) <= 1e-12, (tag, m, float(np.max(np.abs(g[ok] - w[ok]))))


@pytest.mark.parametrize("family", ["ease", "admm"])
def test_fold_in_of_training_rows_equals_the_look_up(family):
    model, X = _fitted(family)
    ids, tr, _ = _split(family)
    for remove_train in (True, False):
        want = model.predict(ids, tr, remove_train=remove_train, as_tensor=True)[0]
        got = model.score_rows(tr, remove_train=remove_train, as_tensor=True)
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == (N_TEST, X.shape[1])
        assert torch.equal(got.cpu().view(torch.int64), want.cpu().view(torch.int64)), (family, remove_train)
        host = model.score_rows(tr, remove_train=remove_train)
        assert isinstance(host, np.ndarray) and np.array_equal(_bits(host), _bits(got.cpu().numpy()))
        assert np.array_equal(np.isneginf(host), (tr.toarray() != 0) & remove_train)
    # a resident matrix is taken as it is
    from rectorch_amd.engine import CsrMatrix
    assert np.array_equal(_bits(model.score_rows(CsrMatrix(tr))), _bits(model.score_rows(tr)))


@pytest.mark.parametrize("family", ["ease", "admm"])
def test_users_the_fit_never_saw(family):
    """rows @ B in numpy float64, B read back from the solver (+ ADMM's bias term: (x - b) C + b, b = the training column sums).
    Bounds: those of the predict parity tests -- EASE 1e-10 absolute (tests/test_gpu_parity.py:872, test_ease_binary_g10), ADMM
    with item_bias 10 x FLOOR["a_nn1_l11_ib1_it7"] = 4.4e-10 relative to max |reference| (tests/test_admm_slim.py:225)."""
    model, X = _fitted(family)
    n_items = X.shape[1]
    rng = np.random.RandomState(17)
    new = (rng.rand(19, n_items) < 0.07).astype(np.float64)
    new[4] = 0.0                                   # a user without history
    known = {row.tobytes() for row in X.toarray()}
    assert all(row.tobytes() not in known for row in new[np.arange(19) != 4]), "the rows must not be training rows"
    if family == "ease":
        B = model._solver.weights().cpu().numpy()
        ref = new @ B
    else:
        Cm = model._solver.copy("C").cpu().numpy()
        b = np.asarray(X.sum(axis=0)).ravel()
        ref = (new - b) @ Cm + b
    got = model.score_rows(csr_matrix(new), remove_train=False)
    err = float(np.max(np.abs(got - ref)))
    print("%s fold-in of new users: max |diff| %.2e, max |ref| %.2e" % (family, err, float(np.max(np.abs(ref)))))
    if family == "ease":
        assert err <= 1e-10
    else:
        assert err / float(np.max(np.abs(ref))) <= 10 * 4.4e-11
    masked = model.score_rows(csr_matrix(new))
    assert np.array_equal(np.isneginf(masked), new != 0)
    assert np.array_equal(_bits(masked[new == 0]), _bits(got[new == 0]))


@pytest.mark.parametrize("family", ["ease", "admm"])
def test_recommend_rows_equals_the_lexsort_of_score_rows(family):
    model, X = _fitted(family)
    _, tr, _ = _split(family)
    n_items = X.shape[1]
    from rectorch_amd.models import _recommend_rows_item_item
    for remove_train in (True, False):
        pred = model.score_rows(tr, remove_train=remove_train)
        for k in (10, n_items - 1):
            items, vals = model.recommend_rows(tr, k=k, remove_train=remove_train)
            assert items.is_cuda and items.dtype == torch.int32 and vals.dtype == torch.float64 and items.shape == (N_TEST, k)
            want = _lexsort(pred, k)
            assert np.array_equal(items.cpu().numpy(), want), (family, remove_train, k)
            assert np.array_equal(_bits(vals.cpu().numpy()), _bits(np.take_along_axis(pred, want, axis=1)))
        a, _ = _recommend_rows_item_item(model, tr, 10, remove_train, chunk=7)       # several fills of the scratch buffer
        assert np.array_equal(a.cpu().numpy(), _lexsort(pred, 10))
    items, vals = model.recommend_rows(tr, k=2000)                                   # above the kernel's 1024: the host sort
    pred = model.score_rows(tr)
    assert np.array_equal(items.cpu().numpy(), _lexsort(pred, n_items))
    assert np.array_equal(_bits(vals.cpu().numpy()), _bits(np.take_along_axis(pred, _lexsort(pred, n_items), axis=1)))
    # the training-row recommend() still gives what it gave: the same lists as the fold-in of the same rows
    ids, tr, _ = _split(family)
    assert torch.equal(model.recommend(ids, tr, k=10)[0].cpu(), model.recommend_rows(tr, k=10)[0].cpu())


@pytest.mark.parametrize("family", ["ease", "admm"])
def test_evaluate_on_the_device_equals_metrics_on_score_rows(family):
    from rectorch_amd.evaluation import _item_item_plan, evaluate
    from rectorch_amd.metrics import Metrics
    from rectorch_amd.samplers import DataSampler
    model, X = _fitted(family)
    _, tr, te = _split(family)
    scores = model.score_rows(tr)
    assert _distinct_rows(scores), "the fixture's scores tie: Metrics' order among them is unspecified"
    want = Metrics.compute(scores, te.toarray(), METRICS)
    smp = DataSampler(tr, te, batch_size=7, shuffle=False)
    assert smp.resident and _item_item_plan(model, smp, METRICS) is not None
    got = evaluate(model, smp, METRICS)
    _close(got, want, (family, "device"))
    from rectorch_amd.evaluation import _evaluate_item_item
    _close(_evaluate_item_item(model, smp, METRICS, chunk=5), want, (family, "device, chunks of 5"))
    # shuffled: per-user arrays in loader order
    np.random.seed(77)
    idx = list(range(N_TEST))                      # the permutation DataSampler draws from this seed
    np.random.shuffle(idx)
    np.random.seed(77)
    got = evaluate(model, DataSampler(tr, te, batch_size=7, shuffle=True), METRICS)
    _close(got, {m: v[idx] for m, v in want.items()}, (family, "shuffled"))
    # the host loop: a host sampler, device_metrics off, a cut-off above the kernel's 1024
    host_smp = DataSampler(tr, te, batch_size=7, shuffle=False, device="cpu")
    assert _item_item_plan(model, host_smp, METRICS) is None
    _close(evaluate(model, host_smp, METRICS), want, (family, "host sampler"))
    model.device_metrics = False
    try:
        assert _item_item_plan(model, smp, METRICS) is None
        _close(evaluate(model, smp, METRICS), want, (family, "device_metrics off"))
    finally:
        del model.device_metrics
    big = METRICS + ["recall@2000"]
    assert _item_item_plan(model, smp, big) is None
    _close(evaluate(model, smp, big), Metrics.compute(scores, te.toarray(), big), (family, "recall@2000"))


@pytest.mark.parametrize("family", ["ease", "admm"])
def test_one_plus_random_device_equals_the_host_loop(family):
    from rectorch_amd.evaluation import _item_item_plan, one_plus_random
    from rectorch_amd.samplers import DataSampler
    model, X = _fitted(family)
    _, tr, te = _split(family)
    mets = ["ndcg@10", "recall@5", "hit@1", "mrr@20"]
    smp = DataSampler(tr, te, batch_size=7, shuffle=False)
    assert _item_item_plan(model, smp, mets) is not None
    random.seed(5)
    dev = one_plus_random(model, smp, mets, r=50)
    state_dev = random.getstate()
    model.device_metrics = False
    try:
        random.seed(5)
        host = one_plus_random(model, smp, mets, r=50)
        state_host = random.getstate()
    finally:
        del model.device_metrics
    assert state_dev == state_host
    n_contests = int((te.toarray() != 0).sum())
    for m in mets:
        assert dev[m].shape == host[m].shape == (n_contests, ) and dev[m].dtype == host[m].dtype, m
        assert np.array_equal(dev[m], host[m]), (family, m)
    # a held-out row with fewer than r negatives: ValueError on both routes
    n_items = X.shape[1]
    crowded = te.toarray()
    crowded[2, :n_items - 20] = 1.0
    short = DataSampler(tr, csr_matrix(crowded), batch_size=7, shuffle=False)
    with pytest.raises(ValueError):
        one_plus_random(model, short, mets, r=50)
    model.device_metrics = False
    try:
        with pytest.raises(ValueError):
            one_plus_random(model, short, mets, r=50)
    finally:
        del model.device_metrics


def test_a_score_rows_override_is_what_evaluate_ranks():
    from rectorch_amd.evaluation import _item_item_plan, evaluate
    from rectorch_amd.metrics import Metrics
    from rectorch_amd.models import EASE
    from rectorch_amd.samplers import DataSampler
    base, X = _fitted("ease")
    _, tr, te = _split("ease")
    te = te.toarray()
    te[:, 17] = 1.0                                # everybody holds item 17 out ...
    trd = tr.toarray()
    trd[:, 17] = 0.0                               # ... and nobody has it

    class Boosted(EASE):
        def score_rows(self, rows, remove_train=True, as_tensor=False):
            scores = super().score_rows(rows, remove_train=remove_train, as_tensor=as_tensor)
            scores[:, 17] += 1e4
            return scores

    model = Boosted(lam=base.lam)
    model._solver = base._solver                   # the same fit
    smp = DataSampler(csr_matrix(trd), csr_matrix(te), batch_size=7, shuffle=False)
    assert _item_item_plan(base, smp, ["mrr@10"]) is not None and _item_item_plan(model, smp, ["mrr@10"]) is None
    got = evaluate(model, smp, ["mrr@10", "hit@1"])
    assert (got["mrr@10"] == 1.0).all() and got["hit@1"].all()
    want = Metrics.compute(model.score_rows(csr_matrix(trd)), te, ["mrr@10", "hit@1"])
    _close(got, want, "override")
    assert not (evaluate(base, smp, ["mrr@10"])["mrr@10"] == 1.0).all()


@pytest.mark.parametrize("family", ["ease", "admm"])
def test_errors(family):
    from rectorch_amd.engine import CsrMatrix
    from rectorch_amd.evaluation import evaluate
    from rectorch_amd.models import ADMM_Slim, EASE
    from rectorch_amd.samplers import DataSampler
    model, X = _fitted(family)
    _, tr, te = _split(family)
    fresh = EASE() if family == "ease" else ADMM_Slim()
    for call in (lambda m: m.score_rows(tr), lambda m: m.recommend_rows(tr), lambda m: evaluate(m, DataSampler(tr, te, batch_size=7, shuffle=False), METRICS)):
        with pytest.raises(RuntimeError):
            call(fresh)
    # a model restored by load_model holds the training users' score matrix, not the item-item matrix
    tmp = tempfile.NamedTemporaryFile()
    model.save_model(tmp.name)
    try:
        loaded = EASE() if family == "ease" else ADMM_Slim()
        loaded.load_model(tmp.name + ".npy")
    finally:
        os.remove(tmp.name + ".npy")
    assert loaded._solver is None and loaded.model is not None
    with pytest.raises(RuntimeError):
        loaded.score_rows(tr)
    with pytest.raises(RuntimeError):
        loaded.recommend_rows(tr)
    model._model = None                            # (save_model materialised the host matrix on the shared model: drop the copy)
    narrow = csr_matrix(tr.toarray()[:, :-1])
    with pytest.raises(ValueError):
        model.score_rows(narrow)
    with pytest.raises(ValueError):
        model.recommend_rows(narrow)
    with pytest.raises(ValueError):
        model._solver.scores(np.arange(3), X=CsrMatrix(narrow))
    with pytest.raises(IndexError):
        model._solver.scores(np.array([0, N_TEST]), X=CsrMatrix(tr))
