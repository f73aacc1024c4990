"""GPU: WMF fitted, folded in, scored, ranked, evaluated, saved and loaded on the device, against the float64 restatement of wmf_ref64.

Training matrices: 67 users x 45 items and 130 x 77, ratings 1 .. 5 at density 0.15, with 24 and 128 factors; alpha = 0.5, lam = 1.  The
fit is compared by max |Y_dev - Y_ref| / max |Y_ref| after 4 iterations from the same Y0; the bound is 16 x the spread between the
restatement's own two formulations (numpy.linalg.solve on matrix products; a loop over entries with scipy's Cholesky), measured in
the same test, floored at 64 * 2^-52.  The measured values are printed as "wmf_ulp:" lines (profiles/wmf_ulp.txt keeps one run's).
"""
import os
import random
import subprocess

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

from conftest import ROOT
import wmf_ref64 as R

pytestmark = pytest.mark.gpu

SHAPES = {"small": (67, 45, 24), "wide": (130, 77, 128)}
ALPHA, LAM, ITERS = 0.5, 1.0, 4
N_TEST = 23
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _data(kind):
    if kind not in _CACHE:
        U, I, _ = SHAPES[kind]
        rng = np.random.RandomState(21 if kind == "small" else 22)
        d = (rng.rand(U, I) < 0.15) * rng.randint(1, 6, size=(U, I)).astype(np.float64)
        d[5] = 0                                    # a user without history
        _CACHE[kind] = csr_matrix(d)
    return _CACHE[kind]


def _fitted(kind):
    """a model fitted once per matrix and shared: no test changes it"""
    key = ("model", kind)
    if key not in _CACHE:
        from rectorch_amd.models import WMF
        m = WMF(factors=SHAPES[kind][2], alpha=ALPHA, lam=LAM, num_iter=ITERS, seed=98765)
        m.train(_data(kind), verbose=0)
        _CACHE[key] = m
    return _CACHE[key]


def _y0(kind):
    _, I, f = SHAPES[kind]
    return np.random.RandomState(98765).normal(0, 0.01, (I, f))


def _split(kind, seed=3):
    X = _data(kind)
    rng = np.random.RandomState(seed)
    ids = rng.choice(np.setdiff1d(np.arange(X.shape[0]), [5]), N_TEST, replace=False)     # (user 5 has no history: every score 0)
    tr = X[ids]
    dense = tr.toarray()
    te = ((rng.rand(*dense.shape) < 0.1) & (dense == 0)).astype(np.float64)
    for u in np.flatnonzero(te.sum(axis=1) == 0):
        te[u, np.flatnonzero(dense[u] == 0)[0]] = 1.0
    return ids, tr, csr_matrix(te)


def _lexsort(scores, k):
    ids = np.broadcast_to(np.arange(scores.shape[1]), scores.shape)
    return np.lexsort((ids, -scores), axis=1)[:, :k]


# ---- the native driver ------------------------------------------------------------------------------------------------------------
def test_native_driver():
    path = os.path.join(ROOT, "build", "native", "test_wmf")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-s", "-f", "wmf.mk"])
    out = subprocess.run(["timeout", "-k", "10", "300", path], capture_output=True, text=True)
    print("\n".join(line for line in out.stdout.splitlines() if line.startswith("wmf_ulp:") or "largest relative error" in line))
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "WMF TESTS PASSED" in out.stdout and "host reference only" not in out.stdout


# ---- the fit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["small", "wide"])
def test_fit_against_the_restatement(kind):
    X = _data(kind)
    m = _fitted(kind)
    Ua, Ya, _ = R.fit(X, _y0(kind), ALPHA, LAM, ITERS, "solve")
    Ub, Yb, _ = R.fit(X, _y0(kind), ALPHA, LAM, ITERS, "loop")
    scale = np.abs(Ya).max()
    spread = np.abs(Ya - Yb).max() / scale
    bound = max(16 * spread, 64 * 2.0 ** -52)
    Y, Uf = m.item_factors, m.user_factors
    assert Y.shape == Ya.shape and Y.dtype == np.float64 and Uf.shape == Ua.shape
    dist = np.abs(Y - Ya).max() / scale
    dist_u = np.abs(Uf - Ua).max() / np.abs(Ua).max()
    print("wmf_ulp: fit %s, %d iterations: max |Y_dev - Y_ref| / max |Y_ref| = %.3e (user factors %.3e); spread of the two formulations "
          "%.3e, bound %.3e" % ("%d x %d x %d" % SHAPES[kind], ITERS, dist, dist_u, spread, bound))
    assert dist <= bound
    assert (Uf[5] == 0).all()                       # the user without history
    t = m._solver.timings()
    assert t["fit_ms"] > 0 and t["gram_ms"] + t["user_ms"] + t["item_ms"] <= t["fit_ms"] * 1.001 + 1e-3
    assert "model size=(%d, %d)" % (SHAPES[kind][1], SHAPES[kind][2]) in str(m)


@pytest.mark.parametrize("kind", ["small", "wide"])
def test_the_objective_of_the_device_factors_does_not_increase(kind):
    """evaluated in numpy from the device's factors after 1 .. 4 iterations (four fits from the same Y0: a fit of k iterations is the
    first k iterations of a longer one, which the bit-equality below also shows); slack: the evaluation's own rounding, one per term"""
    from rectorch_amd.engine import WmfSolver
    X = _data(kind)
    U, I, f = SHAPES[kind]
    obj = []
    for k in range(1, ITERS + 1):
        s = WmfSolver(X, _y0(kind), ALPHA, LAM, k)
        obj.append(R.objective(X, s.factors("users").cpu().numpy(), s.factors("items").cpu().numpy(), ALPHA, LAM))
    print("objective from the device factors:", obj)
    slack = (U * I + (U + I) * f) * 2.0 ** -52
    for a, b in zip(obj, obj[1:]):
        assert b <= a * (1 + slack), obj
    assert obj[-1] < obj[0]
    assert np.array_equal(_bits(s.factors("items").cpu().numpy()), _bits(_fitted(kind).item_factors))


@pytest.mark.parametrize("kind", ["small", "wide"])
def test_two_fits_from_the_same_y0_are_bit_equal(kind):
    from rectorch_amd.engine import WmfSolver
    a = WmfSolver.train(_data(kind), _y0(kind), ALPHA, LAM, ITERS)
    m = _fitted(kind)
    assert np.array_equal(_bits(a.factors("items").cpu().numpy()), _bits(m.item_factors))
    assert np.array_equal(_bits(a.factors("users").cpu().numpy()), _bits(m.user_factors))


def test_the_stand_alone_operators():
    """wmf_systems against numpy (summation-order bound of wmf_ref64's own comparison) and symmetric to the bit; wmf_solve_rows with
    the fitted item factors = the stored user factors' last half-sweep input, i.e. the fold-in of the training rows"""
    from rectorch_amd import engine
    X = _data("small")
    m = _fitted("small")
    Y = m.item_factors
    A, b = engine.wmf_systems(X, Y, ALPHA, LAM)
    assert A.is_cuda and A.dtype == torch.float64 and A.shape == (67, 24, 24) and b.shape == (67, 24)
    A, b = A.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(_bits(A), _bits(A.transpose(0, 2, 1)))
    Ar, br = R.systems(X, Y, ALPHA, LAM)
    n_terms = 45 + int(np.diff(X.indptr).max()) + 1
    mag = (np.abs(Y).T @ np.abs(Y)) * (1 + ALPHA * 5) + LAM
    assert (np.abs(A - Ar) <= 2 * n_terms * 2.0 ** -52 * mag[None]).all()
    assert (np.abs(b - br) <= 2 * n_terms * 2.0 ** -52 * (1 + ALPHA * 5) * np.abs(Y).sum(axis=0)[None]).all()
    ids = np.array([7, 5, 60, 0], dtype=np.int32)
    x = engine.wmf_solve_rows(X, Y, ALPHA, LAM, row_ids=ids).cpu().numpy()
    allx = engine.wmf_solve_rows(X, Y, ALPHA, LAM).cpu().numpy()
    assert np.array_equal(_bits(x), _bits(allx[ids])) and (x[1] == 0).all()


# ---- scoring and lists ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["small", "wide"])
def test_predict_equals_score_rows_and_the_restatement(kind):
    m = _fitted(kind)
    ids, tr, _ = _split(kind)
    I, f = SHAPES[kind][1], SHAPES[kind][2]
    for remove_train in (True, False):
        want = m.predict(ids, tr, remove_train=remove_train, as_tensor=True)[0]
        got = m.score_rows(tr, remove_train=remove_train, as_tensor=True)
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == (N_TEST, I)
        assert torch.equal(got.cpu().view(torch.int64), want.cpu().view(torch.int64)), (kind, remove_train)
        host = m.predict(ids, tr, remove_train=remove_train)[0]
        assert isinstance(host, np.ndarray) and np.array_equal(_bits(host), _bits(got.cpu().numpy()))
        assert np.array_equal(np.isneginf(host), (tr.toarray() != 0) & remove_train)
    # against numpy: the fold-in vector within the formulations' distance (kappa-scaled, as tests/test_wmf_host.py derives), then the
    # dot product within gamma_f sum |x y| of numpy's
    from rectorch_amd import engine
    Y = m.item_factors
    x = engine.wmf_solve_rows(tr, Y, ALPHA, LAM).cpu().numpy()
    A, _ = R.systems(tr, Y, ALPHA, LAM)
    xr = R.half_sweep(tr, Y, ALPHA, LAM)
    n_terms = I + int(np.diff(tr.indptr).max()) + 1
    for u in range(N_TEST):
        assert np.abs(x[u] - xr[u]).max() <= (4 * f * f + 2 * n_terms) * 2.0 ** -52 * np.linalg.cond(A[u]) * max(np.abs(xr[u]).max(), 1e-300), u
    gam = f * 2.0 ** -53 / (1 - f * 2.0 ** -53)
    assert (np.abs(host - x @ Y.T) <= 2 * gam * (np.abs(x) @ np.abs(Y).T) + 1e-300).all()


@pytest.mark.parametrize("kind", ["small", "wide"])
def test_recommend_equals_the_lexsort_of_predict(kind):
    m = _fitted(kind)
    ids, tr, _ = _split(kind)
    I = SHAPES[kind][1]
    for remove_train in (True, False):
        pred = m.predict(ids, tr, remove_train=remove_train)[0]
        for k in (10, I - 1):
            items, vals = m.recommend(ids, tr, k=k, remove_train=remove_train)
            assert items.is_cuda and items.dtype == torch.int32 and vals.dtype == torch.float64 and items.shape == (N_TEST, k)
            want = _lexsort(pred, k)
            assert np.array_equal(items.cpu().numpy(), want), (kind, remove_train, k)
            assert np.array_equal(_bits(vals.cpu().numpy()), _bits(np.take_along_axis(pred, want, axis=1)))


def test_recommend_rows_on_users_the_fit_never_saw():
    m = _fitted("small")
    I = SHAPES["small"][1]
    rng = np.random.RandomState(17)
    new = (rng.rand(19, I) < 0.2) * rng.randint(1, 6, size=(19, I)).astype(np.float64)
    new[4] = 0.0                                   # a user without history
    known = {row.tobytes() for row in _data("small").toarray()}
    assert all(row.tobytes() not in known for row in new[np.arange(19) != 4]), "the rows must not be training rows"
    rows = csr_matrix(new)
    pred = m.score_rows(rows, remove_train=False)
    assert (pred[4] == 0).all() and np.isfinite(pred).all()
    ref = R.scores(rows, m.item_factors, ALPHA, LAM)
    assert np.abs(pred - ref).max() <= 1e-9 * np.abs(ref).max()          # (a sanity distance: the bit-level checks are the driver's)
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
        m = _fitted("wide")
        _, tr, te = _split("wide")
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
    got, want = _device_and_host_metrics()
    g, w = np.asarray(got[name]), np.asarray(want[name])
    assert g.shape == w.shape and g.dtype == w.dtype, name
    if w.dtype != bool:
        print("%s: max |device - host| = %.3g" % (name, float(np.nanmax(np.abs(g.astype(np.float64) - w.astype(np.float64))))))
    assert np.array_equal(g, w, equal_nan=w.dtype != bool), name


def test_metrics_from_lists_on_the_models_own_lists():
    from rectorch_amd.evaluation import metrics_from_lists
    _, want = _device_and_host_metrics()
    m = _fitted("wide")
    _, tr, te = _split("wide")
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
    """The device route ranks the positive first among equal scores, the host route's order among equal scores is unspecified: the
    fixture's scores are distinct, which is asserted."""
    from rectorch_amd.evaluation import _item_item_plan, one_plus_random
    from rectorch_amd.samplers import DataSampler
    m = _fitted("wide")
    _, tr, te = _split("wide")
    for row in m.score_rows(tr):
        fin = row[np.isfinite(row)]
        assert len(np.unique(fin)) == len(fin), "the fixture's scores tie"
    mets = ["ndcg@10", "recall@5", "hit@1", "mrr@20"]
    smp = DataSampler(tr, te, batch_size=7, shuffle=False)
    assert _item_item_plan(m, smp, mets) is not None
    random.seed(5)
    dev = one_plus_random(m, smp, mets, r=30)
    state_dev = random.getstate()
    m.device_metrics = False
    try:
        assert _item_item_plan(m, smp, mets) is None
        random.seed(5)
        host = one_plus_random(m, smp, mets, r=30)
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
    from rectorch_amd.models import WMF
    from rectorch_amd.samplers import DataSampler
    m = _fitted("wide")
    ids, tr, te = _split("wide")
    path = str(tmp_path / "wmf.npy")
    m.save_model(path)
    back = WMF()
    state = back.load_model(path)
    assert sorted(state) == ["alpha", "factors", "item_factors", "lam", "num_iter", "seed", "user_factors"]
    assert (back.factors, back.alpha, back.lam, back.num_iter, back.seed) == (128, ALPHA, LAM, ITERS, 98765)
    assert np.array_equal(_bits(back.item_factors), _bits(m.item_factors)) and np.array_equal(_bits(back.user_factors), _bits(m.user_factors))
    assert np.array_equal(_bits(back._solver.factors("items").cpu().numpy()), _bits(m.item_factors))
    with pytest.raises(RuntimeError):
        back._solver.factors("users")
    for remove_train in (True, False):
        assert np.array_equal(_bits(back.score_rows(tr, remove_train=remove_train)), _bits(m.score_rows(tr, remove_train=remove_train)))
        assert np.array_equal(_bits(back.predict(ids, tr, remove_train=remove_train)[0]), _bits(m.predict(ids, tr, remove_train=remove_train)[0]))
    assert torch.equal(back.recommend_rows(tr, k=10)[0].cpu(), m.recommend_rows(tr, k=10)[0].cpu())
    assert torch.equal(back.recommend(ids, tr, k=10)[0].cpu(), m.recommend(ids, tr, k=10)[0].cpu())
    smp = DataSampler(tr, te, batch_size=7, shuffle=False)
    a, b = evaluate(back, smp, METRICS), evaluate(m, smp, METRICS)
    for name in METRICS:
        assert np.array_equal(np.asarray(a[name]), np.asarray(b[name]), equal_nan=np.asarray(b[name]).dtype != bool), name


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_carry_the_documented_messages():
    from rectorch_amd import _lib, engine
    from rectorch_amd.models import WMF
    X = _data("small")
    Y0 = _y0("small")
    with pytest.raises(_lib.RtxError) as e:
        engine.WmfSolver(X, Y0, ALPHA, 0.0, 2)
    assert "lam must be finite and > 0" in str(e.value)
    with pytest.raises(_lib.RtxError) as e:
        engine.WmfSolver(X, Y0, -1.0, LAM, 2)
    assert "alpha must be finite and >= 0" in str(e.value)
    with pytest.raises(_lib.RtxError) as e:
        engine.WmfSolver(X, np.zeros((45, 129)), ALPHA, LAM, 2)
    assert "f must be in [1, 128]" in str(e.value)
    zeros = X.copy().astype(np.float64)
    zeros.data[3] = 0.0                             # an explicit stored zero
    m = WMF(factors=8, alpha=ALPHA, lam=LAM, num_iter=1)
    with pytest.raises(_lib.RtxError) as e:
        m.train(zeros)
    assert "stores a value <= 0" in str(e.value) and m._solver is None
    with pytest.raises(_lib.RtxError) as e:
        engine.wmf_solve_rows(zeros, Y0, ALPHA, LAM)
    assert "stores a value <= 0" in str(e.value)
    bad = Y0.copy()
    bad[X.indices[0], 1] = np.nan
    with pytest.raises(_lib.RtxError) as e:
        engine.wmf_solve_rows(X, bad, ALPHA, LAM)
    assert "not positive definite" in str(e.value)
    with pytest.raises(ValueError):
        engine.WmfSolver(X, np.zeros((44, 8)), ALPHA, LAM, 1)
    with pytest.raises(ValueError):
        _fitted("small").predict([0, 1], X[:3])
