"""CPU: ItemKNN without a device -- the native driver's host mode, the float64 restatement against its brute force, the binding,
the constructor's refusals and the save-file layout."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.sparse import csr_matrix

from conftest import ROOT
import knn_ref64 as R


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_native_driver_host_mode():
    path = os.path.join(ROOT, "build", "native", "test_knn")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-s", "-f", "knn.mk"])
    out = subprocess.run([path, "--host"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "KNN TESTS PASSED" in out.stdout and "host reference only" in out.stdout


def _matrix(kind, U, n, seed):
    """binary, or half-star ratings; columns 0, n // 2 and n - 1 identical (exact ties across ids), column 1 empty, user 2 empty"""
    rng = np.random.RandomState(seed)
    d = (rng.rand(U, n) < 0.3).astype(np.float64)
    if kind == "rated":
        d *= rng.randint(1, 11, size=d.shape) * 0.5
    if n >= 4:
        d[:, 1] = 0
        d[:, n // 2] = d[:, 0]
        d[:, n - 1] = d[:, 0]
    if U > 2:
        d[2] = 0
    return csr_matrix(d)


@pytest.mark.parametrize("kind,sim", [("binary", "cosine"), ("binary", "jaccard"), ("rated", "cosine")])
@pytest.mark.parametrize("normalize", [False, True])
def test_restatement_against_brute_force(kind, sim, normalize):
    for seed, (U, n) in enumerate([(1, 1), (3, 2), (9, 7), (14, 12), (25, 17)]):
        X = _matrix(kind, U, n, seed)
        for k in sorted({1, 3, max(n - 1, 1), n, n + 5}):
            for shrink in (0.0, 2.5):
                W = R.fit(X, k, shrink, sim, normalize)
                Wd, present, sc = R.brute_force(X, k, shrink, sim, normalize)
                tag = (kind, sim, normalize, U, n, k, shrink)
                assert W.has_sorted_indices and np.array_equal(W.toarray() != 0, present), tag     # (similarities are > 0)
                assert W.nnz == int(present.sum()), tag
                assert np.array_equal(_bits(W.toarray()), _bits(Wd)), tag
                assert np.array_equal(_bits(R.scores(X, W)), _bits(sc)), tag
                # at most k neighbours per item, and a symmetric S
                assert (np.diff(W.tocsc().indptr) <= k).all(), tag
                S = R.similarity(R.gram(X), shrink, sim)
                assert np.array_equal(_bits(S), _bits(S.T)), tag


def test_tie_rule_and_list_order():
    # items 0, 2 and 3 are identical columns, item 1 co-occurs with them once
    X = csr_matrix(np.array([[1, 1, 1, 1], [1, 0, 1, 1], [1, 0, 1, 1], [0, 0, 0, 0]], dtype=np.float64))
    S = R.similarity(R.gram(X), 0.0, "cosine")
    assert S[0, 2] == S[0, 3] == S[2, 3] and np.isneginf(np.diag(S)).all()
    nb = R.neighbours(S, 1)
    assert [int(ids[0]) for ids, _ in nb] == [2, 0, 0, 0]          # the lowest id among the equal best
    nb = R.neighbours(S, 2)
    assert [list(map(int, ids)) for ids, _ in nb] == [[2, 3], [0, 2], [0, 3], [0, 2]]
    W = R.weights(S, 1)
    assert sorted(zip(*W.nonzero())) == [(0, 1), (0, 2), (0, 3), (2, 0)]
    Wn = R.weights(S, 2, normalize=True)
    assert np.allclose(np.asarray(Wn.sum(axis=0)).ravel(), 1.0)
    # a mask row gives -inf exactly at its stored non-zeros
    sc = R.scores(X, W, mask=X)
    assert np.array_equal(np.isneginf(sc), X.toarray() != 0) and (sc[3] == 0).all()
    assert R.fma(0.1, 3.0, -0.3) == 2.7755575615628914e-17      # the product's rounding error survives: one rounding, not two


def test_entry_points_are_exported_declared_and_bound():
    from rectorch_amd import _lib
    raw = C.CDLL(_lib.build())
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rectorch_hip.h")).read(), flags=re.S)
    for name, n_args in (("rtx_knn_similarity", 5), ("rtx_knn_fit", 7), ("rtx_knn_load", 5), ("rtx_knn_destroy", 1), ("rtx_knn_shape", 3),
                         ("rtx_knn_copy", 5), ("rtx_knn_scores", 8), ("rtx_knn_timings", 5)):
        assert hasattr(raw, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in the header" % name
        assert len(m.group(1).split(",")) == n_args, name
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == n_args, name
    assert re.search(r"#define RTX_KNN_COSINE 0\n#define RTX_KNN_JACCARD 1\n", text)
    assert (_lib.RTX_KNN_COSINE, _lib.RTX_KNN_JACCARD) == (0, 1) and _lib.KNN_MAX_K == 1024
    assert _lib.lib().rtx_abi_version() == 8
    # refusals that need no device: NULL arguments, and rtx_knn_load's checks of its host arrays
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rtx_knn_fit(None, 3, 0.0, 0, 0, C.byref(h), None) != 0 and not h.value
    assert lib.rtx_knn_scores(None, None, None, 0, None, None, None, None) != 0
    indptr = np.array([0, 2, 2, 3], dtype=np.int64)
    vals = np.array([1.0, 2.0, 3.0])
    for bad, word in ((np.array([2, 0, 1], dtype=np.int32), "not sorted"), (np.array([0, 3, 1], dtype=np.int32), "outside")):
        rc = lib.rtx_knn_load(3, indptr.ctypes.data_as(C.c_void_p), bad.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), C.byref(h))
        assert rc == -1 and not h.value and word in lib.rtx_last_error().decode()


@pytest.mark.parametrize("kwargs,word", [(dict(k=0), "[1, 1024]"), (dict(k=1025), "[1, 1024]"), (dict(k=2.5), "[1, 1024]"), (dict(k=True), "[1, 1024]"),
                                         (dict(shrink=-0.5), ">= 0"), (dict(shrink=float("nan")), ">= 0"), (dict(shrink=float("inf")), ">= 0"),
                                         (dict(shrink="much"), ">= 0"), (dict(similarity="dice"), "'cosine', 'jaccard'"),
                                         (dict(similarity=None), "'cosine', 'jaccard'")])
def test_constructor_refusals_name_what_is_supported(kwargs, word):
    from rectorch_amd.models import ItemKNN
    with pytest.raises(ValueError) as e:
        ItemKNN(**kwargs)
    assert word in str(e.value) and list(kwargs)[0] in str(e.value)


def test_defaults_repr_and_untrained_errors():
    from rectorch_amd.evaluation import _is_item_item
    from rectorch_amd.models import ItemKNN, RecSysModel
    m = ItemKNN()
    assert (m.k, m.shrink, m.similarity, m.normalize) == (100, 0.0, "cosine", False) and isinstance(m, RecSysModel)
    assert m.W is None and _is_item_item(m)
    assert str(m) == repr(m) == "ItemKNN(k=100, shrink=0.0000, similarity=cosine, normalize=False) - not trained yet!"
    X = csr_matrix(np.eye(3))
    for call in (lambda: m.predict([0], X), lambda: m.recommend([0], X), lambda: m.score_rows(X), lambda: m.recommend_rows(X)):
        with pytest.raises(RuntimeError):
            call()


def test_save_file_layout(tmp_path):
    """np.save of a dict {'k', 'shrink', 'similarity', 'normalize', 'W'} with W a float64 csr_matrix, in the family's style"""
    from rectorch_amd.models import ItemKNN
    m = ItemKNN(k=7, shrink=1.5, similarity="jaccard", normalize=True)
    m._W = R.fit(_matrix("binary", 14, 12, 1), 7, 1.5, "jaccard", True)          # (what a fit leaves behind once W was read)
    path = str(tmp_path / "knn.npy")
    m.save_model(path)
    state = np.load(path, allow_pickle=True)[()]
    assert sorted(state) == ["W", "k", "normalize", "shrink", "similarity"]
    assert (state["k"], state["shrink"], state["similarity"], state["normalize"]) == (7, 1.5, "jaccard", True)
    W = state["W"]
    assert isinstance(W, csr_matrix) and W.dtype == np.float64 and W.shape == (12, 12)
    assert np.array_equal(_bits(W.toarray()), _bits(m._W.toarray()))
