"""CPU: WMF without a device -- the native driver's host mode, the two formulations of the float64 restatement against each other,
the objective's descent, the binding, the constructor's refusals and the save-file layout."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.sparse import csr_matrix

from conftest import ROOT
import wmf_ref64 as R

SHAPES = [(67, 45, 24), (130, 77, 128), (40, 300, 17)]          # users x items x factors (the native driver's first three)
ALPHA, LAM = 0.5, 1.0
EPS = 2.0 ** -52


def _ratings(U, I, seed, density=None):
    rng = np.random.RandomState(seed)
    density = density if density is not None else (0.05 if I == 300 else 0.15)
    return csr_matrix((rng.rand(U, I) < density) * rng.randint(1, 6, size=(U, I)).astype(np.float64))


def _y0(I, f, seed=98765):
    return np.random.RandomState(seed).normal(0, 0.01, (I, f))


def test_native_driver_host_mode():
    path = os.path.join(ROOT, "build", "native", "test_wmf")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-s", "-f", "wmf.mk"])
    out = subprocess.run([path, "--host"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "WMF TESTS PASSED" in out.stdout and "host reference only" in out.stdout


@pytest.mark.parametrize("U,I,f", SHAPES)
def test_the_two_formulations_agree(U, I, f):
    """One half-sweep from the same table.  The systems differ by summation order only: |A_a - A_b| <= 2 gamma_n sum |terms| with
    n = the number of terms (table rows + entries + 1).  The solutions of two backward-stable solvers of systems that close differ
    by at most (c f^2 + 2 n) u kappa(A) relative (Higham, Thm 10.4 for Cholesky, 9.4 for LU without growth, c = 4 taken for both), kappa
    measured per system."""
    X = _ratings(U, I, 3)
    Y = np.random.RandomState(4).normal(0, 0.3, (I, f))
    Aa, ba = R.systems(X, Y, ALPHA, LAM, "solve")
    Ab, bb = R.systems(X, Y, ALPHA, LAM, "loop")
    n_terms = I + int(np.diff(R.canonical(X).indptr).max()) + 1
    mag = (np.abs(Y).T @ np.abs(Y)) * (1 + ALPHA * 5) + LAM
    assert (np.abs(Aa - Ab) <= 2 * n_terms * EPS * mag[None]).all()
    assert (np.abs(ba - bb) <= 2 * n_terms * EPS * (1 + ALPHA * 5) * np.abs(Y).sum(axis=0)[None]).all()
    xa, xb = R.half_sweep(X, Y, ALPHA, LAM, "solve"), R.half_sweep(X, Y, ALPHA, LAM, "loop")
    lens = np.diff(R.canonical(X).indptr)
    assert (xa[lens == 0] == 0).all() and (xb[lens == 0] == 0).all()
    worst = 0.0
    for u in np.flatnonzero(lens):
        bound = (4 * f * f + 2 * n_terms) * EPS * np.linalg.cond(Aa[u]) * np.abs(xa[u]).max()
        err = np.abs(xa[u] - xb[u]).max()
        worst = max(worst, err / bound)
        assert err <= bound, (u, err, bound)
    print("largest distance between the formulations: %.3g of its bound" % worst)


@pytest.mark.parametrize("U,I,f", SHAPES)
def test_the_objective_does_not_increase(U, I, f):
    """every half-sweep minimises the objective exactly in its block of variables, so it can only rise by the rounding of its own
    evaluation: U I + (U + I) f terms of one rounding each, relative to the objective"""
    X = _ratings(U, I, 5)
    _, _, hist = R.fit(X, _y0(I, f), ALPHA, LAM, 4)
    obj = [R.objective(X, Uk, Yk, ALPHA, LAM) for Uk, Yk in hist]
    slack = (U * I + (U + I) * f) * EPS
    print("objective over 4 iterations:", obj)
    for a, b in zip(obj, obj[1:]):
        assert b <= a * (1 + slack), obj
    assert obj[-1] < obj[0]


def test_fit_spread_between_the_formulations_and_empty_rows():
    """the spread that tests/test_wmf_gpu.py scales its bound by, printed; items without a user get zero vectors in both"""
    U, I, f = SHAPES[2]
    X = _ratings(U, I, 7)
    empty = np.flatnonzero(np.diff(R.canonical(X.T).indptr) == 0)
    assert len(empty) >= 12
    Ua, Ya, _ = R.fit(X, _y0(I, f), ALPHA, LAM, 4, "solve")
    Ub, Yb, _ = R.fit(X, _y0(I, f), ALPHA, LAM, 4, "loop")
    assert (Ya[empty] == 0).all() and (Yb[empty] == 0).all()
    spread = np.abs(Ya - Yb).max() / np.abs(Ya).max()
    print("spread of the two formulations after 4 iterations: %.3g" % spread)
    assert spread < 1e-9            # (far above what rounding gives, 1e-15 .. 1e-13: a disagreement of formulas would be O(1))
    S = R.scores(X[:5], Ya, ALPHA, LAM, mask=X[:5])
    assert np.array_equal(np.isneginf(S), X[:5].toarray() != 0)


def test_entry_points_are_exported_declared_and_bound():
    from rectorch_amd import _lib
    raw = C.CDLL(_lib.build())
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rectorch_hip.h")).read(), flags=re.S)
    for name, n_args in (("rtx_wmf_systems", 10), ("rtx_wmf_solve_rows", 10), ("rtx_wmf_fit", 9), ("rtx_wmf_load", 6), ("rtx_wmf_destroy", 1),
                         ("rtx_wmf_shape", 4), ("rtx_wmf_copy", 4), ("rtx_wmf_scores", 9), ("rtx_wmf_timings", 5)):
        assert hasattr(raw, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in the header" % name
        assert len(m.group(1).split(",")) == n_args, name
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == n_args, name
    assert re.search(r"#define RTX_WMF_MAX_FACTORS 128\n", text) and re.search(r"#define RTX_WMF_SEGMENT 4096\b", text)
    assert (_lib.WMF_MAX_FACTORS, _lib.WMF_SEGMENT, _lib.RTX_WMF_ITEMS, _lib.RTX_WMF_USERS) == (128, 4096, 0, 1)
    assert _lib.lib().rtx_abi_version() == 8
    # refusals that need no device: NULL arguments, and the parameter checks of rtx_wmf_load (made before anything touches the device)
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rtx_wmf_fit(None, None, 8, 1.0, 1.0, 1, None, C.byref(h), None) != 0 and not h.value
    assert lib.rtx_wmf_scores(None, None, None, 0, None, None, None, 0, None) != 0
    Y = np.zeros((3, 2))
    for f, alpha, lam, word in ((0, 1.0, 1.0, "f must be in [1, 128]"), (129, 1.0, 1.0, "f must be in [1, 128]"),
                                (2, 1.0, 0.0, "lam must be finite and > 0"), (2, -1.0, 1.0, "alpha must be finite and >= 0")):
        rc = lib.rtx_wmf_load(3, f, alpha, lam, Y.ctypes.data_as(C.c_void_p), C.byref(h))
        assert rc == -1 and not h.value and word in lib.rtx_last_error().decode()


@pytest.mark.parametrize("kwargs,word", [(dict(factors=0), "[1, 128]"), (dict(factors=129), "[1, 128]"), (dict(factors=2.5), "[1, 128]"),
                                         (dict(factors=True), "[1, 128]"), (dict(alpha=-0.5), ">= 0"), (dict(alpha=float("nan")), ">= 0"),
                                         (dict(alpha="much"), ">= 0"), (dict(lam=0.0), "> 0"), (dict(lam=-1.0), "> 0"),
                                         (dict(lam=float("inf")), "> 0"), (dict(num_iter=-1), ">= 0"), (dict(num_iter=1.5), ">= 0")])
def test_constructor_refusals_name_what_is_supported(kwargs, word):
    from rectorch_amd.models import WMF
    with pytest.raises(ValueError) as e:
        WMF(**kwargs)
    assert word in str(e.value) and list(kwargs)[0] in str(e.value)


def test_defaults_repr_and_untrained_errors():
    from rectorch_amd.evaluation import _is_item_item
    from rectorch_amd.models import WMF, RecSysModel
    m = WMF()
    assert (m.factors, m.alpha, m.lam, m.num_iter, m.seed) == (64, 40.0, 1.0, 15, 98765) and isinstance(m, RecSysModel)
    assert m.item_factors is None and m.user_factors is None and _is_item_item(m)
    assert str(m) == repr(m) == "WMF(factors=64, alpha=40.0000, lambda=1.0000, num_iter=15) - not trained yet!"
    X = csr_matrix(np.eye(3))
    for call in (lambda: m.predict([0, 1, 2], X), lambda: m.recommend([0, 1, 2], X), lambda: m.score_rows(X), lambda: m.recommend_rows(X)):
        with pytest.raises(RuntimeError):
            call()


def test_save_file_layout(tmp_path):
    """np.save of a dict of the hyper-parameters and both factor tables, in the family's style"""
    from rectorch_amd.models import WMF
    m = WMF(factors=5, alpha=2.0, lam=0.5, num_iter=3, seed=7)
    m._Y, m._U = np.arange(20.0).reshape(4, 5), np.arange(15.0).reshape(3, 5)      # (what a fit leaves behind once they were read)
    path = str(tmp_path / "wmf.npy")
    m.save_model(path)
    state = np.load(path, allow_pickle=True)[()]
    assert sorted(state) == ["alpha", "factors", "item_factors", "lam", "num_iter", "seed", "user_factors"]
    assert (state["factors"], state["alpha"], state["lam"], state["num_iter"], state["seed"]) == (5, 2.0, 0.5, 3, 7)
    assert np.array_equal(state["item_factors"], m._Y) and np.array_equal(state["user_factors"], m._U)
