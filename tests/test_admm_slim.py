"""ADMM SLIM (reference rectorch/models.py:1389-1577): models.ADMM_Slim / engine.AdmmSolver / rtx_admm_*.

CPU: a numpy float64 restatement of the reference's train() (admm_restated, below) reproduces every g14 golden model, the API
surface matches the reference and a model file the reference wrote loads into a pure look-up.  GPU: every g14 case on the
device, mid-size parity against the restatement, and the full ml-20m shape (determinism of P, one iteration recomputed on
the host from the device's own P, C and Gamma).

Tolerances.  The device computes the reference's float64 algorithm in other summation orders: an exact Gram matrix plus the
rank-1 item-bias term instead of the product of the centred dense X, a Cholesky inverse instead of LAPACK's LU, B_aux as
(G P)^T, and MFMA GEMMs.  It can only be held to the float64 noise floor of that algorithm.  The floor was measured on the CPU
as the distance between admm_restated and admm_restated(block_k=128, other_order=True) -- the same algorithm with the
products P.M summed in reverse 128-wide K blocks and the device's Gram / inverse / B_aux forms -- as max|difference| /
max|model| (max(1, max|model|) for the closed form, whose model is ~1e-16).  Measured floors:

    g14 cases without item_bias:           0 (num_iter = 0) .. 1.8e-14 (FLOOR below, per case)
    g14 cases with item_bias:              1.0e-16 (closed form) .. 4.8e-11
    mid size, reference defaults, num_iter = 50, no item_bias:   1.1e-14 .. 1.6e-14
    mid size, ratings 6000 x 1000 with item_bias:                6.5e-06
    900 x 300, float32 ratings in steps of 0.3 (float64 Gram route), num_iter = 50:   1.2e-14, with item_bias 1.4e-07

The item-bias floor is large because it is intrinsic: the centred Gram matrix carries (n - 2) b b^T, so P is ill-conditioned
(P itself agrees to 6.5e-11) and B_aux = P G cancels ~8 digits; 50 iterations at rho = 1e5 amplify that (C agrees to 3.8e-6).
The blocked product alone moves the same models by 3.2e-14 only.  Every device tolerance below is 10x its case's floor.
"""
import os
import tempfile

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

from conftest import ROOT, load_golden

# measured noise floor of each g14 case (see the module docstring); the device tolerance is 10x
FLOOR = {"a_nn1_l11_ib0_it7": 1.9e-15, "a_nn1_l11_ib1_it7": 4.4e-11, "a_nn1_l10_ib0_it7": 1.9e-15, "a_nn1_l10_ib1_it7": 4.9e-11,
         "a_nn0_l11_ib0_it7": 1.7e-15, "a_nn0_l11_ib1_it7": 4.3e-11, "a_nn0_l10_ib0_it7": 1.2e-16, "a_nn0_l10_ib1_it7": 1.1e-16,
         "a_vanilla_it0": 0.0, "a_vanilla_it1": 6.6e-16, "a_vanilla_it50": 3.5e-15, "b_vanilla_ib0_it30": 2.1e-15,
         "b_vanilla_ib1_it30": 1.1e-11, "a_default_it50": 1.8e-14}


# ------------------------------------------------------------------------------------------------ the restatement
def admm_restated(X, lambda1=5., lambda2=1e3, rho=1e5, nn_constr=True, l1_penalty=True, item_bias=False, num_iter=50,
                  block_k=None, keep=None, other_order=False):
    """reference ADMM_Slim.train (models.py:1464-1522) in numpy float64, step by step; returns the score matrix.
    block_k: compute P.(rho C - Gamma) by K blocks of that width summed in reverse order.  other_order: also form the Gram
    matrix as X^T X + (n - 2) b b^T, invert through a Cholesky factor and take B_aux = (G P)^T, as the device does.  Both
    change only summation orders and rounding: they measure the noise floor.  keep: a dict that receives P, C and Gamma."""
    def soft(a, k):
        return np.maximum(0., a - k) - np.maximum(0., -a - k)

    def pdot(P, M):
        if block_k is None:
            return P.dot(M)
        acc = np.zeros_like(M)
        for lo in reversed(range(0, P.shape[1], block_k)):
            acc += P[:, lo:lo + block_k].dot(M[lo:lo + block_k])
        return acc

    X = np.asarray(X, dtype=np.float64)
    X0 = X
    if item_bias:
        b = X.sum(axis=0)
        X = X - np.outer(np.ones(X.shape[0]), b)
    XtX = X.T.dot(X)
    if other_order and item_bias:
        XtX = X0.T.dot(X0) + np.outer((X0.shape[0] - 2) * b, b)
    d = np.diag_indices(XtX.shape[0])
    XtX[d] += lambda2 + rho
    if other_order:
        W = np.linalg.inv(np.linalg.cholesky(XtX))
        P = W.T.dot(W)
    else:
        P = np.linalg.inv(XtX)
    Gamma = np.zeros(XtX.shape)
    if not nn_constr and not l1_penalty:
        C = np.eye(P.shape[0]) - P * np.diag(1. / np.diag(P))
    else:
        XtX[d] -= lambda2 + rho
        B_aux = XtX.dot(P).T if other_order else P.dot(XtX)
        C = np.zeros(XtX.shape)
        for _ in range(num_iter):
            B_tilde = B_aux + pdot(P, rho * C - Gamma)
            gamma = np.diag(B_tilde) / np.diag(P)
            B = B_tilde - P * np.diag(gamma)
            C = soft(B + Gamma / rho, lambda1 / rho)
            if nn_constr and l1_penalty:
                C = np.maximum(C, 0.)
            elif nn_constr and not l1_penalty:
                C = np.maximum(B, 0.)
            Gamma += rho * (B - C)
    if keep is not None:
        keep.update(P=P, C=C, Gamma=Gamma)
    model = np.dot(X, C)
    if item_bias:
        model += b
    return model


def g14_cases():
    g = load_golden("g14_admm_slim")
    out = []
    for name in g["cases"]:
        name = str(name)
        meta = g["case__%s__meta" % name]
        X = (g["Xb"] if meta[0] else g["Xa"]).astype(np.float64)
        kw = dict(lambda1=meta[1], lambda2=meta[2], rho=meta[3], nn_constr=bool(meta[4]), l1_penalty=bool(meta[5]),
                  item_bias=bool(meta[6]), num_iter=int(meta[7]))
        out.append((name, X, kw, g["case__%s__model" % name]))
    return out


def rel_err(a, ref, floor_one=False):
    scale = float(np.max(np.abs(ref))) if ref.size else 0.0
    if floor_one:
        scale = max(1.0, scale)
    return float(np.max(np.abs(a - ref))) / max(scale, 1e-300)


def closed_form(kw):
    return not kw["nn_constr"] and not kw["l1_penalty"]


# ------------------------------------------------------------------------------------------------ CPU
def test_restatement_reproduces_every_g14_model():
    """1e-12, or 10x the case's floor where that is larger (the item-bias cases, floor up to 4.8e-11): on another host's BLAS
    the reference's own numbers move by that much"""
    cases = g14_cases()
    assert len(cases) == 14 and set(FLOOR) == {c[0] for c in cases}
    for name, X, kw, ref in cases:
        got = admm_restated(X, **kw)
        assert got.shape == ref.shape
        err = rel_err(got, ref, closed_form(kw))
        assert err <= max(1e-12, 10 * FLOOR[name]), (name, err)


def test_g14_cases_exercise_threshold_and_projection():
    """the non-default hyper-parameters make C sparse and the projection active: otherwise the variants would coincide"""
    g = load_golden("g14_admm_slim")
    m = {str(n): g["case__%s__model" % n] for n in g["cases"]}
    assert not np.allclose(m["a_nn1_l11_ib0_it7"], m["a_nn0_l11_ib0_it7"])
    assert not np.allclose(m["a_nn1_l11_ib0_it7"], m["a_nn1_l10_ib0_it7"])
    assert np.max(np.abs(m["a_nn0_l10_ib0_it7"])) < 1e-14                 # closed form: C ~ 0
    assert np.all(m["a_vanilla_it0"] == 0)
    keep = {}
    admm_restated(g["Xa"].astype(np.float64), *g["hp"], num_iter=7, keep=keep)
    assert np.mean(keep["C"] == 0) > 0.5 and np.all(keep["C"] >= 0)


def test_api_surface_and_reference_model_file():
    from rectorch_amd import models
    from rectorch_amd.models import ADMM_Slim
    assert "ADMM_Slim" in models.__all__
    g = load_golden("g14_admm_slim")
    m = ADMM_Slim()
    assert (m.lambda1, m.lambda2, m.rho, m.nn_constr, m.l1_penalty, m.item_bias) == (5., 1e3, 1e5, True, True, False)
    assert m.model is None and str(m) == str(g["str_new"]) and repr(m) == str(m)
    assert "lamdba2" in str(m)
    with pytest.raises(RuntimeError):
        m.predict([0], csr_matrix(np.zeros((1, 3))))
    state = m.load_model(os.path.join(ROOT, "tests", "golden", "g14_reference_admm_model.npy"))
    assert set(state.keys()) == {"lambda1", "lambda2", "rho", "model", "nn_constr", "l1_penalty", "item_bias"}
    assert str(m) == str(g["str_trained"])
    te = csr_matrix(g["te"].astype(np.float64))
    pr = m.predict(g["ids"], te)[0]
    assert np.array_equal(np.isneginf(pr), np.isneginf(g["pred_remove"]))
    assert np.array_equal(pr, g["pred_remove"])
    pk = m.predict(g["ids"], te, remove_train=False)[0]
    assert np.array_equal(pk, g["pred_keep"])
    # save -> load round trip of the look-up model keeps the seven keys
    tmp = tempfile.NamedTemporaryFile()
    m.save_model(tmp.name)
    m2 = ADMM_Slim(1., 2., 3.)
    m2.load_model(tmp.name + ".npy")
    os.remove(tmp.name + ".npy")
    assert np.array_equal(m2.model, m.model) and (m2.lambda1, m2.lambda2, m2.rho) == (5., 1e3, 1e5)


def test_train_without_device_raises():
    from rectorch_amd._lib import RtxError
    from rectorch_amd.models import ADMM_Slim
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible")
    with pytest.raises(RtxError):
        ADMM_Slim().train(csr_matrix(np.eye(4)), num_iter=2)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_g14_every_case_on_device():
    from rectorch_amd.models import ADMM_Slim
    for name, X, kw, ref in g14_cases():
        num_iter = kw.pop("num_iter")
        m = ADMM_Slim(**kw)
        m.train(csr_matrix(X), num_iter=num_iter)
        err = rel_err(m.model, ref, closed_form(kw))
        assert err <= 10 * FLOOR[name], (name, err)


@pytest.mark.gpu
def test_g14_predict_and_str_on_device():
    from rectorch_amd.models import ADMM_Slim
    g = load_golden("g14_admm_slim")
    Xa = csr_matrix(g["Xa"].astype(np.float64))
    te = csr_matrix(g["te"].astype(np.float64))
    m = ADMM_Slim()
    assert str(m) == str(g["str_new"])
    m.train(Xa, num_iter=50)
    assert str(m) == str(g["str_trained"]) and repr(m) == str(m)
    pr = m.predict(g["ids"], te)[0]
    assert pr.shape == g["pred_remove"].shape and pr.dtype == np.float64
    assert np.array_equal(np.isneginf(pr), np.isneginf(g["pred_remove"]))
    fin = np.isfinite(pr)
    tol = 10 * FLOOR["a_default_it50"]
    assert rel_err(pr[fin], g["pred_remove"][fin]) <= tol
    pk = m.predict(g["ids"], te, remove_train=False)[0]
    assert np.all(np.isfinite(pk)) and rel_err(pk, g["pred_keep"]) <= tol
    pt = m.predict(g["ids"], te, as_tensor=True)[0]
    assert pt.is_cuda and pt.dtype == torch.float64
    mb = ADMM_Slim(*g["hp"], item_bias=True)
    mb.train(Xa, num_iter=7)
    assert str(mb) == str(g["str_trained_ib"])
    pb = mb.predict(g["ids"], te)[0]
    assert np.array_equal(np.isneginf(pb), np.isneginf(g["pred_remove_ib"]))
    fin = np.isfinite(pb)
    assert rel_err(pb[fin], g["pred_remove_ib"][fin]) <= 10 * FLOOR["a_nn1_l11_ib1_it7"]
    # save_model materialises the host score matrix; load_model turns the model into a pure look-up
    tmp = tempfile.NamedTemporaryFile()
    m.save_model(tmp.name)
    m2 = ADMM_Slim()
    m2.load_model(tmp.name + ".npy")
    os.remove(tmp.name + ".npy")
    assert m2._solver is None and np.array_equal(m2.model, m.model)
    assert np.array_equal(m2.predict(g["ids"], te)[0][fin], pr[fin])


@pytest.mark.gpu
def test_admm_solver_matrices_and_errors():
    from rectorch_amd._lib import RtxError
    from rectorch_amd.engine import AdmmSolver
    g = load_golden("g14_admm_slim")
    X = g["Xa"].astype(np.float64)
    keep = {}
    admm_restated(X, *g["hp"], num_iter=7, keep=keep)
    s = AdmmSolver(csr_matrix(X), *g["hp"], True, True, False, 7)
    P, C, Gm = (s.copy(w).cpu().numpy() for w in ("P", "C", "Gamma"))
    assert np.array_equal(P, P.T)
    # 10x the floors of these matrices, measured as in the module docstring: P 1.4e-15, C 3.9e-15, Gamma 3.6e-15
    assert rel_err(P, keep["P"]) <= 1.4e-14
    assert rel_err(C, keep["C"]) <= 3.9e-14 and np.all(C >= 0)
    assert rel_err(Gm, keep["Gamma"]) <= 3.6e-14
    t = s.timings()
    assert t["fit_ms"] > 0 and t["iter_ms"] > 0 and t["factor_ms"] > 0
    with pytest.raises(RtxError, match="num_iter"):
        AdmmSolver(csr_matrix(X), 1., 1., 1., True, True, False, -1)
    with pytest.raises(RtxError, match="positive definite"):
        AdmmSolver(csr_matrix(X), 1., -50., 10., True, True, False, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("U,I,ratings,item_bias,floor", [(6000, 1000, False, False, 1.6e-14), (6000, 1000, True, False, 1.2e-14),
                                                         (8000, 2000, False, False, 1.5e-14), (8000, 2000, True, False, 1.5e-14),
                                                         (6000, 1000, True, True, 6.5e-6)])
def test_mid_size_vs_restatement(U, I, ratings, item_bias, floor):
    from rectorch_amd.models import ADMM_Slim
    rng = np.random.RandomState(U + I + ratings)
    X = (rng.rand(U, I) < 0.02).astype(np.float64)
    if ratings:
        X *= rng.randint(1, 6, size=(U, I))
    ref = admm_restated(X, item_bias=item_bias, num_iter=50)
    m = ADMM_Slim(item_bias=item_bias)
    m.train(csr_matrix(X), num_iter=50)
    ids = rng.randint(0, U, size=300)
    got = m.predict(ids, None, remove_train=False)[0]
    err = rel_err(got, ref[ids])
    print("ADMM mid-size %dx%d ratings=%s item_bias=%s: rel err %.2e" % (U, I, ratings, item_bias, err))
    assert err <= 10 * floor, err


@pytest.mark.gpu
@pytest.mark.parametrize("item_bias,floor", [(False, 1.2e-14), (True, 1.4e-7)])
def test_fractional_ratings_take_the_float64_gram_route(item_bias, floor):
    """ratings in steps of 0.3 are no integers under any power-of-two scale, so the Gram matrix comes from the float64 product and
    not from the fp8 / bf16 SYRK: the only iterating fit on that route.  The returned G feeds B_aux = G P, so an element of G the
    product leaves unwritten (it skips the upper-right quadrant of every diagonal 128-block) would show here.  Reference defaults,
    50 iterations, against the restatement on the same float32-rounded X; floors measured as in the module docstring"""
    from rectorch_amd.models import ADMM_Slim
    U, I = 900, 300
    rng = np.random.RandomState(U + I)
    X = ((rng.rand(U, I) < 0.1) * (0.3 * rng.randint(1, 17, size=(U, I)))).astype(np.float32)
    assert not np.array_equal(X * 8, np.rint(X * 8))
    ref = admm_restated(X.astype(np.float64), item_bias=item_bias, num_iter=50)
    m = ADMM_Slim(item_bias=item_bias)
    m.train(csr_matrix(X), num_iter=50)
    err = rel_err(m.model, ref)
    print("ADMM 900x300 ratings in steps of 0.3, item_bias=%s: rel err %.2e (floor %.2e)" % (item_bias, err, floor))
    assert err <= 10 * floor, err


@pytest.mark.gpu
def test_full_size_determinism_and_one_iteration_on_host():
    """ml-20m shape (136 677 x 20 108), reference defaults.  Two fits (num_iter = 2 and 3) give a bitwise identical P; then
    iteration 3 is recomputed on the host in float64 for 16 sampled columns j from the downloaded P, G[:, j] = X^T (X e_j)
    and the columns of C_2 and Gamma_2, and compared with the device's C_3 and Gamma_3.  C >= 0 (nn_constr).
    Floor of this check, measured on the CPU between admm_restated and its other-order form at the same defaults
    (relative to the column block's max): 1.5e-15 (C) / 4.3e-15 (Gamma) at 6000 x 1000, 3.7e-15 / 6.9e-15 on synthetic
    40 000 x 6 000 data.  Asserted: 7e-14, 10x the larger."""
    from rectorch_amd.engine import AdmmSolver, CsrMatrix
    from rectorch_amd.utils import synth_interactions
    U, I = 136677, 20108
    lam1, lam2, rho = 5., 1e3, 1e5
    X = synth_interactions(U, I, seed=20)
    Xd = CsrMatrix(X)
    rng = np.random.RandomState(0)
    cols = np.sort(rng.choice(I, size=16, replace=False))
    tc = torch.as_tensor(cols, device="cuda")
    s2 = AdmmSolver(Xd, lam1, lam2, rho, True, True, False, 2)
    P2 = s2.copy("P")
    C2 = s2.copy("C")[:, tc].cpu().numpy()
    G2 = s2.copy("Gamma")[:, tc].cpu().numpy()
    del s2
    s3 = AdmmSolver(Xd, lam1, lam2, rho, True, True, False, 3)
    P3 = s3.copy("P")
    assert torch.equal(P2, P3)
    del P3
    C3d = s3.copy("C")
    assert float(C3d.min()) >= 0.0
    C3 = C3d[:, tc].cpu().numpy()
    del C3d
    G3 = s3.copy("Gamma")[:, tc].cpu().numpy()
    P = P2.cpu().numpy()
    del P2
    E = np.zeros((I, len(cols)))
    E[cols, np.arange(len(cols))] = 1.0
    Gc = X.T @ (X @ E)                                              # G[:, j] without forming G
    Bt = P @ (Gc + rho * C2 - G2)                                   # B~[:, j] = B_aux[:, j] + P (rho C_2 - Gamma_2)[:, j]
    q = np.arange(len(cols))
    pd = P[cols, cols]
    B = Bt.copy()
    B[cols, q] = Bt[cols, q] - pd * (Bt[cols, q] / pd)
    Ch = np.maximum(np.maximum(0., (B + G2 / rho) - lam1 / rho) - np.maximum(0., -(B + G2 / rho) - lam1 / rho), 0.)
    Gh = G2 + rho * (B - Ch)
    eC = float(np.max(np.abs(C3 - Ch))) / float(np.max(np.abs(Ch)))
    eG = float(np.max(np.abs(G3 - Gh))) / float(np.max(np.abs(Gh)))
    print("ADMM full size, iteration 3 on the host: C rel %.2e, Gamma rel %.2e" % (eC, eG))
    assert eC <= 7e-14 and eG <= 7e-14, (eC, eG)
