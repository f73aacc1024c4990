"""WMF (implicit-feedback ALS) in numpy float64: a restatement of the model's definition (include/rectorch_hip.h) for the tests, in two
formulations that share no arithmetic beyond the definition:

  "solve"  A_u = YᵀY + Y_uᵀ diag(w) Y_u + lam I by matrix products, b_u = Y_uᵀ (1 + w), x_u by numpy.linalg.solve (LU);
  "loop"   A_u and b_u by a loop over the row's entries in stored order (outer products added one by one to a copy of G, itself a
           loop over the table's rows), x_u by scipy.linalg.cho_factor / cho_solve.

w = alpha * r on the stored entries (r as stored: float32 widened to float64), a row without entries gets the zero vector, one
iteration is a user half-sweep followed by an item half-sweep."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.sparse import csr_matrix

FORMULATIONS = ("solve", "loop")


def canonical(X):
    """the matrix as the device holds it: CSR, duplicates summed, indices sorted, values through float32"""
    m = csr_matrix(X).copy()
    m.sum_duplicates()
    m.sort_indices()
    m.data = m.data.astype(np.float32).astype(np.float64)
    return m


def systems(X, Y, alpha, lam, how="solve"):
    """(A [n, f, f], b [n, f]) of every row of X against the factor table Y"""
    X = canonical(X)
    Y = np.asarray(Y, dtype=np.float64)
    n, f = X.shape[0], Y.shape[1]
    A, b = np.empty((n, f, f)), np.empty((n, f))
    if how == "solve":
        G = Y.T @ Y
    else:
        G = np.zeros((f, f))
        for y in Y:
            G += np.outer(y, y)
    for u in range(n):
        idx = X.indices[X.indptr[u]:X.indptr[u + 1]]
        w = alpha * X.data[X.indptr[u]:X.indptr[u + 1]]
        Yu = Y[idx]
        if how == "solve":
            A[u] = G + Yu.T @ (w[:, None] * Yu) + lam * np.eye(f)
            b[u] = Yu.T @ (1.0 + w)
        else:
            Au, bu = G.copy(), np.zeros(f)
            for wk, y in zip(w, Yu):
                Au += wk * np.outer(y, y)
                bu += (1.0 + wk) * y
            A[u] = Au + lam * np.eye(f)
            b[u] = bu
    return A, b


def half_sweep(X, Y, alpha, lam, how="solve"):
    """x_u of every row of X against Y: [n, f]; zero rows for rows without entries"""
    X = canonical(X)
    A, b = systems(X, Y, alpha, lam, how)
    out = np.zeros_like(b)
    for u in range(X.shape[0]):
        if X.indptr[u + 1] == X.indptr[u]:
            continue
        out[u] = np.linalg.solve(A[u], b[u]) if how == "solve" else cho_solve(cho_factor(A[u], lower=True), b[u])
    return out


def fit(X, Y0, alpha, lam, n_iter, how="solve"):
    """(U, Y, history): the factors after n_iter iterations from the item factors Y0, and [(U, Y)] after every iteration"""
    X = canonical(X)
    XT = canonical(X.T)
    Y = np.array(Y0, dtype=np.float64)
    U = np.zeros((X.shape[0], Y.shape[1]))
    history = []
    for _ in range(n_iter):
        U = half_sweep(X, Y, alpha, lam, how)
        Y = half_sweep(XT, U, alpha, lam, how)
        history.append((U, Y))
    return U, Y, history


def objective(X, U, Y, alpha, lam):
    """sum over ALL (u, i) of c_ui (p_ui - x_u . y_i)^2 + lam (|U|^2 + |Y|^2), dense"""
    R = canonical(X).toarray()
    Cw = 1.0 + alpha * R
    P = (R > 0).astype(np.float64)
    E = P - np.asarray(U) @ np.asarray(Y).T
    return float((Cw * E * E).sum() + lam * ((np.asarray(U) ** 2).sum() + (np.asarray(Y) ** 2).sum()))


def scores(rows, Y, alpha, lam, mask=None, how="solve"):
    """fold-in of the rows against the item factors Y, then x_u . y_j; -inf at the non-zero entries of mask"""
    S = half_sweep(rows, Y, alpha, lam, how) @ np.asarray(Y, dtype=np.float64).T
    if mask is not None:
        S[csr_matrix(mask).toarray() != 0] = -np.inf
    return S
