"""ItemKNN in numpy float64: a restatement of the model's definition (include/rectorch_hip.h) for the tests, and a second, brute-force
formulation to cross-check it.  Nothing here imports the package.

    G = XᵀX;  for i != j with G_ij > 0:  cosine  S_ij = G_ij / (sqrt(G_ii) * sqrt(G_jj) + shrink)
                                          jaccard S_ij = G_ij / (G_ii + G_jj - G_ij + shrink)
    every other entry of S is -inf ("no neighbour").  N_k(j): the k best i of row j of S, similarity descending, id ascending among
    equal similarities, finite entries only.  W_ij = S_ij for i in N_k(j) (/ d_j with normalize, d_j = the list's similarities added
    best first).  scores[u][j] = sum over the user's stored entries (i, v), in stored order, of v * W_ij, each term one fma.

``G`` is exact in float64 for integer and dyadic data (every product and partial sum is an integer multiple of a power of two below
2^53), whatever the order of the sum; the tests that ask for equal bits use such data.
"""
from fractions import Fraction

import numpy as np
from scipy.sparse import csr_matrix

SIMILARITIES = ("cosine", "jaccard")


def gram(X):
    d = np.asarray(X.toarray(), dtype=np.float64)
    return d.T @ d


def similarity(G, shrink=0.0, kind="cosine"):
    """S from G, every operation rounded to float64 in the order of the definition (numpy does not contract)."""
    assert kind in SIMILARITIES
    G = np.asarray(G, dtype=np.float64)
    n = G.shape[0]
    diag = np.diag(G).copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "cosine":
            r = np.sqrt(diag)
            den = r[:, None] * r[None, :] + shrink
        else:
            den = ((diag[:, None] + diag[None, :]) - G) + shrink
        S = G / den
    keep = (G > 0) & ~np.eye(n, dtype=bool)
    return np.where(keep, S, -np.inf)


def neighbours(S, k):
    """[(ids, similarities)] per row j of S: N_k(j) in list order."""
    n = S.shape[0]
    out = []
    ids = np.arange(n)
    for j in range(n):
        order = np.lexsort((ids, -S[j]))            # similarity descending, id ascending among equal ones
        order = order[np.isfinite(S[j][order])][:k]
        out.append((order, S[j][order]))
    return out


def list_sum(values):
    d = 0.0
    for v in values:                                # best first, one rounding per term
        d = d + float(v)
    return d


def weights(S, k, normalize=False):
    """W as a float64 csr_matrix by source item (row i, column j), indices ascending."""
    n = S.shape[0]
    rows, cols, vals = [], [], []
    for j, (ids, sims) in enumerate(neighbours(S, k)):
        d = list_sum(sims) if normalize else 1.0
        for i, s in zip(ids, sims):
            rows.append(int(i))
            cols.append(j)
            vals.append(float(s) / d if normalize else float(s))
    W = csr_matrix((np.asarray(vals, dtype=np.float64), (np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64))), shape=(n, n))
    W.sort_indices()
    return W


def fit(X, k, shrink=0.0, kind="cosine", normalize=False):
    return weights(similarity(gram(X), shrink, kind), k, normalize)


def fma(a, b, c):
    """a * b + c rounded once (Python 3.10 has no math.fma): exact rational arithmetic, then the correctly rounded conversion."""
    if a == 1.0:
        return b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def scores(X, W, mask=None):
    """[users, n_items] float64: per user the stored entries of X's row in stored order, W's row of each added by fma; -inf at the
    non-zero entries of mask's row."""
    X = X.tocsr()
    W = W.tocsr()
    out = np.zeros(X.shape, dtype=np.float64)
    for u in range(X.shape[0]):
        o = out[u]
        for e in range(X.indptr[u], X.indptr[u + 1]):
            i, v = X.indices[e], float(X.data[e])
            for p in range(W.indptr[i], W.indptr[i + 1]):
                j = W.indices[p]
                o[j] = fma(v, float(W.data[p]), float(o[j]))
    if mask is not None:
        m = mask.toarray() != 0
        out[m] = -np.inf
    return out


# ---- the second formulation: dense, scalar by scalar ---------------------------------------------------------------------------------
def brute_force(X, k, shrink=0.0, kind="cosine", normalize=False):
    """(W dense [n, n], present bool [n, n], scores [users, n]) straight from the definition, with Python scalars and sorted()."""
    import math
    d = np.asarray(X.toarray(), dtype=np.float64)
    U, n = d.shape
    G = [[math.fsum(d[u, i] * d[u, j] for u in range(U)) for j in range(n)] for i in range(n)]      # exactly rounded sums
    W = np.zeros((n, n))
    present = np.zeros((n, n), dtype=bool)
    for j in range(n):
        cand = []
        for i in range(n):
            if i == j or not G[i][j] > 0:
                continue
            if kind == "cosine":
                den = math.sqrt(G[i][i]) * math.sqrt(G[j][j]) + shrink
            else:
                den = G[i][i] + G[j][j] - G[i][j] + shrink
            cand.append((G[i][j] / den, i))
        cand = sorted(cand, key=lambda c: (-c[0], c[1]))[:k]
        tot = 0.0
        for s, _ in cand:
            tot = tot + s
        for s, i in cand:
            W[i, j] = s / tot if normalize else s
            present[i, j] = True
    Xc = X.tocsr()
    sc = np.zeros((U, n))
    for u in range(U):
        for j in range(n):
            acc = 0.0
            for e in range(Xc.indptr[u], Xc.indptr[u + 1]):
                i = Xc.indices[e]
                if present[i, j]:
                    acc = fma(float(Xc.data[e]), float(W[i, j]), acc)
            sc[u, j] = acc
    return W, present, sc


def ulp_distance(a, b):
    """element-wise distance in units in the last place between finite float64 arrays"""
    def key(x):
        bits = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
        return np.where(bits < 0, np.int64(-2 ** 63) - bits, bits)
    return np.abs(key(a) - key(b))
