"""BPRMF in float64: matrix factorisation trained on sampled (user, positive, negative) triples with the pairwise ranking loss of
Bayesian Personalised Ranking (Rendle, Freudenthaler, Gantner, Schmidt-Thieme, UAI 2009), restated in plain numpy -- no torch and
no HIP.  The package has no device BPRMF yet: this file fixes the semantic a device implementation has to meet and is its judge
(DESIGN 11); tests/test_bpr_host.py checks the restatement against itself.

The model.  U [n_users][f] and Y [n_items][f]; the score of item j for user u is u . y_j; no item bias.
The draws.  Integers only, a pure function of (seed, epoch, sample), over oracle/philox_oracle.py.  An epoch is nnz samples.  Sample s of
epoch e reads r0 = philox4x32_10(seed, FIT_STREAM + e, 2 s) and r1 = (..., 2 s + 1).  p = mulhi32(r0.x, nnz) is a position in the CSR
`indices` (rows sorted): the positive is i = indices[p], the user u is the row whose indptr range holds p.  The NEG_TRIES = 7 candidates
are mulhi32(w, n_items) for w = r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w; the first one the row does not store is the negative j.  If all
seven are stored the sample is SKIPPED (j = -1) and contributes to nothing.
One batch = the samples lo .. lo + batch - 1 of an epoch, every gradient taken at the tables of the batch's start:
    x_t = u_t . (y_i - y_j),  s_t = 1 / (1 + exp(x_t)),
    theta' = theta + lr (sum_t g_t - c reg theta)   for every row theta that c > 0 non-skipped samples touch,
    g_t = s_t (y_i - y_j) for the user, +s_t u_t for the positive item, -s_t u_t for the negative item, summed in ascending t.
batch = 1 is textbook sequential BPR-SGD; rows nobody touched keep their bits.
Fold-in of a row with n entries: x = 0, then fold_in_epochs * n sequential steps of the same rule with batch = 1 on x alone against the
final Y; step t reads its words at (seed, FOLD_STREAM, 2 t [+ 1]), its positive is the row's entry mulhi32(r0.x, n), its negative is found
as above against the row.  The vector depends on the row's content alone; an empty row and a row that stores every item give 0.

The fit is written twice:
  "loop"    one sample after the other: the dot by numpy.dot, the coefficient 1 / (1 + exp(x)), every touched row's sum in a Python loop;
  "vector"  a batch at a time: the dots by einsum, the coefficient as 0.5 (1 + tanh(-x / 2)), the sums by numpy.add.at.
Neither fixes a summation tree, and the two sigmoids round differently: the spread between the two contains the roundings the
definition leaves open, and a device test scales its bound by it (the rule of tests/test_wmf_gpu.py).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import philox_oracle as P       # noqa: E402

NEG_TRIES = 7
FIT_STREAM = 0x1B504D4600000000
FOLD_STREAM = 0x2B504D4600000000


def canonical(X):
    """CSR with sorted, unique column ids: what the device holds"""
    m = X.tocsr().copy()
    m.sum_duplicates()
    m.sort_indices()
    return m


def _mulhi(words, n):
    return ((words.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def _words(seed, offset, samples):
    """uint32 [len(samples)][8]: the words of the two Philox calls of every sample (the second call's are read only when needed, which
    gives the same numbers: the draws are a pure function)"""
    s = np.asarray(samples, dtype=np.uint64)
    r0 = P.philox4x32_10(seed, offset, np.uint64(2) * s)
    r1 = P.philox4x32_10(seed, offset, np.uint64(2) * s + np.uint64(1))
    return np.stack(list(r0) + list(r1), axis=1)


def _negatives(words, rows, n_items):
    """the first of the seven candidates that the sample's row (a set) does not hold, else -1"""
    cand = _mulhi(words[:, 1:1 + NEG_TRIES], n_items)
    out = np.full(len(cand), -1, dtype=np.int64)
    for t, (c, row) in enumerate(zip(cand, rows)):
        for v in c:
            if int(v) not in row:
                out[t] = int(v)
                break
    return out


def draws(X, seed, epoch, lo=0, count=None):
    """(u, i, j) int64 vectors of the samples lo .. lo + count - 1 of an epoch; j = -1: skipped"""
    m = canonical(X)
    nnz, n_items = int(m.nnz), int(m.shape[1])
    count = nnz - lo if count is None else count
    w = _words(seed, FIT_STREAM + int(epoch), np.arange(lo, lo + count))
    p = _mulhi(w[:, 0], nnz)
    i = m.indices[p].astype(np.int64)
    u = np.searchsorted(m.indptr, p, side="right").astype(np.int64) - 1
    sets = [set(m.indices[m.indptr[r]:m.indptr[r + 1]].tolist()) for r in range(m.shape[0])]
    j = _negatives(w, [sets[r] for r in u], n_items)
    return u, i, j


def sigmoid_neg(x, how):
    """sigma(-x), in the two ways the formulations write it"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(x)) if how == "loop" else 0.5 * (1.0 + np.tanh(-0.5 * x))


def batch_loop(U, Y, u, i, j, lr, reg):
    """one batch, sample after sample; returns new tables"""
    GU, GY = {}, {}
    for ut, it, jt in zip(u, i, j):
        if jt < 0:
            continue
        d = Y[it] - Y[jt]
        s = float(sigmoid_neg(float(np.dot(U[ut], d)), "loop"))
        for G, r, g in ((GU, ut, s * d), (GY, it, s * U[ut]), (GY, jt, -s * U[ut])):
            acc, c = G.get(r, (0.0, 0))
            G[r] = (acc + g, c + 1)
    U2, Y2 = U.copy(), Y.copy()
    for T, T2, G in ((U, U2, GU), (Y, Y2, GY)):
        for r, (acc, c) in G.items():
            T2[r] = T[r] + lr * (acc - c * reg * T[r])
    return U2, Y2


def batch_vector(U, Y, u, i, j, lr, reg):
    ok = j >= 0
    u, i, j = u[ok], i[ok], j[ok]
    d = Y[i] - Y[j]
    s = sigmoid_neg(np.einsum("tk,tk->t", U[u], d), "vector")[:, None]
    GU, GY = np.zeros_like(U), np.zeros_like(Y)
    cu, cy = np.zeros(len(U)), np.zeros(len(Y))
    np.add.at(GU, u, s * d)
    np.add.at(cu, u, 1.0)
    rows = np.stack([i, j], axis=1).reshape(-1)               # an item's two roles interleaved by sample
    g = np.stack([s * U[u], -s * U[u]], axis=1).reshape(-1, U.shape[1])
    np.add.at(GY, rows, g)
    np.add.at(cy, rows, 1.0)
    U2, Y2 = U.copy(), Y.copy()
    tu, ty = cu > 0, cy > 0
    U2[tu] = U[tu] + lr * (GU[tu] - (cu[tu] * reg)[:, None] * U[tu])
    Y2[ty] = Y[ty] + lr * (GY[ty] - (cy[ty] * reg)[:, None] * Y[ty])
    return U2, Y2


def fit(X, U0, Y0, lr, reg, epochs, batch, seed, how="loop", history=False):
    """(U, Y[, tables after every epoch]) after `epochs` epochs in batches of `batch`"""
    m = canonical(X)
    step = batch_loop if how == "loop" else batch_vector
    U, Y = np.array(U0, dtype=np.float64), np.array(Y0, dtype=np.float64)
    hist = [(U.copy(), Y.copy())]
    for e in range(epochs):
        u, i, j = draws(m, seed, e)
        for lo in range(0, m.nnz, batch):
            U, Y = step(U, Y, u[lo:lo + batch], i[lo:lo + batch], j[lo:lo + batch], lr, reg)
        hist.append((U.copy(), Y.copy()))
    return (U, Y, hist) if history else (U, Y)


def fit_sequential(X, U0, Y0, lr, reg, epochs, seed):
    """textbook BPR-SGD, one sample at a time, the three rows updated in place from the values before the sample"""
    m = canonical(X)
    U, Y = np.array(U0, dtype=np.float64), np.array(Y0, dtype=np.float64)
    for e in range(epochs):
        for ut, it, jt in zip(*draws(m, seed, e)):
            if jt < 0:
                continue
            uo, d = U[ut].copy(), Y[it] - Y[jt]
            s = float(sigmoid_neg(float(np.dot(uo, d)), "loop"))
            yi, yj = Y[it].copy(), Y[jt].copy()
            U[ut] = uo + lr * ((0.0 + s * d) - 1 * reg * uo)
            Y[it] = yi + lr * ((0.0 + s * uo) - 1 * reg * yi)
            Y[jt] = yj + lr * ((0.0 + -s * uo) - 1 * reg * yj)
    return U, Y


def fold_in(rows, Y, lr, reg, fold_in_epochs, seed, how="loop"):
    """the fold-in vectors [rows][f] of the rows of a sparse matrix against the item factors Y"""
    m = canonical(rows)
    n_items, f = Y.shape
    out = np.zeros((m.shape[0], f))
    for r in range(m.shape[0]):
        row = m.indices[m.indptr[r]:m.indptr[r + 1]].astype(np.int64)
        n = len(row)
        if n == 0 or fold_in_epochs == 0:
            continue
        w = _words(seed, FOLD_STREAM, np.arange(fold_in_epochs * n))
        pos = row[_mulhi(w[:, 0], n)]
        neg = _negatives(w, [set(row.tolist())] * len(w), n_items)
        x = np.zeros(f)
        for it, jt in zip(pos, neg):
            if jt < 0:
                continue
            d = Y[it] - Y[jt]
            s = float(sigmoid_neg(float(np.dot(x, d)), how))
            x = x + lr * (s * d - reg * x)
        out[r] = x
    return out


def scores(rows, Y, lr, reg, fold_in_epochs, seed, mask=None):
    S = fold_in(rows, Y, lr, reg, fold_in_epochs, seed) @ Y.T
    if mask is not None:
        S[mask.toarray() != 0] = -np.inf
    return S


def auc(X, U, Y):
    """mean over the users with a positive and a negative of P(score of a stored item > score of one not stored), ties a half"""
    m = canonical(X)
    dense = m.toarray() != 0
    S = U @ Y.T
    vals = []
    for r in range(m.shape[0]):
        pos, neg = S[r][dense[r]], S[r][~dense[r]]
        if len(pos) and len(neg):
            diff = pos[:, None] - neg[None, :]
            vals.append(((diff > 0).sum() + 0.5 * (diff == 0).sum()) / diff.size)
    return float(np.mean(vals))


def objective(U, Y, u, i, j, reg):
    """the BPR objective on a fixed set of triples: sum -ln sigma(x_uij) + reg / 2 (|u|^2 + |y_i|^2 + |y_j|^2), skipped triples left out"""
    ok = j >= 0
    u, i, j = u[ok], i[ok], j[ok]
    x = np.einsum("tk,tk->t", U[u], Y[i] - Y[j])
    return float(np.sum(np.logaddexp(0.0, -x)) + 0.5 * reg * np.sum(U[u] ** 2 + Y[i] ** 2 + Y[j] ** 2))
