"""BPRMF's batch rule and fold-in on the host (``rtx_bpr_update_host`` / ``rtx_bpr_fold_in_host``, plain C++, no device needed): the
float64 definition, operation by operation, that a device trainer is held to -- beside :class:`rectorch_amd.samplers.BprTripleSampler`,
which draws the triples.  ``include/rectorch_hip.h`` ("BPRMF rule") has the text.  Nothing here is a training path: the package trains
on the MI355X only, and it has no device BPRMF yet.
"""
import ctypes as C

import numpy as np
from scipy.sparse import csr_matrix

from ._lib import check, lib

__all__ = ["update", "fold_in"]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _table(t, name):
    t = np.array(t, dtype=np.float64, order="C")            # a copy: the caller's table is never written
    if t.ndim != 2:
        raise ValueError("bpr_rule: %s must be a matrix [rows, f], got shape %s" % (name, t.shape))
    return t


def update(U, Y, u, i, j, lr, reg, s=None, want_s=False):
    """One batch of BPRMF's rule on copies of the float64 tables ``U`` ``[n_users, f]`` and ``Y`` ``[n_items, f]``: ``(U', Y')`` -- and
    the coefficients ``s_t`` used with ``want_s``.  ``u, i, j``: the batch's triples (``j = -1``: skipped), e.g. one batch of a
    :class:`BprTripleSampler`.  Every gradient is taken at ``U`` and ``Y``; rows nobody touches keep their bits.  ``s``: coefficients to
    use instead of ``1 / (1 + exp(u_t · (y_i − y_j)))`` -- given another implementation's ``s_t``, the result is what that
    implementation has to produce bit for bit."""
    U, Y = _table(U, "U"), _table(Y, "Y")
    if U.shape[1] != Y.shape[1]:
        raise ValueError("bpr_rule: the tables must have one width, got %d and %d" % (U.shape[1], Y.shape[1]))
    u, i, j = (np.ascontiguousarray(t, dtype=np.int32) for t in (u, i, j))
    if not (u.ndim == i.ndim == j.ndim == 1 and len(u) == len(i) == len(j)):
        raise ValueError("bpr_rule: the triples must be three vectors of one length, got shapes %s, %s, %s" % (u.shape, i.shape, j.shape))
    if s is not None:
        s = np.ascontiguousarray(s, dtype=np.float64)
        if s.shape != u.shape:
            raise ValueError("bpr_rule: %d coefficients for %d samples" % (s.size, len(u)))
    s_out = np.empty(len(u), dtype=np.float64) if want_s else None
    check(lib().rtx_bpr_update_host(_ptr(U), _ptr(Y), U.shape[0], Y.shape[0], U.shape[1], _ptr(u), _ptr(i), _ptr(j), len(u),
                                    C.c_double(float(lr)), C.c_double(float(reg)), _ptr(s), _ptr(s_out)))
    return (U, Y, s_out) if want_s else (U, Y)


def fold_in(rows, Y, lr, reg, fold_in_epochs, seed):
    """The fold-in vectors ``[rows, f]`` of the rows of a scipy sparse matrix (only the pattern is read; a sorted, duplicate-free copy
    is used) against the item factors ``Y``: per row ``fold_in_epochs`` passes of single-sample steps from ``x = 0``.  A function of
    each row's content alone; an empty row and a row that stores every item give zeros."""
    Y = _table(Y, "Y")
    m = csr_matrix(rows, copy=True)
    m.sum_duplicates()
    m.sort_indices()
    if m.shape[1] != Y.shape[0]:
        raise ValueError("bpr_rule: the rows have %d columns, the item factors %d rows" % (m.shape[1], Y.shape[0]))
    indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(m.indices, dtype=np.int32)
    out = np.empty((m.shape[0], Y.shape[1]), dtype=np.float64)
    check(lib().rtx_bpr_fold_in_host(_ptr(indptr), _ptr(indices), m.shape[0], m.shape[1], _ptr(Y), Y.shape[1], C.c_double(float(lr)),
                                     C.c_double(float(reg)), int(fold_in_epochs), C.c_uint64(int(seed)), _ptr(out)))
    return out
