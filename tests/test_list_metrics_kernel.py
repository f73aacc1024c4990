"""GPU: ``rtx_list_metrics`` (k_list_metrics) against the numpy half of ``evaluation.metrics_from_lists``.

Bound: max |diff| <= 1e-12, NaNs in the same places, hit exactly -- the project's device-versus-host bound for these metrics
(tests/test_gpu_parity.py, test_evaluate_device_equals_host_evaluate): both sides add the same float64 terms, at most 1500 of them
here, in different orders, and log2 differs by an ulp at most.  Shapes: users 1, 3, 4, 5, 130 (four users per workgroup: partial and
several workgroups), list lengths 1, 63, 64, 65, 1024, 1500 (a lane owns the ranks lane, lane + 64, ...), 70 and 2100 items,
cut-offs below, at and above the list length.  A list longer than the catalogue continues with ids no row stores (relevance 0).
"""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

pytestmark = pytest.mark.gpu

NS = (1, 3, 4, 5, 130)
KLIST = (1, 63, 64, 65, 1024, 1500)
NAMES = ("ndcg", "recall", "hit", "mrr")


def _heldout(n, n_items, ratings, rng):
    te = (rng.rand(n, n_items) < 0.05).astype(np.float32)
    if n >= 3:
        te[1] = 0.0                                # no held-out item
        te[2] = 0.0
        te[2, n_items - 1] = 1.0                   # one, the last column
    if n >= 5:
        te[4] = 1.0                                # every item
        te[3] = 0.0
        te[3, 0] = 1.0                             # one, the first column
    if ratings:
        te *= rng.randint(1, 6, size=te.shape)
    return te


def _lists(n, K, n_items, rng):
    width = max(K, n_items)
    return np.stack([rng.permutation(width)[:K] for _ in range(n)]).astype(np.int32)


def _cutoffs(K):
    return sorted({1, max(1, K // 2), max(1, K - 1), K, K + 1, K + 700})


def _host(items, te, ks, rows=None):
    from rectorch_amd.evaluation import metrics_from_lists
    res = metrics_from_lists(items, csr_matrix(te), ["%s@%d" % (nm, k) for nm in NAMES for k in ks], rows=rows)
    return {nm: np.stack([res["%s@%d" % (nm, k)] for k in ks]) for nm in NAMES}


def _compare(got, want, tag):
    worst = 0.0
    for nm, g in zip(NAMES, got):
        g, w = g.cpu().numpy(), np.asarray(want[nm], dtype=np.float64)
        assert g.shape == w.shape, (tag, nm, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, nm)
        ok = ~np.isnan(w)
        if nm == "hit":
            assert np.array_equal(g[ok], w[ok]), (tag, nm)
        elif ok.any():
            worst = max(worst, float(np.max(np.abs(g[ok] - w[ok]))))
    assert worst <= 1e-12, (tag, worst)
    return worst


@pytest.mark.parametrize("n_items,ratings", [(70, False), (70, True), (2100, False), (2100, True)])
def test_kernel_equals_the_numpy_half(n_items, ratings):
    from rectorch_amd.engine import CsrMatrix, list_metrics
    rng = np.random.RandomState(n_items + ratings)
    worst, case = 0.0, 0
    for n in NS:
        te = _heldout(n, n_items, ratings, rng)
        perm = rng.permutation(n).astype(np.int32)
        held = CsrMatrix(csr_matrix(te))
        assert held.binary == (not ratings)
        for K in KLIST:
            items = _lists(n, K, n_items, rng)
            ks = _cutoffs(K)
            mode = case % 3                        # row numbers: none, the identity, a permutation
            case += 1
            rows = None if mode == 0 else (np.arange(n, dtype=np.int32) if mode == 1 else perm)
            got = list_metrics(torch.from_numpy(items).cuda(), held, None if rows is None else torch.from_numpy(rows).cuda(), ks)
            assert all(t.is_cuda and t.dtype == torch.float64 and t.shape == (len(ks), n) for t in got)
            worst = max(worst, _compare(got, _host(items, te, ks, rows), (n, K, mode)))
    print("list_metrics vs numpy, %d items, ratings=%s: max |diff| %.2e over %d cases" % (n_items, ratings, worst, case))


def test_more_than_sixteen_cutoffs_a_strided_list_tensor_and_out():
    from rectorch_amd.engine import CsrMatrix, list_metrics
    rng = np.random.RandomState(8)
    n, K, n_items = 6, 40, 70
    te = _heldout(n, n_items, True, rng)
    held = CsrMatrix(csr_matrix(te))
    wide = torch.from_numpy(_lists(n, K + 9, n_items, rng)).cuda()
    items = wide[:, :K]                            # ld = K + 9
    ks = list(range(1, 36, 2))                     # 18 cut-offs: two launches
    out = tuple(torch.full((len(ks), n), -7.0, dtype=torch.float64, device="cuda") for _ in range(4))
    got = list_metrics(items, held, None, ks, out=out)
    assert all(g is o for g, o in zip(got, out))
    _compare(got, _host(items.cpu().numpy(), te, ks), "18 cut-offs")


def test_c_abi_null_outputs_out_ld_and_bad_arguments():
    from rectorch_amd import _lib
    from rectorch_amd.engine import CsrMatrix, list_metrics
    lib = _lib.lib()
    rng = np.random.RandomState(9)
    n, K, n_items, ld_out = 5, 65, 70, 11
    te = _heldout(n, n_items, False, rng)
    held = CsrMatrix(csr_matrix(te))
    items = torch.from_numpy(_lists(n, K, n_items, rng)).cuda()
    ks = [3, 65, 80]
    arr = (C.c_int32 * 3)(*ks)
    want = [t.cpu().numpy() for t in list_metrics(items, held, None, ks)]
    st = _lib.stream_ptr()

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    for skip in (None, 0, 1, 2, 3):                # every output present, then each one NULL in turn; out_ld = 11 > n
        outs = [None if q == skip else torch.full((3, ld_out), -7.0, dtype=torch.float64, device="cuda") for q in range(4)]
        assert lib.rtx_list_metrics(p(items), K, n, K, held.handle, None, arr, 3, *[p(t) for t in outs], ld_out, st) == 0
        torch.cuda.synchronize()
        for q, t in enumerate(outs):
            if t is not None:
                t = t.cpu().numpy()
                assert np.array_equal(t[:, :n], want[q], equal_nan=True), (skip, q)
                assert (t[:, n:] == -7.0).all(), (skip, q)      # nothing written between the rows
    # n = 0: a no-op, whatever the pointers
    assert lib.rtx_list_metrics(None, K, 0, K, held.handle, None, arr, 3, None, None, None, None, 0, st) == 0
    empty = list_metrics(torch.empty((0, K), dtype=torch.int32, device="cuda"), held, None, ks)
    assert all(t.shape == (3, 0) for t in empty)
    out = torch.zeros((3, n), dtype=torch.float64, device="cuda")
    bad = [
        (None, K, n, K, held.handle, None, arr, 3),            # items NULL
        (p(items), K, n, K, None, None, arr, 3),               # held-out matrix NULL
        (p(items), K, n, K, held.handle, None, None, 3),       # cut-offs NULL
        (p(items), K, n, 0, held.handle, None, arr, 3),        # K = 0
        (p(items), K - 1, n, K, held.handle, None, arr, 3),    # ld < K
        (p(items), K, -1, K, held.handle, None, arr, 3),       # n < 0
        (p(items), K, n, K, held.handle, None, arr, 0),        # no cut-off
        (p(items), K, n, K, held.handle, None, arr, 17),       # more than the launch takes
    ]
    for args in bad:
        assert lib.rtx_list_metrics(*args, p(out), None, None, None, n, st) == -1, args
    assert lib.rtx_list_metrics(p(items), K, n, K, held.handle, None, arr, 3, p(out), None, None, None, n - 1, st) == -1   # out_ld < n
    zero = (C.c_int32 * 3)(3, 0, 5)
    assert lib.rtx_list_metrics(p(items), K, n, K, held.handle, None, zero, 3, p(out), None, None, None, n, st) == -1      # k = 0
    small = CsrMatrix(csr_matrix(te[:3]))
    assert lib.rtx_list_metrics(p(items), K, n, K, small.handle, None, arr, 3, p(out), None, None, None, n, st) == -1      # n > rows
    with pytest.raises(_lib.RtxError):
        list_metrics(items.long(), held, None, ks)


def test_empty_rows_get_what_topk_metrics_writes_and_the_two_kernels_agree():
    """(a) users without held-out items: NaN / NaN / 0 / 0, exactly what k_topk_metrics' epilogue writes for them;
    (b) tie-free float32 scores at [9, 2100]: the lists of k_topk_items scored here against k_topk_metrics on the scores."""
    from rectorch_amd.engine import CsrMatrix, list_metrics, topk_items, topk_metrics
    rng = np.random.RandomState(10)
    n, n_items = 9, 2100
    s = rng.standard_normal((n, n_items)).astype(np.float32)
    assert all(len(np.unique(row)) == n_items for row in s)
    te = _heldout(n, n_items, True, rng)
    te[6] = 0.0
    empty = np.flatnonzero(te.sum(axis=1) == 0)
    assert set(empty) == {1, 6}
    held = CsrMatrix(csr_matrix(te))
    scores = torch.from_numpy(s).cuda()
    ks = [1, 20, 100]
    want = topk_metrics(scores, held, None, ks, rank_metrics=True)
    items, _ = topk_items(scores, 100)
    got = list_metrics(items, held, None, ks)
    worst = 0.0
    for nm, g, w in zip(NAMES, got, want):
        g, w = g.cpu().numpy(), w.cpu().numpy()
        assert np.array_equal(g[:, empty], w[:, empty], equal_nan=True), nm
        assert np.array_equal(np.isnan(g), np.isnan(w)), nm
        ok = ~np.isnan(w)
        worst = max(worst, float(np.max(np.abs(g[ok] - w[ok]))))
    assert np.isnan(got[0].cpu().numpy()[:, empty]).all() and np.isnan(got[1].cpu().numpy()[:, empty]).all()
    assert (got[2].cpu().numpy()[:, empty] == 0).all() and (got[3].cpu().numpy()[:, empty] == 0).all()
    print("list_metrics(topk_items) vs topk_metrics: max |diff| %.2e" % worst)
    assert worst <= 1e-12


def test_metrics_from_lists_dispatches_to_the_kernel():
    from rectorch_amd.engine import CsrMatrix
    from rectorch_amd.evaluation import metrics_from_lists
    rng = np.random.RandomState(11)
    n, K, n_items = 7, 30, 70
    te = _heldout(n, n_items, True, rng)
    items = _lists(n, K, n_items, rng)
    mets = ["ndcg@10", "recall@30", "hit@2", "mrr@50"]
    want = metrics_from_lists(items, csr_matrix(te), mets)
    got = metrics_from_lists(torch.from_numpy(items).cuda(), CsrMatrix(csr_matrix(te)), mets)
    for m in mets:
        assert got[m].dtype == want[m].dtype and got[m].shape == (n, ), m
        if m.startswith("hit"):
            assert np.array_equal(got[m], want[m])
        else:
            assert np.allclose(got[m], want[m], rtol=0, atol=1e-12, equal_nan=True), m
