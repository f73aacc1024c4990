"""GPU: the top-N list kernel (rectorch_amd/csrc/recommend.hip) through ``rectorch_amd.engine.topk_items``.

Oracle: numpy on the host -- the exclusion written as -inf into a copy of the scores, ``np.lexsort((ids, -scores))[:k]``.  Item ids
must be equal, scores bitwise equal (a zero of either sign where the oracle holds a zero).  There is no tolerance: the selection is
comparisons only and the reported scores are copies of input elements.

Widths: 7 (< k: K is clamped), 1001 (not a multiple of 4: the scalar tail; once more with the tensor offset by one element, so the
rows are not 16-byte aligned), 4096, 20108 (the burst width) and 20484 (above 20 x 1024: the streamed form).  Batch 5 everywhere.
"""
import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

pytestmark = pytest.mark.gpu

B = 5
KS = (1, 10, 256, 257, 1000, 1024)
WIDTHS = [(7, 0), (1001, 0), (1001, 1), (4096, 0), (20108, 0), (20484, 0)]
DTYPES = {"f32": (np.float32, np.int32), "f64": (np.float64, np.int64)}


def _score_rows(n, np_dtype, seed):
    """[B, n]: normal (float64: its top entries 1 + j 2^-40, distinct doubles that are ONE float); quantised to 8 values (far more
    than 1024 ties at the bound when n is large); all equal; normal with -inf entries; negative with zeros of both signs on top"""
    rng = np.random.RandomState(seed)
    s = np.empty((B, n), dtype=np_dtype)
    s[0] = rng.standard_normal(n)
    if np_dtype is np.float64:
        m = min(n, 300)
        s[0] = np.minimum(s[0] * 0.1, 0.9)
        s[0, rng.choice(n, m, replace=False)] = 1.0 + rng.permutation(m) * 2.0 ** -40
        assert len(np.unique(s[0].astype(np.float32))) < len(np.unique(s[0]))
    s[1] = np.floor(rng.random_sample(n) * 8) / 4 - 1
    s[2] = 0.25
    s[3] = rng.standard_normal(n)
    s[3, rng.random_sample(n) < 0.1] = -np.inf
    s[4] = -1.0 - np.abs(rng.standard_normal(n))
    zeros = rng.choice(n, min(n, 12), replace=False)
    s[4, zeros] = np.where(np.arange(len(zeros)) % 2 == 0, -0.0, 0.0)
    return s


def _exclusion(n, s, seed):
    """dense [B, n] float32 image of the exclusion rows and the boolean mask it stands for: 30 % of the items; all but
    min(5, n - 1) items (fewer than k are left); random with STORED ZEROS (they must not exclude); random; some of row 4's zeros"""
    rng = np.random.RandomState(seed + 1)
    e = np.zeros((B, n), dtype=np.float32)
    stored = np.zeros((B, n), dtype=bool)
    e[0] = rng.random_sample(n) < 0.3
    e[1] = 1
    e[1, rng.choice(n, min(5, n - 1), replace=False)] = 0
    e[2] = (rng.random_sample(n) < 0.2) * 3.0        # (ratings: values other than 1)
    stored[2] = (e[2] != 0) | (rng.random_sample(n) < 0.2)
    e[3] = rng.random_sample(n) < 0.5
    e[4, np.flatnonzero(s[4] == 0)[::3]] = 1
    stored |= e != 0
    return e, stored


def _csr_with_stored_zeros(e, stored, order):
    """rows order[0], order[1], ... of (e, stored) as a CSR matrix that keeps the stored zeros"""
    indptr, indices, data = [0], [], []
    for r in order:
        cols = np.flatnonzero(stored[r])
        indices.extend(cols.tolist())
        data.extend(e[r, cols].tolist())
        indptr.append(len(indices))
    return csr_matrix((np.array(data, np.float32), np.array(indices, np.int32), np.array(indptr, np.int64)), shape=(len(order), e.shape[1]))


def _oracle_order(s, excluded):
    s = s.copy()
    if excluded is not None:
        s[excluded] = -np.inf
    ids = np.broadcast_to(np.arange(s.shape[1]), s.shape)
    return s, np.lexsort((ids, -s), axis=1)


def _check(items, vals, s_masked, order, k, int_dtype, tag):
    kk = min(k, s_masked.shape[1])
    want_items = order[:, :kk]
    got_items = items.cpu().numpy()
    assert got_items.shape == (B, kk) and got_items.dtype == np.int32, tag
    assert np.array_equal(got_items, want_items), (tag, np.argwhere(got_items != want_items)[:4])
    if vals is not None:
        want = np.take_along_axis(s_masked, want_items, axis=1)
        got = vals.cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, tag
        same = (got.view(int_dtype) == want.view(int_dtype)) | ((want == 0) & (got == 0))
        assert same.all(), (tag, np.argwhere(~same)[:4])


def _device_scores(s, offset):
    """the rows on the device; offset = 1: the tensor starts one element into its allocation"""
    t = torch.from_numpy(s)
    buf = torch.empty(s.size + offset, dtype=t.dtype, device="cuda")
    view = buf[offset:].view(s.shape)
    view.copy_(t)
    assert view.data_ptr() == buf.data_ptr() + offset * t.element_size()
    return view


@pytest.mark.parametrize("width,offset", WIDTHS)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_topk_items_equals_lexsort(dtype, width, offset):
    from rectorch_amd.engine import CsrMatrix, topk_items
    np_dtype, int_dtype = DTYPES[dtype]
    s = _score_rows(width, np_dtype, 100 + width)
    e, stored = _exclusion(width, s, width)
    dev = _device_scores(s, offset)
    before = dev.clone()
    # exclusion: none; the users' rows in batch order; the rows scattered over a larger matrix and named by excl_row_ids
    perm = [6, 2, 7, 0, 4]
    scattered = [3, 4, 1, 0, 4, 2, 0, 2]             # matrix row perm[b] holds user b's row; the others are decoys
    for b, r in enumerate(perm):
        scattered[r] = b
    modes = [("none", None, None, None),
             ("rows", CsrMatrix(_csr_with_stored_zeros(e, stored, range(B))), None, e != 0),
             ("row_ids", CsrMatrix(_csr_with_stored_zeros(e, stored, scattered)), torch.tensor(perm, dtype=torch.int32, device="cuda"),
              e != 0)]
    for name, excl, rows, excluded in modes:
        s_masked, order = _oracle_order(s, excluded)
        for k in KS:
            items, vals = topk_items(dev, k, excl, rows)
            _check(items, vals, s_masked, order, k, int_dtype, (dtype, width, offset, name, k))
        # item_scores = NULL: the same ids
        items_only, none = topk_items(dev, 10, excl, rows, want_scores=False)
        assert none is None
        _check(items_only, None, s_masked, order, 10, int_dtype, (dtype, width, offset, name, "ids only"))
    assert torch.equal(dev.view(torch.int32 if dtype == "f32" else torch.int64), before.view(torch.int32 if dtype == "f32" else torch.int64)), \
        "the exclusion must not write to the scores"


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_k_above_1024_is_the_host_route_only(dtype):
    """k = 2000: topk_items refuses it, recommend_host -- and recommend, which goes there -- give the lexsort"""
    from rectorch_amd._lib import RtxError
    from rectorch_amd.engine import topk_items
    from rectorch_amd.evaluation import recommend, recommend_host
    np_dtype, int_dtype = DTYPES[dtype]
    s = _score_rows(4096, np_dtype, 5)
    dev = _device_scores(s, 0)
    for bad in (2000, 1025, 0, -3):
        with pytest.raises(RtxError):
            topk_items(dev, bad)

    class Scores:                                    # a model whose predict returns what it is given
        def predict(self, x, remove_train=True):
            return (x, )

    s_masked, order = _oracle_order(s, None)
    for fn in (recommend_host, recommend):
        items, vals = fn(Scores(), [(dev, None)], k=2000)
        assert items.is_cuda and vals.is_cuda
        _check(items, vals, s_masked, order, 2000, int_dtype, (dtype, fn.__name__))


def test_topk_items_argument_errors():
    from rectorch_amd import _lib
    from rectorch_amd.engine import topk_items
    C = __import__("ctypes")
    s = torch.zeros((2, 8), device="cuda")
    items = torch.empty((2, 3), dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    lib = _lib.lib()
    assert lib.rtx_topk_items(p(s), _lib.RTX_F32, 8, 2, 8, None, None, 3, None, None, None) == -1          # items NULL
    assert b"items" in lib.rtx_last_error()
    assert lib.rtx_topk_items(p(s), 1, 8, 2, 8, None, None, 3, p(items), None, None) == -1                 # unknown dtype
    assert b"dtype" in lib.rtx_last_error()
    assert lib.rtx_topk_items(p(s), _lib.RTX_F32, 8, 2, 8, None, None, 0, p(items), None, None) == -1
    assert lib.rtx_topk_items(p(s), _lib.RTX_F32, 8, 2, 8, None, None, 1025, p(items), None, None) == -1
    assert b"1024" in lib.rtx_last_error()
    with pytest.raises(_lib.RtxError):
        topk_items(s.to(torch.float16), 3)
    # the dispatcher's op is the same call
    from rectorch_amd import ops  # noqa: F401
    a, b = torch.ops.rectorch_hip.topk_items(s, 3, 0, None)
    assert a.tolist() == [[0, 1, 2], [0, 1, 2]] and b.tolist() == [[0.0] * 3] * 2
