r"""Batch samplers with the reference's API (rectorch/samplers.py:18-107) and a device-resident fast path.

``DataSampler`` keeps the rating matrices in HBM as CSR (uploaded once) and forms every batch on the
MI355X with the LDS-staged gather kernel, instead of the reference's per-batch scipy fancy-index +
``toarray()`` + float64->float32 copy on the host (the reference's CPU hot spot #1, ~164 ms per 500-user
batch).  Iterating it yields the same ``(data_tr, data_te | None)`` pairs of float32 ``[B, n_items]``
tensors in the same order (the permutation comes from the same global-numpy-RNG shuffle), now resident on the
device; ``iter_rows()`` yields only row numbers for trainers that take the sparse rows directly.
"""
import numpy as np
import torch
from scipy.sparse import csr_matrix, hstack

from .engine import CondBuilder, CsrMatrix, RowBatch, SvaeEvalPack, SvaePack, SvaeTarget, tag_rows

__all__ = ['Sampler', 'DataSampler', 'ConditionedDataSampler', 'BalancedConditionedDataSampler',
           'EmptyConditionedDataSampler', 'SVAE_Sampler', 'BprTripleSampler', 'pack_conditions', 'plan_batches', 'is_resident_conditioned']


class Sampler():
    r"""Sampler base class (reference samplers.py:18-40): a generator of batches.  Sub-classes implement
    ``__len__`` (number of batches) and ``__iter__``."""
    def __init__(self, *args, **kargs):
        pass

    def __len__(self):
        """Return the number of batches."""
        raise NotImplementedError

    def __iter__(self):
        """Iterate through the batches yielding a batch at a time."""
        raise NotImplementedError


class DataSampler(Sampler):
    r"""Plain batches of users, in order or shuffled (counterpart of reference samplers.py:43-107).

    Arguments (the first four are the reference's, positionally compatible; the attributes of the same names are public):

    * ``sparse_data_tr`` -- scipy CSR matrix, one row per user: what the model reads.
    * ``sparse_data_te`` -- optional CSR matrix of the same users: the second element of every yielded pair (held-out
      items at evaluation time); ``None`` yields ``None`` there.
    * ``batch_size`` -- users per batch (the last batch may be shorter); default 1.
    * ``shuffle`` -- draw a fresh permutation of the users from numpy's GLOBAL generator at every ``iter()``; default on.
    * ``device`` (not in the reference) -- ``None`` picks the MI355X when one is visible: the matrices are uploaded once
      and batches are formed by the gather kernel; ``"cpu"`` reproduces the reference's host behaviour (scipy slicing +
      ``toarray()``) for callers without a HIP device.  It is not a compute path of this package.
    * ``user_ids`` (not in the reference; for :class:`rectorch_amd.nets.CDAE_net`) -- the user id of every row: ``"rows"``
      (row ``r`` is user ``r``), an int array of one id per row with ``-1`` for users the model has no vector for, or
      ``None`` (no ids).  Checked once, here, on the host: one id per row, every id ``>= -1``, no id twice (a batch must not
      name a user twice, and a batch is any subset of the rows).  Every batch then carries its ids: ``RowBatch.users`` (a
      device int32 slice) on the fast path and in the tag of the dense tensors ``__iter__`` yields, the attribute
      ``_rtx_users`` (int32, on the host) of ``data_tr`` in the CPU fall-back.  ``max_user_id`` is the largest id (-1: none).
    """
    def __init__(self,
                 sparse_data_tr,
                 sparse_data_te=None,
                 batch_size=1,
                 shuffle=True,
                 device=None,
                 user_ids=None):
        super(DataSampler, self).__init__()
        self.sparse_data_tr = sparse_data_tr
        self.sparse_data_te = sparse_data_te
        self.batch_size = batch_size
        self.shuffle = shuffle
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self._csr_tr = self._csr_te = None
        self._src = (None, None)
        self.user_ids, self.max_user_id = self._check_user_ids(user_ids, sparse_data_tr.shape[0])
        self._user_ids_dev = None

    @staticmethod
    def _check_user_ids(user_ids, n_rows):
        """``(ids, largest id)``: ``None`` / ``"rows"`` as given, anything else as a checked int32 array of one id per row"""
        if user_ids is None:
            return None, -1
        if isinstance(user_ids, str):
            if user_ids != "rows":
                raise ValueError("user_ids = %r; supported: 'rows' (row r is user r), an int array of one id per row (-1: unknown "
                                 "user), or None" % (user_ids,))
            return "rows", n_rows - 1
        ids = np.asarray(user_ids.cpu() if isinstance(user_ids, torch.Tensor) else user_ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("user_ids must be a one-dimensional int array (one id per row, -1: unknown user), got %s of shape %s"
                             % (ids.dtype, ids.shape))
        if ids.shape[0] != n_rows:
            raise ValueError("user_ids holds %d ids for %d rows: one id per row is needed" % (ids.shape[0], n_rows))
        ids = ids.astype(np.int64)
        if ids.size and (ids.min() < -1 or ids.max() >= 2 ** 31):
            raise ValueError("user_ids must lie in [-1, 2^31): the smallest is %d, the largest %d (-1 marks an unknown user)"
                             % (ids.min(), ids.max()))
        known = ids[ids >= 0]
        uniq, counts = np.unique(known, return_counts=True)
        if (counts > 1).any():
            raise ValueError("user_ids names user %d for %d rows: an id may appear once (the rows of a batch update their users' "
                             "vectors without atomics); give the other rows -1" % (uniq[counts > 1][0], counts[counts > 1][0]))
        return ids.astype(np.int32), int(known.max()) if known.size else -1

    def _batch_users(self, rows):
        """the user ids of the batch ``rows`` (device int32 row numbers) as a device int32 tensor, or None"""
        if self.user_ids is None:
            return None
        if isinstance(self.user_ids, str):
            return rows
        if self._user_ids_dev is None or self._user_ids_dev.device != rows.device:
            self._user_ids_dev = torch.from_numpy(self.user_ids).to(rows.device)
        return self._user_ids_dev.index_select(0, rows.long())

    def __len__(self):
        return int(np.ceil(self.sparse_data_tr.shape[0] / self.batch_size))

    @property
    def resident(self):
        return self.device.type == "cuda"

    def _upload(self):
        # re-upload if the user swapped the matrices (attributes are public, as in the reference)
        if self._src[0] is not self.sparse_data_tr:
            self._csr_tr = CsrMatrix(self.sparse_data_tr)
        if self._src[1] is not self.sparse_data_te:
            self._csr_te = None if self.sparse_data_te is None else CsrMatrix(self.sparse_data_te)
            if self._csr_te is not None:
                # same users; a conditioned input matrix carries its condition columns after the items (CMultiVAE)
                assert self._csr_te.shape[0] == self._csr_tr.shape[0] and self._csr_te.shape[1] <= self._csr_tr.shape[1], \
                    "tr and te matrices must have the same shape"
        self._src = (self.sparse_data_tr, self.sparse_data_te)

    def _order(self):
        n = self.sparse_data_tr.shape[0]
        idxlist = list(range(n))
        if self.shuffle:
            np.random.shuffle(idxlist)      # global numpy RNG, fresh permutation per iter() (samplers.py:93-95)
        return n, idxlist

    def iter_rows(self):
        """Fast path: yields :class:`rectorch_amd.engine.RowBatch` (row numbers on the device), nothing dense."""
        assert self.resident, "iter_rows() needs the device-resident sampler"
        self._upload()
        if self.shuffle:
            n, idxlist = self._order()
            rows = torch.from_numpy(np.asarray(idxlist, dtype=np.int32)).to(self.device)
        else:
            # the identity order of a validation / test loader: one device arange, kept (a Python list of n ints turned into an array
            # and copied to the device was 250 us of every evaluate() call -- a tenth of the whole call at 10 000 users)
            n = self.sparse_data_tr.shape[0]
            rows = getattr(self, "_seq_rows", None)
            if rows is None or rows.numel() != n or rows.device != self.device:
                rows = self._seq_rows = torch.arange(n, dtype=torch.int32, device=self.device)
        for start_idx in range(0, n, self.batch_size):
            end_idx = min(start_idx + self.batch_size, n)
            r = rows[start_idx:end_idx]
            yield RowBatch(self._csr_tr, self._csr_te, r, users=self._batch_users(r))

    def __iter__(self):
        if not self.resident:
            yield from self._iter_host()
            return
        for rb in self.iter_rows():
            # tagged: the trainer skips the dense detour when it gets this tensor back UNMODIFIED
            data_tr = tag_rows(self._csr_tr.gather_dense(rb.rows), rb)
            data_te = None
            if self._csr_te is not None:
                data_te = tag_rows(self._csr_te.gather_dense(rb.rows), rb)
            yield data_tr, data_te

    def _iter_host(self):
        # the reference's host behaviour, for callers without a HIP device (samplers.py:91-107)
        n, idxlist = self._order()
        for start_idx in range(0, n, self.batch_size):
            end_idx = min(start_idx + self.batch_size, n)
            data_tr = self.sparse_data_tr[idxlist[start_idx:end_idx]]
            data_tr = torch.FloatTensor(data_tr.toarray())
            if self.user_ids is not None:
                rows = np.asarray(idxlist[start_idx:end_idx], dtype=np.int32)
                data_tr._rtx_users = torch.from_numpy(rows if isinstance(self.user_ids, str) else self.user_ids[rows])
            data_te = None
            if self.sparse_data_te is not None:
                data_te = self.sparse_data_te[idxlist[start_idx:end_idx]]
                data_te = torch.FloatTensor(data_te.toarray())
            yield data_tr, data_te


def _sparse_pair(data_tr, data_te):
    """``(input rows, target rows)`` of one batch as two device-resident :class:`RowBatch` objects over the same row
    ids -- what the ``sparse=True`` samplers yield in place of the dense ``(data, target)`` tensors.  It is a PAIR like
    every other sampler's item: ``train_epoch`` / ``evaluate`` / ``one_plus_random`` unpack it unchanged."""
    tr, te = CsrMatrix(data_tr), CsrMatrix(data_te)
    rows = torch.arange(data_tr.shape[0], dtype=torch.int32, device="cuda")
    return RowBatch(tr, te, rows), RowBatch(te, None, rows)


def pack_conditions(iid2cids, n_cond, n_items):
    """The item -> condition lists as the bitmap the device builder tests target items against: ``(bits, any)`` with ``bits``
    uint32 ``[n_items, ceil(n_cond / 32)]`` -- bit ``c % 32`` of word ``c // 32`` of row *i* set when condition *c* is in item *i*'s
    list -- and ``any`` uint32 ``[ceil(n_items / 32)]``, bit ``i % 32`` of word ``i // 32`` set when item *i* has at least one
    condition.  Items without an entry in ``iid2cids`` have none.  Host only."""
    W = (int(n_cond) + 31) // 32
    bits = np.zeros((int(n_items), W), dtype=np.uint32)
    any_ = np.zeros((int(n_items) + 31) // 32, dtype=np.uint32)
    for i, cids in iid2cids.items():
        i = int(i)
        if not 0 <= i < n_items:
            raise ValueError("iid2cids names item %d of %d" % (i, n_items))
        for c in cids:
            c = int(c)
            if not 0 <= c < n_cond:
                raise ValueError("item %d lists condition %d of %d" % (i, c, n_cond))
            bits[i, c >> 5] |= np.uint32(1 << (c & 31))
            any_[i >> 5] |= np.uint32(1 << (i & 31))
    return bits, any_


def plan_batches(idxlist, batch_size, keep):
    """The batches of one epoch of a resident conditioned sampler: the example order ``idxlist`` cut into ``batch_size`` pieces --
    the cut comes BEFORE the drop, as in the host samplers -- each reduced to its kept examples (``keep``: bool per example),
    a piece that becomes empty skipped.  List of int32 arrays of example ids.  Host only."""
    order = np.asarray(idxlist, dtype=np.int64)
    keep = np.asarray(keep, dtype=bool)
    out = []
    for start in range(0, len(order), batch_size):
        ids = order[start:start + batch_size]
        ids = ids[keep[ids]]
        if len(ids):
            out.append(ids.astype(np.int32))
    return out


def is_resident_conditioned(loader):
    """True for a conditioned sampler constructed with ``resident=True`` (its ``iter_rows()`` yields device-built batches)"""
    return isinstance(loader, _ResidentConditioned) and bool(loader.resident)


class _ResidentConditioned:
    """``resident=True`` of the three conditioned samplers: the batches are built on the device (csrc/cond_rows.hip) from
    matrices, bitmap and example table uploaded ONCE; per epoch only the example order is uploaded."""
    resident = False

    def _make_resident(self, n_cond, bitmap, examples):
        tr = CsrMatrix(self.sparse_data_tr)
        te = tr if self.sparse_data_te is None or self.sparse_data_te is self.sparse_data_tr else CsrMatrix(self.sparse_data_te)
        examples = np.asarray(examples, dtype=np.int64).reshape(-1, 2)
        self._cond = CondBuilder(tr, te, n_cond, bitmap, examples[:, 0], examples[:, 1], max_batch=self.batch_size)
        # what the host samplers drop: the examples whose filtered target is empty (nothing when targets are not filtered)
        self._keep = self._cond.target_len != 0 if bitmap is not None else np.ones(len(examples), dtype=bool)
        self._rows = torch.arange(self.batch_size, dtype=torch.int32, device="cuda")
        self.resident = True

    def _n_examples(self):
        return len(self.examples)

    def _example_order(self):
        """the epoch's example order: the host samplers' own shuffle of the same list, so a seed gives the same batches"""
        idxlist = list(range(self._n_examples()))
        if self.shuffle:
            np.random.shuffle(idxlist)
        return idxlist

    def iter_rows(self):
        """yields :class:`rectorch_amd.engine.RowBatch` ``(input rows, target rows, 0..b-1)`` over a slot of the builder's ring.
        A batch is valid until the ring comes round (its matrices raise ``RtxError`` afterwards): consume them as they come."""
        assert self.resident, "iter_rows() needs resident=True"
        plan = plan_batches(self._example_order(), self.batch_size, self._keep)
        if not plan:
            return
        flat = np.concatenate(plan)
        ids = torch.from_numpy(flat).to("cuda")                  # the whole epoch's example ids, once
        lo = 0
        for b in plan:
            n = len(b)
            tr, te = self._cond.build(ids[lo:lo + n], n, int(self._cond.in_len[b].sum()), int(self._cond.target_len[b].sum()))
            lo += n
            yield RowBatch(tr, te, self._rows[:n])

    def _iter_resident(self):
        for rb in self.iter_rows():
            yield rb, RowBatch(rb.te, None, rb.rows)             # the pair _sparse_pair yields


class ConditionedDataSampler(_ResidentConditioned, Sampler):
    r"""Data sampler with conditioned filtering for :class:`rectorch_amd.models.CMultiVAE` (reference
    samplers.py:108-234).

    Every user appears once unconditioned -- example ``(row, -1)`` -- and once per condition known to at least one of
    the user's items -- ``(row, c)``.  A batch is the examples' training rows with the ``n_cond`` one-hot condition
    columns appended, and as target the test rows restricted to the items valid under the example's condition (all
    items having any condition when unconditioned); examples whose filtered target is empty are dropped.

    This is host-side bookkeeping, as in the reference; the batches it yields are what the MI355X engine consumes.
    With ``sparse=True`` (not in the reference) the pair is yielded as two :class:`rectorch_amd.engine.RowBatch`
    objects (input rows, target rows) over small per-batch CSR matrices uploaded to HBM, so nothing dense of width
    ``n_items`` crosses PCIe.

    With ``resident=True`` (not in the reference either; needs a HIP device) nothing is assembled on the host per batch: the
    matrices, the item -> condition bitmap and the example table are uploaded once at construction, and every batch is written
    by the device into a small ring of CSR pairs; the same pairs of :class:`RowBatch` come out, in the same order for the same
    seed.  A yielded batch stays valid for the next two batches only: consume the batches as they come (``list(sampler)``
    followed by training on its first element raises ``RtxError``).  The matrices are those given at construction.

    Arguments: ``iid2cids`` (dict item id -> list of the conditions, integers below ``n_cond``, the item satisfies),
    ``n_cond`` (how many conditions exist), ``sparse_data_tr`` / ``sparse_data_te`` (CSR matrices of the users' input and
    target items; the target defaults to the input), ``batch_size`` (examples per batch, default 1), ``shuffle``
    (permute the examples with numpy's global generator before batching, default on), ``sparse`` and ``resident`` (see above).
    """
    def __init__(self,
                 iid2cids,
                 n_cond,
                 sparse_data_tr,
                 sparse_data_te=None,
                 batch_size=1,
                 shuffle=True,
                 sparse=False,
                 resident=False):
        super(ConditionedDataSampler, self).__init__()
        self.sparse_data_tr = sparse_data_tr
        self.sparse_data_te = sparse_data_te
        self.iid2cids = iid2cids
        self.batch_size = batch_size
        self.n_cond = n_cond
        self.shuffle = shuffle
        self.sparse = sparse
        self._compute_conditions()
        if resident:
            self._make_resident_conditioned()

    def _make_resident_conditioned(self):
        n_items = self.sparse_data_tr.shape[1]
        self._make_resident(self.n_cond, pack_conditions(self.iid2cids, self.n_cond, n_items), self.examples)

    def _row_conditions(self):
        """row -> the set of conditions of the row's items.  Built as a union of per-item sets in column order so that
        iterating it visits the conditions in the order the reference's own sets do (samplers.py:171-174)."""
        tr = self.sparse_data_tr.tocsr()
        out = {}
        for r in range(tr.shape[0]):
            cols = tr.indices[tr.indptr[r]:tr.indptr[r + 1]][tr.data[tr.indptr[r]:tr.indptr[r + 1]] != 0]
            out[r] = set.union(*[set(self.iid2cids[c]) for c in np.sort(cols)])
        return out

    def _item_condition_matrix(self):
        items = list(self.iid2cids)
        rows = np.repeat(items, [len(self.iid2cids[m]) for m in items]).astype(np.int64)
        cols = np.array([g for m in items for g in self.iid2cids[m]], dtype=np.int64)
        return csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(len(self.iid2cids), self.n_cond))

    def _compute_conditions(self):
        r2cond = self._row_conditions()
        ex = [(r, -1) for r in r2cond]
        ex += [(r, c) for r in r2cond for c in r2cond[r]]
        self.examples = np.array(ex)
        self.M = self._item_condition_matrix()

    def __len__(self):
        return int(np.ceil(len(self.examples) / self.batch_size))

    def _batch(self, ex):
        """(input rows [b, n_items + n_cond], filtered target rows [b, n_items]) as scipy CSR, empty targets dropped"""
        n = len(ex)
        rows_, conds = ex[:, 0], ex[:, 1]
        has = conds >= 0
        onehot = csr_matrix((np.ones(int(has.sum())), (np.nonzero(has)[0], conds[has])), shape=(n, self.n_cond))
        data_tr = hstack([self.sparse_data_tr[rows_], onehot], format="csr")
        if self.sparse_data_te is None:
            self.sparse_data_te = self.sparse_data_tr
        # an unconditioned example admits every condition
        allow = onehot.tolil()
        allow[np.nonzero(~has)[0], :] = 1
        filtered = allow.tocsr().dot(self.M.transpose().tocsr()) > 0
        data_te = self.sparse_data_te[rows_].multiply(filtered).tocsr()
        keep = np.diff(data_te.indptr) != 0
        return data_tr[keep], data_te[keep]

    def _emit(self, data_tr, data_te):
        if self.sparse:
            return _sparse_pair(data_tr, data_te)
        return torch.FloatTensor(data_tr.toarray()), torch.FloatTensor(data_te.toarray())

    def __iter__(self):
        if self.resident:
            yield from self._iter_resident()
            return
        n = len(self.examples)
        idxlist = list(range(n))
        if self.shuffle:
            np.random.shuffle(idxlist)
        for start_idx in range(0, n, self.batch_size):
            end_idx = min(start_idx + self.batch_size, n)
            data_tr, data_te = self._batch(self.examples[idxlist[start_idx:end_idx]])
            yield self._emit(data_tr, data_te)


class BalancedConditionedDataSampler(ConditionedDataSampler):
    r"""Sub-sampled version of :class:`ConditionedDataSampler` (reference samplers.py:237-338): every user once
    unconditioned, plus for each condition *c* ``m = int(num_cond_examples * subsample / n_cond)`` users drawn with
    replacement (``np.random.choice``) among those knowing *c*.

    ``subsample`` (in (0, 1], default 0.2) is the fraction of conditioned examples kept; the other arguments are
    :class:`ConditionedDataSampler`'s, without ``shuffle`` (the reference has none here either).
    """
    def __init__(self,
                 iid2cids,
                 n_cond,
                 sparse_data_tr,
                 sparse_data_te=None,
                 batch_size=1,
                 subsample=.2,
                 sparse=False,
                 resident=False):
        super(BalancedConditionedDataSampler, self).__init__(iid2cids,
                                                             n_cond,
                                                             sparse_data_tr,
                                                             sparse_data_te,
                                                             batch_size,
                                                             sparse=sparse)
        self.subsample = subsample
        self._compute_sampled_conditions()
        if resident:
            self._make_resident_conditioned()      # (after the draws: the example table is what np.random.choice picked)

    def _compute_conditions(self):
        r2cond = self._row_conditions()
        self.examples = {-1: list(r2cond.keys())}
        for c in range(self.n_cond):
            self.examples[c] = [r for r in r2cond if c in r2cond[r]]
        self.num_cond_examples = sum(len(self.examples[c]) for c in range(self.n_cond))
        self.M = self._item_condition_matrix()

    def _compute_sampled_conditions(self):
        data = [(r, -1) for r in self.examples[-1]]
        m = int(self.num_cond_examples * self.subsample / self.n_cond)
        for c in range(self.n_cond):
            data += [(r, c) for r in np.random.choice(self.examples[c], m)]
        self.examples = np.array(data)

    def __len__(self):
        m = int(self.num_cond_examples * self.subsample) + self.sparse_data_tr.shape[0]
        return int(np.ceil(m / self.batch_size))


class EmptyConditionedDataSampler(_ResidentConditioned, Sampler):
    r"""Unconditioned batches for :class:`rectorch_amd.models.CMultiVAE` (reference samplers.py:341-419): like
    :class:`DataSampler`, with ``cond_size`` zero columns appended to the input rows.

    ``cond_size`` is the number of condition columns to append; the remaining arguments are :class:`DataSampler`'s, ``sparse``
    and ``resident`` :class:`ConditionedDataSampler`'s (every example is ``(row, -1)``, targets are not filtered, nothing is
    dropped).
    """
    def __init__(self,
                 cond_size,
                 sparse_data_tr,
                 sparse_data_te=None,
                 batch_size=1,
                 shuffle=True,
                 sparse=False,
                 resident=False):
        super(EmptyConditionedDataSampler, self).__init__()
        self.sparse_data_tr = sparse_data_tr
        self.sparse_data_te = sparse_data_te
        self.batch_size = batch_size
        self.cond_size = cond_size
        self.shuffle = shuffle
        self.sparse = sparse
        if resident:
            n = sparse_data_tr.shape[0]
            self._make_resident(cond_size, None, np.stack([np.arange(n), np.full(n, -1)], axis=1))

    def __len__(self):
        return int(np.ceil(self.sparse_data_tr.shape[0] / self.batch_size))

    def _n_examples(self):
        return self.sparse_data_tr.shape[0]

    def __iter__(self):
        if self.resident:
            yield from self._iter_resident()
            return
        n = self.sparse_data_tr.shape[0]
        idxlist = list(range(n))
        if self.shuffle:
            np.random.shuffle(idxlist)
        for start_idx in range(0, n, self.batch_size):
            rows = idxlist[start_idx:min(start_idx + self.batch_size, n)]
            data_tr = self.sparse_data_tr[rows]
            data_tr = hstack([data_tr, csr_matrix((data_tr.shape[0], self.cond_size))], format="csr")
            if self.sparse_data_te is None:
                self.sparse_data_te = self.sparse_data_tr
            data_te = self.sparse_data_te[rows]
            if self.sparse:
                yield _sparse_pair(data_tr, data_te)
            else:
                yield torch.FloatTensor(data_tr.toarray()), torch.FloatTensor(data_te.toarray())


class SVAE_Sampler(Sampler):
    r"""Sampler of user sequences for :class:`rectorch_amd.models.SVAE` (reference samplers.py:446-571): one user per
    batch, ``x`` = the LongTensor ``[1, T]`` of all but the user's last item, ``y`` = the multi-hot targets
    ``[1, T, num_items]``: at step *t* the next item (``'next'``), the next ``k`` items (``'next_k'``) or all the
    remaining ones (``'postfix'``); with ``is_training=False`` a single row ``[1, 1, num_items]`` holding the user's
    test items.

    With ``sparse=True`` (not in the reference) ``y`` is a :class:`rectorch_amd.engine.SvaeTarget` -- the same rows as
    a CSR on the device -- so no ``T x num_items`` dense tensor is built or copied per user.

    Arguments: ``num_items``; ``dict_data_tr`` (dict user -> list of item ids in interaction order, users numbered from
    0); ``dict_data_te`` (dict user -> test items; required when ``is_training`` is off); ``pred_type`` (``'next_k'``
    -- the default -- ``'next'`` or ``'postfix'``); ``k`` (items to predict for ``'next_k'``, at least 1); ``shuffle``
    (visit the users in a random order drawn from numpy's global generator, default on); ``is_training`` (default on);
    ``sparse`` (see above); ``pack`` (not in the reference, default 1 = one user per batch and per optimizer step, as the
    reference): with ``pack = N > 1`` a training batch is a :class:`rectorch_amd.engine.SvaePack` of up to ``N`` users --
    yielded as ``(pack, pack)`` -- on which :meth:`rectorch_amd.models.SVAE.train_batch` takes ONE Adam step for the mean of the
    users' losses (gradient accumulation over the pack).  A pack costs its LONGEST recurrence, so the (shuffled) users are
    grouped by length inside windows of ``16 * N`` users and the packs of a window visited in random order; ``pack_tokens``
    bounds the time steps of one pack (default 16 384).

    With ``is_training=False`` and ``pack = N > 1`` (not in the reference either) a batch is ``(SvaeEvalPack, RowBatch)``: up to
    ``N`` users -- and at most ``pack_tokens`` time steps -- cut CONSECUTIVELY from the visiting order (never sorted by length: the
    results of an evaluation come back in loader order), and their rows of ONE device-resident binary ``[n_users, num_items]`` CSR
    of all users' test items, uploaded once per sampler.  :meth:`rectorch_amd.models.SVAE.predict` scores such a pack in one call
    and :func:`rectorch_amd.evaluation.evaluate` ranks it on the device.  Users with fewer than two training items have no time
    step to score and are SKIPPED, as training packs skip them (``pack=1`` yields them with an empty ``x``, as the reference does).
    """
    def __init__(self,
                 num_items,
                 dict_data_tr,
                 dict_data_te=None,
                 pred_type="next_k",
                 k=1,
                 shuffle=True,
                 is_training=True,
                 sparse=False,
                 pack=1,
                 pack_tokens=16384):
        super(SVAE_Sampler, self).__init__()
        if pred_type == "next_k":
            assert k >= 1, "If pred_type == 'next_k' then 'k' must be a positive integer."
        self.pred_type = pred_type
        self.dict_data_tr = dict_data_tr
        self.dict_data_te = dict_data_te
        self.shuffle = shuffle
        self.num_items = num_items
        self.k = k
        self.is_training = is_training
        self.sparse = sparse
        assert pack >= 1 and pack_tokens >= 1
        self.pack = int(pack)
        self.pack_tokens = int(pack_tokens)

    def __len__(self):
        if self.pack > 1 and self.is_training:
            # packs of the unshuffled order; a shuffled epoch may differ by a pack or two (the token bound cuts differently)
            return sum(len(w) for w in self._pack_windows(list(range(len(self.dict_data_tr)))))
        if self.pack > 1:
            return len(self._eval_packs(list(range(len(self.dict_data_tr)))))
        return len(self.dict_data_tr)

    def _eval_packs(self, idxlist):
        """the users of ``idxlist`` cut, IN ORDER, into packs (lists of users) of at most ``pack`` users and ``pack_tokens`` time
        steps (a user longer than that is a pack of its own); users without a time step (fewer than 2 items) are skipped"""
        packs, cur, tok = [], [], 0
        for u in idxlist:
            t = len(self.dict_data_tr[u]) - 1
            if t < 1:
                continue
            if cur and (len(cur) == self.pack or tok + t > self.pack_tokens):
                packs.append(cur)
                cur, tok = [], 0
            cur.append(u)
            tok += t
        if cur:
            packs.append(cur)
        return packs

    def _heldout_csr(self):
        """every user's distinct test items as ONE binary [n_users, num_items] scipy CSR (row u = the reference's ``y[0, 0, te] = 1``)"""
        n = len(self.dict_data_tr)
        rows = [list(dict.fromkeys(self.dict_data_te.get(u, ()))) for u in range(n)]
        indptr = np.zeros(n + 1, dtype=np.int64)
        indptr[1:] = np.cumsum([len(r) for r in rows])
        indices = np.fromiter((i for r in rows for i in r), dtype=np.int32, count=int(indptr[-1]))
        return csr_matrix((np.ones(len(indices), dtype=np.float32), indices, indptr), shape=(n, self.num_items))

    def _heldout_resident(self):
        if getattr(self, "_te_src", None) is not self.dict_data_te:      # uploaded once; again if the caller swapped the dict
            self._te_csr = CsrMatrix(self._heldout_csr())
            self._te_src = self.dict_data_te
        return self._te_csr

    def _pack_windows(self, idxlist):
        """the users of ``idxlist`` cut into windows of 16 * pack, each sorted by length and cut into packs (lists of users)
        of at most ``pack`` users and ``pack_tokens`` time steps; users without a time step (fewer than 2 items) are skipped"""
        window = 16 * self.pack
        out = []
        for w0 in range(0, len(idxlist), window):
            win = [u for u in idxlist[w0:w0 + window] if len(self.dict_data_tr[u]) >= 2]
            win.sort(key=lambda u: len(self.dict_data_tr[u]))
            packs, cur, tok = [], [], 0
            for u in win:
                t = len(self.dict_data_tr[u]) - 1
                if cur and (len(cur) == self.pack or tok + t > self.pack_tokens):
                    packs.append(cur)
                    cur, tok = [], 0
                cur.append(u)
                tok += t
            if cur:
                packs.append(cur)
            out.append(packs)
        return out

    def _target_rows(self, user):
        """the distinct target items of every time step of ``user`` (list of lists)"""
        seq = self.dict_data_tr[user]
        if not self.is_training:
            return [list(dict.fromkeys(self.dict_data_te[user]))]
        rows = []
        for t in range(len(seq) - 1):
            if self.pred_type == 'next':
                r = [seq[t + 1]]
            elif self.pred_type == 'next_k':
                r = seq[t + 1:][:self.k]
            elif self.pred_type == 'postfix':
                r = seq[t + 1:]
            else:
                r = []
            rows.append(list(dict.fromkeys(r)))
        return rows

    def __iter__(self):
        idxlist = list(range(len(self.dict_data_tr)))
        if self.shuffle:
            np.random.shuffle(idxlist)
        if self.pack > 1 and self.is_training:
            for packs in self._pack_windows(idxlist):
                order = np.random.permutation(len(packs)) if self.shuffle else range(len(packs))
                for pi in order:
                    users = packs[pi]
                    p = SvaePack([self.dict_data_tr[u][:-1] for u in users], [self._target_rows(u) for u in users], users)
                    yield p, p
            return
        if self.pack > 1:
            te = self._heldout_resident()
            for users in self._eval_packs(idxlist):
                rows = torch.from_numpy(np.asarray(users, dtype=np.int32)).to("cuda")
                yield SvaeEvalPack([self.dict_data_tr[u][:-1] for u in users], users), RowBatch(te, None, rows)
            return
        for user in idxlist:
            rows = self._target_rows(user)
            x = torch.LongTensor([self.dict_data_tr[user][:-1]])
            if self.sparse:
                yield x, SvaeTarget(rows)
                continue
            y = torch.zeros(1, len(rows), self.num_items)
            for t, r in enumerate(rows):
                y[0, t, r] = 1.
            yield x, y


class BprTripleSampler(Sampler):
    r"""The sampled ``(user, positive, negative)`` triples of pairwise-ranking matrix factorisation (Bayesian Personalised Ranking,
    Rendle et al., UAI 2009): the package's first negative sampler.  (The reference has none; ``include/rectorch_hip.h`` holds the
    definition, "BPR triples".)

    An epoch is ``nnz`` samples.  Every sample draws a stored entry ``(u, i)`` of the matrix uniformly and, as its negative ``j``,
    the first of seven candidate items that row ``u`` does not store; when all seven are stored the sample is skipped, ``j = -1``.
    The draws are Philox integers, a pure function of ``(seed, epoch, sample)``: two samplers of one matrix and seed give the same
    triples in any batching, and epoch ``e`` does not depend on the epochs before it.  They are drawn on the host by
    ``rtx_bpr_draw_host`` (plain C++, no device needed); a row without entries is never drawn.

    * ``sparse_data`` -- scipy sparse matrix, users x items; only its pattern is read (a sorted, duplicate-free copy is kept).
    * ``batch_size`` -- samples per batch (the last batch of an epoch may be shorter); default 4096.
    * ``seed`` -- an integer in ``[0, 2^64)``; default 98765.

    Iterating yields the batches of epoch ``self.epoch`` as triples ``(u, i, j)`` of int32 :class:`numpy.ndarray` and then
    advances ``self.epoch``; :meth:`draw` gives any window of any epoch.
    """
    def __init__(self, sparse_data, batch_size=4096, seed=98765):
        super(BprTripleSampler, self).__init__()
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or int(batch_size) < 1:
            raise ValueError("BprTripleSampler: batch_size = %r is not supported; supported: an integer >= 1" % (batch_size,))
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError("BprTripleSampler: seed = %r is not supported; supported: an integer in [0, 2^64)" % (seed,))
        m = csr_matrix(sparse_data, copy=True)
        m.sum_duplicates()
        m.sort_indices()
        if m.nnz == 0:
            raise ValueError("BprTripleSampler: the matrix holds no entries; supported: at least one stored entry to sample")
        if m.nnz >= 2 ** 31 or m.shape[0] >= 2 ** 31 or m.shape[1] >= 2 ** 31:
            raise ValueError("BprTripleSampler: a matrix of shape %s with %d entries is not supported; supported: all three below 2^31"
                             % (m.shape, m.nnz))
        self.shape = m.shape
        self.nnz = int(m.nnz)
        self.batch_size = int(batch_size)
        self.seed = int(seed)
        self.epoch = 0
        self._indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
        self._indices = np.ascontiguousarray(m.indices, dtype=np.int32)
        import ctypes as C
        from ._lib import check, lib
        check(lib().rtx_bpr_check_rows_host(self._indptr.ctypes.data_as(C.c_void_p), self._indices.ctypes.data_as(C.c_void_p), self.shape[0],
                                            self.shape[1]))        # once: every draw relies on it

    def __len__(self):
        return (self.nnz + self.batch_size - 1) // self.batch_size

    def draw(self, epoch, lo=0, count=None):
        """``(u, i, j)``, int32 arrays: the samples ``lo .. lo + count - 1`` (default: to the epoch's end) of epoch ``epoch``."""
        import ctypes as C
        from ._lib import check, lib
        count = self.nnz - int(lo) if count is None else int(count)
        out = [np.empty(max(count, 0), dtype=np.int32) for _ in range(3)]
        check(lib().rtx_bpr_draw_host(self._indptr.ctypes.data_as(C.c_void_p), self._indices.ctypes.data_as(C.c_void_p), self.shape[0],
                                      self.shape[1], C.c_uint64(self.seed), int(epoch), int(lo), count,
                                      *[t.ctypes.data_as(C.c_void_p) for t in out]))
        return tuple(out)

    def __iter__(self):
        epoch = self.epoch
        self.epoch += 1
        for lo in range(0, self.nnz, self.batch_size):
            yield self.draw(epoch, lo, min(self.batch_size, self.nnz - lo))
