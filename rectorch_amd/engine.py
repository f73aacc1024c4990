"""Python handles over the C ABI: device-resident CSR matrices and the Mult-VAE/DAE engine.

PyTorch is plumbing here (device memory, streams): tensors are passed to librectorch_hip as raw device
pointers on torch's current HIP stream.  No arithmetic of the path is done by torch.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import Batch, Step, check, lib, stream_ptr


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class CsrMatrix:
    """A scipy CSR matrix uploaded once to HBM (indptr int64, indices int32, values float32 or
    implicit ones).  Replaces the per-batch ``sparse[idx].toarray()`` of the reference's DataSampler
    (rectorch/samplers.py:99-105)."""

    def __init__(self, sparse):
        _lib.require_gpu()
        m = sparse.tocsr().copy()
        m.sum_duplicates()
        m.sort_indices()          # the device metrics binary-search the held-out rows
        self.shape = m.shape
        self.nnz = int(m.nnz)
        indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(m.indices, dtype=np.int32)
        data = np.asarray(m.data)
        self.binary = bool(np.all(data == 1))
        values = None if self.binary else np.ascontiguousarray(data, dtype=np.float32)
        h = C.c_void_p()
        check(lib().rtx_csr_upload(indptr.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p),
                                   None if values is None else values.ctypes.data_as(C.c_void_p),
                                   C.c_int64(m.shape[0]), C.c_int32(m.shape[1]), C.byref(h)))
        self.handle = h

    @property
    def op_handle(self):
        """integer handle for the ``torch.ops.rectorch_hip`` custom ops (rectorch_amd/ops.py)"""
        from . import ops
        return ops.register_handle(self)

    def gather_dense(self, row_ids, out=None):
        """float32 [len(row_ids), n_cols] device tensor holding the given rows (K1 in dense form)."""
        n = int(row_ids.numel())
        if out is None:
            out = torch.empty((n, self.shape[1]), dtype=torch.float32, device=row_ids.device)
        if n:
            check(lib().rtx_csr_gather_dense(self.handle, _ptr(row_ids), n, _ptr(out), stream_ptr()))
        return out

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                lib().rtx_csr_destroy(h)
            except Exception:
                pass
            self.handle = None


COND_SLOTS = 4     # slots of a CondBuilder's ring (csrc/cond_rows.hip: three can have readers a build is not ordered behind)


class SlotCsr:
    """One matrix of a :class:`CondBuilder` slot as the consumers of :class:`CsrMatrix` see it (``.handle``, ``.shape``,
    ``.binary``, ``gather_dense``).  A light view: the handle belongs to the builder and is never destroyed from here.  It
    remembers the slot's generation: once the ring has come round and the slot holds another batch, ``.handle`` raises instead
    of handing out the wrong rows."""
    __slots__ = ("_handle", "shape", "binary", "_ring", "_slot", "_gen")

    def __init__(self, handle, shape, binary, ring, slot, gen):
        self._handle, self.shape, self.binary = handle, shape, binary
        self._ring, self._slot, self._gen = ring, slot, gen

    @property
    def handle(self):
        if self._ring._gens[self._slot] != self._gen:
            raise _lib.RtxError("batch overwritten: a resident conditioned sampler keeps only the last S-1 batches (S = %d slots; "
                                "batch %d of slot %d was replaced by batch %d) -- consume the batches as they are yielded"
                                % (len(self._ring._gens), self._gen, self._slot, self._ring._gens[self._slot]))
        return self._handle

    gather_dense = CsrMatrix.gather_dense


class CondBuilder:
    """One ``rtx_cond``: the conditioned batches of :class:`rectorch_amd.models.CMultiVAE` built on the device
    (csrc/cond_rows.hip) from the resident ``tr`` / ``te`` matrices, the item -> condition bitmap and the example table
    ``(row, condition)``; ``bitmap``: ``(bits uint32 [n_items, W], any uint32 [ceil(n_items / 32)])`` or None (no filter).

    ``in_len`` / ``target_len`` (host int32 ``[n_ex]``): every example's input and filtered target length, counted once by the
    device; an example with ``target_len == 0`` is one the samplers drop.  :meth:`build` writes the next slot of the ring."""

    def __init__(self, tr, te, n_cond, bitmap, ex_rows, ex_conds, max_batch, n_slots=COND_SLOTS):
        _lib.require_gpu()
        self.tr, self.te = tr, tr if te is None else te        # (kept alive: the C object only references them)
        self.n_cond, self.max_batch, self.n_slots = int(n_cond), int(max_batch), int(n_slots)
        ex_rows = np.ascontiguousarray(ex_rows, dtype=np.int32)
        ex_conds = np.ascontiguousarray(ex_conds, dtype=np.int32)
        assert ex_rows.shape == ex_conds.shape and ex_rows.ndim == 1
        self.n_ex = len(ex_rows)
        bits = any_ = None
        if bitmap is not None:
            bits = np.ascontiguousarray(bitmap[0], dtype=np.uint32)
            any_ = np.ascontiguousarray(bitmap[1], dtype=np.uint32)
            n_items, W = self.tr.shape[1], (self.n_cond + 31) // 32
            if bits.shape != (n_items, W) or any_.shape != ((n_items + 31) // 32,):
                raise _lib.RtxError("condition bitmap must be [%d, %d] + [%d] words, got %s + %s"
                                    % (n_items, W, (n_items + 31) // 32, bits.shape, any_.shape))
        h = C.c_void_p()
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(lib().rtx_cond_create(self.tr.handle, self.te.handle, self.n_cond, vp(bits), vp(any_), vp(ex_rows), vp(ex_conds),
                                    C.c_int64(self.n_ex), self.max_batch, self.n_slots, C.byref(h)))
        self.handle = h
        self.in_len = np.zeros(self.n_ex, dtype=np.int32)
        self.target_len = np.zeros(self.n_ex, dtype=np.int32)
        check(lib().rtx_cond_lengths(h, vp(self.in_len), vp(self.target_len)))
        self._slots = []
        for s in range(self.n_slots):
            a, t = C.c_void_p(), C.c_void_p()
            check(lib().rtx_cond_slot(h, s, C.byref(a), C.byref(t)))
            self._slots.append((a, t))
        self._gens = [0] * self.n_slots      # the batch number (1-based count of builds) each slot holds
        self._built = 0

    def build(self, ex_ids, batch, nnz_in=-1, nnz_target=-1):
        """enqueue the build of the ring's next slot from the device int32 example ids ``ex_ids[:batch]`` on the current stream;
        returns ``(input, target)`` as :class:`SlotCsr` views of ``batch`` rows"""
        batch = int(batch)
        slot = self._built % self.n_slots
        check(lib().rtx_cond_build(self.handle, slot, _ptr(ex_ids), batch, C.c_int64(int(nnz_in)), C.c_int64(int(nnz_target)), stream_ptr()))
        self._built += 1
        self._gens[slot] = self._built
        a, t = self._slots[slot]
        return (SlotCsr(a, (batch, self.tr.shape[1] + self.n_cond), self.tr.binary, self, slot, self._built),
                SlotCsr(t, (batch, self.te.shape[1]), self.te.binary, self, slot, self._built))

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                lib().rtx_cond_destroy(h)
            except Exception:
                pass
            self.handle = None


class RowBatch:
    """What the resident DataSampler hands to the trainer on the fast path: row numbers only."""
    __slots__ = ("tr", "te", "rows", "global_len", "users")

    def __init__(self, tr, te, rows, global_len=None, users=None):
        self.tr, self.te, self.rows = tr, te, rows
        # the rows' user ids for a CDAE_net (device int32, parallel to rows; -1: no user vector), or None (DataSampler(user_ids=...))
        self.users = users
        # data parallel: users in the GLOBAL batch this one is a rank's slice of (rectorch_amd.parallel.shard_batch): the step's
        # 1 / global-batch scale then needs no collective and no host sync
        self.global_len = global_len

    def __len__(self):
        return int(self.rows.numel())


def tag_rows(t, rb):
    """Mark the dense tensor ``t`` as the image of the resident rows ``rb`` (what the device DataSampler yields).  The tag
    carries the tensor's version counter: once the caller edits ``t`` in place (``x.clamp_``, ``x[:, cold] = 0`` ...)
    the tag is stale and the tensor's CONTENTS are used, as the reference would (rectorch/models.py:819-822)."""
    t._rtx_rows = rb
    t._rtx_ver = t._version
    return t


def tagged_rows(t):
    """The RowBatch ``t`` was gathered from, or None when ``t`` is not tagged or was modified since."""
    rb = getattr(t, "_rtx_rows", None)
    if rb is not None and getattr(t, "_rtx_ver", None) == t._version:
        return rb
    return None


def batch_users(x, users=None):
    """The user ids that come with the batch ``x`` (for a CDAE_net): ``users`` when given, else ``RowBatch.users``, the ids in the tag
    of a dense tensor a device DataSampler yielded, or the ``_rtx_users`` attribute of a CPU sampler's tensor; None when there are none."""
    if users is not None:
        return users
    rb = x if isinstance(x, RowBatch) else tagged_rows(x)
    if rb is not None:
        return rb.users
    return getattr(x, "_rtx_users", None)


def _check_width(t, n_items, what):
    if n_items is not None and (t.dim() != 2 or t.shape[1] != n_items):
        raise _lib.RtxError("%s must be [batch, %d] (n_items of the network), got %s" % (what, n_items, tuple(t.shape)))


def make_batch(x, target=None, keep=None, n_items=None, n_in=None):
    """Build the C ``rtx_batch`` for ``x`` (a RowBatch, or a dense [B, n_items] device tensor, or a dense
    tensor carrying the RowBatch it was gathered from).  ``keep`` collects tensors that must outlive the call."""
    b = Batch()
    rb = x if isinstance(x, RowBatch) else tagged_rows(x)
    if rb is not None:
        b.csr = rb.tr.handle
        b.row_ids = rb.rows.data_ptr()
        b.batch = len(rb)
        if target is None and rb.te is not None and isinstance(x, RowBatch) and x.te is not None:
            b.target_csr = rb.te.handle
    else:
        _check_width(x, n_in if n_in is not None else n_items, "the input batch")
        x = x.to(torch.float32).contiguous()
        if keep is not None:
            keep.append(x)
        b.x_dense = x.data_ptr()
        b.batch = x.shape[0]
    if target is not None:
        trb = None if isinstance(target, RowBatch) else tagged_rows(target)
        if isinstance(target, RowBatch) and rb is not None and target.rows is rb.rows:
            b.target_csr = target.tr.handle      # the (input rows, target rows) pair of a sparse sampler
        elif trb is not None and rb is not None and trb.rows is rb.rows and trb.te is not None:
            b.target_csr = trb.te.handle
        else:
            if isinstance(target, RowBatch):
                target = target.tr.gather_dense(target.rows)
            _check_width(target, n_items, "the target batch")
            target = target.to(torch.float32).contiguous()
            if keep is not None:
                keep.append(target)
            if rb is not None:
                # input by rows, target dense: densify the input as well (mixed forms are not in the ABI)
                xin = rb.tr.gather_dense(rb.rows)
                if keep is not None:
                    keep.append(xin)
                b.csr = None
                b.row_ids = None
                b.x_dense = xin.data_ptr()
            b.target_dense = target.data_ptr()
    return b


class Engine:
    """One ``rtx_engine``: a network's compute state at one numerics mode, bound to the network's float32
    master parameters (the nn.Parameters themselves) and, for training, to gradient buffers and the Adam
    moments held in ``torch.optim.Adam``'s state."""

    def __init__(self, enc_dims, dec_dims, variant, dropout, numerics="bf16", max_batch=512, splitk=0, cond_dim=0):
        _lib.require_gpu()
        self.enc_dims, self.dec_dims = [int(d) for d in enc_dims], [int(d) for d in dec_dims]
        self.variant, self.numerics = variant, numerics
        self.max_batch = int(max_batch)
        self.n_items, self.latent = self.enc_dims[0], self.enc_dims[-1]
        self.cond_dim = int(cond_dim)
        self.n_in = self.n_items + self.cond_dim      # input columns: items, then the condition one-hot (CMultiVAE)
        cfg = _lib.make_cfg(self.enc_dims, self.dec_dims, variant, numerics, dropout, max_batch, splitk, cond_dim)
        h = C.c_void_p()
        check(lib().rtx_engine_create(C.byref(cfg), C.byref(h)))
        self.handle = h
        self.n_tensors = lib().rtx_engine_n_tensors(h)
        self._bound = None
        self._keep = []
        # measurement / debugging: RTX_ENGINE_OPTS="hop_values=0,prefetch=0" sets engine options (rtx_engine_set_option) on
        # every engine this process creates -- A/B runs of whole test files without touching them
        for kv in filter(None, os.environ.get("RTX_ENGINE_OPTS", "").split(",")):
            k, v = kv.split("=")
            check(lib().rtx_engine_set_option(h, k.strip().encode(), int(v)))

    @property
    def op_handle(self):
        """integer handle for the ``torch.ops.rectorch_hip`` custom ops (rectorch_amd/ops.py)"""
        from . import ops
        return ops.register_handle(self)

    # ---- binding --------------------------------------------------------------------------------
    def bind(self, params, grads=None, exp_avg=None, exp_avg_sq=None):
        n = self.n_tensors
        assert len(params) == n, "expected %d parameter tensors, got %d" % (n, len(params))
        rows, cols = C.c_int32(), C.c_int32()
        for t, p in enumerate(params):
            check(lib().rtx_engine_tensor_shape(self.handle, t, C.byref(rows), C.byref(cols)))
            want = (rows.value, cols.value) if p.dim() == 2 else (rows.value,)
            if tuple(p.shape) != want or p.dtype != torch.float32 or not p.is_contiguous() or not p.is_cuda:
                raise _lib.RtxError("parameter %d must be a contiguous float32 HIP tensor of shape %s, got %s %s on %s"
                                    % (t, want, tuple(p.shape), p.dtype, p.device))
        arr_t = C.c_void_p * n

        def arr(ts):
            return None if ts is None else arr_t(*[t.data_ptr() for t in ts])
        check(lib().rtx_engine_bind(self.handle, arr(params), arr(grads), arr(exp_avg), arr(exp_avg_sq)))
        self._bound = (list(params), grads, exp_avg, exp_avg_sq)   # keep the tensors alive

    def sync_shadows(self):
        check(lib().rtx_engine_sync_shadows(self.handle, stream_ptr()))

    # ---- CDAE's user node -------------------------------------------------------------------------
    def bind_users(self, V, exp_avg=None, exp_avg_sq=None):
        """``rtx_engine_bind_users``: the user table float32 ``[n_users, latent]`` and, for training, SparseAdam's two moments of the
        same shape (None unbinds).  Re-binds only when a tensor's storage changed."""
        if V is None:
            if getattr(self, "_users_key", None) is not None:
                check(lib().rtx_engine_bind_users(self.handle, None, None, None, 0))
            self._users_key = self._users_keep = None
            return
        for t in (V, exp_avg, exp_avg_sq):
            if t is not None and (tuple(t.shape) != (V.shape[0], self.latent) or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
                raise _lib.RtxError("the user table and its moments must be contiguous float32 HIP tensors of shape [n_users, %d], got %s %s on %s"
                                    % (self.latent, tuple(t.shape), t.dtype, t.device))
        key = tuple(None if t is None else t.data_ptr() for t in (V, exp_avg, exp_avg_sq)) + (V.shape[0],)
        if getattr(self, "_users_key", None) != key:
            check(lib().rtx_engine_bind_users(self.handle, _ptr(V), _ptr(exp_avg), _ptr(exp_avg_sq), int(V.shape[0])))
            self._users_key, self._users_keep = key, (V, exp_avg, exp_avg_sq)

    def set_users(self, users, batch=None, lr=0.0, beta1=0.0, beta2=0.0, eps=0.0, step=0):
        """``rtx_engine_set_users``: the user ids (int tensor, one per batch row; None: no user term) of the NEXT forward, encode or
        training call, with SparseAdam's scalars for a training call"""
        if users is None:
            if getattr(self, "_users_key", None) is not None:
                check(lib().rtx_engine_set_users(self.handle, None, 0.0, 0.0, 0.0, 0.0, 0))
            self._users_ids = None
            return
        dev = torch.device("cuda", torch.cuda.current_device())
        users = torch.as_tensor(users).to(device=dev, dtype=torch.int32).contiguous()
        if users.dim() != 1 or (batch is not None and users.numel() != batch):
            raise _lib.RtxError("users must hold one id per batch row (%s), got shape %s" % (batch, tuple(users.shape)))
        self._users_ids = users          # alive until the call that consumes them has been enqueued (stream-ordered afterwards)
        check(lib().rtx_engine_set_users(self.handle, _ptr(users), float(lr), float(beta1), float(beta2), float(eps), int(step)))

    # ---- forward family ---------------------------------------------------------------------------
    def _step(self, seed=0, offset=0, mask=None, noise=None, **kw):
        s = Step()
        s.seed, s.offset = int(seed) & (2 ** 64 - 1), int(offset)
        s.dropout_mask = None if mask is None else mask.data_ptr()
        s.eps_noise = None if noise is None else noise.data_ptr()
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def forward(self, x, training=False, remove_train=False, seed=0, offset=0, mask=None, noise=None, out=None, want_latent=True):
        """``out``: a float32 ``[>= batch, n_items]`` tensor to receive the scores (a loop over many batches reuses two of them instead
        of allocating 40 MB per batch); ``want_latent=False`` skips the (mu, logvar) outputs of a VAE."""
        keep = []
        b = make_batch(x, keep=keep, n_items=self.n_items, n_in=self.n_in)
        dev = torch.device("cuda", torch.cuda.current_device())
        if out is not None:
            assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] >= b.batch and out.shape[1] == self.n_items
            logits = out[:b.batch]
        else:
            logits = torch.empty((b.batch, self.n_items), dtype=torch.float32, device=dev)
        mu = logvar = None
        if self.variant in ("vae", "gvae") and want_latent:
            mu = torch.empty((b.batch, self.latent), dtype=torch.float32, device=dev)
            logvar = torch.empty_like(mu)
        st = self._step(seed, offset, mask, noise)
        check(lib().rtx_engine_forward(self.handle, C.byref(b), int(training), C.byref(st), int(remove_train),
                                       _ptr(logits), _ptr(mu), _ptr(logvar), stream_ptr()))
        return logits, mu, logvar

    def evaluate_topk(self, tr, te, rows, offsets, ks, scratch=None, rank_metrics=False):
        """``rtx_engine_evaluate_topk``: every batch ``rows[offsets[i]:offsets[i + 1]]`` (device int32 row numbers into the resident
        :class:`CsrMatrix` pair ``tr`` / ``te``) scored in eval mode with the train items at -inf and reduced to nDCG@k / Recall@k, all
        enqueued by ONE call.  Returns float64 device tensors ``(ndcg, recall)`` of shape ``[len(ks), len(rows)]``; with
        ``rank_metrics=True`` (``rtx_engine_evaluate_topk_ex``) ``(ndcg, recall, hit, mrr)``, hit as 1.0 / 0.0."""
        offs = (C.c_int64 * len(offsets))(*[int(o) for o in offsets])
        ks = [int(k) for k in ks]
        arr = (C.c_int32 * len(ks))(*ks)
        total = int(offsets[-1] - offsets[0])
        bmax = max(int(b) - int(a) for a, b in zip(offsets[:-1], offsets[1:])) if len(offsets) > 1 else 0
        dev = rows.device
        if scratch is None or scratch.shape[0] < bmax:
            scratch = torch.empty((max(bmax, 1), self.n_items), dtype=torch.float32, device=dev)
        ndcg = torch.empty((len(ks), total), dtype=torch.float64, device=dev)
        recall = torch.empty_like(ndcg)
        if rank_metrics:
            hit, mrr = torch.empty_like(ndcg), torch.empty_like(ndcg)
            check(lib().rtx_engine_evaluate_topk_ex(self.handle, tr.handle, te.handle, _ptr(rows), offs, len(offsets) - 1, arr, len(ks),
                                                    _ptr(scratch), _ptr(ndcg), _ptr(recall), _ptr(hit), _ptr(mrr), stream_ptr()))
            return ndcg, recall, hit, mrr
        check(lib().rtx_engine_evaluate_topk(self.handle, tr.handle, te.handle, _ptr(rows), offs, len(offsets) - 1, arr, len(ks),
                                             _ptr(scratch), _ptr(ndcg), _ptr(recall), stream_ptr()))
        return ndcg, recall

    def recommend(self, tr, rows, offsets, k, remove_train=True, scratch=None):
        """``rtx_engine_recommend``: every batch ``rows[offsets[i]:offsets[i + 1]]`` (device int32 row numbers into the resident
        :class:`CsrMatrix` ``tr``) scored in eval mode and reduced to its ``K = min(k, n_items)`` best items (``k <= 1024``), the users'
        own items of ``tr`` excluded with ``remove_train``; all enqueued by ONE call.  Returns device tensors ``(items int32
        [len(rows), K], scores float32 [len(rows), K])``, user j of ``rows`` in row j: score descending, item id ascending among
        equal scores."""
        offs = (C.c_int64 * len(offsets))(*[int(o) for o in offsets])
        total = int(offsets[-1] - offsets[0])
        bmax = max(int(b) - int(a) for a, b in zip(offsets[:-1], offsets[1:])) if len(offsets) > 1 else 0
        dev = rows.device
        if scratch is None or scratch.shape[0] < bmax:
            scratch = torch.empty((max(bmax, 1), self.n_items), dtype=torch.float32, device=dev)
        kk = max(min(int(k), self.n_items), 0)
        items = torch.empty((total, kk), dtype=torch.int32, device=dev)
        scores = torch.empty((total, kk), dtype=torch.float32, device=dev)
        check(lib().rtx_engine_recommend(self.handle, tr.handle, _ptr(rows), offs, len(offsets) - 1, int(k), int(bool(remove_train)),
                                         _ptr(scratch), _ptr(items), _ptr(scores), stream_ptr()))
        return items, scores

    def encode(self, x, training=False, seed=0, offset=0, mask=None):
        keep = []
        b = make_batch(x, keep=keep, n_items=self.n_items, n_in=self.n_in)
        dev = torch.device("cuda", torch.cuda.current_device())
        o0 = torch.empty((b.batch, self.latent), dtype=torch.float32, device=dev)
        o1 = torch.empty_like(o0) if self.variant in ("vae", "gvae") else None
        st = self._step(seed, offset, mask, None)
        check(lib().rtx_engine_encode(self.handle, C.byref(b), int(training), C.byref(st), _ptr(o0), _ptr(o1), stream_ptr()))
        return o0, o1

    def decode(self, z):
        _check_width(z, self.latent, "z")
        z = z.contiguous().float()
        logits = torch.empty((z.shape[0], self.n_items), dtype=torch.float32, device=z.device)
        check(lib().rtx_engine_decode(self.handle, _ptr(z), z.shape[0], _ptr(logits), stream_ptr()))
        return logits

    # ---- training ---------------------------------------------------------------------------------
    def loss_grads(self, x, target, step, loss_out, loss_accum=None, layer_cb=None):
        keep = []
        b = make_batch(x, target, keep=keep, n_items=self.n_items, n_in=self.n_in)
        cb = _lib.LAYER_CB(layer_cb) if layer_cb is not None else _lib.LAYER_CB()
        check(lib().rtx_engine_loss_grads(self.handle, C.byref(b), C.byref(step), _ptr(loss_out), _ptr(loss_accum),
                                          cb, None, stream_ptr()))

    def forward_train(self, x, step):
        """``rtx_engine_forward_train``: the training-mode forward of the fused step (the draws of ``step``) that keeps its
        activations in the engine.  Returns ``(out, mu, logvar, ticket, batch, keep)``: the public outputs (``mu`` / ``logvar`` None
        for the DAE variants), the ticket :meth:`backward` wants back, and the C batch with the tensors that keep it alive."""
        keep = []
        b = make_batch(x, keep=keep, n_items=self.n_items, n_in=self.n_in)
        dev = torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((b.batch, self.n_items), dtype=torch.float32, device=dev)
        mu = logvar = None
        if self.variant in ("vae", "gvae"):
            mu = torch.empty((b.batch, self.latent), dtype=torch.float32, device=dev)
            logvar = torch.empty_like(mu)
        ticket = C.c_uint64()
        check(lib().rtx_engine_forward_train(self.handle, C.byref(b), C.byref(step), _ptr(out), _ptr(mu), _ptr(logvar),
                                             C.byref(ticket), stream_ptr()))
        return out, mu, logvar, ticket.value, b, keep

    def backward(self, batch, step, ticket, d_out, d_mu=None, d_logvar=None):
        """``rtx_engine_backward``: the backward chain from the caller's ``d loss / d out`` (float32 ``[batch, n_items]``, unit
        column stride) and, for the VAE variants, ``d loss / d mu`` / ``d loss / d logvar`` into the bound gradient buffers.
        A stale ticket raises :class:`RtxError` before anything is enqueued."""
        if d_out.dtype != torch.float32 or d_out.dim() != 2 or d_out.stride(1) != 1 or d_out.shape != (batch.batch, self.n_items):
            d_out = d_out.to(torch.float32).expand(batch.batch, self.n_items).contiguous()
        ld = d_out.stride(0) if batch.batch > 1 else self.n_items
        if ld < self.n_items:           # (an expanded row: stride 0)
            d_out = d_out.contiguous()
            ld = self.n_items
        if d_mu is not None:
            d_mu, d_logvar = d_mu.to(torch.float32).contiguous(), d_logvar.to(torch.float32).contiguous()
        check(lib().rtx_engine_backward(self.handle, C.byref(batch), C.byref(step), C.c_uint64(ticket), _ptr(d_out), C.c_int64(ld),
                                        _ptr(d_mu), _ptr(d_logvar), _lib.LAYER_CB(), None, stream_ptr()))

    # ---- the same route cut in two at z ------------------------------------------------------------
    def encode_train(self, x, step):
        """``rtx_engine_encode_train``: the encoder half of the training forward (dropout from ``step``), activations kept in the
        engine.  Returns ``(out0, out1, ticket, batch, keep)``: ``(mu, logvar)`` of the VAE variants or ``(h, None)``, the ticket
        :meth:`encode_backward` wants back, and the C batch with the tensors that keep it alive."""
        keep = []
        b = make_batch(x, keep=keep, n_items=self.n_items, n_in=self.n_in)
        dev = torch.device("cuda", torch.cuda.current_device())
        o0 = torch.empty((b.batch, self.latent), dtype=torch.float32, device=dev)
        o1 = torch.empty_like(o0) if self.variant in ("vae", "gvae") else None
        ticket = C.c_uint64()
        check(lib().rtx_engine_encode_train(self.handle, C.byref(b), C.byref(step), _ptr(o0), _ptr(o1), C.byref(ticket), stream_ptr()))
        return o0, o1, ticket.value, b, keep

    def encode_backward(self, batch, step, ticket, d_out0, d_out1=None):
        """``rtx_engine_encode_backward``: the encoder layers' gradients into the bound buffers from ``d loss / d mu`` and
        ``d loss / d logvar`` (VAE variants) or ``d loss / d h``, float32 ``[batch, latent]``.  A stale ticket raises
        :class:`RtxError` before anything is enqueued."""
        d_out0 = d_out0.to(torch.float32).expand(batch.batch, self.latent).contiguous()
        if d_out1 is not None:
            d_out1 = d_out1.to(torch.float32).expand(batch.batch, self.latent).contiguous()
        check(lib().rtx_engine_encode_backward(self.handle, C.byref(batch), C.byref(step), C.c_uint64(ticket), _ptr(d_out0), _ptr(d_out1),
                                               _lib.LAYER_CB(), None, stream_ptr()))

    def decode_train(self, z):
        """``rtx_engine_decode_train``: the decoder half of the training forward on ``z`` float32 ``[n, latent]``, ``n`` any batch
        up to ``max_batch``.  Returns ``(out, ticket)``."""
        _check_width(z, self.latent, "z")
        z = z.detach().to(torch.float32).contiguous()
        out = torch.empty((z.shape[0], self.n_items), dtype=torch.float32, device=z.device)
        ticket = C.c_uint64()
        check(lib().rtx_engine_decode_train(self.handle, _ptr(z), z.shape[0], _ptr(out), C.byref(ticket), stream_ptr()))
        return out, ticket.value

    def decode_backward(self, n, ticket, d_out, want_dz=True):
        """``rtx_engine_decode_backward``: the decoder layers' gradients into the bound buffers from ``d loss / d out`` (float32
        ``[n, n_items]``); returns ``d loss / d z`` float32 ``[n, latent]`` (None without ``want_dz``: its product is skipped)."""
        if d_out.dtype != torch.float32 or d_out.dim() != 2 or d_out.stride(1) != 1 or d_out.shape != (n, self.n_items):
            d_out = d_out.to(torch.float32).expand(n, self.n_items).contiguous()
        ld = d_out.stride(0) if n > 1 else self.n_items
        if ld < self.n_items:           # (an expanded row: stride 0)
            d_out = d_out.contiguous()
            ld = self.n_items
        d_z = torch.empty((n, self.latent), dtype=torch.float32, device=d_out.device) if want_dz else None
        step = Step()
        check(lib().rtx_engine_decode_backward(self.handle, int(n), C.byref(step), C.c_uint64(ticket), _ptr(d_out), C.c_int64(ld),
                                               _ptr(d_z), _lib.LAYER_CB(), None, stream_ptr()))
        return d_z

    def bind_grads16(self, ptrs):
        """device addresses of the bf16 gradient images, one per tensor (None unbinds): steps flagged RTX_STEP_GRADS_BF16 write
        their gradients there instead of into the float32 buffers"""
        if ptrs is None:
            check(lib().rtx_engine_bind_grads16(self.handle, None))
            self._g16_key = None
            return
        key = tuple(int(p) for p in ptrs)
        if getattr(self, "_g16_key", None) != key:
            check(lib().rtx_engine_bind_grads16(self.handle, (C.c_void_p * len(key))(*key)))
            self._g16_key = key

    def apply_adam(self, step):
        check(lib().rtx_engine_apply_adam(self.handle, C.byref(step), stream_ptr()))

    def set_optimizer(self, kind, flags=0, momentum=0.0, dampening=0.0, alpha=0.0, lr_decay=0.0):
        """``rtx_engine_set_optimizer``: the update rule of every later optimizer launch of this engine (``_lib.RTX_OPTIM_*``)"""
        o = _lib.Optim(int(kind), int(flags), float(momentum), float(dampening), float(alpha), float(lr_decay))
        check(lib().rtx_engine_set_optimizer(self.handle, C.byref(o)))

    def set_grad_clip(self, mode, bound=0.0):
        """``rtx_engine_set_grad_clip``: gradient clipping in front of every later optimizer launch of this engine
        (``_lib.RTX_CLIP_*``); between any two steps"""
        check(lib().rtx_engine_set_grad_clip(self.handle, int(mode), float(bound)))

    def set_grad_accum(self, mode, scale=1.0):
        """``rtx_engine_set_grad_accum``: the weight-gradient products of the next backward passes weight their gradient into the
        bound gradient buffers (``_lib.RTX_ACCUM_FIRST``: ``scale * g``; ``RTX_ACCUM_ADD``: ``fma(scale, g, acc)``) instead of
        storing over them; the next optimizer launch sets the mode back to ``RTX_ACCUM_OFF``"""
        check(lib().rtx_engine_set_grad_accum(self.handle, int(mode), float(scale)))

    def wait_grad_norm(self, step_count, timeout_s=0.0):
        """``(total norm, coefficient)`` of the LAST optimizer step enqueued, whose step count is ``step_count``, from the host
        mailbox: the stream is not drained (``rtx_engine_wait_grad_norm``)"""
        out = (C.c_float * 2)()
        check(lib().rtx_engine_wait_grad_norm(self.handle, int(step_count), out, float(timeout_s)))
        return float(out[0]), float(out[1])

    def apply_adam_layers(self, step, layer_lo, layer_hi, grads_bf16=None):
        """Adam + shadow refresh of layers [layer_lo, layer_hi) on the CURRENT stream; ``grads_bf16``: list of device
        addresses (one per bound tensor) of the bf16 image of the reduced gradients, or None."""
        arr = None
        if grads_bf16 is not None:
            arr = (C.c_void_p * self.n_tensors)(*[C.c_void_p(int(a)) for a in grads_bf16])
        check(lib().rtx_engine_apply_adam_layers(self.handle, C.byref(step), int(layer_lo), int(layer_hi), arr, stream_ptr()))

    def apply_adam_rows(self, step, layer, row_lo, row_hi, with_bias=True, w_grad_bf16=None, b_grad_bf16=None):
        """sharded optimizer: Adam on rows [row_lo, row_hi) of layer ``layer``'s weight matrix (+ its replicated bias) on the
        CURRENT stream; ``*_grad_bf16``: device addresses of the bf16 images of the reduced gradients, or None."""
        check(lib().rtx_engine_apply_adam_rows(self.handle, C.byref(step), int(layer), int(row_lo), int(row_hi), int(bool(with_bias)),
                                               None if w_grad_bf16 is None else C.c_void_p(int(w_grad_bf16)),
                                               None if b_grad_bf16 is None else C.c_void_p(int(b_grad_bf16)), stream_ptr()))

    def shadow_tensor(self, layer):
        """the compute copy of layer ``layer``'s weight matrix as a torch tensor ALIASING the engine's buffer
        ([padded_rows, ld], bfloat16 or float32): what a sharded-optimizer step all-gathers in place."""
        base, rows, ld, eb = C.c_void_p(), C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().rtx_engine_shadow_region(self.handle, int(layer), C.byref(base), C.byref(rows), C.byref(ld), C.byref(eb)))

        class _Alias:     # __cuda_array_interface__ is honoured by PyTorch-ROCm as well
            pass
        al = _Alias()
        n = rows.value * ld.value
        al.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i2" if eb.value == 2 else "<f4", "data": (base.value, False), "version": 2}
        t = torch.as_tensor(al, device="cuda")
        if eb.value == 2:
            t = t.view(torch.bfloat16)
        return t.view(rows.value, ld.value)

    def train_step(self, x, target, step, loss_out, loss_accum=None):
        keep = []
        b = make_batch(x, target, keep=keep, n_items=self.n_items, n_in=self.n_in)
        check(lib().rtx_engine_train_step(self.handle, C.byref(b), C.byref(step), _ptr(loss_out), _ptr(loss_accum),
                                          stream_ptr()))

    def set_next_batch(self, x, target=None, seed=0, offset=0):
        """announce the batch (a :class:`RowBatch`) and the dropout seed of the training step AFTER the next ``train_step`` call:
        that call gathers it on the engine's side stream under its last weight kernel (``rtx_engine_set_next_batch``; a hint).
        Returns False (and announces nothing) for batches the engine cannot prefetch (dense tensors)."""
        if x is None:
            check(lib().rtx_engine_set_next_batch(self.handle, None, None))
            self._next_keep = None
            return False
        if not isinstance(x, RowBatch) or (target is not None and not isinstance(target, RowBatch)):
            return False
        b = make_batch(x, target, keep=None, n_items=self.n_items, n_in=self.n_in)
        if not b.csr or b.x_dense or b.target_dense:
            return False
        st = self._step(seed=seed, offset=offset)
        check(lib().rtx_engine_set_next_batch(self.handle, C.byref(b), C.byref(st)))
        self._next_keep = (x, target)         # the row ids stay alive (and unchanged) until that step has run
        return True

    def join(self):
        """resolve a join left open by a training step flagged ``RTX_STEP_DEFER_JOIN``: the current stream continues only after
        everything that step put on the engine's side stream (no-op when nothing is open)"""
        check(lib().rtx_engine_join(self.handle, stream_ptr()))

    def loss_mailbox(self, enable=True):
        """every training step also reports {loss, step count} to coherent host memory (``wait_loss``)"""
        check(lib().rtx_engine_loss_mailbox(self.handle, int(bool(enable))))
        self._mailbox = bool(enable)

    def wait_loss(self, step_count, timeout_s=0.0):
        """the loss of the training step whose Adam step count is ``step_count``: spins on the host mailbox, no stream drain
        (reference models.py:835 ``return loss.item()``)"""
        out = C.c_float()
        check(lib().rtx_engine_wait_loss(self.handle, int(step_count), C.byref(out), float(timeout_s)))
        return out.value

    # ---- data parallel, scheduled by the engine (rtx_engine_dp_attach / rtx_engine_train_step_dp) --------------------
    def dp_attach(self, plan):
        """``plan``: a :class:`rectorch_amd.parallel.NativePlan` (rank, world, sharded, comm dtype and ONE of an RCCL
        communicator, caller-supplied collectives, or emulation), or None to detach."""
        if plan is None:
            check(lib().rtx_engine_dp_attach(self.handle, None))
            old, self._dp_plan, self._dp_any_sharded = getattr(self, "_dp_plan", None), None, False
            if old is not None and hasattr(old, "_forget"):
                old._forget(self)
            return
        cfg = plan.c_cfg()            # (the sharding threshold travels in the cfg: nothing of an earlier plan stays in the engine)
        old = getattr(self, "_dp_plan", None)
        check(lib().rtx_engine_dp_attach(self.handle, C.byref(cfg)))     # (the C side releases an earlier attachment first)
        if old is not None and old is not plan and hasattr(old, "_forget"):
            old._forget(self)         # the old plan's close() must not detach this engine from its new plan
        self._dp_plan = plan          # keeps the communicator / callback objects alive as long as the engine uses them
        # what the ENGINE decided to shard (a plan that asks for the sharded optimizer on a network of small matrices shards nothing)
        self._dp_any_sharded = any(self.dp_owned_rows(l)[2] for l in range(self.n_tensors // 2))
        if hasattr(plan, "_remember"):
            plan._remember(self)

    def train_step_dp(self, x, target, step, loss_out, loss_accum=None):
        """one rank's train_batch of a data-parallel job: forward + loss + backward on this rank's users, the gradient exchange
        and the optimizer in ONE call (``step.inv_batch`` = 1 / global batch)"""
        keep = []
        b = make_batch(x, target, keep=keep, n_items=self.n_items, n_in=self.n_in)
        check(lib().rtx_engine_train_step_dp(self.handle, C.byref(b), C.byref(step), _ptr(loss_out), _ptr(loss_accum), stream_ptr()))

    def dp_owned_rows(self, layer):
        """(row_lo, row_hi, sharded) of layer ``layer``'s weight matrix: the rows whose float32 master and Adam moments this rank
        keeps current under the sharded optimizer"""
        lo, hi, sh = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().rtx_engine_dp_owned_rows(self.handle, int(layer), C.byref(lo), C.byref(hi), C.byref(sh)))
        return lo.value, hi.value, bool(sh.value)

    # ---- instrumentation --------------------------------------------------------------------------
    def set_option(self, key, value):
        """measurement knobs of the engine ("fuse_adam", "two_stream", "lse_fuse", "dw_cfg", "splitk", ...; include/rectorch_hip.h)"""
        check(lib().rtx_engine_set_option(self.handle, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int32()
        check(lib().rtx_engine_get_option(self.handle, key.encode(), C.byref(v)))
        return v.value

    def set_timing(self, site=None, enable=True):
        check(lib().rtx_engine_set_timing(self.handle, None if site is None else site.encode(), int(enable)))

    def get_timings(self):
        cap = 64
        names = (C.c_char * 48 * cap)()
        ms = (C.c_float * cap)()
        cnt = (C.c_int32 * cap)()
        n = C.c_int32()
        check(lib().rtx_engine_get_timings(self.handle, cap, names, ms, cnt, C.byref(n)))
        return {names[i].value.decode(): (float(ms[i]), int(cnt[i])) for i in range(n.value)}

    def step_cost(self, batch):
        b, f = C.c_double(), C.c_double()
        check(lib().rtx_engine_step_cost(self.handle, int(batch), C.byref(b), C.byref(f)))
        return b.value, f.value

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                lib().rtx_engine_destroy(h)
            except Exception:
                pass
            self.handle = None


def _loss_operands(a, b, mu=None, logvar=None):
    """what every dense loss below starts from: its tensors on the current device as contiguous float32 (without ``mu`` there is no
    KL term and ``logvar`` is dropped), and a 0-dim float32 tensor there for the result"""
    _lib.require_gpu()
    if mu is None:
        logvar = None
    elif logvar is None:
        raise _lib.RtxError("loss: mu was given without logvar")
    dev = torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((), dtype=torch.float32, device=dev)
    return [None if t is None else t.to(dev, torch.float32).contiguous() for t in (a, b, mu, logvar)] + [out]


def _wants_grad(targets, *operands):
    """True when a dense loss has to carry a ``grad_fn``: grad mode is on and one of ``operands`` requires grad.  ``targets``
    (name -> tensor) are constants of every loss here: one that requires grad is refused by name."""
    if not torch.is_grad_enabled():
        return False
    for name, t in targets.items():
        if t is not None and t.requires_grad:
            raise ValueError("%s requires grad: the loss has no gradient with respect to its target -- pass %s.detach()" % (name, name))
    return any(t is not None and t.requires_grad for t in operands)


def _times(grad, g, needed):
    """one saved gradient (at unit upstream gradient) times the upstream ``g``: one device op, no host read of ``g``"""
    return grad * g if needed else None


def _kl_loss_forward(ctx, entry, recon, x, mu, logvar, *scalars):
    """the forward of the two losses with a KL term: ONE call of ``entry`` (``rtx_multinomial_loss_grad(..., beta, ...)`` /
    ``rtx_bce_kl_loss_grad``) writes the value and the gradients at unit upstream gradient, which are saved for backward"""
    out = torch.empty((), dtype=torch.float32, device=recon.device)
    grads = [torch.empty_like(recon)] + ([] if mu is None else [torch.empty_like(mu), torch.empty_like(logvar)])
    d_mu, d_logvar = (None, None) if mu is None else (_ptr(grads[1]), _ptr(grads[2]))
    check(entry(_ptr(recon), _ptr(x), recon.shape[0], recon.shape[1], _ptr(mu), _ptr(logvar), 0 if mu is None else mu.shape[1],
                *scalars, _ptr(out), _ptr(grads[0]), d_mu, d_logvar, stream_ptr()))
    ctx.save_for_backward(*grads)
    return out


def _kl_loss_backward(ctx, g):
    """(d recon, None for the target, d mu, d logvar)"""
    grads, need = ctx.saved_tensors, ctx.needs_input_grad
    kl = len(grads) == 3
    return (_times(grads[0], g, need[0]), None, _times(grads[1], g, need[2]) if kl else None,
            _times(grads[2], g, need[3]) if kl else None)


class _MultinomialLoss(torch.autograd.Function):
    """``rtx_multinomial_loss_grad``; operands contiguous float32 on the device"""

    @staticmethod
    def forward(ctx, recon, x, mu, logvar, beta):
        return _kl_loss_forward(ctx, lib().rtx_multinomial_loss_grad, recon, x, mu, logvar, float(beta))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _kl_loss_backward(ctx, g) + (None,)


class _BceKlLoss(torch.autograd.Function):
    """``rtx_bce_kl_loss_grad``; operands contiguous float32 on the device"""

    @staticmethod
    def forward(ctx, recon, x, mu, logvar):
        return _kl_loss_forward(ctx, lib().rtx_bce_kl_loss_grad, recon, x, mu, logvar)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _kl_loss_backward(ctx, g)


class _MseLoss(torch.autograd.Function):
    """``rtx_mse_loss_grad``; operands contiguous float32 ``[rows, n_items]``"""

    @staticmethod
    def forward(ctx, prediction, ground_truth):
        out = torch.empty((), dtype=torch.float32, device=prediction.device)
        grad = torch.empty_like(prediction)
        check(lib().rtx_mse_loss_grad(_ptr(prediction), _ptr(ground_truth), prediction.shape[0], prediction.shape[1], _ptr(out),
                                      _ptr(grad), stream_ptr()))
        ctx.save_for_backward(grad)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _times(ctx.saved_tensors[0], g, ctx.needs_input_grad[0]), None


class _SumL2Norms(torch.autograd.Function):
    """``rtx_sum_l2_norms_grad``; operands contiguous float32 on one device"""

    @staticmethod
    def forward(ctx, *ts):
        n = len(ts)
        grads = [torch.empty_like(t) for t in ts]
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        gptrs = (C.c_void_p * n)(*[t.data_ptr() for t in grads])
        sizes = (C.c_int64 * n)(*[t.numel() for t in ts])
        out = torch.empty((), dtype=torch.float32, device=ts[0].device)
        check(lib().rtx_sum_l2_norms_grad(ptrs, sizes, n, _ptr(out), gptrs, stream_ptr()))
        ctx.save_for_backward(*grads)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return tuple(_times(d, g, need) for d, need in zip(ctx.saved_tensors, ctx.needs_input_grad))


class _Reparam(torch.autograd.Function):
    """``rtx_reparam`` / ``rtx_reparam_grad``; ``mu`` / ``logvar`` contiguous float32 ``[n, latent]`` on the device"""

    @staticmethod
    def forward(ctx, mu, logvar, seed, noise):
        z, eps = torch.empty_like(mu), torch.empty_like(mu)
        check(lib().rtx_reparam(_ptr(mu), _ptr(logvar), mu.shape[0], mu.shape[1], _ptr(noise), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                C.c_uint64(0), _ptr(z), _ptr(eps), stream_ptr()))
        ctx.save_for_backward(logvar, eps)
        return z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        logvar, eps = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = g.to(torch.float32).expand(logvar.shape).contiguous()
        d_mu = torch.empty_like(logvar) if need[0] else None
        d_logvar = torch.empty_like(logvar) if need[1] else None
        if need[0] or need[1]:
            check(lib().rtx_reparam_grad(_ptr(g), _ptr(logvar), _ptr(eps), logvar.shape[0], logvar.shape[1], _ptr(d_mu), _ptr(d_logvar),
                                         stream_ptr()))
        return d_mu, d_logvar, None, None


def reparameterize(mu, logvar, seed=0, noise=None):
    """``z = mu + eps * exp(logvar / 2)`` on float32 ``[n, latent]`` device tensors (``rtx_reparam``): the VAE head's sampling step
    as an operator of its own, in the head's own arithmetic.  ``eps`` is ``noise`` (``[n, latent]``) when given, else the fused
    head's draw for ``seed`` at index ``b * latent + j``.  With grad mode on and ``mu`` or ``logvar`` requiring grad, ``z`` carries
    a ``grad_fn`` (``rtx_reparam_grad``: ``d mu = d z``, ``d logvar = d z eps exp(logvar / 2) / 2``)."""
    _lib.require_gpu()
    if mu.dim() != 2 or mu.shape != logvar.shape:
        raise _lib.RtxError("reparameterize: mu and logvar must both be [n, latent], got %s and %s" % (tuple(mu.shape), tuple(logvar.shape)))
    dev = torch.device("cuda", torch.cuda.current_device())
    mu, logvar = mu.to(dev, torch.float32).contiguous(), logvar.to(dev, torch.float32).contiguous()
    if noise is not None:
        if tuple(noise.shape) != tuple(mu.shape):
            raise _lib.RtxError("reparameterize: the injected noise must be %s, got %s" % (tuple(mu.shape), tuple(noise.shape)))
        noise = noise.detach().to(dev, torch.float32).contiguous()
    return _Reparam.apply(mu, logvar, seed, noise)


def multinomial_loss(recon, x, mu=None, logvar=None, beta=0.0):
    """``-mean_b sum_i log_softmax(recon)_bi x_bi + beta * KLD`` as a 0-dim device tensor
    (reference MultiVAE.loss_function, rectorch/models.py:813-815).  With grad mode on and ``recon``, ``mu`` or ``logvar`` requiring
    grad the result carries a ``grad_fn`` (``rtx_multinomial_loss_grad``: the same value, and the gradients from the same launch)."""
    grad = _wants_grad({"x": x}, recon, mu, logvar)
    recon, x, mu, logvar, out = _loss_operands(recon, x, mu, logvar)
    if grad:
        return _MultinomialLoss.apply(recon, x, mu, logvar, float(beta))
    check(lib().rtx_multinomial_loss(_ptr(recon), _ptr(x), recon.shape[0], recon.shape[1], _ptr(mu), _ptr(logvar),
                                     0 if mu is None else mu.shape[1], float(beta), _ptr(out), stream_ptr()))
    return out


def bce_kl_loss(recon, x, mu=None, logvar=None):
    """``F.binary_cross_entropy(recon, x) + KLD`` as a 0-dim device tensor: the BCE is the mean over every element, with
    ``log`` and ``log1p`` clamped at -100 as torch does; KLD ``= -0.5 mean_b sum_z (1 + logvar - mu^2 - exp(logvar))``
    (reference VAE.loss_function, rectorch/models.py:581-583).  ``recon`` holds probabilities (the sigmoid outputs).
    Differentiable like :func:`multinomial_loss` (``rtx_bce_kl_loss_grad``)."""
    grad = _wants_grad({"x": x}, recon, mu, logvar)
    recon, x, mu, logvar, out = _loss_operands(recon, x, mu, logvar)
    if recon.shape != x.shape or recon.dim() != 2:
        raise _lib.RtxError("bce_kl_loss: recon and x must be [batch, n_items] alike, got %s and %s"
                            % (tuple(recon.shape), tuple(x.shape)))
    if grad:
        return _BceKlLoss.apply(recon, x, mu, logvar)
    check(lib().rtx_bce_kl_loss(_ptr(recon), _ptr(x), recon.shape[0], recon.shape[1], _ptr(mu), _ptr(logvar),
                                0 if mu is None else mu.shape[1], _ptr(out), stream_ptr()))
    return out


def mse_loss(prediction, ground_truth):
    """``torch.nn.MSELoss()(ground_truth, prediction)`` as a 0-dim device tensor: the mean over every element of
    ``(ground_truth - prediction)^2`` (reference AETrainer.loss_function, rectorch/models.py:347-377).  Differentiable with
    respect to ``prediction`` like :func:`multinomial_loss` (``rtx_mse_loss_grad``)."""
    grad = _wants_grad({"ground_truth": ground_truth}, prediction)
    prediction, ground_truth, _, _, out = _loss_operands(prediction, ground_truth)
    if prediction.shape != ground_truth.shape or prediction.numel() == 0:
        raise _lib.RtxError("mse_loss: prediction and ground_truth must be non-empty tensors of one shape, got %s and %s"
                            % (tuple(prediction.shape), tuple(ground_truth.shape)))
    # (the mean runs over every element: any shape is a [batch, n_items] matrix for it)
    n_items = prediction.shape[-1] if prediction.dim() >= 1 else 1
    prediction = prediction.reshape(-1, n_items)      # (contiguous: views)
    ground_truth = ground_truth.reshape(-1, n_items)
    if grad:
        return _MseLoss.apply(prediction, ground_truth)
    check(lib().rtx_mse_loss(_ptr(prediction), _ptr(ground_truth), prediction.shape[0], n_items, _ptr(out), stream_ptr()))
    return out


def sum_l2_norms(tensors):
    """``sum_t ||tensor_t||_2`` as a 0-dim device tensor (the regulariser of MultiDAE.loss_function,
    reference rectorch/models.py:702-706).  Differentiable with respect to every listed tensor that requires grad
    (``rtx_sum_l2_norms_grad``: ``tensor_t / ||tensor_t||_2``, zeros where the norm is zero)."""
    _lib.require_gpu()
    tensors = list(tensors)
    if _wants_grad({}, *tensors):
        return _SumL2Norms.apply(*[t.to(torch.float32).contiguous() for t in tensors])
    ts = [t.contiguous() for t in tensors]
    n = len(ts)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    sizes = (C.c_int64 * n)(*[t.numel() for t in ts])
    out = torch.empty((), dtype=torch.float32, device=ts[0].device)
    check(lib().rtx_sum_l2_norms(ptrs, sizes, n, _ptr(out), stream_ptr()))
    return out


def grad_norm(tensors, norm_type=2.0):
    """The global norm of up to 32 float32 device tensors as a 0-dim device tensor (``rtx_grad_norm``; ``norm_type`` 2 or
    ``inf``): what ``torch.nn.utils.clip_grad_norm_`` returns for them, from the norm kernels of the device's gradient clipping --
    accumulated in double in a fixed order, so two calls on the same data agree to the bit."""
    _lib.require_gpu()
    norm_type = float(norm_type)
    if norm_type != 2.0 and norm_type != float("inf"):
        raise ValueError("grad_norm: norm_type %r is not supported; supported: 2.0 and float('inf')" % (norm_type,))
    ts = [t.detach().to(torch.float32).contiguous() for t in tensors]
    n = len(ts)
    if not 1 <= n <= 32:
        raise ValueError("grad_norm: 1 to 32 tensors at a time, got %d" % n)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in ts])
    sizes = (C.c_int64 * n)(*[t.numel() for t in ts])
    out = torch.empty((), dtype=torch.float32, device=ts[0].device)
    check(lib().rtx_grad_norm(ptrs, sizes, n, norm_type, _ptr(out), stream_ptr()))
    return out


def topk_metrics(scores, heldout, rows, ks, want_topk=False, out=None, rank_metrics=False):
    """nDCG@k and Recall@k for every k in ``ks`` (reference rectorch/metrics.py:136-147, 187-196) computed on the
    device from a score tensor ``[B, n_items]`` and the users' held-out rows of a resident :class:`CsrMatrix`.
    Returns ``(ndcg [len(ks), B], recall [len(ks), B])`` as float64 device tensors (+ the sorted top-k item ids).
    ``out``: a pair of contiguous float64 ``[len(ks), B]`` tensors to write into (no allocation per batch).
    ``rank_metrics=True`` (``rtx_topk_metrics_ex``): hit@k (1.0 / 0.0) and mrr@k (metrics.py:231-238, 272-285) follow recall,
    ``(ndcg, recall, hit, mrr[, topk])``; ``out`` then holds four tensors."""
    _lib.require_gpu()
    scores = scores.contiguous()
    B, n_items = scores.shape
    ks = [int(k) for k in ks]
    arr = (C.c_int32 * len(ks))(*ks)
    if out is not None:
        assert len(out) == (4 if rank_metrics else 2)
        for t in out:
            assert t.shape == (len(ks), B) and t.is_contiguous() and t.dtype == torch.float64
        res = tuple(out)
    else:
        res = tuple(torch.empty((len(ks), B), dtype=torch.float64, device=scores.device) for _ in range(4 if rank_metrics else 2))
    kmax = min(max(ks), n_items)
    topk = torch.empty((B, kmax), dtype=torch.int32, device=scores.device) if want_topk else None
    if rank_metrics:
        check(lib().rtx_topk_metrics_ex(_ptr(scores), n_items, B, n_items, heldout.handle, _ptr(rows), arr, len(ks),
                                        *[_ptr(t) for t in res], _ptr(topk), 0, stream_ptr()))
    else:
        check(lib().rtx_topk_metrics(_ptr(scores), n_items, B, n_items, heldout.handle, _ptr(rows), arr, len(ks),
                                     *[_ptr(t) for t in res], _ptr(topk), 0, stream_ptr()))
    return res + (topk,) if want_topk else res


TOPK_ITEMS_MAX = 1024


def topk_items(scores, k, excl=None, rows=None, want_scores=True, out=None):
    """``rtx_topk_items``: the ``K = min(k, n_items)`` best items of every row of the device tensor ``scores`` (``[B, n_items]``,
    float32 or float64, unit column stride) and their scores, ``1 <= k <= 1024``.  Order: score descending, item id ascending among
    equal scores (``-0.0 == +0.0``; float64 rows compare as full doubles; ``-inf`` ranks last; NaN is out of contract).
    ``excl``: a resident :class:`CsrMatrix` whose row b -- or row ``rows[b]`` (device int32) -- lists items that rank as ``-inf``
    (stored non-zero entries; the score tensor is not written to).  Returns ``(items int32 [B, K], scores [B, K] of the input's
    dtype)``; ``want_scores=False`` skips the second output (``None``).  ``out``: a pair of contiguous tensors to write into."""
    _lib.require_gpu()
    if scores.dim() != 2 or scores.dtype not in (torch.float32, torch.float64) or not scores.is_cuda:
        raise _lib.RtxError("topk_items: scores must be a 2-d float32 or float64 device tensor, got %s %s on %s"
                            % (tuple(scores.shape), scores.dtype, scores.device))
    B, n_items = scores.shape
    if scores.stride(1) != 1 or (B > 1 and scores.stride(0) < n_items):
        scores = scores.contiguous()
    ld = scores.stride(0) if B > 1 else n_items
    if rows is not None:
        rows = rows.to(device=scores.device, dtype=torch.int32).contiguous()
        if rows.numel() != B:
            raise _lib.RtxError("topk_items: %d row numbers for %d score rows" % (rows.numel(), B))
    kk = max(min(int(k), n_items), 0)
    if out is not None:
        items, vals = out
        assert items.shape == (B, kk) and items.dtype == torch.int32 and items.is_contiguous()
        assert vals is None or (vals.shape == (B, kk) and vals.dtype == scores.dtype and vals.is_contiguous())
    else:
        items = torch.empty((B, kk), dtype=torch.int32, device=scores.device)
        vals = torch.empty((B, kk), dtype=scores.dtype, device=scores.device) if want_scores else None
    dtype = _lib.RTX_F64 if scores.dtype == torch.float64 else _lib.RTX_F32
    check(lib().rtx_topk_items(_ptr(scores), dtype, ld, B, n_items, None if excl is None else excl.handle, _ptr(rows), int(k),
                               _ptr(items), _ptr(vals), stream_ptr()))
    return items, vals


def opr_draw(heldout, rows, n_items, r, pin=False):
    """The negatives ``one_plus_random`` (reference rectorch/evaluation.py:113-178) draws with Python's ``random.sample`` for the
    held-out positives of the users ``rows``, drawn by ``rtx_opr_draw`` on the host from -- and advancing -- the state of the
    ``random`` module, index for index as the reference's loop would.  ``heldout``: host CSR arrays ``(indptr int64, indices int32,
    values float32 or None)``.  Returns ``(contest_row, contest_item, draws [contests, r], short_row)`` as int32 host tensors (pinned
    with ``pin``): the contests row-major, positives ascending; ``short_row`` is the first row with fewer than ``r`` negatives (-1:
    none), where drawing stopped and ``random.sample`` raises."""
    import random
    indptr, indices, values = heldout
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    cap = int((indptr[rows.astype(np.int64) + 1] - indptr[rows]).sum())     # stored entries: >= the contests
    crow = torch.empty(cap, dtype=torch.int32, pin_memory=pin)
    citem = torch.empty(cap, dtype=torch.int32, pin_memory=pin)
    draws = torch.empty((cap, r), dtype=torch.int32, pin_memory=pin)
    version, words, gauss = random.getstate()
    st = (C.c_uint32 * 625)(*words)
    n, short = C.c_int64(), C.c_int32()
    check(lib().rtx_opr_draw(st, indptr.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p),
                             None if values is None else values.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p),
                             len(rows), int(n_items), int(r), cap, _ptr(crow), _ptr(citem), _ptr(draws), C.byref(n), C.byref(short)))
    random.setstate((version, tuple(st), gauss))
    n = n.value
    return crow[:n], citem[:n], draws[:n], short.value


def opr_rank(scores, contest_row, contest_item, draws, out=None):
    """``rtx_opr_rank`` / ``rtx_opr_rank_f64``: for every contest, how many of its ``r`` drawn negatives score strictly above the
    positive (the positive wins ties) in the device score rows ``scores [B, n_items]``, float32 or float64 (the comparison is made in
    the rows' own type).  Device int32 tensor ``[contests]``."""
    if scores.dtype not in (torch.float32, torch.float64):
        raise _lib.RtxError("opr_rank: scores must be float32 or float64, got %s" % scores.dtype)
    scores = scores.contiguous()
    n, r = draws.shape
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=scores.device)
    fn = lib().rtx_opr_rank_f64 if scores.dtype == torch.float64 else lib().rtx_opr_rank
    check(fn(_ptr(scores), scores.shape[1], scores.shape[0], scores.shape[1], _ptr(contest_row), _ptr(contest_item),
             _ptr(draws), n, r, _ptr(out), stream_ptr()))
    return out


LIST_METRICS_MAX_KS = 16


def list_metrics(items, heldout, rows, ks, out=None):
    """``rtx_list_metrics``: nDCG@k, Recall@k, hit@k and mrr@k (rectorch_amd/metrics.py) of ranked item lists -- ``items``, a device
    int32 tensor ``[n, K]`` with unit column stride, every row best first, as :func:`topk_items` and ``recommend`` return them --
    against the users' held-out rows of a resident :class:`CsrMatrix`: row b of it, or row ``rows[b]`` (device int32, nullable).
    Any ``K >= 1``; a cut-off above ``K`` counts the ``K`` ranked items.  Returns ``(ndcg, recall, hit, mrr)``, float64 device
    tensors ``[len(ks), n]`` (hit as 1.0 / 0.0; a user without held-out items gets NaN, NaN, 0, 0, as :func:`topk_metrics` gives).
    ``out``: four contiguous float64 ``[len(ks), n]`` tensors to write into."""
    _lib.require_gpu()
    if items.dim() != 2 or items.dtype != torch.int32 or not items.is_cuda:
        raise _lib.RtxError("list_metrics: items must be a 2-d int32 device tensor, got %s %s on %s"
                            % (tuple(items.shape), items.dtype, items.device))
    n, K = items.shape
    if K < 1:
        raise _lib.RtxError("list_metrics: the lists are empty (K = 0)")
    if items.stride(1) != 1 or (n > 1 and items.stride(0) < K):
        items = items.contiguous()
    ld = items.stride(0) if n > 1 else K
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 1:
        raise _lib.RtxError("list_metrics: cut-offs must be >= 1, got %s" % (ks,))
    if rows is not None:
        rows = rows.to(device=items.device, dtype=torch.int32).contiguous()
        if rows.numel() != n:
            raise _lib.RtxError("list_metrics: %d row numbers for %d lists" % (rows.numel(), n))
    if out is not None:
        assert len(out) == 4
        for t in out:
            assert t.shape == (len(ks), n) and t.is_contiguous() and t.dtype == torch.float64
        res = tuple(out)
    else:
        res = tuple(torch.empty((len(ks), n), dtype=torch.float64, device=items.device) for _ in range(4))
    for lo in range(0, len(ks), LIST_METRICS_MAX_KS):          # (the kernel takes 16 cut-offs a launch: rows lo .. of the outputs)
        part = ks[lo:lo + LIST_METRICS_MAX_KS]
        arr = (C.c_int32 * len(part))(*part)
        check(lib().rtx_list_metrics(_ptr(items), ld, n, K, heldout.handle, _ptr(rows), arr, len(part),
                                     *[_ptr(t[lo:]) for t in res], max(n, 0), stream_ptr()))
    return res


class _ResidentSolver:
    """What the device-resident solvers of the fold-in family share (EASE, ADMM SLIM, ItemKNN, WMF: fitted once, kept in HBM, scored by
    users' sparse rows): the native ``handle`` and its destruction, the fit's ``timings``, and ``scores``.  A subclass names its native
    calls -- ``_DESTROY``, ``_SCORES``, ``_TIMINGS`` (the function, then its four keys) -- and sets ``handle``, ``n_items`` and ``train``:
    the resident training matrix, or ``None`` where the model was loaded from its weights (then ``scores`` needs ``X`` and refuses
    without it in the words of ``_NO_TRAIN``)."""
    handle = None
    _DESTROY = _SCORES = _NO_TRAIN = None
    _TIMINGS = ()

    @staticmethod
    def _resident(train):
        return train if isinstance(train, CsrMatrix) else CsrMatrix(train)

    def timings(self):
        """HIP-event durations (ms) of the fit under the keys of ``_TIMINGS``: the total, then three phases (zeros for a loaded
        model)."""
        v = [C.c_double() for _ in range(4)]
        check(getattr(lib(), self._TIMINGS[0])(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(self._TIMINGS[1:], (x.value for x in v)))

    def _scores_call(self, *args):
        return getattr(lib(), self._SCORES)(*args)

    def scores(self, row_ids, mask=None, out=None, X=None, mask_rows=None):
        """The score rows of the users ``row_ids`` as a float64 device tensor ``[len(row_ids), n_items]`` (written into ``out`` when
        given), ``-inf`` at the non-zero entries of ``mask`` (a :class:`CsrMatrix` whose row b belongs to ``row_ids[b]``; reference
        models.py:1055-1056).  ``X``: a :class:`CsrMatrix` over the same items to take the rows from instead of the training matrix --
        fold-in of users the fit never saw.  ``mask_rows`` (device int32, one per user): the mask's row of every user instead of row
        b."""
        if X is None and self.train is None:
            raise RuntimeError(self._NO_TRAIN)
        src = self.train if X is None else X
        n_items = self.n_items
        if src.shape[1] != n_items:
            raise ValueError("the rows' matrix has %d columns, the model has %d items" % (src.shape[1], n_items))
        row_ids = torch.as_tensor(row_ids, dtype=torch.int32).to("cuda").contiguous()
        n = int(row_ids.numel())
        if n and (int(row_ids.min()) < 0 or int(row_ids.max()) >= src.shape[0]):
            raise IndexError("user index out of range for the %s matrix (%d users)" % ("training" if X is None else "given", src.shape[0]))
        if mask is not None:
            if mask.shape[1] != n_items or (mask_rows is None and mask.shape[0] != n):
                raise ValueError("mask matrix has shape %s, expected (%d, %d)" % (mask.shape, n, n_items))
            if mask_rows is not None:
                mask_rows = torch.as_tensor(mask_rows, dtype=torch.int32).to("cuda").contiguous()
                if mask_rows.numel() != n:
                    raise ValueError("%d mask row numbers for %d users" % (mask_rows.numel(), n))
                if n and (int(mask_rows.min()) < 0 or int(mask_rows.max()) >= mask.shape[0]):
                    raise IndexError("mask row out of range for the mask matrix (%d rows)" % mask.shape[0])
        if out is None:
            out = torch.empty((n, n_items), dtype=torch.float64, device="cuda")
        if n:
            check(self._scores_call(self.handle, src.handle, _ptr(row_ids), n, None if mask is None else mask.handle,
                                    _ptr(mask_rows) if mask is not None else None, _ptr(out), stream_ptr()))
        return out

    def __del__(self):
        h = self.handle
        if h is not None and h.value:
            try:
                getattr(lib(), self._DESTROY)(h)
            except Exception:
                pass
            self.handle = None


class EaseSolver(_ResidentSolver):
    """Device-resident EASE model: the item-item matrix ``B`` of reference ``EASE.train`` (rectorch/models.py:
    1015-1024) computed by ``rtx_ease_fit`` (Gram matrix, f64 Cholesky, inverse -- all MFMA) and kept in HBM.  ``scores``: ``(X B)[row_ids]``
    (reference models.py:1025 + 1054)."""
    _DESTROY, _SCORES = "rtx_ease_destroy", "rtx_ease_scores"
    _TIMINGS = ("rtx_ease_timings", "fit_ms", "gram_ms", "chol_ms", "inv_ms")      # total, Gram matrix, Cholesky, inverse + P = W^T W

    def __init__(self, train, lam):
        _lib.require_gpu()
        self.train = self._resident(train)
        self.lam = float(lam)
        h = C.c_void_p()
        check(lib().rtx_ease_fit(self.train.handle, C.c_double(self.lam), C.byref(h), stream_ptr()))
        self.handle = h
        self.n_items = int(self.train.shape[1])

    def weights(self):
        """``B`` as a float64 device tensor [n_items, n_items] (a copy)."""
        out = torch.empty((self.n_items, self.n_items), dtype=torch.float64, device="cuda")
        check(lib().rtx_ease_copy_weights(self.handle, _ptr(out), stream_ptr()))
        return out


class AdmmSolver(_ResidentSolver):
    """Device-resident ADMM SLIM model: the matrix ``C`` of reference ``ADMM_Slim.train`` (rectorch/models.py:1464-1522)
    computed by ``rtx_admm_fit`` (EASE's Gram matrix / Cholesky / inverse, then one fused f64 MFMA GEMM launch per
    iteration) and kept in HBM with ``P`` and ``Gamma``.  ``scores``: ``(X C [+ b])[row_ids]`` (reference models.py:1524-1531)."""
    _DESTROY, _SCORES = "rtx_admm_destroy", "rtx_admm_scores"
    _TIMINGS = ("rtx_admm_timings", "fit_ms", "factor_ms", "baux_ms", "iter_ms")   # total, Gram + Cholesky + P, B_aux = P G, all iterations

    MATRICES = {"P": 0, "C": 1, "Gamma": 2}

    def __init__(self, train, lambda1, lambda2, rho, nn_constr, l1_penalty, item_bias, num_iter):
        _lib.require_gpu()
        self.train = self._resident(train)
        self.item_bias = bool(item_bias)
        h = C.c_void_p()
        check(lib().rtx_admm_fit(self.train.handle, C.c_double(float(lambda1)), C.c_double(float(lambda2)), C.c_double(float(rho)),
                                 int(bool(nn_constr)), int(bool(l1_penalty)), int(self.item_bias), int(num_iter), C.byref(h),
                                 stream_ptr()))
        self.handle = h
        self.n_items = int(self.train.shape[1])

    def copy(self, what):
        """``P``, ``C`` or ``Gamma`` as a float64 device tensor [n_items, n_items] (a copy)."""
        out = torch.empty((self.n_items, self.n_items), dtype=torch.float64, device="cuda")
        check(lib().rtx_admm_copy(self.handle, self.MATRICES[what], _ptr(out), stream_ptr()))
        return out


def _knn_similarity_id(similarity):
    if similarity not in _lib.KNN_SIMILARITIES:
        raise ValueError("similarity %r is not supported; supported: %s" % (similarity, ", ".join(sorted(_lib.KNN_SIMILARITIES))))
    return _lib.KNN_SIMILARITIES[similarity]


def knn_similarity(X, shrink=0.0, similarity="cosine"):
    """``rtx_knn_similarity``: the item-item similarity matrix of ItemKNN as a float64 device tensor ``[n_items, n_items]`` --
    ``G = XᵀX`` on the matrix cores, then cosine ``G_ij / (sqrt(G_ii) sqrt(G_jj) + shrink)`` or jaccard ``G_ij / (G_ii + G_jj - G_ij +
    shrink)`` (binary data only); ``-inf`` on the diagonal and where ``G_ij`` is not positive ("no neighbour").  Symmetric to the bit.
    ``X``: a scipy CSR matrix or a resident :class:`CsrMatrix`."""
    _lib.require_gpu()
    sim = _knn_similarity_id(similarity)
    X = X if isinstance(X, CsrMatrix) else CsrMatrix(X)
    n = int(X.shape[1])
    out = torch.empty((n, n), dtype=torch.float64, device="cuda")
    check(lib().rtx_knn_similarity(X.handle, C.c_double(float(shrink)), sim, _ptr(out), stream_ptr()))
    return out


class KnnSolver(_ResidentSolver):
    """Device-resident ItemKNN model: the sparse item-item matrix ``W`` (CSR by source item) fitted by ``rtx_knn_fit`` -- Gram matrix
    on MFMA, similarity, the float64 list kernel for the per-item top-k, an ordered CSR build -- and kept in HBM.  ``train``: the
    resident training matrix, or ``None`` for a model built by :meth:`from_csr` (then ``scores`` needs ``X``).  ``scores``:
    ``(X W)[row_ids]``, summed over each user's stored entries in their stored order."""
    _DESTROY, _SCORES = "rtx_knn_destroy", "rtx_knn_scores"
    _TIMINGS = ("rtx_knn_timings", "fit_ms", "gram_ms", "sim_ms", "select_ms")     # total, Gram matrix, similarity, selection
    _NO_TRAIN = ("this ItemKNN model was loaded from its W matrix and holds no training matrix to look users up in: "
                 "pass their rows (score_rows / recommend_rows)")

    def __init__(self, train, k, shrink=0.0, similarity="cosine", normalize=False):
        _lib.require_gpu()
        sim = _knn_similarity_id(similarity)
        self.train = self._resident(train)
        h = C.c_void_p()
        check(lib().rtx_knn_fit(self.train.handle, int(k), C.c_double(float(shrink)), sim, int(bool(normalize)), C.byref(h), stream_ptr()))
        self.handle = h
        self.n_items = int(self.train.shape[1])

    @classmethod
    def from_csr(cls, W):
        """A solver over a given ``W`` (``scipy.sparse`` matrix ``[n_items, n_items]``, rows = source items) through ``rtx_knn_load``:
        what :meth:`weights` / ``ItemKNN.W`` hand out.  It has no training matrix."""
        _lib.require_gpu()
        m = W.tocsr().astype(np.float64)
        if m.shape[0] != m.shape[1]:
            raise ValueError("W must be square (n_items x n_items), got %s" % (m.shape,))
        if not m.has_sorted_indices:
            m = m.copy()
            m.sort_indices()
        indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(m.indices, dtype=np.int32)
        values = np.ascontiguousarray(m.data, dtype=np.float64)
        self = cls.__new__(cls)
        self.train = None
        h = C.c_void_p()
        check(lib().rtx_knn_load(int(m.shape[0]), indptr.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p),
                                 values.ctypes.data_as(C.c_void_p), C.byref(h)))
        self.handle = h
        self.n_items = int(m.shape[0])
        return self

    @property
    def nnz(self):
        n, nnz = C.c_int32(), C.c_int64()
        check(lib().rtx_knn_shape(self.handle, C.byref(n), C.byref(nnz)))
        return int(nnz.value)

    def weights(self):
        """``W`` as a device CSR triple ``(indptr int64 [n_items + 1], indices int32 [nnz], values float64 [nnz])`` (copies)."""
        nnz = self.nnz
        indptr = torch.empty(self.n_items + 1, dtype=torch.int64, device="cuda")
        indices = torch.empty(nnz, dtype=torch.int32, device="cuda")
        values = torch.empty(nnz, dtype=torch.float64, device="cuda")
        check(lib().rtx_knn_copy(self.handle, _ptr(indptr), _ptr(indices) if nnz else None, _ptr(values) if nnz else None, stream_ptr()))
        return indptr, indices, values


def _wmf_factor_table(Y, n_rows):
    Y = torch.as_tensor(Y, dtype=torch.float64).to("cuda").contiguous()
    if Y.dim() != 2 or Y.shape[0] != n_rows:
        raise ValueError("the factor table has shape %s, expected (%d, f)" % (tuple(Y.shape), n_rows))
    return Y


def _wmf_row_ids(row_ids, X):
    """(device int32 row numbers or None, how many rows): the kernels trust them, so they are range-checked here"""
    if row_ids is None:
        return None, int(X.shape[0])
    row_ids = torch.as_tensor(row_ids, dtype=torch.int32).to("cuda").contiguous()
    n = int(row_ids.numel())
    if n and (int(row_ids.min()) < 0 or int(row_ids.max()) >= X.shape[0]):
        raise IndexError("row index out of range for the matrix (%d rows)" % X.shape[0])
    return row_ids, n


def wmf_systems(X, Y, alpha, lam, row_ids=None):
    """``rtx_wmf_systems``: the normal equations of WMF's half-sweep alone -- ``(A, b)``, float64 device tensors ``[n, f, f]`` (full,
    symmetric to the bit) and ``[n, f]``, of the rows ``row_ids`` (default: every row) of ``X`` (scipy CSR or :class:`CsrMatrix`)
    against the factor table ``Y`` ``[X.shape[1], f]``:  ``A_u = YᵀY + Σ (alpha r) y yᵀ + lam I``,  ``b_u = Σ (1 + alpha r) y``."""
    _lib.require_gpu()
    X = X if isinstance(X, CsrMatrix) else CsrMatrix(X)
    Y = _wmf_factor_table(Y, X.shape[1])
    f = int(Y.shape[1])
    row_ids, n = _wmf_row_ids(row_ids, X)
    A = torch.empty((n, f, f), dtype=torch.float64, device="cuda")
    b = torch.empty((n, f), dtype=torch.float64, device="cuda")
    check(lib().rtx_wmf_systems(X.handle, _ptr(row_ids), n, _ptr(Y), f, C.c_double(float(alpha)), C.c_double(float(lam)), _ptr(A), _ptr(b),
                                stream_ptr()))
    return A, b


def wmf_solve_rows(X, Y, alpha, lam, row_ids=None):
    """``rtx_wmf_solve_rows``: one half-sweep of WMF's alternating least squares -- the vectors ``x_u = A_u⁻¹ b_u`` (see
    :func:`wmf_systems`) of the rows ``row_ids`` (default: every row) of ``X`` against the factor table ``Y``, a float64 device tensor
    ``[n, f]``; a row without entries gets the zero vector.  With the final item factors this is the fold-in of any user."""
    _lib.require_gpu()
    X = X if isinstance(X, CsrMatrix) else CsrMatrix(X)
    Y = _wmf_factor_table(Y, X.shape[1])
    f = int(Y.shape[1])
    row_ids, n = _wmf_row_ids(row_ids, X)
    out = torch.empty((n, f), dtype=torch.float64, device="cuda")
    check(lib().rtx_wmf_solve_rows(X.handle, _ptr(row_ids), n, _ptr(Y), int(Y.shape[0]), f, C.c_double(float(alpha)), C.c_double(float(lam)),
                                   _ptr(out), stream_ptr()))
    return out


class WmfSolver(_ResidentSolver):
    """Device-resident WMF model (implicit-feedback ALS; the definition is in ``include/rectorch_hip.h``): the item factors ``Y`` and
    the user factors of the last user half-sweep, fitted by ``rtx_wmf_fit`` -- per row one normal-equation system built on f64 MFMA
    from gathered factor rows and solved by Cholesky in LDS -- and kept in HBM.  ``train``: the resident training matrix, or ``None``
    for a model built by :meth:`from_factors` (then ``scores`` needs ``X``).  ``scores``: fold-in and scores in one call -- every user's
    vector is solved from the user's row against the item factors, then ``x_u · y_j`` over all items."""
    _DESTROY, _SCORES = "rtx_wmf_destroy", "rtx_wmf_scores"
    # total, and summed over the iterations: the Gram matrices, the user half-sweeps, the item half-sweeps
    _TIMINGS = ("rtx_wmf_timings", "fit_ms", "gram_ms", "user_ms", "item_ms")
    _NO_TRAIN = ("this WMF model was loaded from its item factors and holds no training matrix to look users up in: "
                 "pass their rows (score_rows / recommend_rows)")

    TABLES = {"items": _lib.RTX_WMF_ITEMS, "users": _lib.RTX_WMF_USERS}

    def __init__(self, train, Y0, alpha, lam, num_iter):
        _lib.require_gpu()
        from scipy.sparse import csr_matrix
        if isinstance(train, CsrMatrix):
            raise TypeError("WmfSolver needs the scipy training matrix: it uploads its transpose as well")
        m = csr_matrix(train)
        Y0 = np.ascontiguousarray(Y0, dtype=np.float64)
        if Y0.ndim != 2 or Y0.shape[0] != m.shape[1]:
            raise ValueError("the initial item factors have shape %s, expected (%d, f)" % (Y0.shape, m.shape[1]))
        self.train = CsrMatrix(m)
        mt = m.T.tocsr()
        mt.sort_indices()
        self.train_t = CsrMatrix(mt)
        self.alpha, self.lam = float(alpha), float(lam)
        h = C.c_void_p()
        check(lib().rtx_wmf_fit(self.train.handle, self.train_t.handle, int(Y0.shape[1]), C.c_double(self.alpha), C.c_double(self.lam),
                                int(num_iter), Y0.ctypes.data_as(C.c_void_p), C.byref(h), stream_ptr()))
        self.handle = h
        self.n_users, self.n_items, self.factors_dim = int(m.shape[0]), int(m.shape[1]), int(Y0.shape[1])

    @classmethod
    def train(cls, train, Y0, alpha, lam, num_iter):
        """The fit as a named constructor, beside :meth:`from_factors` (on an instance ``train`` is the resident training matrix)."""
        return cls(train, Y0, alpha, lam, num_iter)

    @classmethod
    def from_factors(cls, Y, alpha, lam):
        """A solver over given item factors (``[n_items, f]``) through ``rtx_wmf_load``: it folds any rows in, and holds neither a
        training matrix nor user factors."""
        _lib.require_gpu()
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim != 2:
            raise ValueError("the item factors must be a matrix [n_items, f], got shape %s" % (Y.shape,))
        self = cls.__new__(cls)
        self.train = None
        self.train_t = None
        self.alpha, self.lam = float(alpha), float(lam)
        h = C.c_void_p()
        check(lib().rtx_wmf_load(int(Y.shape[0]), int(Y.shape[1]), C.c_double(self.alpha), C.c_double(self.lam), Y.ctypes.data_as(C.c_void_p),
                                 C.byref(h)))
        self.handle = h
        self.n_users, self.n_items, self.factors_dim = 0, int(Y.shape[0]), int(Y.shape[1])
        return self

    def factors(self, what="items"):
        """The item factors ``[n_items, f]`` or the user factors of the last user half-sweep ``[n_users, f]`` as a float64 device
        tensor (a copy)."""
        if what not in self.TABLES:
            raise ValueError("factors(%r): supported: 'items', 'users'" % (what,))
        if what == "users" and not self.n_users:
            raise RuntimeError("this WMF model was loaded from its item factors and holds no user factors: fold the users' rows in")
        out = torch.empty((self.n_items if what == "items" else self.n_users, self.factors_dim), dtype=torch.float64, device="cuda")
        check(lib().rtx_wmf_copy(self.handle, self.TABLES[what], _ptr(out), stream_ptr()))
        return out

    def _scores_call(self, *args):
        *head, stream = args                        # rtx_wmf_scores takes the row stride of ``out`` before the stream
        return lib().rtx_wmf_scores(*head, self.n_items, stream)


def user_rows_adam(V, exp_avg, exp_avg_sq, user_ids, g, lr, beta1, beta2, eps, step, latent=None):
    """``rtx_user_rows_adam``: torch.optim.SparseAdam's update of the rows ``user_ids[b]`` of ``V`` / ``exp_avg`` / ``exp_avg_sq``
    (float32 ``[n_users, ld]``, possibly column slices of wider tensors: ``ld`` is their row stride) from ``g`` float32
    ``[batch, >= latent]``, in place, on the current stream; ids outside ``[0, n_users)`` are skipped, the ids must be distinct.
    It is the update the CDAE training step applies inside its backward pass (include/rectorch_hip.h "CDAE")."""
    latent = int(V.shape[1] if latent is None else latent)
    for t in (V, exp_avg, exp_avg_sq):
        assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape == V.shape and t.stride(0) == V.stride(0)
    assert g.dtype == torch.float32 and g.dim() == 2 and g.stride(1) == 1 and g.shape[1] >= latent
    assert user_ids.dtype == torch.int32 and user_ids.is_contiguous() and user_ids.numel() == g.shape[0]
    check(lib().rtx_user_rows_adam(_ptr(V), _ptr(exp_avg), _ptr(exp_avg_sq), int(V.stride(0)), int(V.shape[0]), _ptr(user_ids), _ptr(g),
                                   int(g.stride(0)), int(g.shape[0]), latent, float(lr), float(beta1), float(beta2), float(eps), int(step),
                                   stream_ptr()))


def cast_f32_bf16(src, dst):
    """``dst`` (bfloat16) = round-to-nearest-even of ``src`` (float32), same number of elements, on the current stream."""
    assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16 and src.numel() == dst.numel()
    check(lib().rtx_cast_f32_bf16(_ptr(src), _ptr(dst), src.numel(), stream_ptr()))


class SvaeTarget:
    """Compact loss target of one SVAE sequence: the multi-hot rows of the reference's ``y_batch_s`` [1, T, n_items]
    (samplers.py:539-562) as a CSR over the T steps, plus the likelihood normaliser ``d`` the reference's training path
    ends up with (the ones of the FIRST step: ``train_batch`` flattens the target before ``loss_function`` sums
    ``x[0, :n_items]``, models.py:822 + 1623)."""
    __slots__ = ("indptr", "indices", "d", "n_steps")

    def __init__(self, rows, device="cuda"):
        """``rows``: list (one per time step) of distinct item ids"""
        ptr = np.zeros(len(rows) + 1, dtype=np.int64)
        for t, r in enumerate(rows):
            ptr[t + 1] = ptr[t] + len(r)
        idx = np.fromiter((i for r in rows for i in r), dtype=np.int32, count=int(ptr[-1]))
        self.indptr = torch.from_numpy(ptr).to(device)
        self.indices = torch.from_numpy(idx).to(device)
        self.d = float(len(rows[0])) if rows else 0.0
        self.n_steps = len(rows)


class SvaePack:
    """Several user sequences for ONE optimizer step (``SVAE_Sampler(pack=N)``; not in the reference): the input items of all
    users concatenated on the device, the row range of every user, and the targets of all time steps as one CSR.

    ``seqs``: list of item-id lists (the model inputs, i.e. all but each user's last item); ``target_rows``: per user the list
    (one entry per time step) of distinct target items.  ``d`` keeps, per user, the likelihood normaliser the reference's
    training path uses (the ones of the user's FIRST step, see :class:`SvaeTarget`)."""
    __slots__ = ("items", "seq_ptr", "lens", "indptr", "indices", "d", "n_steps", "users")

    def __init__(self, seqs, target_rows, users=None, device="cuda"):
        assert len(seqs) == len(target_rows) and len(seqs) >= 1
        self.lens = [len(q) for q in seqs]
        for q, rows in zip(seqs, target_rows):
            assert len(q) == len(rows) and len(q) >= 1, "every sequence needs one target row per time step"
        sp = np.zeros(len(seqs) + 1, dtype=np.int32)
        sp[1:] = np.cumsum(self.lens)
        self.n_steps = int(sp[-1])
        self.items = torch.from_numpy(np.fromiter((i for q in seqs for i in q), dtype=np.int32, count=self.n_steps)).to(device)
        self.seq_ptr = torch.from_numpy(sp).to(device)
        ptr = np.zeros(self.n_steps + 1, dtype=np.int64)
        ptr[1:] = np.cumsum(np.fromiter((len(r) for rows in target_rows for r in rows), dtype=np.int64, count=self.n_steps))
        self.indptr = torch.from_numpy(ptr).to(device)
        self.indices = torch.from_numpy(np.fromiter((i for rows in target_rows for r in rows for i in r), dtype=np.int32,
                                                    count=int(ptr[-1]))).to(device)
        self.d = [float(len(rows[0])) for rows in target_rows]
        self.users = list(users) if users is not None else None

    def __len__(self):
        return len(self.lens)

    def row_scales(self, beta):
        """per-row loss factors of the pack's step: (1 / (d_u N), beta / (T_u N)) repeated over each user's rows, as ONE device
        tensor [2, n_steps] (numpy on the host: torch.repeat_interleave on CPU tensors costs milliseconds)"""
        n = len(self.lens)
        lens = np.asarray(self.lens)
        nll = np.array([1.0 / (d * n) if d != 0 else np.inf for d in self.d], dtype=np.float32)
        kl = (np.float32(beta) / (lens * n)).astype(np.float32)
        both = np.stack([np.repeat(nll, lens), np.repeat(kl, lens)])
        return torch.from_numpy(both).to(self.items.device)


class SvaeEvalPack:
    """Several user sequences scored at once (``SVAE_Sampler(is_training=False, pack=N)``; not in the reference): the input items
    of all users concatenated on the device and the row range of every user.  Unlike :class:`SvaePack` it carries no per-step
    targets: :meth:`SvaeEngine.predict_pack` scores each user's last step only.

    ``seqs``: list of non-empty item-id lists (the model inputs, i.e. all but each user's last training item); ``users``: their
    ids, in the same order."""
    __slots__ = ("items", "seq_ptr", "lens", "n_steps", "users")

    def __init__(self, seqs, users=None, device="cuda"):
        assert len(seqs) >= 1
        self.lens = [len(q) for q in seqs]
        assert min(self.lens) >= 1, "every sequence needs at least one time step"
        sp = np.zeros(len(seqs) + 1, dtype=np.int32)
        sp[1:] = np.cumsum(self.lens)
        self.n_steps = int(sp[-1])
        self.items = torch.from_numpy(np.fromiter((i for q in seqs for i in q), dtype=np.int32, count=self.n_steps)).to(device)
        self.seq_ptr = torch.from_numpy(sp).to(device)
        self.users = list(users) if users is not None else None

    def __len__(self):
        return len(self.lens)


class SvaeEngine:
    """One ``rtx_svae``: the SVAE network's compute state (embedding -> GRU -> VAE head -> decoder, float32), bound to
    the network's parameters and, for training, to gradient buffers and the Adam moments (see :class:`Engine`)."""

    def __init__(self, n_items, embed_size, rnn_size, enc_dims, dec_dims, max_len=256):
        _lib.require_gpu()
        cfg = _lib.SvaeCfg()
        cfg.n_items, cfg.embed_size, cfg.rnn_size = int(n_items), int(embed_size), int(rnn_size)
        if len(enc_dims) - 1 > _lib.MAX_LAYERS or len(dec_dims) - 1 > _lib.MAX_LAYERS:
            raise _lib.RtxError("at most %d layers per encoder/decoder are supported" % _lib.MAX_LAYERS)
        cfg.n_enc, cfg.n_dec = len(enc_dims) - 1, len(dec_dims) - 1
        for i, d in enumerate(enc_dims):
            cfg.enc_dims[i] = int(d)
        for i, d in enumerate(dec_dims):
            cfg.dec_dims[i] = int(d)
        cfg.max_len = int(max_len)
        self.max_len, self.n_items, self.latent = int(max_len), int(n_items), int(enc_dims[-1])
        h = C.c_void_p()
        check(lib().rtx_svae_create(C.byref(cfg), C.byref(h)))
        self.handle = h
        self.n_tensors = lib().rtx_svae_n_tensors(h)
        self._keep = []

    def loss_mailbox(self, enable=True):
        """``rtx_svae_loss_mailbox``: every training step also reports its loss to coherent host memory as soon as it is final"""
        check(lib().rtx_svae_loss_mailbox(self.handle, int(bool(enable))))
        self._mailbox = bool(enable)

    def wait_loss(self, timeout_s=60.0):
        """the loss of the LAST step enqueued, without draining the stream behind it (``rtx_svae_wait_loss``)"""
        out = C.c_float()
        check(lib().rtx_svae_wait_loss(self.handle, C.byref(out), float(timeout_s)))
        return float(out.value)

    def set_option(self, key, value):
        """``"gemm_bf16"``: bf16 operands / float32 accumulate in every matrix product of the model (include/rectorch_hip.h)"""
        check(lib().rtx_svae_set_option(self.handle, key.encode(), int(value)))

    def get_option(self, key):
        """``"gemm_bf16"``, or the recurrence kernel this engine launches: ``"gru_fwd"`` / ``"gru_bwd"`` -> 0 generic,
        1 weight-resident on 1024 threads (backward only), 2 whole rows (forward only), 3 K-sliced (include/rectorch_hip.h)"""
        v = C.c_int32()
        check(lib().rtx_svae_get_option(self.handle, key.encode(), C.byref(v)))
        return v.value

    def bind(self, params, grads=None, exp_avg=None, exp_avg_sq=None):
        n = self.n_tensors
        assert len(params) == n, "expected %d parameter tensors, got %d" % (n, len(params))
        rows, cols = C.c_int32(), C.c_int32()
        for t, p in enumerate(params):
            check(lib().rtx_svae_tensor_shape(self.handle, t, C.byref(rows), C.byref(cols)))
            want = (rows.value,) if cols.value == 1 and p.dim() == 1 else (rows.value, cols.value)
            if tuple(p.shape) != want or p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                raise _lib.RtxError("parameter %d must be a contiguous float32 device tensor of shape %s, got %s %s on %s"
                                    % (t, want, tuple(p.shape), p.dtype, p.device))

        def arr(ts):
            if ts is None:
                return None
            return (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        self._keep = [params, grads, exp_avg, exp_avg_sq]
        check(lib().rtx_svae_bind(self.handle, arr(params), arr(grads), arr(exp_avg), arr(exp_avg_sq)))

    @staticmethod
    def _items(x):
        return x.reshape(-1).to("cuda", torch.int32).contiguous()

    def forward(self, x, noise=None, seed=0, remove_train=False, want_all=True):
        """SVAE_net.forward on one sequence: (logits [T, n_items] or None, last-step logits [n_items], mu, logvar)."""
        items = self._items(x)
        T = int(items.numel())
        dev = items.device
        la = torch.empty((T, self.n_items), dtype=torch.float32, device=dev) if want_all else None
        ll = torch.empty((self.n_items,), dtype=torch.float32, device=dev)
        mu = torch.empty((T, self.latent), dtype=torch.float32, device=dev)
        lv = torch.empty_like(mu)
        if noise is not None:
            noise = noise.to(dev, torch.float32).contiguous()
        check(lib().rtx_svae_forward(self.handle, _ptr(items), T, _ptr(noise), C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint64(0),
                                     int(remove_train), _ptr(la), _ptr(ll), _ptr(mu), _ptr(lv), stream_ptr()))
        return la, ll, mu, lv

    def train_step(self, x, target, step, loss_out, loss_accum=None):
        items = self._items(x)
        T = int(items.numel())
        if isinstance(target, SvaeTarget):
            assert target.n_steps == T, "the target has %d steps, the sequence %d" % (target.n_steps, T)
            ptr, idx, dense = target.indptr, target.indices, None
        else:
            dense = target.reshape(T, -1).to(items.device, torch.float32).contiguous()
            if dense.shape[1] != self.n_items:
                raise _lib.RtxError("the target must be [1, T, %d], got %s" % (self.n_items, tuple(target.shape)))
            ptr = idx = None
        check(lib().rtx_svae_train_step(self.handle, _ptr(items), T, _ptr(ptr), _ptr(idx), _ptr(dense), C.byref(step), _ptr(loss_out),
                                        _ptr(loss_accum), stream_ptr()))

    def train_pack(self, pack, step, beta, loss_out, loss_accum=None):
        """one optimizer step on the users of ``pack`` (:class:`SvaePack`): mean over the pack of the per-user SVAE loss"""
        if pack.n_steps > self.max_len:
            raise _lib.RtxError("the pack holds %d time steps, the engine was sized for %d" % (pack.n_steps, self.max_len))
        sc = pack.row_scales(beta)
        check(lib().rtx_svae_train_pack(self.handle, _ptr(pack.items), pack.n_steps, _ptr(pack.seq_ptr), len(pack), _ptr(sc[0]), _ptr(sc[1]),
                                        _ptr(pack.indptr), _ptr(pack.indices), C.byref(step), _ptr(loss_out), _ptr(loss_accum), stream_ptr()))

    def predict_pack(self, pack, noise=None, seed=0, remove_train=True):
        """``SVAE.predict`` for the users of ``pack`` (:class:`SvaeEvalPack`, or anything with its ``items`` / ``seq_ptr`` /
        ``n_steps``) in one call: ``(scores [N, n_items], mu [N, latent], logvar [N, latent])`` of every user's LAST step.
        ``noise``: ``[n_steps, latent]`` draws, of which user *u* takes the row of its last step; None samples with ``seed``."""
        n = len(pack)
        if pack.n_steps > self.max_len:
            raise _lib.RtxError("the pack holds %d time steps, the engine was sized for %d" % (pack.n_steps, self.max_len))
        dev = pack.items.device
        if noise is not None:
            noise = noise.to(dev, torch.float32).contiguous()
            if noise.dim() != 2 or noise.shape[0] < pack.n_steps or noise.shape[1] != self.latent:
                raise _lib.RtxError("the noise of a pack must be [n_steps = %d (or more rows), latent = %d], got %s"
                                    % (pack.n_steps, self.latent, tuple(noise.shape)))
        scores = torch.empty((n, self.n_items), dtype=torch.float32, device=dev)
        mu = torch.empty((n, self.latent), dtype=torch.float32, device=dev)
        lv = torch.empty_like(mu)
        check(lib().rtx_svae_predict_pack(self.handle, _ptr(pack.items), pack.n_steps, _ptr(pack.seq_ptr), n, _ptr(noise),
                                          C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint64(0), int(bool(remove_train)), _ptr(scores),
                                          _ptr(mu), _ptr(lv), stream_ptr()))
        return scores, mu, lv

    # ---- a loss computed outside the engine ---------------------------------------------------------------------------
    def _seqs(self, x):
        """(items, seq_ptr or None, n_seq, kept tensors) of a ``[1, T]`` sequence or of a :class:`SvaePack` / :class:`SvaeEvalPack`"""
        if hasattr(x, "seq_ptr"):
            if x.n_steps > self.max_len:
                raise _lib.RtxError("the pack holds %d time steps, the engine was sized for %d" % (x.n_steps, self.max_len))
            return x.items, x.seq_ptr, len(x), x
        return self._items(x), None, 1, None

    def forward_train(self, x, step):
        """``rtx_svae_forward_train``: the forward of the fused step (the draws of ``step``: ``seed`` / ``offset`` or an injected
        ``eps_noise``) on a ``[1, T]`` sequence or a pack, keeping its activations in the engine.  Returns ``(logits [T, n_items],
        mu, logvar [T, latent], ticket, seqs)``: the rows of all time steps, the ticket :meth:`backward` wants back, and the
        ``(items, seq_ptr, n_seq, keep)`` it names the sequences with."""
        seqs = self._seqs(x)
        items, seq_ptr, n_seq, _ = seqs
        T = int(items.numel())
        dev = items.device
        logits = torch.empty((T, self.n_items), dtype=torch.float32, device=dev)
        mu = torch.empty((T, self.latent), dtype=torch.float32, device=dev)
        lv = torch.empty_like(mu)
        ticket = C.c_uint64()
        check(lib().rtx_svae_forward_train(self.handle, _ptr(items), T, _ptr(seq_ptr), n_seq, step.eps_noise, C.c_uint64(step.seed),
                                           C.c_uint64(step.offset), _ptr(logits), _ptr(mu), _ptr(lv), C.byref(ticket), stream_ptr()))
        return logits, mu, lv, ticket.value, seqs

    def backward(self, seqs, ticket, d_logits, d_mu=None, d_logvar=None):
        """``rtx_svae_backward``: the backward chain from the caller's ``d loss / d logits`` (float32 ``[T, n_items]``, unit column
        stride; None: the loss does not depend on the logits) and ``d loss / d mu`` / ``d loss / d logvar`` (``[T, latent]``, either
        None) into the bound gradient buffers.  ``seqs``: what :meth:`forward_train` returned.  A stale ticket raises
        :class:`RtxError` before anything is enqueued."""
        items, seq_ptr, n_seq, _ = seqs
        T = int(items.numel())
        ld = self.n_items
        if d_logits is not None:
            if d_logits.dtype != torch.float32 or d_logits.dim() != 2 or d_logits.stride(1) != 1 or d_logits.shape != (T, self.n_items):
                d_logits = d_logits.to(torch.float32).expand(T, self.n_items).contiguous()
            ld = d_logits.stride(0) if T > 1 else self.n_items
            if ld < self.n_items:           # (an expanded row: stride 0)
                d_logits = d_logits.contiguous()
                ld = self.n_items
        if d_mu is not None:
            d_mu = d_mu.to(torch.float32).expand(T, self.latent).contiguous()
        if d_logvar is not None:
            d_logvar = d_logvar.to(torch.float32).expand(T, self.latent).contiguous()
        check(lib().rtx_svae_backward(self.handle, _ptr(items), T, _ptr(seq_ptr), n_seq, C.c_uint64(ticket), _ptr(d_logits), C.c_int64(ld),
                                      _ptr(d_mu), _ptr(d_logvar), stream_ptr()))

    def apply_adam(self, step):
        """``rtx_svae_apply_adam``: the fused step's Adam over the bound tensors, from the bound gradient buffers"""
        check(lib().rtx_svae_apply_adam(self.handle, C.byref(step), stream_ptr()))

    def set_optimizer(self, kind, flags=0, momentum=0.0, dampening=0.0, alpha=0.0, lr_decay=0.0):
        """``rtx_svae_set_optimizer``: the update rule of every later optimizer launch of this handle (``_lib.RTX_OPTIM_*``)"""
        o = _lib.Optim(int(kind), int(flags), float(momentum), float(dampening), float(alpha), float(lr_decay))
        check(lib().rtx_svae_set_optimizer(self.handle, C.byref(o)))

    def set_grad_clip(self, mode, bound=0.0):
        """``rtx_svae_set_grad_clip``: gradient clipping in front of every later optimizer launch of this handle"""
        check(lib().rtx_svae_set_grad_clip(self.handle, int(mode), float(bound)))

    def wait_grad_norm(self, step_count=None, timeout_s=0.0):
        """``(total norm, coefficient)`` of the LAST optimizer step enqueued (``rtx_svae_wait_grad_norm``; ``step_count`` is
        accepted for the signature of :meth:`Engine.wait_grad_norm` and not checked)"""
        out = (C.c_float * 2)()
        check(lib().rtx_svae_wait_grad_norm(self.handle, out, float(timeout_s)))
        return float(out[0]), float(out[1])

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                lib().rtx_svae_destroy(h)
            except Exception:
                pass
            self.handle = None
