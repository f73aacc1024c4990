r"""Evaluation utilities with the reference's API (rectorch/evaluation.py:11-178).

These are the host-side consumers of the hot path: they iterate a sampler, call ``model.predict`` (the HIP
forward) and score the returned logits with :class:`rectorch_amd.metrics.Metrics`.  The duck-typed contract
is the reference's: ``predict(x)[0]`` supports ``.cpu().numpy()``, samplers yield ``(data_tr, heldout)``
pairs supporting ``.view``, ``.shape`` and ``.cpu().numpy()`` (evaluation.py:100-103).
"""
from functools import partial
import inspect
import random

import numpy as np
import torch

from .metrics import Metrics

__all__ = ['ValidFunc', 'evaluate', 'evaluate_host', 'evaluate_device', 'one_plus_random', 'one_plus_random_host',
           'one_plus_random_device', 'recommend', 'recommend_host', 'metrics_from_lists']

DEVICE_TOPK_MAX = 1024


class ValidFunc():
    """Wrapper adapting an evaluation function to the ``(model, test_loader, metric_list)`` signature the
    trainers call (reference evaluation.py:11-64): extra keyword arguments are bound at construction and the
    remaining positional arguments must be exactly those three names.

    >>> opr = ValidFunc(one_plus_random, r=5)
    >>> opr
    ValidFunc(fun='one_plus_random', params={'r': 5})
    """
    def __init__(self, func, **kwargs):
        self.func_name = func.__name__
        self.function = partial(func, **kwargs)
        args = inspect.getfullargspec(self.function).args
        assert args == ["model", "test_loader", "metric_list"],\
            "A (partial) validation function must have the following kwargs: model, test_loader and\
            metric_list"

    def __call__(self, model, test_loader, metric):
        return self.function(model, test_loader, [metric])[metric]

    def __str__(self):
        kwdefargs = inspect.getfullargspec(self.function).kwonlydefaults
        return "ValidFunc(fun='%s', params=%s)" % (self.func_name, kwdefargs)

    def __repr__(self):
        return str(self)


def _to_numpy(t):
    from .engine import RowBatch
    if isinstance(t, RowBatch):            # rows of a device-resident CSR (sparse samplers): densify on the device
        return t.tr.gather_dense(t.rows).cpu().numpy()
    t = t.view(t.shape[0], -1)
    return t.cpu().numpy()


class _PerUserResults:
    """per-metric lists of per-batch arrays -> one array per metric, in loader order (reference evaluation.py:104-109)"""
    def __init__(self, metric_list):
        self._parts = {m: [] for m in metric_list}

    def add(self, batch_result):
        for m, values in batch_result.items():
            self._parts[m].append(values)

    def finish(self):
        return {m: np.concatenate(parts) for m, parts in self._parts.items()}


def _predict_numpy(model, data_tr):
    """scores of one batch as a host array; the resident-rows shortcut of the device sampler survives the reshape"""
    from .engine import RowBatch, SvaeEvalPack, tag_rows, tagged_rows
    if isinstance(data_tr, (RowBatch, SvaeEvalPack)):      # (a pack of SVAE users: one score row per user)
        return model.predict(data_tr)[0].cpu().numpy()
    data_tensor = data_tr.view(data_tr.shape[0], -1)
    rows = tagged_rows(data_tr)
    if rows is not None:
        tag_rows(data_tensor, rows)
    if getattr(data_tr, "_rtx_users", None) is not None:       # (a host sampler's user ids, for a CDAE_net)
        data_tensor._rtx_users = data_tr._rtx_users
    return model.predict(data_tensor)[0].cpu().numpy()


def evaluate_host(model, test_loader, metric_list):
    r"""The reference's loop as it is written (evaluation.py:100-109): ``predict`` per batch, the ``[B, n_items]`` scores and the
    held-out rows copied to the host, :class:`Metrics` in numpy.  What :func:`evaluate` falls back to."""
    out = _PerUserResults(metric_list)
    for data_tr, heldout in test_loader:
        out.add(Metrics.compute(_predict_numpy(model, data_tr), _to_numpy(heldout), metric_list))
    return out.finish()


def evaluate(model, test_loader, metric_list):
    r"""Evaluate ``model`` on every batch of ``test_loader`` with every metric of ``metric_list``
    (``"name@k"`` strings).  Returns ``dict metric -> per-user numpy array`` in loader order
    (reference evaluation.py:67-110).

    Same signature, same values -- and since round 5 the same SPEED as :func:`evaluate_device` wherever that applies: a
    device-resident :class:`DataSampler` with held-out rows and ``ndcg@k`` / ``recall@k`` / ``hit@k`` / ``mrr@k`` metrics (k <= 1024) are scored by the
    top-k kernel on the GPU (4.3 M users/s against 8 K through the host loop), so ``model.train(...)``'s default
    ``valid_func=ValidFunc(evaluate)`` no longer spends its time copying score matrices.  Everything else -- other metrics, host
    samplers, models without the device path, ``model.device_metrics = False`` -- takes the reference's loop
    (:func:`evaluate_host`); the two agree to 1e-12 (``test_evaluate_device_equals_host_evaluate``).  A subclass that overrides
    ``predict`` always takes the host loop (its override is what the reference would call).  Ties: among EQUAL scores the device
    top-k keeps the lower item index where numpy's argpartition order is unspecified; metrics differ only if a held-out item ties
    with a non-held-out one exactly at rank k.

    :class:`rectorch_amd.models.SVAE` has a device route of its own: an ``SVAE_Sampler(is_training=False, pack=N > 1)`` yields
    packs of users, ``predict`` scores a pack in one call (every user's last step only) and the same top-k kernel ranks it against
    the sampler's resident held-out matrix, under the same conditions (the four metrics, the framework's ``predict``,
    ``model.device_metrics``).  With ``pack=1`` it is the reference's loop, one user at a time.

    A conditioned sampler constructed with ``resident=True`` (:class:`rectorch_amd.models.CMultiVAE`) is scored and ranked the same
    way, batch by batch as the device builds them, under the same conditions; per-user arrays come in loader order with the dropped
    examples absent, as the host loop leaves them out.

    :class:`rectorch_amd.models.EASE` and :class:`rectorch_amd.models.ADMM_Slim` (whose ``predict`` takes user ids, so the
    reference cannot evaluate them this way) are evaluated by FOLD-IN with a ``DataSampler(test_tr, test_te, ...)``: the loader's
    ``tr`` rows times the item-item matrix (``model.score_rows``), the same rows excluded from the ranking.  Under the conditions
    above -- with ``score_rows`` in the place of ``predict`` -- nothing of width ``n_items`` leaves the device: per chunk of users
    ``rtx_ease_scores`` / ``rtx_admm_scores`` into one float64 scratch buffer, the float64 selection kernel, and the list-metrics
    kernel (``rtx_list_metrics``) against the ``te`` rows.  Everything else is ``score_rows`` to numpy and :class:`Metrics`.
    :class:`rectorch_amd.models.ItemKNN` and :class:`rectorch_amd.models.WMF` take the same route with ``rtx_knn_scores`` /
    ``rtx_wmf_scores`` (WMF's fold-in is one user solve against the item factors, then ``x_u . y_j``)."""
    if _is_item_item(model):
        return _evaluate_item_item(model, test_loader, metric_list)
    if (_device_route(model, test_loader, metric_list) or _svae_route(model, test_loader, metric_list)
            or _cond_route(model, test_loader, metric_list)):
        return evaluate_device(model, test_loader, metric_list)
    return evaluate_host(model, test_loader, metric_list)


def _device_route(model, test_loader, metric_list):
    """whether :func:`evaluate` / :func:`one_plus_random` hand ``model`` and ``test_loader`` to their device route"""
    return bool(getattr(model, "device_metrics", True) and _topk_plan(test_loader, metric_list) is not None
                and hasattr(model, "_predict_tuple") and _predict_is_ours(model))


def _predict_is_ours(model):
    """True when ``model.predict`` is the framework's own method.  The reference always scores through ``model.predict``
    (evaluation.py:100-109), so a user subclass that overrides it (re-ranking, filtering, an ensemble) must be evaluated through
    that override: the device route calls the engine's scorer directly and would silently bypass it."""
    return _method_is_ours(model, "predict")


def _method_is_ours(model, name):
    """the rule of :func:`_predict_is_ours` for the method ``name`` (``score_rows`` of the item-item models)"""
    fn = getattr(type(model), name, None)
    mod = getattr(fn, "__module__", "") or ""
    return name not in vars(model) and mod.startswith(__name__.rsplit(".", 1)[0] + ".")


def _rank_metrics_plan(metric_list):
    """[(metric, name, k)] when every metric is one of ``ndcg / recall / hit / mrr @ k`` with 1 <= k <= 1024, else None"""
    parsed = []
    for m in metric_list:
        name, _, k = m.partition("@")
        if name.lower() not in RANK_METRICS or not k.isdigit() or not 1 <= int(k) <= DEVICE_TOPK_MAX:
            return None
        parsed.append((m, name.lower(), int(k)))
    return parsed or None


def _svae_plan(model, test_loader, metric_list):
    """[(metric, name, k)] when ``test_loader`` is an :class:`SVAE_Sampler` yielding evaluation packs (``is_training`` off,
    ``pack > 1``), ``model.predict`` is the framework's own and takes such packs, and the top-k kernel knows every metric; else None"""
    from .samplers import SVAE_Sampler
    from .models import SVAE
    if not (isinstance(test_loader, SVAE_Sampler) and not test_loader.is_training and test_loader.pack > 1
            and test_loader.dict_data_te is not None and isinstance(model, SVAE) and _predict_is_ours(model)):
        return None
    return _rank_metrics_plan(metric_list)


def _svae_route(model, test_loader, metric_list):
    """whether :func:`evaluate` scores and ranks the packs of an SVAE loader on the device"""
    return bool(getattr(model, "device_metrics", True) and _svae_plan(model, test_loader, metric_list) is not None)


def _cond_plan(model, test_loader, metric_list):
    """[(metric, name, k)] when ``test_loader`` is a conditioned sampler with ``resident=True`` (its batches are pairs of small
    CSR matrices the device builds), ``model.predict`` is the framework's own and the top-k kernel knows every metric; else None"""
    from .samplers import is_resident_conditioned
    if not (is_resident_conditioned(test_loader) and hasattr(model, "_predict_tuple") and _predict_is_ours(model)):
        return None
    return _rank_metrics_plan(metric_list)


def _cond_route(model, test_loader, metric_list):
    """whether :func:`evaluate` scores and ranks the batches of a resident conditioned loader on the device"""
    return bool(getattr(model, "device_metrics", True) and _cond_plan(model, test_loader, metric_list) is not None)


def _evaluate_svae_packs(model, test_loader, parsed, metric_list):
    """SVAE on the device: per pack of users ``predict`` (every user's last step, one call) and the top-k kernel on the pack's rows
    of the resident held-out matrix; ONE device -> host copy after the last pack.  Per-user arrays in loader order.

    A resident conditioned loader takes the same loop: it yields ``(input rows, target rows)`` pairs of :class:`RowBatch`, LAZILY --
    a batch lives in a ring of device buffers and is consumed before the ring comes round -- ``predict`` scores the input rows
    (-inf at their item columns) and the kernel ranks them against the batch's target matrix.  Dropped examples are absent, as the
    host loop leaves them out."""
    from .engine import topk_metrics
    ks = sorted({k for _, _, k in parsed})
    rank_metrics = any(name in ("hit", "mrr") for _, name, _ in parsed)
    extra = {"rank_metrics": True} if rank_metrics else {}
    out = _PerUserResults(metric_list)
    per_pack = []
    for pack, heldout in test_loader:
        scores = model.predict(pack)[0]                  # [users of the pack, n_items], -inf at each user's own input items
        per_pack.append(torch.stack(topk_metrics(scores, heldout.tr, heldout.rows, ks, **extra)))
    if not per_pack:
        return out.finish()
    res = torch.cat(per_pack, dim=2).cpu().numpy()       # [metric kinds, cut-offs, users]
    res = dict(zip(RANK_METRICS, res))
    if rank_metrics:
        res["hit"] = res["hit"].astype(bool)             # Metrics.hit_at_k: a bool array
    out.add({m: res[name][ks.index(k)] for m, name, k in parsed})
    return out.finish()


def _device_plan(test_loader, metric_list):
    """[(metric, name, k)] when every metric can be computed by the device kernel on this loader, else None"""
    from .samplers import DataSampler
    parsed = []
    for m in metric_list:
        name, _, k = m.partition("@")
        if name.lower() not in ("ndcg", "recall") or not k.isdigit() or not 1 <= int(k) <= DEVICE_TOPK_MAX:
            return None
        parsed.append((m, name.lower(), int(k)))
    resident = isinstance(test_loader, DataSampler) and test_loader.resident and test_loader.sparse_data_te is not None
    return parsed if (parsed and resident) else None


RANK_METRICS = ("ndcg", "recall", "hit", "mrr")


def _topk_plan(test_loader, metric_list):
    """[(metric, name, k)] when every metric is one of ``ndcg / recall / hit / mrr @ k`` with 1 <= k <= 1024 and the loader is a
    device-resident :class:`DataSampler` with held-out rows, else None.  (:func:`_device_plan` is the planner of the nDCG / Recall
    kernel alone, before hit@k and mrr@k ran on the device.)"""
    from .samplers import DataSampler
    parsed = []
    for m in metric_list:
        name, _, k = m.partition("@")
        if name.lower() not in RANK_METRICS or not k.isdigit() or not 1 <= int(k) <= DEVICE_TOPK_MAX:
            return None
        parsed.append((m, name.lower(), int(k)))
    resident = isinstance(test_loader, DataSampler) and test_loader.resident and test_loader.sparse_data_te is not None
    return parsed if (parsed and resident) else None


def evaluate_device(model, test_loader, metric_list):
    r"""Same contract and same values as :func:`evaluate`, computed on the MI355X.

    With a device-resident :class:`rectorch_amd.samplers.DataSampler` holding the ``(tr, heldout)`` matrices,
    ``predict`` takes the sparse rows directly and the ``ndcg@k`` / ``recall@k`` metrics are computed by a top-k
    kernel on the GPU, so per batch only ``len(metric_list) x B`` doubles cross PCIe instead of the ``[B, n_items]``
    score matrix (40 MB per 500 users at the ml-20m shape) followed by a host ``argpartition``.  ``hit@k`` and ``mrr@k`` come
    from the same kernel (two more reductions over the ranked relevances; hit@k as a ``bool`` array, as ``Metrics.hit_at_k``).
    Usable as a validation function: ``model.train(..., valid_func=ValidFunc(evaluate_device))``.  Anything it cannot do on the
    device (other metrics, k > 1024, a host sampler) goes through :func:`evaluate`.  The packs of an
    ``SVAE_Sampler(is_training=False, pack=N > 1)`` are scored by ``SVAE.predict`` and ranked by the same kernel.
    """
    from .engine import topk_metrics, RowBatch
    parsed = _svae_plan(model, test_loader, metric_list)
    if parsed is None:
        parsed = _cond_plan(model, test_loader, metric_list)
    if parsed is not None:
        return _evaluate_svae_packs(model, test_loader, parsed, metric_list)
    parsed = _topk_plan(test_loader, metric_list)
    if parsed is None:
        return evaluate_host(model, test_loader, metric_list)
    ks = sorted({k for _, _, k in parsed})
    rank_metrics = any(name in ("hit", "mrr") for _, name, _ in parsed)       # the kernel's second instantiation: only when asked
    extra = {"rank_metrics": True} if rank_metrics else {}
    out = _PerUserResults(metric_list)
    # Round 6, after the selection kernel went from 41 to 20 us per 500 users: the GPU is busy ~103 us per batch
    # (profiles/r6_eval_timeline.txt) and the host needed as long to get through one iteration of a Python loop (predict -> ctypes ->
    # eight launches, the selection kernel's call, two allocations).  When `predict` is the framework's own (a user's override must be
    # what scores, as in the reference) the WHOLE loop is one C call -- rtx_engine_evaluate_topk enqueues forward, -inf scatter and
    # selection kernel batch after batch into one scores buffer and one [cut-off][user] metrics buffer -- and ONE device -> host copy
    # follows.  (Measured and dropped earlier this round: the selection kernel on a second stream under the next forward -- both
    # contend for the same CUs; and the Python loop with reused buffers: +-1 %.)
    batches = list(test_loader.iter_rows())
    if not batches:
        return out.finish()
    # (VAE(VAE_net) has _variant "gvae": its predict samples z with one seed per batch and returns sigmoid probabilities, so it
    #  takes the per-batch loop below -- the one-call loop scores in eval mode without either)
    # (a CDAE_net too: its batches carry user ids, which the one-call loop does not take -- predict() per batch, ranked on the device)
    fast = (_predict_is_ours(model) and hasattr(model, "_predict_engine") and getattr(model, "_variant", None) in ("vae", "dae")
            and not getattr(model, "_is_cdae", False)
            and all(isinstance(model.network._as_input(rb), RowBatch) and rb.tr is batches[0].tr and rb.te is batches[0].te for rb in batches))
    import os
    if os.environ.get("RTX_EVAL_SIMPLE_LOOP"): fast = False          # (measurement: the per-batch Python loop)
    if fast:
        eng = model._predict_engine(max(len(rb) for rb in batches))
        offsets = np.concatenate([[0], np.cumsum([len(rb) for rb in batches])])
        base, off0 = batches[0].rows._base, batches[0].rows.storage_offset()
        if (base is not None and base.dim() == 1 and base.is_contiguous()
                and all(rb.rows._base is base and rb.rows.storage_offset() == off0 + int(o) for rb, o in zip(batches, offsets))):
            rows = base[off0:off0 + int(offsets[-1])]        # the sampler's batches are consecutive slices of ONE row-number tensor
        else:
            rows = torch.cat([rb.rows for rb in batches])
        res = eng.evaluate_topk(batches[0].tr, batches[0].te, rows, offsets, ks, **extra)
    else:
        per_batch = []
        for rb in batches:
            scores = model.predict(rb)[0]                # HIP forward on the sparse rows, -inf at the train items
            per_batch.append(topk_metrics(scores, rb.te, rb.rows, ks, **extra))
        # ONE device -> host copy for the whole loader (the per-batch .cpu() of round 3 was a host sync per 500 users)
        res = [torch.cat([p[i] for p in per_batch], dim=1) for i in range(len(per_batch[0]))]
    res = dict(zip(RANK_METRICS, (t.cpu().numpy() for t in res)))
    res["hit"] = res["hit"].astype(bool) if rank_metrics else None           # Metrics.hit_at_k: a bool array
    out.add({m: res[name][ks.index(k)] for m, name, k in parsed})
    return out.finish()


def one_plus_random(model, test_loader, metric_list, r=1000):
    r"""One-plus-random evaluation (reference evaluation.py:113-178): for every held-out positive of every
    user, rank it against ``r`` random items the user has not interacted with in the held-out part and
    compute the metrics on those ``r + 1`` scores (the positive is column 0).  Raises ``ValueError`` when
    fewer than ``r`` negatives exist.

    Where :func:`evaluate` takes its device route (a device-resident :class:`DataSampler` with held-out rows, the framework's own
    ``predict``, ``model.device_metrics``, every metric ``ndcg / recall / hit / mrr @ k``) this is :func:`one_plus_random_device`:
    the same draws from Python's ``random`` state, the same values.  Everything else is the reference's loop
    (:func:`one_plus_random_host`).  ``EASE`` / ``ADMM_Slim`` are scored by fold-in of the loader's ``tr`` rows (see
    :func:`evaluate`): on the device under the same conditions, else ``score_rows`` to numpy and the reference's loop."""
    if _is_item_item(model) or _device_route(model, test_loader, metric_list):        # (item-item models: it picks their route)
        return one_plus_random_device(model, test_loader, metric_list, r=r)
    return one_plus_random_host(model, test_loader, metric_list, r=r)


def one_plus_random_host(model, test_loader, metric_list, r=1000):
    r"""The reference's one-plus-random loop as it is written (evaluation.py:113-178): the scores and held-out rows of every batch
    copied to the host, the negatives of every positive drawn by ``random.sample`` from a sorted Python list, a ``[contests, r + 1]``
    array scored by :class:`Metrics`."""
    return _opr_host_loop(((_predict_numpy(model, data_tr), _to_numpy(heldout)) for data_tr, heldout in test_loader), metric_list, r)


def _opr_host_loop(batches, metric_list, r):
    """:func:`one_plus_random_host` on ``(scores, heldout)`` pairs of host arrays, one per batch of the loader"""
    out = _PerUserResults(metric_list)
    for scores, heldout in batches:
        all_items = set(range(heldout.shape[1]))
        contests = []
        for u, i in zip(*heldout.nonzero()):                 # one contest per held-out positive, in row-major order
            negatives = sorted(all_items - set(heldout[u].nonzero()[0].tolist()))
            contests.append(scores[u][[i] + random.sample(negatives, r)])   # the same draws as the reference's sampler
        pred = np.array(contests)
        truth = np.zeros_like(pred)
        truth[:, 0] = 1
        out.add(Metrics.compute(pred, truth, metric_list))
    return out.finish()


def _opr_metrics(rank, r, name, k):
    """One metric of :func:`one_plus_random` from the positive's 0-based place ``rank`` among its ``r + 1`` scores: with the positive
    the only relevant column, ``Metrics.*_at_k`` on the ``[contests, r + 1]`` matrix reduce to these (IDCG = discount[0] = 1,
    recall's denominator = 1), in the dtypes they return."""
    kk = min(k, r + 1)
    inside = rank < kk
    if name == "ndcg":
        discount = 1. / np.log2(np.arange(2, kk + 2))                  # the array Metrics.ndcg_at_k builds
        return np.where(inside, discount[np.minimum(rank, kk - 1)], 0.)
    if name == "recall":
        return inside.astype(np.float32) / np.ones(len(rank), np.int64)   # float32 hits / int64 count: float64, as Metrics.recall_at_k
    if name == "hit":
        return inside
    return np.where(inside, 1. / (1. + rank), 0.)                          # mrr


def one_plus_random_device(model, test_loader, metric_list, r=1000):
    r"""Same contract, same draws and same values as :func:`one_plus_random`, with the scores left on the MI355X.

    Per batch: the negatives of every held-out positive are drawn on the host by ``rtx_opr_draw`` -- Python's ``random.sample``
    reproduced index for index from ``random.getstate()``, whose state it advances exactly as the reference's loop does -- and
    uploaded as item ids; ``predict`` scores the batch on the device (train items at -inf) and ``rtx_opr_rank`` counts, per contest,
    the negatives scoring above the positive (one wavefront each).  Only that rank, 4 bytes per contest, comes back; the metrics
    are functions of it.  The host draws batch i + 1 while the device scores batch i.  Ties: the positive (column 0) ranks first
    among equal scores -- the lower-column rule of the top-k kernel -- where numpy's argpartition order is unspecified.

    Anything it cannot do on the device (another loader, other metrics) goes through :func:`one_plus_random_host`.

    ``EASE`` / ``ADMM_Slim``: the loader's ``tr`` rows are folded in (``rtx_ease_scores`` / ``rtx_admm_scores``, float64, the rows' own
    items at -inf) and ranked by ``rtx_opr_rank_f64``; the draws are the same call."""
    from .engine import opr_draw, opr_rank
    if _is_item_item(model):
        parsed = _item_item_plan(model, test_loader, metric_list)
        if parsed is None:
            return _opr_host_loop(_item_item_host_batches(model, test_loader), metric_list, r)
        solver = model._solver

        def score_batch(rb):
            return solver.scores(rb.rows, rb.tr, X=rb.tr, mask_rows=rb.rows)
    else:
        parsed = _topk_plan(test_loader, metric_list)
        if parsed is None or test_loader.sparse_data_tr.shape[1] != test_loader.sparse_data_te.shape[1]:
            return one_plus_random_host(model, test_loader, metric_list, r=r)

        def score_batch(rb):
            return model.predict(rb)[0]              # HIP forward on the sparse rows, -inf at the train items
    te = test_loader.sparse_data_te.tocsr().copy()
    te.sum_duplicates()                    # (sorted, summed: the held-out row CsrMatrix uploads, dense.nonzero() of the host loop)
    held = (np.ascontiguousarray(te.indptr, dtype=np.int64), np.ascontiguousarray(te.indices, dtype=np.int32),
            np.ascontiguousarray(te.data, dtype=np.float32))
    n_items = te.shape[1]
    batches = list(test_loader.iter_rows())
    rows_host = torch.cat([rb.rows for rb in batches]).cpu().numpy() if batches else np.zeros(0, np.int32)
    ranks, lo = [], 0
    for rb in batches:
        rows = rows_host[lo:lo + len(rb)]
        lo += len(rb)
        crow, citem, draws, short = opr_draw(held, rows, n_items, r, pin=True)   # (the device is still busy with the last batch)
        if short >= 0:
            raise ValueError("Sample larger than population or is negative")     # random.sample's, at the same point of its state
        if len(crow) == 0:
            raise IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")   # the host loop's, too
        dev = rb.rows.device
        crow, citem, draws = (t.to(dev, non_blocking=True) for t in (crow, citem, draws))
        scores = score_batch(rb)
        assert scores.shape[1] == n_items, (scores.shape, n_items)
        ranks.append(opr_rank(scores, crow, citem, draws))
    rank = torch.cat(ranks).cpu().numpy() if ranks else np.zeros(0, np.int32)
    assert (rank >= 0).all()
    out = _PerUserResults(metric_list)
    if len(rank):
        out.add({m: _opr_metrics(rank, r, name, k) for m, name, k in parsed})
    return out.finish()


# ---- the fold-in family: every models._FoldInModel (the item-item models EASE, ADMM_Slim, ItemKNN; WMF, whose fold-in is one solve per user)
ITEM_ITEM_EVAL_CHUNK = 1024      # users per pass of the device route: one [chunk, n_items] float64 scratch buffer


def _is_item_item(model):
    from .models import _FoldInModel
    return isinstance(model, _FoldInModel)


def _item_item_plan(model, test_loader, metric_list):
    """[(metric, name, k)] when :func:`evaluate` / :func:`one_plus_random` keep an item-item model's scores on the device: a
    device-resident :class:`DataSampler` with held-out rows of the model's width, the four metrics with k <= 1024,
    ``model.device_metrics`` not False, a fitted solver and the framework's own ``score_rows`` (a subclass's override must be what
    scores: the rule of :func:`_predict_is_ours`); else None"""
    parsed = _topk_plan(test_loader, metric_list)
    solver = getattr(model, "_solver", None)
    if (parsed is None or solver is None or not getattr(model, "device_metrics", True) or not _method_is_ours(model, "score_rows")
            or test_loader.sparse_data_tr.shape[1] != solver.n_items or test_loader.sparse_data_te.shape[1] != solver.n_items):
        return None
    return parsed


def _item_item_host_batches(model, test_loader):
    """``(scores, heldout)`` host arrays per batch of ``test_loader``: ``model.score_rows`` on the batch's ``tr`` rows (fold-in,
    their own items at -inf) and the dense held-out rows.  A resident :class:`DataSampler` is walked by row numbers and its scipy
    matrices are sliced; any other loader's dense batches are made sparse again."""
    from scipy.sparse import csr_matrix
    from .samplers import DataSampler
    if isinstance(test_loader, DataSampler) and test_loader.resident and test_loader.sparse_data_te is not None:
        tr, te = test_loader.sparse_data_tr.tocsr(), test_loader.sparse_data_te.tocsr()
        for rb in test_loader.iter_rows():
            ids = rb.rows.cpu().numpy()
            yield np.asarray(model.score_rows(tr[ids])), te[ids].toarray()
        return
    for data_tr, heldout in test_loader:
        yield np.asarray(model.score_rows(csr_matrix(_to_numpy(data_tr)))), _to_numpy(heldout)


def _evaluate_item_item(model, test_loader, metric_list, chunk=ITEM_ITEM_EVAL_CHUNK):
    """:func:`evaluate` for EASE / ADMM_Slim / ItemKNN / WMF.  Device route (:func:`_item_item_plan`): the loader's users in chunks of
    ``chunk`` -- their ``tr`` rows times the item-item matrix into ONE float64 scratch buffer, the float64 selection kernel with the same rows
    as its exclusion, the list-metrics kernel against their ``te`` rows -- and ONE device -> host copy at the end.  Otherwise the
    host loop: ``score_rows`` to numpy, :class:`Metrics`."""
    parsed = _item_item_plan(model, test_loader, metric_list)
    out = _PerUserResults(metric_list)
    if parsed is None:
        for scores, heldout in _item_item_host_batches(model, test_loader):
            out.add(Metrics.compute(scores, heldout, metric_list))
        return out.finish()
    from .engine import list_metrics, topk_items
    batches = list(test_loader.iter_rows())
    if not batches:
        return out.finish()
    solver, tr, te = model._solver, batches[0].tr, batches[0].te
    rows = torch.cat([rb.rows for rb in batches]) if len(batches) > 1 else batches[0].rows
    n, n_items = int(rows.numel()), solver.n_items
    ks = sorted({k for _, _, k in parsed})
    kmax = min(ks[-1], n_items)
    scratch = torch.empty((min(chunk, n), n_items), dtype=torch.float64, device=rows.device)
    items = torch.empty((min(chunk, n), kmax), dtype=torch.int32, device=rows.device)
    parts = []
    for lo in range(0, n, chunk):
        ids = rows[lo:lo + chunk]
        m = int(ids.numel())
        scores = solver.scores(ids, None, out=scratch[:m], X=tr)
        topk_items(scores, kmax, tr, ids, want_scores=False, out=(items[:m], None))
        parts.append(torch.stack(list_metrics(items[:m], te, ids, ks)))
    res = dict(zip(RANK_METRICS, torch.cat(parts, dim=2).cpu().numpy()))      # [metric kinds, cut-offs, users]
    res["hit"] = res["hit"].astype(bool)                                         # Metrics.hit_at_k: a bool array
    out.add({m: res[name][ks.index(k)] for m, name, k in parsed})
    return out.finish()


# ---- metrics of ready-made lists ----------------------------------------------------------------------------------------------
def _lists_plan(metric_list):
    parsed = []
    for m in metric_list:
        name, _, k = m.partition("@")
        if name.lower() not in RANK_METRICS or not k.isdigit() or int(k) < 1:
            raise ValueError("metrics_from_lists knows ndcg@k, recall@k, hit@k and mrr@k (k >= 1), got '%s'" % m)
        parsed.append((m, name.lower(), int(k)))
    return parsed


def _metrics_from_lists_host(items, heldout, parsed, rows=None, chunk=4096):
    """numpy half of :func:`metrics_from_lists`: :class:`Metrics`' definitions with the ranked list in the place of the
    argpartition + argsort, ``kk = min(k, K)`` (an id outside the matrix has relevance 0)"""
    items = np.asarray(items)
    if items.ndim != 2 or items.shape[1] < 1:
        raise ValueError("items must be [users, K >= 1], got %s" % (items.shape,))
    n, K = items.shape
    te = heldout.tocsr()
    if rows is not None:
        te = te[np.asarray(rows).astype(np.int64)]
    if te.shape[0] < n:
        raise ValueError("%d lists for %d held-out rows" % (n, te.shape[0]))
    n_items = te.shape[1]
    res = {m: [] for m, _, _ in parsed}
    for lo in range(0, n, chunk):
        it = items[lo:lo + chunk].astype(np.int64)
        truth = te[lo:lo + len(it)].toarray().astype(np.float64)
        valid = (it >= 0) & (it < n_items)
        rel = np.where(valid, np.take_along_axis(truth, np.where(valid, it, 0), axis=1), 0.)     # [users, K], rank order
        total, n_pos = truth.sum(axis=1).astype(np.int64), (truth > 0).sum(axis=1)
        for m, name, k in parsed:
            kk = min(k, K)
            top = rel[:, :kk]
            with np.errstate(divide="ignore", invalid="ignore"):
                if name == "ndcg":
                    discount = 1. / np.log2(np.arange(2, kk + 2))
                    ideal_cum = np.concatenate(([0.], np.cumsum(discount)))
                    val = (top * discount).sum(axis=1) / ideal_cum[np.minimum(total, kk)]
                elif name == "recall":
                    val = (top > 0).sum(axis=1).astype(np.float32) / np.minimum(kk, n_pos)
                elif name == "hit":
                    val = (top > 0).any(axis=1)
                else:
                    hit = top != 0
                    val = np.where(hit.any(axis=1), 1. / (1. + np.argmax(hit, axis=1)), 0.)
            res[m].append(val)
    return {m: np.concatenate(v) if v else np.zeros(0) for m, v in res.items()}


def metrics_from_lists(items, heldout, metric_list, rows=None):
    r"""``ndcg@k`` / ``recall@k`` / ``hit@k`` / ``mrr@k`` of ready-made ranked lists -- ``items [users, K]``, every row best first,
    what :func:`recommend` and the models' ``recommend`` / ``recommend_rows`` return -- against the users' held-out rows.  Returns
    ``dict metric -> per-user numpy array`` in the dtypes of :func:`evaluate` (hit@k as ``bool``).  The definitions are
    :class:`Metrics`' with the list in the place of the sort: a cut-off above ``K`` counts the ``K`` ranked items, so the lists
    must be at least as long as the largest ``k`` for the values to be :class:`Metrics`' own.

    Device int32 lists with a resident :class:`rectorch_amd.engine.CsrMatrix` go to the list-metrics kernel
    (``rtx_list_metrics``; one copy of ``len(metric_list) x users`` doubles comes back); host arrays with a scipy matrix are
    computed in numpy.  ``rows``: the held-out row of every list (default: list b belongs to row b)."""
    from .engine import CsrMatrix, list_metrics
    parsed = _lists_plan(metric_list)
    if isinstance(heldout, CsrMatrix):
        if not (torch.is_tensor(items) and items.is_cuda):
            raise TypeError("a resident CsrMatrix takes device lists (an int32 device tensor); host lists take a scipy matrix")
        if rows is not None:
            rows = torch.as_tensor(rows).to(items.device)
        ks = sorted({k for _, _, k in parsed})
        res = dict(zip(RANK_METRICS, torch.stack(list_metrics(items.to(torch.int32), heldout, rows, ks)).cpu().numpy()))
        res["hit"] = res["hit"].astype(bool)
        return {m: res[name][ks.index(k)] for m, name, k in parsed}
    if torch.is_tensor(items):
        items = items.cpu().numpy()
    if torch.is_tensor(rows):
        rows = rows.cpu().numpy()
    return _metrics_from_lists_host(items, heldout, parsed, rows)


# ---- top-N recommendation lists ---------------------------------------------------------------------------------------------
def _lexsort_topk(scores, k):
    """The first ``min(k, n_items)`` items of every row of the host array ``scores`` and their scores: score descending, item id
    ascending among equal scores (``-0.0 == +0.0``), ``-inf`` last -- ``np.lexsort((ids, -scores))``."""
    scores = np.asarray(scores)
    n = scores.shape[1]
    ids = np.broadcast_to(np.arange(n), scores.shape)
    order = np.lexsort((ids, -scores), axis=1)[:, :max(min(int(k), n), 0)]
    return order.astype(np.int32), np.take_along_axis(scores, order, axis=1)


def _predict_scores(model, data_tr, remove_train):
    """``model.predict`` on one batch of a loader, ``remove_train`` passed through; the resident-rows shortcut of the device sampler
    survives the reshape (as in :func:`evaluate_host`)"""
    from .engine import RowBatch, SvaeEvalPack, tag_rows, tagged_rows
    if isinstance(data_tr, (RowBatch, SvaeEvalPack)):
        return model.predict(data_tr, remove_train=remove_train)[0]
    data_tensor = data_tr.view(data_tr.shape[0], -1)
    rows = tagged_rows(data_tr)
    if rows is not None:
        tag_rows(data_tensor, rows)
    if getattr(data_tr, "_rtx_users", None) is not None:       # (a host sampler's user ids, for a CDAE_net)
        data_tensor._rtx_users = data_tr._rtx_users
    return model.predict(data_tensor, remove_train=remove_train)[0]


def _cat_lists(parts, device, score_dtype=torch.float32):
    if not parts:
        return (torch.empty((0, 0), dtype=torch.int32, device=device), torch.empty((0, 0), dtype=score_dtype, device=device))
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def recommend_host(model, test_loader, k=100, remove_train=True):
    r"""What a user of the reference writes to get recommendation lists: ``model.predict`` per batch, the ``[B, n_items]`` scores
    copied to the host, ``numpy.lexsort((ids, -scores))``.  Same contract and same values as :func:`recommend` (its fallback for
    ``k > 1024`` and ``model.device_metrics = False``, and the yardstick of its tests); the two tensors live where ``predict``'s
    scores do."""
    parts, dev = [], torch.device("cpu")
    for data_tr, _ in test_loader:
        scores = _predict_scores(model, data_tr, remove_train)
        if torch.is_tensor(scores):
            dev = scores.device
            scores = scores.cpu().numpy()
        items, vals = _lexsort_topk(scores, k)
        parts.append((torch.from_numpy(items), torch.from_numpy(np.ascontiguousarray(vals))))
    items, vals = _cat_lists(parts, "cpu")
    return items.to(dev), vals.to(dev)


def _recommend_route(model, test_loader, k):
    """Which way :func:`recommend` goes: ``"host"`` (:func:`recommend_host`: ``k`` above the kernel's 1024, or
    ``model.device_metrics = False``), ``"engine"`` (the whole loader in one C call: a device-resident :class:`DataSampler`, the
    framework's own ``predict``, a Mult-VAE / Mult-DAE engine) or ``"batch"`` (``model.predict`` per batch, the selection kernel
    on its scores: everything else, a subclass that overrides ``predict`` included)."""
    from .samplers import DataSampler
    from .engine import TOPK_ITEMS_MAX
    if int(k) < 1:
        raise ValueError("recommend: k must be >= 1, got %s" % (k,))
    if int(k) > TOPK_ITEMS_MAX or not getattr(model, "device_metrics", True):
        return "host"
    resident = isinstance(test_loader, DataSampler) and test_loader.resident
    if (resident and _predict_is_ours(model) and hasattr(model, "_predict_engine")
            and getattr(model, "_variant", None) in ("vae", "dae") and not getattr(model, "_is_cdae", False)):
        return "engine"      # (a CDAE_net's batches carry user ids, which the one-call loop does not take: "batch")
    return "batch"


def recommend(model, test_loader, k=100, remove_train=True):
    r"""The ``k`` best items of every user of ``test_loader`` and their scores, computed on the MI355X: ``(items, scores)``, device
    tensors of shape ``[users, min(k, n_items)]`` in loader order, ``items`` int32, ``scores`` in the dtype ``model.predict``
    scores in.  A list is ordered by score descending, item id ascending among equal scores; with ``remove_train`` the items of the
    user's input row rank as :math:`-\infty` (and fill the tail of the list, by ascending id, when fewer than ``k`` others exist).

    Routes (they mirror :func:`evaluate`'s): a device-resident :class:`DataSampler` with the framework's own ``predict`` of a
    Mult-VAE / Mult-DAE model is ONE C call for the whole loader (``rtx_engine_recommend``: forward and selection kernel batch
    after batch, the train items excluded inside the selection); every other loader and model -- ``VAE(VAE_net)``, ``CMultiVAE``
    and its conditioned samplers, the packs of an ``SVAE_Sampler(is_training=False, pack=N)``, host samplers, a subclass that
    overrides ``predict`` -- is ``model.predict(batch, remove_train=...)`` followed by the selection kernel on the returned
    scores (``rtx_topk_items``); ``k > 1024`` and ``model.device_metrics = False`` take :func:`recommend_host`."""
    from .engine import topk_items, RowBatch
    route = _recommend_route(model, test_loader, k)
    if route == "host":
        return recommend_host(model, test_loader, k=k, remove_train=remove_train)
    ours_resident = route == "engine" or (route == "batch" and _predict_is_ours(model) and hasattr(model, "_predict_tuple")
                                          and hasattr(test_loader, "iter_rows") and getattr(test_loader, "resident", False))
    if ours_resident and route != "engine":
        # (lazily: the batches of a resident conditioned sampler live in a ring of device buffers and are consumed as they come)
        loader = ((rb, None) for rb in test_loader.iter_rows())
    elif ours_resident:
        batches = list(test_loader.iter_rows())      # row numbers only: nothing dense is gathered for the framework's own predict
        if batches and all(isinstance(model.network._as_input(rb), RowBatch) and rb.tr is batches[0].tr for rb in batches):
            eng = model._predict_engine(max(len(rb) for rb in batches))
            offsets = np.concatenate([[0], np.cumsum([len(rb) for rb in batches])])
            rows = torch.cat([rb.rows for rb in batches]) if len(batches) > 1 else batches[0].rows
            return eng.recommend(batches[0].tr, rows.contiguous(), offsets, k, remove_train=remove_train)
        loader = ((rb, None) for rb in batches)
    else:
        loader = test_loader
    parts = []
    for data_tr, _ in loader:
        scores = _predict_scores(model, data_tr, remove_train)
        scores = torch.as_tensor(scores)
        if scores.dtype not in (torch.float32, torch.float64):
            scores = scores.float()
        parts.append(topk_items(scores.to("cuda"), k))
    return _cat_lists(parts, "cuda")
