"""CPU: the host half of the resident conditioned samplers -- the item -> condition bitmap and the per-epoch batch plan -- and the
unchanged default of the ``resident`` keyword (no device needed)."""
import inspect

import numpy as np
import pytest
from scipy.sparse import csr_matrix

from conftest import load_golden


def _g11():
    g = load_golden("g11_conditioned_samplers")
    iid2cids = {}
    for i, c in zip(g["iid2cids_items"], g["iid2cids_conds"]):
        iid2cids.setdefault(int(i), []).append(int(c))
    return g, iid2cids, csr_matrix(g["tr"]), csr_matrix(g["te"]), int(g["n_cond"])


@pytest.mark.parametrize("n_cond", [1, 31, 32, 33, 70])
def test_bitmap_packing_equals_dense_restatement(n_cond):
    from rectorch_amd.samplers import pack_conditions
    rng = np.random.RandomState(n_cond)
    n_items = 75                                 # three words of "any" bits, the last one partly used
    dense = rng.rand(n_items, n_cond) < 0.3
    dense[3, :] = False                          # an item with an empty condition list
    dense[64, :] = False
    dense[5, :] = True                           # an item with every condition
    dense[74, :] = True
    iid2cids = {i: [int(c) for c in np.nonzero(dense[i])[0]] for i in range(n_items)}
    del iid2cids[64]                             # ... and one without an entry at all: no condition either
    bits, any_ = pack_conditions(iid2cids, n_cond, n_items)
    W = (n_cond + 31) // 32
    assert bits.dtype == np.uint32 and bits.shape == (n_items, W)
    assert any_.dtype == np.uint32 and any_.shape == ((n_items + 31) // 32,)
    c = np.arange(W * 32)
    unpacked = ((bits[:, c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)
    assert np.array_equal(unpacked[:, :n_cond], dense)
    assert not unpacked[:, n_cond:].any()        # no bit beyond the last condition
    i = np.arange(len(any_) * 32)
    any_unpacked = ((any_[i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)
    assert np.array_equal(any_unpacked[:n_items], dense.any(axis=1))
    assert not any_unpacked[n_items:].any()


def test_bitmap_packing_rejects_ids_out_of_range():
    from rectorch_amd.samplers import pack_conditions
    with pytest.raises(ValueError):
        pack_conditions({0: [3]}, 3, 4)
    with pytest.raises(ValueError):
        pack_conditions({4: [0]}, 3, 4)


def _keep_flags(examples, te, iid2cids):
    """numpy restatement of the samplers' filter: an example is kept when its target row has an item valid under its condition"""
    te = te.tocsr()
    keep = []
    for r, c in examples:
        items = te.indices[te.indptr[r]:te.indptr[r + 1]]
        keep.append(any((len(iid2cids[int(i)]) > 0) if c < 0 else (c in iid2cids[int(i)]) for i in items))
    return np.array(keep, dtype=bool)


def test_batch_plan_follows_the_reference_batches_g11():
    """example order, kept ids per batch and skipped batches for the fixture's seeds: the row counts are the reference's"""
    from rectorch_amd.samplers import (BalancedConditionedDataSampler, ConditionedDataSampler, EmptyConditionedDataSampler,
                                       plan_batches)
    g, iid2cids, tr, te, nc = _g11()

    def check(prefix, sampler, te_m, filtered, seed):
        keep = _keep_flags(sampler.examples, te_m, iid2cids) if filtered else np.ones(sampler._n_examples(), dtype=bool)
        np.random.seed(seed)
        order = sampler._example_order()
        np.random.seed(seed)
        want = list(range(sampler._n_examples()))
        if sampler.shuffle:
            np.random.shuffle(want)
        assert order == want                                   # the host samplers' own draw
        plan = plan_batches(order, sampler.batch_size, keep)
        ref_rows = [g["%s_tr_%d" % (prefix, i)].shape[0] for i in range(int(g["%s_n_batches" % prefix]))]
        assert [len(b) for b in plan] == [n for n in ref_rows if n]        # a batch emptied by the drop is skipped
        assert sum(len(b) for b in plan) == int(keep.sum())
        bs, flat = sampler.batch_size, np.concatenate(plan)
        assert np.array_equal(flat, np.array([e for e in order if keep[e]]))   # order kept, only dropped examples missing
        for b in plan:                                          # the cut into batches is made BEFORE the drop
            pos = [order.index(int(e)) for e in b]
            assert b.dtype == np.int32 and len({p // bs for p in pos}) == 1
        return keep, ref_rows

    s1 = ConditionedDataSampler(iid2cids, nc, tr, te, batch_size=7, shuffle=True)
    keep, ref_rows = check("cds", s1, te, True, 5)
    assert (~keep).sum() > 0 and sum(ref_rows) < len(s1.examples)          # the fixture does drop examples
    np.random.seed(6)
    s2 = BalancedConditionedDataSampler(iid2cids, nc, tr, None, batch_size=9, subsample=0.3)
    assert np.array_equal(s2.examples, g["bal_examples"])
    check("bal", s2, tr, True, 7)
    s3 = EmptyConditionedDataSampler(nc, tr, te, batch_size=10, shuffle=True)
    check("emp", s3, te, False, 8)


def test_plan_skips_a_batch_emptied_by_the_drop():
    from rectorch_amd.samplers import plan_batches
    keep = np.array([1, 1, 0, 0, 0, 1, 0, 1, 1], dtype=bool)
    plan = plan_batches(list(range(9)), 2, keep)               # cuts: [0 1] [2 3] [4 5] [6 7] [8]
    assert [b.tolist() for b in plan] == [[0, 1], [5], [7], [8]]
    assert plan_batches([], 4, np.zeros(0, dtype=bool)) == []
    assert plan_batches([0, 1], 4, np.zeros(2, dtype=bool)) == []


def test_resident_is_the_last_keyword_and_off_by_default():
    from rectorch_amd.samplers import (BalancedConditionedDataSampler, ConditionedDataSampler, EmptyConditionedDataSampler,
                                       is_resident_conditioned)
    for cls in (ConditionedDataSampler, BalancedConditionedDataSampler, EmptyConditionedDataSampler):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[-1].name == "resident" and params[-1].default is False, cls
    g, iid2cids, tr, te, nc = _g11()
    # without the keyword: the host sampler, to the bit what the reference's batches are (no device is touched)
    np.random.seed(5)
    s1 = ConditionedDataSampler(iid2cids, nc, tr, te, batch_size=7, shuffle=True)
    assert s1.resident is False and not is_resident_conditioned(s1)
    n = 0
    for i, (a, b) in enumerate(s1):
        assert np.array_equal(a.numpy(), g["cds_tr_%d" % i]) and np.array_equal(b.numpy(), g["cds_te_%d" % i])
        n += 1
    assert n == int(g["cds_n_batches"])
    np.random.seed(8)
    s3 = EmptyConditionedDataSampler(nc, tr, te, batch_size=10, shuffle=True)
    assert s3.resident is False and not is_resident_conditioned(s3)
    for i, (a, b) in enumerate(s3):
        assert np.array_equal(a.numpy(), g["emp_tr_%d" % i]) and np.array_equal(b.numpy(), g["emp_te_%d" % i])


def test_resident_needs_a_device():
    import torch
    from rectorch_amd import _lib
    from rectorch_amd.samplers import EmptyConditionedDataSampler, is_resident_conditioned
    g, iid2cids, tr, te, nc = _g11()
    if torch.cuda.is_available():
        assert is_resident_conditioned(EmptyConditionedDataSampler(nc, tr, te, batch_size=10, resident=True))
        return
    with pytest.raises(_lib.RtxError):
        EmptyConditionedDataSampler(nc, tr, te, batch_size=10, resident=True)
