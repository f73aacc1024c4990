"""GPU: the resident conditioned samplers (``resident=True``) -- batches built on the device by csrc/cond_rows.hip -- against the
host samplers that ``tests/golden/g11_conditioned_samplers.npz`` pins to the reference, and through every consumer."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_native_path():
    from rectorch_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()          # raises if librectorch_hip.so is missing: no fallback


def _g11():
    g = load_golden("g11_conditioned_samplers")
    iid2cids = {}
    for i, c in zip(g["iid2cids_items"], g["iid2cids_conds"]):
        iid2cids.setdefault(int(i), []).append(int(c))
    return g, iid2cids, csr_matrix(g["tr"]), csr_matrix(g["te"]), int(g["n_cond"])


def _dense(rb):
    """a RowBatch over slot matrices -> host float32 array"""
    return rb.tr.gather_dense(rb.rows).cpu().numpy()


class _CsrLayout(C.Structure):      # struct rtx_csr (csrc/rtx_kernels.h): the test reads a slot's arrays back through it
    _fields_ = [("indptr", C.c_void_p), ("indices", C.c_void_p), ("values", C.c_void_p), ("n_rows", C.c_int64), ("nnz", C.c_int64),
                ("n_cols", C.c_int32), ("max_row_len", C.c_int32)]


def _device_array(ptr, n, typestr):
    class _Alias:
        pass
    al = _Alias()
    al.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}
    return torch.as_tensor(al, device="cuda").cpu().numpy().copy()


def _check_slot_csr(m, dense):
    """the slot matrix ``m`` read back: indptr non-decreasing and ending at the number of entries written, column ids strictly
    ascending inside every row and inside the matrix, values (or implicit ones) equal to ``dense``"""
    lay = _CsrLayout.from_address(m.handle.value)
    n = dense.shape[0]
    assert lay.n_rows == n and lay.n_cols == dense.shape[1]
    indptr = _device_array(lay.indptr, n + 1, "<i8")
    assert indptr[0] == 0 and np.all(np.diff(indptr) >= 0)
    nnz = int(np.count_nonzero(dense))
    assert indptr[-1] == nnz == lay.nnz
    if nnz == 0:
        return
    indices = _device_array(lay.indices, nnz, "<i4")
    values = _device_array(lay.values, nnz, "<f4") if lay.values else np.ones(nnz, np.float32)
    assert (lay.values is None) == bool(m.binary)
    for b in range(n):
        cols = indices[indptr[b]:indptr[b + 1]]
        assert np.all(np.diff(cols) > 0) and (len(cols) == 0 or (cols[0] >= 0 and cols[-1] < dense.shape[1]))
        assert np.array_equal(cols, np.nonzero(dense[b])[0])
        assert np.array_equal(values[indptr[b]:indptr[b + 1]], dense[b][cols])


# ---- 1. g11 parity ----------------------------------------------------------------------------------------------------------------
def test_resident_samplers_match_reference_g11():
    from rectorch_amd.samplers import BalancedConditionedDataSampler, ConditionedDataSampler, EmptyConditionedDataSampler
    g, iid2cids, tr, te, nc = _g11()

    def check(prefix, sampler):
        assert sampler.resident
        n = 0
        for i, (a, b) in enumerate(sampler):
            want_tr, want_te = g["%s_tr_%d" % (prefix, i)], g["%s_te_%d" % (prefix, i)]
            got_tr, got_te = _dense(a), _dense(b)
            assert got_tr.shape == want_tr.shape and got_te.shape == want_te.shape, (prefix, i)
            assert np.array_equal(got_tr, want_tr) and np.array_equal(got_te, want_te), (prefix, i)
            assert np.array_equal(a.te.gather_dense(a.rows).cpu().numpy(), want_te)      # the pair's first element carries the target too
            n += 1
        assert n == int(g["%s_n_batches" % prefix])

    np.random.seed(5)
    s1 = ConditionedDataSampler(iid2cids, nc, tr, te, batch_size=7, shuffle=True, resident=True)
    assert np.array_equal(s1.examples, g["cds_examples"]) and len(s1) == int(g["cds_len"])
    check("cds", s1)
    np.random.seed(6)
    s2 = BalancedConditionedDataSampler(iid2cids, nc, tr, None, batch_size=9, subsample=0.3, resident=True)
    assert np.array_equal(s2.examples, g["bal_examples"]) and len(s2) == int(g["bal_len"])
    np.random.seed(7)
    check("bal", s2)
    np.random.seed(8)
    s3 = EmptyConditionedDataSampler(nc, tr, te, batch_size=10, shuffle=True, resident=True)
    check("emp", s3)


# ---- 2. edge shapes -----------------------------------------------------------------------------------------------------------------
U_EDGE, I_EDGE = 40, 300
N_LO, N_HI = 150, 299       # items [150, 299) have NO condition; item 299 has every condition; items [0, 150) have one or two


def _edge_data(n_cond, valued):
    """U = 40 users over 300 items.  tr rows 0..4 have 1, 63, 64, 65 and 130 entries (wave-pass boundaries of the copy); te rows
    0..11 are (1, 64, 129 entries) x (everything / nothing / only the first / only the last entry survives the filter);
    user 12 has only items without a condition: its single example (12, -1) is dropped."""
    rng = np.random.RandomState(100 + n_cond)
    iid2cids = {i: sorted({i % n_cond, (i * 7) % n_cond}) for i in range(N_LO)}
    iid2cids.update({i: [] for i in range(N_LO, N_HI)})
    iid2cids[N_HI] = list(range(n_cond))
    tr_rows, te_rows = [], []
    for u in range(U_EDGE):
        tr_rows.append(np.sort(rng.choice(N_HI + 1, size=rng.randint(2, 40), replace=False)))
        te_rows.append(np.sort(rng.choice(N_HI + 1, size=rng.randint(1, 30), replace=False)))
    for u, n in enumerate((1, 63, 64, 65, 130)):
        tr_rows[u] = np.sort(rng.choice(N_LO, size=n, replace=False))
    u = 0
    for n in (1, 64, 129):
        cond_items = np.sort(rng.choice(N_LO, size=n, replace=False))
        bare_items = np.sort(rng.choice(np.arange(N_LO, N_HI), size=n, replace=False))
        te_rows[u] = cond_items                                                  # everything survives (unconditioned example)
        te_rows[u + 1] = bare_items                                              # nothing survives
        te_rows[u + 2] = np.concatenate([cond_items[:1], bare_items[:n - 1]])    # only the first entry
        te_rows[u + 3] = np.concatenate([bare_items[:n - 1], [N_HI]])            # only the last entry
        u += 4
    tr_rows[12] = np.array([N_LO + 3, N_LO + 70, N_HI - 1])
    te_rows[12] = np.array([N_LO + 5, N_HI - 2])

    def mat(rows):
        indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
        idx = np.concatenate(rows)
        data = rng.randint(1, 6, size=len(idx)).astype(np.float64) if valued else np.ones(len(idx))
        return csr_matrix((data, idx, indptr), shape=(len(rows), I_EDGE))
    return iid2cids, mat(tr_rows), mat(te_rows)


def _host_batches(sampler):
    """the host sampler's batches as arrays, the ones its drop emptied left out (the resident sampler skips them)"""
    for a, b in sampler:
        if a.shape[0]:
            yield a.numpy(), b.numpy()


def _compare_with_host(res, host, n_cond, seed=11):
    """every batch of ``res`` (resident) bit-equal to the host sampler's; both draw their order from numpy's global generator, so
    the host's epoch is taken first and the generator seeded again for the resident one.  Returns the batch sizes."""
    n, sizes = 0, []
    np.random.seed(seed)
    host_it = iter(list(_host_batches(host)))
    np.random.seed(seed)
    for a, b in res:
        want_tr, want_te = next(host_it)
        got_tr, got_te = _dense(a), _dense(b)
        assert got_tr.shape == want_tr.shape and got_te.shape == want_te.shape
        assert np.array_equal(got_tr, want_tr) and np.array_equal(got_te, want_te), n
        assert got_tr.shape[1] == I_EDGE + n_cond and np.all(got_te.any(axis=1))
        _check_slot_csr(a.tr, got_tr)
        _check_slot_csr(b.tr, got_te)
        sizes.append(len(a))
        n += 1
    assert next(host_it, None) is None
    return sizes


@pytest.mark.parametrize("n_cond", [1, 32, 33, 70])
def test_edge_shapes_equal_the_host_sampler(n_cond):
    from rectorch_amd.engine import CondBuilder, CsrMatrix, RowBatch
    from rectorch_amd.samplers import ConditionedDataSampler, pack_conditions, plan_batches
    for valued in (False, True):
        iid2cids, tr, te = _edge_data(n_cond, valued)
        host0 = ConditionedDataSampler(iid2cids, n_cond, tr, te, batch_size=7, shuffle=False)
        ex = host0.examples
        # the crafted rows are there: lengths at the wave-pass boundaries, and the four filter outcomes at every length
        assert [tr[u].nnz for u in range(5)] == [1, 63, 64, 65, 130] and [te[u].nnz for u in range(0, 12, 4)] == [1, 64, 129]
        assert [tuple(e) for e in ex if e[0] == 12] == [(12, -1)]
        # batch 7 (a last short batch; shuffled and in order), batch 1 (every dropped example is a batch that becomes empty)
        for bs, shuffle, users in ((7, False, U_EDGE), (7, True, U_EDGE), (1, False, 13)):
            if bs == 1 and n_cond not in (1, 33):
                continue                                             # (one user per batch is slow on the host side: two widths do)
            trs, tes = tr[:users], te[:users]
            np.random.seed(11)
            host = ConditionedDataSampler(iid2cids, n_cond, trs, tes, batch_size=bs, shuffle=shuffle)
            np.random.seed(11)
            res = ConditionedDataSampler(iid2cids, n_cond, trs, tes, batch_size=bs, shuffle=shuffle, resident=True)
            assert res._cond.te.binary == (not valued) and res._cond.tr.binary == (not valued)
            keep = res._keep
            assert not keep[[i for i, e in enumerate(res.examples) if e[0] in (1, 5, 9, 12)]].any()     # "nothing survives" + user 12
            assert len(res.examples) % bs != 0 or bs == 1                                                 # the last cut is a short one
            for u in (2, 3, 6, 7, 10, 11):                                                                # first / last entry only
                assert res._cond.target_len[[i for i, e in enumerate(res.examples) if e[0] == u and e[1] == -1]].tolist() == [1]
            for u, n in ((0, 1), (4, 64), (8, 129)):                                                      # everything survives
                assert res._cond.target_len[[i for i, e in enumerate(res.examples) if e[0] == u and e[1] == -1]].tolist() == [n]
            sizes = _compare_with_host(res, host, n_cond)
            assert sum(sizes) == int(keep.sum()) < len(res.examples)
            if bs == 1:
                assert len(sizes) < len(res)                         # batches emptied by the drop were skipped
            else:
                assert min(sizes) < bs and sizes[-1] < bs            # short batches, the last one among them
        # batch 300 in a builder sized for 512: the scan kernel carries across its rounds of 256.  Once against the te rows
        # (heavy drops: short batches), once with the input rows as targets (hardly a drop: batches above 256 rows)
        ex, all_sizes = host0.examples, []
        for te_m in (te, None):
            host = ConditionedDataSampler(iid2cids, n_cond, tr, te_m, batch_size=300, shuffle=False)
            mtr = CsrMatrix(tr)
            cb = CondBuilder(mtr, None if te_m is None else CsrMatrix(te_m), n_cond, pack_conditions(iid2cids, n_cond, I_EDGE),
                             ex[:, 0], ex[:, 1], max_batch=512)
            plan = plan_batches(list(range(len(ex))), 300, cb.target_len != 0)
            rows = torch.arange(512, dtype=torch.int32, device="cuda")

            def built():
                for ids in plan:
                    a, t = cb.build(torch.from_numpy(ids).to("cuda"), len(ids), int(cb.in_len[ids].sum()), int(cb.target_len[ids].sum()))
                    yield RowBatch(a, t, rows[:len(ids)]), RowBatch(t, None, rows[:len(ids)])
            all_sizes += _compare_with_host(built(), host, n_cond)
        if n_cond > 1:
            assert max(all_sizes) > 256, all_sizes                   # more than one round of the scan


# ---- 3. training equality -----------------------------------------------------------------------------------------------------------
def make_cvae(cond, enc, dec, p, sd, **kw):
    from rectorch_amd.nets import CMultiVAE_net
    from rectorch_amd.models import CMultiVAE
    net = CMultiVAE_net(cond, list(dec), list(enc), dropout=p)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return net, CMultiVAE(net, **kw)


def _small_problem(seed, U=40, I=96, C_=3, with_te=False):
    rng = np.random.RandomState(seed)
    tr = csr_matrix((rng.rand(U, I) < 0.15).astype(np.float32))
    tr = csr_matrix(tr + csr_matrix((np.ones(U), (np.arange(U), np.arange(U) % I)), shape=(U, I)))
    tr.data[:] = 1.0
    te = None
    if with_te:
        te = csr_matrix((rng.rand(U, I) < 0.1).astype(np.float32))
        te = csr_matrix(te + csr_matrix((np.ones(U), (np.arange(U), (np.arange(U) * 5 + 1) % I)), shape=(U, I)))
        te.data[:] = 1.0
    iid2cids = {i: sorted({int(i % C_), int((i * 7) % C_)}) for i in range(I)}
    return tr, te, iid2cids


def _params(net):
    return [p.detach().cpu().numpy().copy() for p in net._param_list()]


def test_training_on_resident_batches_equals_sparse_batches_fp32():
    """the engine sees the same CSR content from a slot as from the sparse=True pair: float32 losses and parameters are EQUAL"""
    from rectorch_amd.samplers import ConditionedDataSampler
    from rectorch_amd.utils.hashinit import hash_state_dict
    U, I, C_, H, L = 40, 96, 3, 24, 8
    tr, _, iid2cids = _small_problem(4)
    sd = hash_state_dict([I + C_, H, L], [L, H, I], "vae", 5, 1.0)
    losses, after_batches, after_epoch = {}, {}, {}
    for kind in ("sparse", "resident"):
        kw = {"sparse": True} if kind == "sparse" else {"resident": True}
        torch.manual_seed(123)
        net, model = make_cvae(C_, [I, H, L], [L, H, I], 0.0, sd, beta=0.1, numerics="fp32")
        sampler = ConditionedDataSampler(iid2cids, C_, tr, None, batch_size=16, shuffle=False, **kw)
        losses[kind] = [model.train_batch(data, gt) for data, gt in sampler]
        after_batches[kind] = _params(net)
        torch.manual_seed(321)
        net, model = make_cvae(C_, [I, H, L], [L, H, I], 0.0, sd, beta=0.1, numerics="fp32")
        model.train_epoch(1, sampler, verbose=0)             # resident: the back-to-back branch, look-ahead inside
        after_epoch[kind] = _params(net)
    print("losses sparse  ", losses["sparse"])
    print("losses resident", losses["resident"])
    for d in (after_batches, after_epoch):
        print("max |param diff|", max(float(np.max(np.abs(a - b))) for a, b in zip(d["sparse"], d["resident"])))
    assert len(losses["resident"]) == len(losses["sparse"]) > 3
    assert losses["resident"] == losses["sparse"]
    for d in (after_batches, after_epoch):
        for a, b in zip(d["sparse"], d["resident"]):
            assert np.array_equal(a, b)


def _ring_run(tr, te, iid2cids, C_, dims, sd, B, prefetch, epochs=1):
    from rectorch_amd.samplers import ConditionedDataSampler
    I, H, L = dims
    net, model = make_cvae(C_, [I, H, L], [L, H, I], 0.5, sd, beta=0.2, numerics="bf16")
    net.to("cuda")
    model.prefetch_batches = prefetch
    np.random.seed(3)
    torch.manual_seed(17)
    sampler = ConditionedDataSampler(iid2cids, C_, tr, te, batch_size=B, shuffle=True, resident=True)
    for ep in range(1, epochs + 1):
        model.train_epoch(ep, sampler, verbose=0)
    loss_sum = float(model._rtx.loss_buf[0].item())      # the last step's loss (train_epoch has read and cleared the running sum)
    eng = net._rtx_engines["bf16"]
    return _params(net), loss_sum, (eng.get_option("prefetch_hits"), eng.get_option("prefetch_issued")), sampler


def test_ring_reuse_prefetch_on_and_off_are_bit_identical_bf16():
    """train_epoch in bf16 over more than 2 S + 1 batches, with and without the engine's batch prefetch: bit-identical parameters.
    Once at the shapes of the float32 test, once with first / last layers large enough for the two-stream step, where the batch
    after the next one is built while the side stream may still gather the next one -- the case the ring of slots is sized for."""
    from rectorch_amd.engine import COND_SLOTS
    from rectorch_amd.samplers import plan_batches
    from rectorch_amd.utils import synth_interactions
    from rectorch_amd.utils.hashinit import hash_state_dict
    cases = []
    tr, _, iid2cids = _small_problem(4)
    cases.append((tr, None, iid2cids, 3, (96, 24, 8), 16, False))
    I, H, L, B, C_ = 3000, 600, 200, 192, 3
    X = synth_interactions(600, I, mu=3.5, sigma=0.9, dmax=I // 2, seed=13)
    cases.append((X, None, {i: sorted({i % C_, (i * 7) % C_}) for i in range(I)}, C_, (I, H, L), B, True))
    for tr, te, iid2cids, C_, dims, B, big in cases:
        sd = hash_state_dict([dims[0] + C_, dims[1], dims[2]], [dims[2], dims[1], dims[0]], "vae", 5, 1.0)
        res = {}
        for prefetch in (True, False):
            res[prefetch] = _ring_run(tr, te, iid2cids, C_, dims, sd, B, prefetch, epochs=2)
        sampler = res[True][3]
        n_batches = len(plan_batches(list(range(len(sampler.examples))), B, sampler._keep))
        assert n_batches >= 2 * COND_SLOTS + 1, n_batches                      # every slot is reused
        print("batches", n_batches, "prefetch (hits, issued)", res[True][2], res[False][2], "last losses", res[True][1], res[False][1])
        assert res[False][2] == (0, 0)
        if big:
            assert res[True][2] == (2 * (n_batches - 1),) * 2, res[True][2]    # every step but an epoch's first started from a prefetched image
        assert res[True][1] == res[False][1]
        for a, b in zip(res[True][0], res[False][0]):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- 4. public consumers ------------------------------------------------------------------------------------------------------------
def test_resident_samplers_through_the_public_consumers(tmp_path):
    from rectorch_amd.evaluation import evaluate, recommend
    from rectorch_amd.models import CMultiVAE
    from rectorch_amd.samplers import ConditionedDataSampler, EmptyConditionedDataSampler
    from rectorch_amd.utils.hashinit import hash_state_dict
    U, I, C_, H, L = 48, 96, 3, 24, 8
    tr, te, iid2cids = _small_problem(5, U=U, with_te=True)
    sd = hash_state_dict([I + C_, H, L], [L, H, I], "vae", 5, 1.0)
    metrics = ["ndcg@10", "recall@5", "hit@3", "mrr@10"]
    # every item has the one condition i % 3: without the items of condition 2 among the targets every example (r, 2) is dropped
    te_drop = csr_matrix(te.multiply(csr_matrix(np.tile(np.arange(I) % C_ != 2, (U, 1)).astype(np.float64))))
    te_drop.eliminate_zeros()

    class Reranked(CMultiVAE):
        def predict(self, x, remove_train=True):
            out = super().predict(x, remove_train)
            return (out[0] * 0.5,) + tuple(out[1:])

    res = {}
    for resident in (False, True):
        kw = {"resident": True} if resident else {"sparse": False}
        torch.manual_seed(7)
        net, model = make_cvae(C_, [I, H, L], [L, H, I], 0.0, sd, beta=0.1, numerics="fp32")
        train_s = ConditionedDataSampler(iid2cids, C_, tr, None, batch_size=16, shuffle=False, **kw)
        valid_s = EmptyConditionedDataSampler(C_, tr, te, batch_size=16, shuffle=False, **kw)
        cond_s = ConditionedDataSampler(iid2cids, C_, tr, te_drop, batch_size=16, shuffle=False, **kw)  # drops examples
        model.train(train_s, valid_s, "ndcg@10", num_epochs=2, best_path=str(tmp_path / ("cmvae_res_%d.pth" % resident)), verbose=1)
        out = {"params": _params(net)}
        out["ev"] = evaluate(model, valid_s, metrics)
        out["ev_cond"] = evaluate(model, cond_s, metrics)
        out["rec"] = [t.cpu().numpy() for t in recommend(model, valid_s, k=10)]
        out["rec_cond"] = [t.cpu().numpy() for t in model.recommend(cond_s, k=10)]
        model.device_metrics = False                         # the host loop
        out["ev_host"] = evaluate(model, cond_s, metrics)
        out["rec_host"] = [t.cpu().numpy() for t in recommend(model, cond_s, k=10)]
        sub = Reranked(net, beta=0.1, numerics="fp32")       # an overridden predict must be what scores: the host loop again
        out["ev_sub"] = evaluate(sub, cond_s, metrics)
        out["rec_sub"] = [t.cpu().numpy() for t in recommend(sub, cond_s, k=10)]
        res[resident] = out
    n_cond_rows = len(res[False]["ev_cond"]["ndcg@10"])
    assert U < n_cond_rows < len(cond_s.examples)            # dropped examples are absent, as in the host loop
    for key in ("ev", "ev_cond", "ev_host", "ev_sub"):
        for m in metrics:
            a, b = res[True][key][m], res[False][key][m]
            assert a.shape == b.shape == ((U,) if key == "ev" else (n_cond_rows,)) and a.dtype == b.dtype, (key, m)
            np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-7, err_msg="%s %s" % (key, m))
    for m in metrics:                                        # the device route agrees with the host loop of the same loader
        np.testing.assert_allclose(res[True]["ev_cond"][m], res[True]["ev_host"][m], rtol=1e-6, atol=1e-7)
    for key in ("rec", "rec_cond", "rec_host", "rec_sub"):
        assert np.array_equal(res[True][key][0], res[False][key][0]), key
        np.testing.assert_allclose(res[True][key][1], res[False][key][1], rtol=1e-6, atol=1e-7)
    assert np.array_equal(res[True]["rec_cond"][0], res[True]["rec_host"][0])
    for a, b in zip(res[True]["params"], res[False]["params"]):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-7)


def test_evaluate_takes_the_device_route_for_resident_loaders():
    from rectorch_amd import evaluation
    from rectorch_amd.samplers import EmptyConditionedDataSampler
    from rectorch_amd.utils.hashinit import hash_state_dict
    U, I, C_, H, L = 48, 96, 3, 24, 8
    tr, te, iid2cids = _small_problem(5, U=U, with_te=True)
    net, model = make_cvae(C_, [I, H, L], [L, H, I], 0.0, hash_state_dict([I + C_, H, L], [L, H, I], "vae", 5, 1.0), numerics="fp32")
    res_s = EmptyConditionedDataSampler(C_, tr, te, batch_size=16, shuffle=False, resident=True)
    host_s = EmptyConditionedDataSampler(C_, tr, te, batch_size=16, shuffle=False)
    assert evaluation._cond_route(model, res_s, ["ndcg@10", "mrr@3"])
    assert not evaluation._cond_route(model, host_s, ["ndcg@10"])
    assert not evaluation._cond_route(model, res_s, ["ndcg@2000"]) and not evaluation._cond_route(model, res_s, ["precision@5"])
    model.device_metrics = False
    assert not evaluation._cond_route(model, res_s, ["ndcg@10"])


def test_data_parallel_plan_refuses_a_resident_conditioned_sampler():
    from rectorch_amd import _lib
    from rectorch_amd.samplers import ConditionedDataSampler
    from rectorch_amd.utils.hashinit import hash_state_dict
    U, I, C_, H, L = 40, 96, 3, 24, 8
    tr, _, iid2cids = _small_problem(4)
    net, model = make_cvae(C_, [I, H, L], [L, H, I], 0.0, hash_state_dict([I + C_, H, L], [L, H, I], "vae", 5, 1.0), numerics="fp32")
    model._rtx.reducer = object()                            # any attached plan
    sampler = ConditionedDataSampler(iid2cids, C_, tr, None, batch_size=16, shuffle=False, resident=True)
    with pytest.raises(_lib.RtxError, match="data-parallel"):
        model.train_epoch(1, sampler, verbose=0)


# ---- 5. stale batch -----------------------------------------------------------------------------------------------------------------
def test_a_batch_kept_past_the_ring_raises():
    from rectorch_amd import _lib
    from rectorch_amd.engine import COND_SLOTS
    from rectorch_amd.samplers import ConditionedDataSampler
    from rectorch_amd.utils.hashinit import hash_state_dict
    U, I, C_, H, L = 40, 96, 3, 24, 8
    tr, _, iid2cids = _small_problem(4)
    net, model = make_cvae(C_, [I, H, L], [L, H, I], 0.0, hash_state_dict([I + C_, H, L], [L, H, I], "vae", 5, 1.0), numerics="fp32")
    sampler = ConditionedDataSampler(iid2cids, C_, tr, None, batch_size=16, shuffle=False, resident=True)
    batches = list(sampler.iter_rows())
    assert len(batches) > COND_SLOTS
    with pytest.raises(_lib.RtxError, match="batch overwritten"):
        model.train_batch(batches[0], None)
    with pytest.raises(_lib.RtxError, match="batch overwritten"):
        _dense(batches[0])
    assert np.isfinite(model.train_batch(batches[-1], None))             # the newest batches are intact
    assert _dense(batches[-COND_SLOTS]).shape[1] == I + C_


# ---- 6. exports and lifetime ---------------------------------------------------------------------------------------------------------
def test_cond_symbols_are_exported_and_bound():
    from rectorch_amd import _lib
    src = open(os.path.join(ROOT, "include", "rectorch_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    syms = sorted(set(re.findall(r"\b(rtx_cond_[a-z0-9_]+)\s*\(", src)))
    assert len(syms) >= 4 and {"rtx_cond_create", "rtx_cond_destroy"} <= set(syms)
    raw = C.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), s
        assert s in _lib.SIGNATURES and getattr(_lib.lib(), s).argtypes == _lib.SIGNATURES[s][1], s
    assert _lib.lib().rtx_abi_version() == 8


def test_create_destroy_does_not_grow_and_null_bitmap_leaves_targets_unfiltered():
    from rectorch_amd import _lib
    from rectorch_amd.engine import CondBuilder, CsrMatrix
    from rectorch_amd.samplers import pack_conditions
    iid2cids, tr, te = _edge_data(33, True)
    mtr, mte = CsrMatrix(tr), CsrMatrix(te)
    ex_rows = np.arange(U_EDGE, dtype=np.int32)
    ex_conds = np.full(U_EDGE, -1, dtype=np.int32)
    bitmap = pack_conditions(iid2cids, 33, I_EDGE)
    first = None
    for i in range(50):
        cb = CondBuilder(mtr, mte, 33, bitmap if i % 2 else None, ex_rows, ex_conds, max_batch=64)
        ids = torch.arange(U_EDGE, dtype=torch.int32, device="cuda")
        a, t = cb.build(ids, U_EDGE)
        got = t.gather_dense(ids).cpu().numpy()
        del cb, a, t
        if first is None:
            first = torch.cuda.memory_allocated()
        assert torch.cuda.memory_allocated() <= first, i
    # a NULL bitmap: every example keeps its whole target row, values as stored; the input row gets no condition entry for c = -1
    cb = CondBuilder(mtr, mte, 33, None, ex_rows, ex_conds, max_batch=64)
    assert np.array_equal(cb.target_len, np.diff(te.indptr)) and np.array_equal(cb.in_len, np.diff(tr.indptr))
    ids = torch.arange(U_EDGE, dtype=torch.int32, device="cuda")
    a, t = cb.build(ids, U_EDGE)
    assert np.array_equal(t.gather_dense(ids).cpu().numpy(), te.toarray().astype(np.float32))
    want_in = np.concatenate([tr.toarray(), np.zeros((U_EDGE, 33))], axis=1).astype(np.float32)
    assert np.array_equal(a.gather_dense(ids).cpu().numpy(), want_in)
    # the same examples filtered: only items with a condition survive
    cb2 = CondBuilder(mtr, mte, 33, bitmap, ex_rows, ex_conds, max_batch=64)
    has = np.array([len(iid2cids[i]) > 0 for i in range(I_EDGE)])
    a2, t2 = cb2.build(ids, U_EDGE)
    assert np.array_equal(t2.gather_dense(ids).cpu().numpy(), (te.toarray() * has).astype(np.float32))
    # bad arguments are refused on the host, nothing is launched
    with pytest.raises(_lib.RtxError):
        CondBuilder(mtr, mte, 33, None, np.array([U_EDGE], np.int32), np.array([-1], np.int32), max_batch=8)      # row out of range
    with pytest.raises(_lib.RtxError):
        CondBuilder(mtr, mte, 33, None, np.array([0], np.int32), np.array([33], np.int32), max_batch=8)           # condition out of range
    with pytest.raises(_lib.RtxError):
        CondBuilder(mtr, mte, 33, None, ex_rows, ex_conds, max_batch=8, n_slots=2)                                 # too few slots
    with pytest.raises(_lib.RtxError):
        cb.build(ids, 65)                                                                                          # beyond max_batch
