"""GPU: hit@k and mrr@k on the device, and one-plus-random evaluation on the device.

* hit@k / mrr@k from the top-k kernel (k_topk_metrics<NV, true>) against a float64 restatement of the reference's metrics
  (rectorch/metrics.py:231-238, 272-285) at cut-offs 1 .. 1024, one width per kernel route (20108 burst, 20480 widest burst,
  20484 streamed, 4099 streamed and not a multiple of 4, 700 fewer items than K), through the one-call route, the per-batch route
  (RTX_EVAL_SIMPLE_LOOP) and the host loop.  Held-out rows hold ratings -- negative ones included, where mrr's `!= 0` and hit's
  `> 0` differ -- stored zeros, and empty rows; the `ties` cases put thousands of equal scores at the bound (the radix fall-back).
* one_plus_random: the device route (one_plus_random_device) against the reference's loop (one_plus_random_host) with the same
  seed: equal values and dtypes, and random.getstate() equal afterwards, for r = 1, 20 and 1000 on widths on both sides of
  random.sample's setsize; the ValueError of a user with too few negatives; users without held-out items; a held-out item that is
  also a train item (its score is -inf: a tie, compared with the stated rule -- the positive first -- instead of numpy's order).
"""
import random

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

from test_gpu_parity import EVAL_KS, _eval_oracle, _eval_rows, make_dae, make_vae

pytestmark = pytest.mark.gpu

NAMES = ("ndcg", "recall", "hit", "mrr")


def _rank_oracle(scores, held, ks):
    """hit@k and mrr@k in float64, items ordered by score descending, then id ascending (the kernel's tie rule); which results
    are determined is _eval_oracle's `det` / `det_all` (every tie group they look at is uniform in relevance)"""
    U, I = scores.shape
    ids = np.arange(I)
    hit, mrr, mrr_gt0 = np.zeros((len(ks), U), bool), np.zeros((len(ks), U)), np.zeros((len(ks), U))
    for u in range(U):
        relv = held[u, np.lexsort((ids, -scores[u].astype(np.float64)))]
        for q, k in enumerate(ks):
            top = relv[:min(k, I)]
            hit[q, u] = (top > 0).any()
            nz, gt = np.flatnonzero(top != 0), np.flatnonzero(top > 0)
            mrr[q, u] = 1. / (1. + nz[0]) if nz.size else 0.
            mrr_gt0[q, u] = 1. / (1. + gt[0]) if gt.size else 0.      # what a `> 0` test would give: must differ somewhere
    return hit, mrr, mrr_gt0


RANK_CASES = [("vae", "fp32", I, False) for I in (20108, 20480, 20484, 4099, 700)]
RANK_CASES += [("dae", "fp32", 20108, True), ("vae", "fp32", 20484, True)]


@pytest.mark.parametrize("variant,numerics,I,ties", RANK_CASES, ids=["%s-%d%s" % (v, I, "-ties" if t else "") for v, n, I, t in RANK_CASES])
def test_hit_mrr_vs_float64_oracle(variant, numerics, I, ties, monkeypatch):
    from rectorch_amd.utils import hash_state_dict
    from rectorch_amd.samplers import DataSampler
    from rectorch_amd.evaluation import evaluate, evaluate_host, evaluate_device
    from rectorch_amd import engine as E
    U, H, L = 48, 64, 32
    tr, te = _eval_rows(I, U, seed=I + 7 * ties + 1, ties=ties)
    rng = np.random.RandomState(I)
    if not ties:
        te.data = rng.choice([-1.0, 0.5, 3.0, 5.0], size=te.nnz)       # ratings; -1: relevant for mrr (!= 0), not for hit (> 0)
        te.data[te.indptr[10]:te.indptr[12]] = 0.0                       # stored zeros in two held-out rows
        te.data[te.indptr[12]] = -1.0                                    # (user 12: a negative rating at its first entry)
        for u in range(U):                   # (a row whose ratings sum below -1 has no IDCG length: not a case of these metrics)
            seg = te.data[te.indptr[u]:te.indptr[u + 1]]
            if seg.sum() < 0:
                seg[seg < 0] = 0.5
    sd = hash_state_dict([I, H, L], [L, H, I], variant, 53 + I, bias_std=0.5)
    if ties:
        sd["dec_layers.1.weight"][:] = 0
        b = np.zeros(I, sd["dec_layers.1.bias"].dtype)
        b[0::24] = 2.0
        b[1::24] = b[2::24] = 1.0
        b[3::24] = -0.5
        sd["dec_layers.1.bias"] = b
    make = make_vae if variant == "vae" else make_dae
    net, model = make([I, H, L], [L, H, I], 0.5, sd, predict_numerics=numerics)
    smp = DataSampler(tr, te, batch_size=20, shuffle=False)
    mets = ["%s@%d" % (m, k) for k in EVAL_KS for m in NAMES]

    scores = np.concatenate([model.predict(rb)[0].cpu().numpy() for rb in smp.iter_rows()])
    if not ties:                             # users 1-3 (600 held-out items): the best-scored one rated -1
        for u in (1, 2, 3):
            a, b = te.indptr[u], te.indptr[u + 1]
            te.data[a + np.argmax(scores[u, te.indices[a:b]])] = -1.0
        smp = DataSampler(tr, te.copy(), batch_size=20, shuffle=False)
    held = te.toarray().astype(np.float64)
    nd, rc, det, det_all = _eval_oracle(scores, held, EVAL_KS)
    hit, mrr, mrr_gt0 = _rank_oracle(scores, held, EVAL_KS)
    for q in range(len(EVAL_KS)):
        assert det[q].mean() >= 0.9 and det_all[q].mean() >= 0.9, (EVAL_KS[q], det[q].mean(), det_all[q].mean())
    if not ties:                             # a -1 rating ranked above every positive one: `!= 0` and `> 0` disagree
        assert ((mrr != mrr_gt0) & det).any()

    calls, loops = [], []
    one_call, per_batch = E.Engine.evaluate_topk, E.topk_metrics
    monkeypatch.setattr(E.Engine, "evaluate_topk", lambda self, *a, **k: calls.append(k) or one_call(self, *a, **k))
    monkeypatch.setattr(E, "topk_metrics", lambda *a, **k: loops.append(k) or per_batch(*a, **k))
    fast = evaluate_device(model, smp, mets)
    auto = evaluate(model, smp, mets)
    assert calls == [{"rank_metrics": True}] * 2          # one call each, hit and mrr requested
    monkeypatch.setenv("RTX_EVAL_SIMPLE_LOOP", "1")
    loop = evaluate_device(model, smp, mets)
    monkeypatch.delenv("RTX_EVAL_SIMPLE_LOOP")
    assert len(calls) == 2 and loops == [{"rank_metrics": True}] * 3        # the per-batch route: 20 + 20 + 8 users
    host = evaluate_host(model, smp, mets)

    want = {"ndcg": nd, "recall": rc, "hit": hit, "mrr": mrr}
    wrong = []
    for q, k in enumerate(EVAL_KS):
        d, da = det[q], det_all[q]
        for name in NAMES:
            m = "%s@%d" % (name, k)
            assert np.array_equal(auto[m], fast[m], equal_nan=True), m
            for route, got in (("one-call", fast[m]), ("per-batch", loop[m]), ("host", host[m])):
                assert got.shape == (U,) and got.dtype == host[m].dtype, (route, m, got.dtype, host[m].dtype)
            for route, got, mask in (("one-call", fast[m], d), ("per-batch", loop[m], d), ("host", host[m], da)):
                bad = np.flatnonzero(mask & ~np.isclose(got, want[name][q], rtol=1e-12, atol=0, equal_nan=True))
                if bad.size:
                    wrong.append("%s %s: users %s" % (route, m, bad.tolist()))
            if not np.allclose(fast[m][da], host[m][da], rtol=1e-12, atol=0, equal_nan=True):
                wrong.append("one-call != host %s" % m)
    assert not wrong, "\n".join(wrong)
    assert fast["hit@10"].dtype == bool and fast["mrr@10"].dtype == np.float64
    assert not fast["hit@1024"][0] and fast["mrr@1024"][0] == 0.0          # user 0: empty held-out row


def test_rank_metrics_keyword_leaves_the_old_calls_alone():
    """topk_metrics / Engine.evaluate_topk without rank_metrics return what they returned; with it, nDCG / Recall are unchanged"""
    from rectorch_amd.engine import CsrMatrix, topk_metrics
    from rectorch_amd.metrics import Metrics
    rng = np.random.RandomState(2)
    B, I = 37, 3001
    sc = rng.randn(B, I).astype(np.float32)
    held = (rng.rand(B, I) < 0.01) * rng.choice([-2.0, 1.0, 4.0], size=(B, I))
    held[3] = 0
    hm = CsrMatrix(csr_matrix(held))
    rows = torch.arange(B, dtype=torch.int32, device="cuda")
    ks = [1, 5, 50, 300]
    s = torch.from_numpy(sc).cuda()
    two = topk_metrics(s, hm, rows, ks)
    four = topk_metrics(s, hm, rows, ks, rank_metrics=True)
    assert len(two) == 2 and len(four) == 4
    for a, b in zip(two, four[:2]):
        assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
    for q, k in enumerate(ks):          # continuous random scores: no ties, the host order is the kernel's
        assert np.array_equal(four[2][q].cpu().numpy().astype(bool), Metrics.hit_at_k(sc, held, k))
        assert np.allclose(four[3][q].cpu().numpy(), Metrics.mrr_at_k(sc, held, k), rtol=1e-12, atol=0)


# --------------------------------------------------------------------------------------------------------- one-plus-random
def _opr_rows(I, U, seed, n_te=(1, 6)):
    """train / held-out CSR matrices for one-plus-random: user 0 has no held-out item, user 1 holds out one of its train items (the
    positive scores -inf), user 2 has a stored zero in its held-out row and a negative rating (a positive: dense.nonzero())"""
    rng = np.random.RandomState(seed)
    tr_rows, te_rows, te_vals = [], [], []
    for u in range(U):
        perm = rng.permutation(I)
        n_tr = rng.randint(3, max(4, min(200, I // 4))) if u != 1 else I // 2
        k = 0 if u == 0 else rng.randint(*n_te)
        tr, te = np.sort(perm[:n_tr]), perm[n_tr:n_tr + k]
        if u == 1:
            te = np.append(te, tr[0])
        vals = np.ones(len(te))
        if u == 2 and len(te) >= 2:
            vals[0], vals[1] = 0.0, -1.0
        o = np.argsort(te)
        tr_rows.append(tr)
        te_rows.append(te[o])
        te_vals.append(vals[o])

    def csr(rows, vals):
        indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows])))
        return csr_matrix((np.concatenate(vals), np.concatenate(rows).astype(np.int32), indptr), shape=(U, I))
    return csr(tr_rows, [np.ones(len(r)) for r in tr_rows]), csr(te_rows, te_vals)


def _opr_tie_rule(scores, held, r, metric_list):
    """the reference's loop (random.sample per positive, row-major) with the ties of each contest broken by the stated rule -- the
    positive, column 0, before equal scores -- by replacing the contest's scores with their place in that order; then Metrics"""
    from rectorch_amd.metrics import Metrics
    n_items = held.shape[1]
    contests = []
    for u, i in zip(*held.nonzero()):
        negatives = sorted(set(range(n_items)) - set(held[u].nonzero()[0].tolist()))
        contests.append(scores[u][[i] + random.sample(negatives, r)])
    pred = np.array(contests).astype(np.float64)
    order = np.lexsort((np.broadcast_to(np.arange(r + 1), pred.shape), -pred), axis=1)
    place = np.empty_like(order)
    np.put_along_axis(place, order, np.arange(r + 1)[None, :].repeat(len(pred), 0), axis=1)
    truth = np.zeros_like(pred, dtype=np.float32)
    truth[:, 0] = 1
    return Metrics.compute(-place.astype(np.float32), truth, metric_list), pred


OPR_CASES = [(1, 20), (1, 700), (20, 86), (20, 700), (1000, 4099), (1000, 20108)]     # (r, I): pool / set branch of random.sample
OPR_METS = ["ndcg@10", "recall@5", "hit@1", "mrr@100", "NDCG@1000", "hit@20", "mrr@1", "recall@1024"]


@pytest.mark.parametrize("r,I", OPR_CASES, ids=["r%d-I%d" % c for c in OPR_CASES])
def test_one_plus_random_device_equals_host(r, I, monkeypatch):
    from rectorch_amd.utils import hash_state_dict
    from rectorch_amd.samplers import DataSampler
    from rectorch_amd.evaluation import one_plus_random, one_plus_random_host, ValidFunc
    from rectorch_amd import engine as E
    U, H, L = 24, 32, 16
    tr, te = _opr_rows(I, U, seed=I + r, n_te=(1, 6) if I > 20 else (1, 3))
    sd = hash_state_dict([I, H, L], [L, H, I], "vae", 17 + I, bias_std=0.5)
    net, model = make_vae([I, H, L], [L, H, I], 0.5, sd)
    smp = DataSampler(tr, te, batch_size=10, shuffle=False)     # 10 + 10 + 4 users
    ranked = []
    opr_rank = E.opr_rank
    monkeypatch.setattr(E, "opr_rank", lambda *a, **k: ranked.append(1) or opr_rank(*a, **k))

    random.seed(r + I)
    got = one_plus_random(model, smp, OPR_METS, r=r)
    st_dev = random.getstate()
    assert len(ranked) == 3                                      # the device route ran, one rank launch per batch
    random.seed(r + I)
    host = one_plus_random_host(model, smp, OPR_METS, r=r)
    assert random.getstate() == st_dev
    assert len(ranked) == 3

    scores = np.concatenate([model.predict(rb)[0].cpu().numpy() for rb in smp.iter_rows()])
    random.seed(r + I)
    rule, pred = _opr_tie_rule(scores, te.toarray().astype(np.float32), r, OPR_METS)
    assert random.getstate() == st_dev
    untied = (pred[:, 1:] != pred[:, :1]).all(axis=1)
    assert untied.sum() >= 0.8 * len(untied)
    assert r < 20 or (~untied).sum() >= 1                        # user 1's -inf positive ties with the train items it drew
    assert np.isneginf(pred[~untied, 0]).all()
    for m in OPR_METS:
        assert got[m].dtype == host[m].dtype and got[m].shape == host[m].shape == (len(pred),), m
        assert np.array_equal(got[m], rule[m]), m
        assert np.array_equal(got[m][untied], host[m][untied]), m

    vf = ValidFunc(one_plus_random, r=r)                         # as a trainer's validation function
    random.seed(1)
    v = vf(model, smp, "mrr@100")
    assert len(ranked) == 6
    random.seed(1)
    assert np.array_equal(v, _opr_tie_rule(scores, te.toarray().astype(np.float32), r, ["mrr@100"])[0]["mrr@100"])


def test_one_plus_random_too_few_negatives_and_routing(monkeypatch):
    """a user with fewer than r negatives: ValueError on both routes, with the random state at the same point; a metric the device
    route does not take (k > 1024) and device_metrics = False take the reference's loop"""
    from rectorch_amd.utils import hash_state_dict
    from rectorch_amd.samplers import DataSampler
    from rectorch_amd.evaluation import one_plus_random, one_plus_random_host, one_plus_random_device
    from rectorch_amd import engine as E
    I, U, H, L, r = 700, 30, 32, 16, 20
    tr, te = _opr_rows(I, U, seed=5)
    te = te.tolil()
    te[17, np.arange(0, 685)] = 1.0                              # user 17 (second batch): 15 negatives < r
    te = te.tocsr()
    sd = hash_state_dict([I, H, L], [L, H, I], "vae", 3, bias_std=0.5)
    net, model = make_vae([I, H, L], [L, H, I], 0.5, sd)
    smp = DataSampler(tr, te, batch_size=10, shuffle=False)
    ranked = []
    opr_rank = E.opr_rank
    monkeypatch.setattr(E, "opr_rank", lambda *a, **k: ranked.append(1) or opr_rank(*a, **k))
    random.seed(0)
    with pytest.raises(ValueError):
        one_plus_random(model, smp, ["ndcg@10"], r=r)
    st_dev = random.getstate()
    assert len(ranked) == 1                                      # the first batch was ranked on the device, the second raised
    random.seed(0)
    with pytest.raises(ValueError):
        one_plus_random_host(model, smp, ["ndcg@10"], r=r)
    assert random.getstate() == st_dev

    te2 = te.tolil()
    te2[17, :] = 0
    te2 = te2.tocsr()
    te2.eliminate_zeros()
    smp2 = DataSampler(tr, te2, batch_size=10, shuffle=False)
    random.seed(4)
    a = one_plus_random_device(model, smp2, ["ndcg@10", "ndcg@2000"], r=r)      # k > 1024: the host loop
    random.seed(4)
    b = one_plus_random_host(model, smp2, ["ndcg@10", "ndcg@2000"], r=r)
    assert len(ranked) == 1 and all(np.array_equal(a[m], b[m]) for m in ("ndcg@10", "ndcg@2000"))
    model.device_metrics = False
    random.seed(4)
    one_plus_random(model, smp2, ["ndcg@10"], r=r)
    model.device_metrics = True
    assert len(ranked) == 1
    random.seed(4)
    one_plus_random(model, smp2, ["ndcg@10"], r=r)
    assert len(ranked) == 4
