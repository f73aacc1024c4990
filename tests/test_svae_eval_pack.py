"""SVAE scoring and evaluation in packs of users: rtx_svae_predict_pack (rectorch_amd/csrc/svae.hip) -> SvaeEngine.predict_pack ->
SVAE.predict(SvaeEvalPack) -> SVAE_Sampler(is_training=False, pack=N) -> evaluate().

GPU tests compare with the float64 oracle (oracle/svae_oracle.py) at the shapes of tests/test_svae_routes.py (I=120, E=24, H=32,
L=8, D=40, injected eps).  Bounds: finite scores, mu and logvar 2e-5 relative to the largest reference entry (`rel`, the bound of
test_svae_gru_route_vs_oracle for last-step scores), -inf positions identical; metric values 1e-12, hit@k exactly.

The CPU tests cover the export, its binding and the sampler's plan of packs (everything of it that needs no device).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

GENERIC, ALL, ROWS, KS = 0, 1, 2, 3
KNOBS = ("RTX_SVAE_GRU_ROWS", "RTX_SVAE_GRU_KS", "RTX_SVAE_GRU_BWD_KS")
L_ = 8
LENS = (1, 2, 157, 33, 1)      # length 1: the user's last row is its first row; 157 > 64: more than one tile of rows in the recurrence's GEMMs


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-30, np.max(np.abs(b))))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


def _knobs(monkeypatch, **off):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in off.items():
        monkeypatch.setenv("RTX_SVAE_GRU_" + k, str(v))


def _state_dict(R, seed, I=120, E=24, H=32, L=L_, D=40):
    from rectorch_amd.nets import SVAE_net
    torch.manual_seed(seed)
    net = SVAE_net(n_items=I, embed_size=E, rnn_size=R, dec_dims=[L, D, I], enc_dims=[R, H, L])
    return net, {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}


def _make(R, seed, I=120, beta=0.2, **kw):
    from oracle.svae_oracle import SvaeOracle
    from rectorch_amd.models import SVAE
    net, sd = _state_dict(R, seed, I=I)
    model = SVAE(net.to("cuda"), beta=beta, anneal_steps=0, **kw)
    return net, model, SvaeOracle(sd, n_enc=2, n_dec=2, beta=beta)


def _pack_of(rng, lens, I):
    from rectorch_amd.engine import SvaeEvalPack
    seqs = [rng.randint(0, I, size=n).tolist() for n in lens]
    pack = SvaeEvalPack(seqs, users=list(range(len(lens))))
    eps = rng.randn(pack.n_steps, L_).astype(np.float32)
    return seqs, pack, eps


def _oracle_rows(orc, seqs, eps, remove_train=True):
    """per user (scores, mu, logvar) of the last step, each user with its own rows of the concatenated noise"""
    out, o = [], 0
    for q in seqs:
        pr, mu, lv = orc.predict(np.array(q), eps[o:o + len(q)].astype(np.float64), remove_train=remove_train)
        out.append((pr, mu[-1], lv[-1]))
        o += len(q)
    return out


def _compare(tag, got, want, bound):
    """-inf positions identical; finite scores, mu, logvar of every user within `bound` (printed before it is asserted)"""
    pr, mu, lv = (t.cpu().numpy() for t in got)
    assert pr.shape[0] == mu.shape[0] == lv.shape[0] == len(want)
    worst = [0.0, 0.0, 0.0]
    for u, (pref, muref, lvref) in enumerate(want):
        assert np.array_equal(np.isneginf(pr[u]), np.isneginf(pref)), (tag, u)
        assert not np.isnan(pr[u]).any() and not np.isposinf(pr[u]).any(), (tag, u)
        fin = np.isfinite(pref)
        for i, e in enumerate((rel(pr[u][fin], pref[fin]), rel(mu[u], muref), rel(lv[u], lvref))):
            worst[i] = max(worst[i], e)
    print("%s: scores %.2e, mu %.2e, logvar %.2e (worst user)" % (tag, *worst))
    assert max(worst) < bound, (tag, worst)
    return worst


# (R, switches turned off, the forward recurrence that must have run)
ROUTES = [(3, {}, ROWS), (64, {"ROWS": 0}, GENERIC), (150, {}, KS), (205, {}, GENERIC)]


@pytest.mark.gpu
@pytest.mark.parametrize("I", [120, 121])      # 121: score rows that are no multiple of 4 floats
@pytest.mark.parametrize("R,off,fwd", ROUTES, ids=["R%d" % c[0] for c in ROUTES])
def test_predict_pack_vs_oracle_every_route(R, off, fwd, I, monkeypatch):
    """one pack of users of 1, 2, 157, 33 and 1 steps, and a pack of exactly one user, behind every forward recurrence kernel:
    per user the oracle's predict, with and without the -inf at the user's own items"""
    _knobs(monkeypatch, **off)
    net, model, orc = _make(R, seed=300 + R, I=I)
    rng = np.random.RandomState(R + I)
    for lens in (LENS, (7,), (1,)):
        seqs, pack, eps = _pack_of(rng, lens, I)
        model._rtx.inject = (None, dev(eps))
        got = model.predict(pack)
        got_keep = model.predict(pack, remove_train=False)
        model._rtx.inject = None
        tag = "R=%d I=%d lens=%s" % (R, I, lens)
        assert tuple(got[0].shape) == (len(lens), I) and tuple(got[1].shape) == tuple(got[2].shape) == (len(lens), L_)
        _compare(tag, got, _oracle_rows(orc, seqs, eps), 2e-5)
        assert torch.isfinite(got_keep[0]).all()            # remove_train=False: no -inf anywhere
        _compare(tag + " keep", got_keep, _oracle_rows(orc, seqs, eps, remove_train=False), 2e-5)
    assert net._svae_engine.get_option("gru_fwd") == fwd


@pytest.mark.gpu
def test_predict_pack_bf16_products_vs_oracle(monkeypatch):
    """SVAE(numerics="bf16"): the pack's products on the bf16 MFMA.  The existing bf16 SVAE parity test,
    test_svae_bf16_products_vs_oracle (tests/test_gpu_parity.py), bounds the loss (5e-5) and the gradients (3e-2, "bf16 operands")
    and has no figure of its own for last-step scores.  The scores are, like the gradients, the end of a chain of products with
    bf16-rounded operands (unit round-off 2^-9 per operand, 2^-8 per term, five products deep: input projection, two encoder and
    two decoder layers: 5 * 2^-8 = 2e-2), so that test's bound for such quantities, 3e-2, is the one used here (measured: scores
    5.7e-3, mu 7.1e-3, logvar 6.9e-3), and the arithmetic must differ from the float32 mode's."""
    _knobs(monkeypatch)
    I, R = 120, 150
    rng = np.random.RandomState(7)
    seqs = eps = None
    out = {}
    for mode in ("fp32", "bf16"):
        net, model, orc = _make(R, seed=451, I=I, numerics=mode)
        if seqs is None:
            seqs, pack, eps = _pack_of(rng, LENS, I)
        model._rtx.inject = (None, dev(eps))
        out[mode] = model.predict(pack)
        model._rtx.inject = None
        assert net._svae_engine.get_option("gemm_bf16") == (mode == "bf16")
    want = _oracle_rows(orc, seqs, eps)
    _compare("fp32 mode", out["fp32"], want, 2e-5)
    _compare("bf16 mode", out["bf16"], want, 3e-2)
    assert not torch.equal(out["fp32"][0], out["bf16"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("R,off,fwd", [ROUTES[0], ROUTES[2]], ids=["R3", "R150"])
def test_predict_pack_equals_per_user_predict(R, off, fwd, monkeypatch):
    """the packed scores against predict(x) of each user under the same injected noise rows: 2e-5 (not bit identity: M differs,
    and so may the split of K), the same -inf positions"""
    _knobs(monkeypatch, **off)
    I = 121
    net, model, _ = _make(R, seed=77 + R, I=I)
    rng = np.random.RandomState(R)
    seqs, pack, eps = _pack_of(rng, LENS, I)
    model._rtx.inject = (None, dev(eps))
    got = model.predict(pack)
    want, o = [], 0
    for q in seqs:
        model._rtx.inject = (None, dev(eps[o:o + len(q)]))
        pr, mu, lv = model.predict(torch.LongTensor([q]))
        assert tuple(pr.shape) == (1, I) and tuple(mu.shape) == (len(q), L_)
        want.append((pr.cpu().numpy()[0], mu.cpu().numpy()[-1], lv.cpu().numpy()[-1]))
        o += len(q)
    model._rtx.inject = None
    _compare("R=%d pack vs per-user" % R, got, want, 2e-5)
    assert net._svae_engine.get_option("gru_fwd") == fwd


# ------------------------------------------------------------------------------------------------ sampler
PACK_TOKENS = 12


def _sampler_data():
    """11 users: user 2 has one training item (no time step: skipped), user 5's 13 items alone reach pack_tokens = 12, users 0 and
    7 repeat test items"""
    rng = np.random.RandomState(5)
    n_items = 40
    lens = [4, 6, 1, 3, 5, 13, 2, 4, 9, 3, 2]
    tr = {u: rng.randint(0, n_items, size=n).tolist() for u, n in enumerate(lens)}
    te = {u: rng.choice(n_items, size=3, replace=False).tolist() for u in tr}
    te[0] = te[0] + [te[0][0], te[0][1]]
    te[7] = [te[7][2]] + te[7] + [te[7][0]]
    return n_items, tr, te


def _check_packs(packs, tr, order):
    """consecutive in `order`, short users skipped, at most 4 users and PACK_TOKENS steps (one longer user: alone)"""
    flat = [u for p in packs for u in p]
    assert flat == [u for u in order if len(tr[u]) >= 2]
    for p in packs:
        steps = sum(len(tr[u]) - 1 for u in p)
        assert 1 <= len(p) <= 4 and (steps <= PACK_TOKENS or len(p) == 1), (p, steps)
    for p, q in zip(packs, packs[1:]):      # greedy: the next user did not fit
        assert len(p) == 4 or sum(len(tr[u]) - 1 for u in p) + len(tr[q[0]]) - 1 > PACK_TOKENS, (p, q)


def test_eval_sampler_plan_of_packs():
    """CPU: the packs an eval sampler cuts (no device object is built), __len__, and pack=1 exactly as the reference lays it out"""
    from rectorch_amd.samplers import SVAE_Sampler
    n_items, tr, te = _sampler_data()
    sm = SVAE_Sampler(n_items, tr, te, is_training=False, pack=4, pack_tokens=PACK_TOKENS, shuffle=False)
    packs = sm._eval_packs(list(range(len(tr))))
    _check_packs(packs, tr, list(range(len(tr))))
    assert [5] in packs and all(2 not in p for p in packs)
    # steps per user: 3 5 - 2 4 12 1 3 8 2 1, cut greedily at 4 users or 12 steps
    assert len(sm) == len(packs) == 5
    assert packs == [[0, 1, 3], [4], [5], [6, 7, 8], [9, 10]]
    order = [10, 3, 5, 2, 0, 9, 8, 1, 4, 7, 6]
    _check_packs(sm._eval_packs(order), tr, order)
    held = sm._heldout_csr()
    assert held.shape == (len(tr), n_items) and held.dtype == np.float32
    for u in tr:
        want = np.zeros(n_items, dtype=np.float32)
        want[te[u]] = 1.
        assert np.array_equal(held[u].toarray()[0], want), u      # binary although users 0 and 7 repeat items
    # pack=1: the reference's layout, one user per batch, the short user included (an empty x)
    one = SVAE_Sampler(n_items, tr, te, is_training=False, pack=1, pack_tokens=PACK_TOKENS, shuffle=False)
    assert len(one) == len(tr)
    got = list(one)
    assert len(got) == len(tr)
    for u, (x, y) in enumerate(got):
        wx = torch.LongTensor([tr[u][:-1]])
        wy = torch.zeros(1, 1, n_items)
        wy[0, 0, te[u]] = 1.
        assert x.dtype == wx.dtype and x.shape == wx.shape and torch.equal(x, wx), u
        assert y.dtype == wy.dtype and y.shape == wy.shape and torch.equal(y, wy), u
    # training packs are what they were: sorted by length inside a window
    trn = SVAE_Sampler(n_items, tr, te, is_training=True, pack=4, pack_tokens=PACK_TOKENS, shuffle=False)
    assert trn._pack_windows(list(range(len(tr))))[0][0] == [6, 10, 3, 9]


@pytest.mark.gpu
def test_eval_sampler_yields_packs_and_heldout_rows():
    """what the sampler yields on the device: SvaeEvalPack + RowBatch over ONE resident [n_users, num_items] matrix"""
    from rectorch_amd.engine import CsrMatrix, RowBatch, SvaeEvalPack
    from rectorch_amd.evaluation import _to_numpy
    from rectorch_amd.samplers import SVAE_Sampler
    n_items, tr, te = _sampler_data()
    sm = SVAE_Sampler(n_items, tr, te, is_training=False, pack=4, pack_tokens=PACK_TOKENS, shuffle=False)
    got = list(sm)
    assert len(got) == len(sm) == 5
    _check_packs([p.users for p, _ in got], tr, list(range(len(tr))))
    mats = set()
    for pack, held in got:
        assert isinstance(pack, SvaeEvalPack) and isinstance(held, RowBatch) and isinstance(held.tr, CsrMatrix)
        assert not hasattr(pack, "indptr")
        assert len(pack) == len(held) == len(pack.users) and pack.n_steps == sum(pack.lens)
        assert pack.lens == [len(tr[u]) - 1 for u in pack.users]
        assert pack.items.dtype == torch.int32 and pack.items.cpu().tolist() == [i for u in pack.users for i in tr[u][:-1]]
        assert pack.seq_ptr.cpu().tolist() == [0] + np.cumsum(pack.lens).tolist()
        assert held.rows.cpu().tolist() == pack.users
        assert held.tr.shape == (len(tr), n_items) and held.tr.binary
        mats.add(id(held.tr))
        dense = _to_numpy(held)
        for r, u in enumerate(pack.users):
            want = np.zeros(n_items, dtype=np.float32)
            want[te[u]] = 1.                                   # the reference's y[0, 0, te] = 1
            assert np.array_equal(dense[r], want), u
    assert len(mats) == 1
    assert next(iter(sm))[1].tr is got[0][1].tr               # uploaded once per sampler, not per epoch


# ------------------------------------------------------------------------------------------------ evaluate, end to end
EVAL_METRICS = ["ndcg@5", "recall@5", "hit@3", "mrr@10"]
EVAL_SEED = 3          # found on the CPU (see _eval_case): the rank gaps below hold for every user
EVAL_R, EVAL_I = 64, 120


def _eval_case(seed):
    """users, held-out items, noise and the visiting order of the end-to-end case, and the float64 oracle's scores of every
    scored user in that order.  Returns None when, for some user and some cut-off k of EVAL_METRICS, the oracle's k-th and
    (k+1)-th finite scores are closer than 1e-3 of the user's largest |finite score| -- 50 times the score bound (2e-5 of the same
    quantity), so that no rank can flip inside the tolerance."""
    from oracle.svae_oracle import SvaeOracle
    from rectorch_amd.samplers import SVAE_Sampler
    _, sd = _state_dict(EVAL_R, 900 + seed, I=EVAL_I)
    orc = SvaeOracle(sd, n_enc=2, n_dec=2, beta=0.2)
    rng = np.random.RandomState(seed)
    lens = [5, 9, 1, 21, 3, 13, 2, 30, 7, 16, 11]          # user 2: no time step, skipped
    tr = {u: rng.randint(0, EVAL_I, size=n).tolist() for u, n in enumerate(lens)}
    te = {u: rng.choice(EVAL_I, size=4, replace=False).tolist() + [int(rng.randint(0, EVAL_I))] for u in tr}
    noise = rng.randn(64, L_).astype(np.float32)            # one array for every pack: user u takes the row of its last step IN ITS PACK
    sm = SVAE_Sampler(EVAL_I, tr, te, is_training=False, pack=4, pack_tokens=40, shuffle=True)
    np.random.seed(seed)
    order = list(range(len(tr)))
    np.random.shuffle(order)                                # the sampler's own draw
    packs = sm._eval_packs(order)
    users, scores = [], []
    for p in packs:
        last = np.cumsum([len(tr[u]) - 1 for u in p]) - 1
        for u, r in zip(p, last):
            eps = np.zeros((len(tr[u]) - 1, L_))
            eps[-1] = noise[r]
            pr = orc.predict(np.array(tr[u][:-1]), eps)[0]
            fin = np.sort(pr[np.isfinite(pr)])[::-1]
            for k in (3, 5, 10):
                if len(fin) <= k or fin[k - 1] - fin[k] <= 1e-3 * np.max(np.abs(fin)):
                    return None
            users.append(u)
            scores.append(pr)
    heldout = np.zeros((len(users), EVAL_I), dtype=np.float32)
    for r, u in enumerate(users):
        heldout[r, te[u]] = 1.
    return dict(tr=tr, te=te, noise=noise, sampler=sm, order=order, users=users, scores=np.array(scores), heldout=heldout, sd=sd)


def test_eval_case_rank_gaps_hold_for_every_user():
    """CPU: the condition of the end-to-end test, on the oracle's scores alone"""
    case = _eval_case(EVAL_SEED)
    assert case is not None
    assert len(case["users"]) == 10 and 2 not in case["users"]
    assert case["users"] == [u for u in case["order"] if u != 2] != sorted(case["users"])


@pytest.mark.gpu
def test_evaluate_packed_sampler_end_to_end(monkeypatch):
    """evaluate() over packs against Metrics.compute on the ORACLE's float64 scores, per user and in loader order; the host loop
    (device_metrics off, or a metric the kernel does not know) gives the same"""
    from rectorch_amd import evaluation
    from rectorch_amd.evaluation import evaluate, evaluate_device, evaluate_host
    from rectorch_amd.metrics import Metrics
    from rectorch_amd.models import SVAE
    from rectorch_amd.nets import SVAE_net
    _knobs(monkeypatch)
    case = _eval_case(EVAL_SEED)
    assert case is not None, "the rank gaps must hold for every user before anything is compared"
    want = Metrics.compute(case["scores"], case["heldout"], EVAL_METRICS)
    net = SVAE_net(n_items=EVAL_I, embed_size=24, rnn_size=EVAL_R, dec_dims=[L_, 40, EVAL_I], enc_dims=[EVAL_R, 32, L_])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in case["sd"].items()})
    model = SVAE(net.to("cuda"), beta=0.2, anneal_steps=0)
    model._rtx.inject = (None, dev(case["noise"]))
    sm = case["sampler"]
    calls = []
    real = evaluation._evaluate_svae_packs
    monkeypatch.setattr(evaluation, "_evaluate_svae_packs", lambda *a: calls.append(1) or real(*a))

    def run(fn, metrics):
        np.random.seed(EVAL_SEED)          # the visiting order of the case
        return fn(model, sm, metrics)

    def check(tag, got, metrics=EVAL_METRICS):
        assert list(got) == list(metrics), tag
        for m in metrics:
            assert got[m].shape == (len(case["users"]),) and got[m].dtype == want[m].dtype, (tag, m, got[m].dtype)
            if m.startswith("hit"):
                assert np.array_equal(got[m], want[m]), (tag, m)
            else:
                assert np.max(np.abs(got[m] - want[m])) <= 1e-12, (tag, m, got[m], want[m])

    check("evaluate", run(evaluate, EVAL_METRICS))
    assert len(calls) == 1                                   # the device route ran
    check("evaluate_device", run(evaluate_device, EVAL_METRICS))
    assert len(calls) == 2
    check("ndcg / recall only", run(evaluate, EVAL_METRICS[:2]), EVAL_METRICS[:2])
    assert len(calls) == 3
    check("evaluate_host", run(evaluate_host, EVAL_METRICS))
    model.device_metrics = False
    check("device_metrics = False", run(evaluate, EVAL_METRICS))
    model.device_metrics = True
    assert len(calls) == 3                                   # ... both through the host loop
    # a metric the top-k kernel does not know: the whole list takes the host loop, without error
    got = run(evaluate, ["recall@5", "ndcg_at_k"])
    assert len(calls) == 3
    assert np.max(np.abs(got["recall@5"] - want["recall@5"])) <= 1e-12 and got["ndcg_at_k"].shape == (len(case["users"]),)
    model._rtx.inject = None


# ------------------------------------------------------------------------------------------------ bad calls, the export
@pytest.mark.gpu
def test_predict_pack_bad_calls_raise_before_any_launch(monkeypatch):
    """argument checks only: a pack longer than the engine's max_len, no sequence at all, a NULL seq_ptr"""
    from rectorch_amd import _lib
    from rectorch_amd.engine import SvaeEngine, SvaeEvalPack
    _knobs(monkeypatch)
    eng = SvaeEngine(50, 8, 16, [16, 12, 4], [4, 12, 50], max_len=8)
    params = []
    rows, cols = ctypes.c_int32(), ctypes.c_int32()
    for t in range(eng.n_tensors):
        _lib.check(_lib.lib().rtx_svae_tensor_shape(eng.handle, t, ctypes.byref(rows), ctypes.byref(cols)))
        params.append(torch.zeros((rows.value,) if cols.value == 1 else (rows.value, cols.value), device="cuda"))
    eng.bind(params)
    long_pack = SvaeEvalPack([[1, 2, 3, 4, 5], [6, 7, 8, 9]])       # 9 steps > max_len = 8
    with pytest.raises(_lib.RtxError):
        eng.predict_pack(long_pack)
    st = _lib.stream_ptr()
    ok = SvaeEvalPack([[1, 2, 3], [4]])
    out = torch.full((2, 50), 7.0, device="cuda")
    args = lambda items, n_steps, seq_ptr, n: (eng.handle, items, n_steps, seq_ptr, n, None, ctypes.c_uint64(0), ctypes.c_uint64(0), 1,
                                               ctypes.c_void_p(out.data_ptr()), None, None, st)
    p_items, p_seq = ctypes.c_void_p(ok.items.data_ptr()), ctypes.c_void_p(ok.seq_ptr.data_ptr())
    lp_items, lp_seq = ctypes.c_void_p(long_pack.items.data_ptr()), ctypes.c_void_p(long_pack.seq_ptr.data_ptr())
    f = _lib.lib().rtx_svae_predict_pack
    assert f(*args(lp_items, long_pack.n_steps, lp_seq, 2)) != 0     # the library's own max_len check
    assert f(*args(p_items, ok.n_steps, p_seq, 0)) != 0              # n_seq = 0
    assert f(*args(p_items, ok.n_steps, None, 2)) != 0               # NULL seq_ptr
    assert f(*args(p_items, ok.n_steps, p_seq, 5)) != 0              # more sequences than steps
    with pytest.raises(_lib.RtxError):
        _lib.check(f(*args(p_items, ok.n_steps, p_seq, 0)))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                  # nothing was launched
    sc, mu, lv = eng.predict_pack(ok)                                # and the well-formed call goes through
    assert tuple(sc.shape) == (2, 50) and tuple(mu.shape) == (2, 4)
    assert torch.isneginf(sc).sum().item() == 4


def test_library_exports_predict_pack_with_the_headers_argument_count():
    """CPU: the symbol is exported, and _lib binds it with as many arguments as include/rectorch_hip.h declares"""
    from rectorch_amd import _lib
    lib = ctypes.CDLL(_lib.build())
    assert hasattr(lib, "rtx_svae_predict_pack")
    text = open(os.path.join(ROOT, "include", "rectorch_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+rtx_svae_predict_pack\s*\(([^)]*)\)\s*;", text)
    assert m, "rtx_svae_predict_pack is not declared in the header"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    res, args = _lib.SIGNATURES["rtx_svae_predict_pack"]
    assert res is ctypes.c_int and len(args) == n_args == 13
    assert _lib.lib().rtx_abi_version() == 8
