"""GPU (-m gpu): CDAE -- the user node of the one-layer denoising autoencoder (include/rectorch_hip.h "CDAE") -- against the float64
restatement tests/cdae_ref64.py, with the dropout keep-masks injected (model._rtx.inject, as the G4 / G16 tests do).

Shapes: 300 items, 70 users; latent 50 (padded to 64: 14 masked columns, a float4 that straddles the last valid one, rows of V that
are not 16-byte aligned) and 64 (no padding, float4 rows); batches of 37 (a partial 16-row tile) and 64; ids a shuffled subset that
holds user 0, user 69 and several -1; three batches per epoch, the last one short.

Bounds are the project's own for the same quantity at the same numerics, cited where they are asserted.  The measured distances are
printed (profiles/cdae_ulp.txt keeps one run's).
"""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import cdae_ref64 as R
from test_optimizers_host import E24

from rectorch_amd.nets import CDAE_net         # noqa: F401  (the feature: without it nothing below can run)

pytestmark = pytest.mark.gpu

SHAPES = [(50, 37), (64, 64), (50, 64), (64, 37)]
LR = 1e-3


@pytest.fixture(scope="module", autouse=True)
def _require_native_path():
    from rectorch_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def case_of(latent, batch):
    return R.make_case(latent, n_rows=2 * batch + batch * 27 // 37, batch=batch)


def load(net, c, V=None):
    with torch.no_grad():
        for p, k in zip(net._param_list(), ("W0", "b0", "W1", "b1")):
            p.copy_(torch.from_numpy(c[k]))
        if V is not None:
            net.user_factors.weight.copy_(torch.from_numpy(np.asarray(V, np.float32)))


def make(c, trainer="dae", numerics="fp32", V="case", plain=False, lam=0.2, **kw):
    """MultiDAE / AETrainer over a CDAE_net (or, ``plain``, the MultiDAE_net of the same weights)"""
    from rectorch_amd.nets import CDAE_net, MultiDAE_net
    from rectorch_amd.models import AETrainer, MultiDAE
    net = MultiDAE_net([c["latent"], R.N_ITEMS], dropout=0.5) if plain else CDAE_net(R.N_ITEMS, R.N_USERS, c["latent"], dropout=0.5)
    load(net, c, None if plain else (c["V"] if isinstance(V, str) else V))
    model = MultiDAE(net, lam=lam, learning_rate=LR, numerics=numerics, **kw) if trainer == "dae" else AETrainer(net, learning_rate=LR, numerics=numerics, **kw)
    return net, model


def sampler(c, ids="case", te=None, **kw):
    from rectorch_amd.samplers import DataSampler
    kw.setdefault("shuffle", False)
    return DataSampler(csr_matrix(c["X"]), te, batch_size=c["batches"][0][1], user_ids=c["ids"] if isinstance(ids, str) else ids, **kw)


def moments0(c, seed=5):
    """distinctive starting moments for every row (|m| / sqrt(v) < 1, so a step still moves a parameter by about lr at most)"""
    rng = np.random.default_rng(seed)
    shape = (R.N_USERS, c["latent"])
    return (rng.standard_normal(shape) * 0.005).astype(np.float32), ((0.02 * (1 + rng.random(shape))) ** 2).astype(np.float32)


def set_moments(model, m0, v0):
    _, st = model._user_optim_state()
    st["exp_avg"].copy_(torch.from_numpy(m0))
    st["exp_avg_sq"].copy_(torch.from_numpy(v0))


def table(model):
    p = model.network.user_factors.weight
    st = model.user_optimizer.state[p]
    return host(p).copy(), host(st["exp_avg"]).copy(), host(st["exp_avg_sq"]).copy()


def state_of(model):
    model._join()
    torch.cuda.synchronize()
    dense = [host(p).copy() for p in model.network._param_list()]
    opt = [host(model.optimizer.state[p][k]).copy() for p in model.network._param_list() for k in ("exp_avg", "exp_avg_sq")]
    return dense + opt + list(table(model))


def assert_bit_equal(a, b, tag):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(bits(x), bits(y)), (tag, i, float(np.max(np.abs(x - y))))


# ------------------------------------------------------------------------------------------------ 1. eval forward, fp32
@pytest.mark.parametrize("latent,batch", SHAPES)
def test_eval_forward_fp32(latent, batch):
    c = case_of(latent, batch)
    x, ids = c["X"][:batch], c["ids"][:batch]
    net, model = make(c)
    _, plain = make(c, plain=True)
    ref = R.CdaeRef64([c["W0"], c["b0"], c["W1"], c["b1"]], c["V"])
    want = ref.forward(x, ids).detach().numpy()
    got = host(model.predict(dev(x), remove_train=False, users=dev(ids, torch.int32))[0])
    err = float(np.max(np.abs(got - want)))
    print("cdae eval forward fp32 latent %d batch %d: max abs %.3g" % (latent, batch, err))
    assert err < 1e-5                      # tests/test_plain_autoencoder.py: eval outputs `err < 1e-5`
    base = host(plain.predict(dev(x), remove_train=False)[0])
    none = ids < 0
    assert none.sum() >= 3 and (~none).sum() >= 10
    assert np.array_equal(got[none], base[none])                                                     # id -1: MultiDAE_net's forward
    assert np.array_equal(host(model.predict(dev(x), remove_train=False)[0]), base)                  # no ids at all
    far = np.where(none, R.N_USERS + 5, -7).astype(np.int32)                                         # outside [-1, n_users): as -1
    assert np.array_equal(host(model.predict(dev(x), remove_train=False, users=dev(far, torch.int32))[0]), base)
    assert not np.array_equal(got[~none], base[~none])
    # the network's own forward and encode take the ids too
    net.eval()
    assert np.array_equal(host(net(dev(x), dev(ids, torch.int32))), got)
    h = host(net.encode(dev(x), dev(ids, torch.int32)))
    assert h.shape == (batch, latent) and float(np.max(np.abs(h @ c["W1"].astype(np.float64).T + c["b1"] - want))) < 1e-5


# ------------------------------------------------------------------------------------------------ 2. zero table
@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
@pytest.mark.parametrize("latent,batch", SHAPES[:2])
def test_zero_table_equals_the_tableless_engine(latent, batch, numerics):
    c = case_of(latent, batch)
    x, ids, mask = c["X"][:batch], c["ids"][:batch], dev(c["masks"][0], torch.uint8)
    outs = []
    for plain in (True, False):
        # (lam = 0 for the bit-for-bit step: see run_epoch)
        net, model = make(c, numerics=numerics, V=np.zeros((R.N_USERS, latent)), plain=plain, predict_numerics=numerics, lam=0.0)
        users = None if plain else dev(ids, torch.int32)
        kw = {} if plain else {"users": users}
        o = [host(model.predict(dev(x), remove_train=False, **kw)[0]), host(model.predict(dev(x), remove_train=True, **kw)[0])]
        model._rtx.inject = (mask, None)
        o.append(np.float32(model.train_batch(dev(x), **kw)))
        model._join()
        o += [host(p) for p in net._param_list()]
        outs.append(o)
    for a, b in zip(*outs):
        assert np.array_equal(np.asarray(a) + np.float32(0.0) == np.asarray(b) + np.float32(0.0), np.ones(np.shape(a), bool))


# ------------------------------------------------------------------------------------------------ 3. three training steps
@pytest.mark.parametrize("trainer", ["dae", "ae"])
@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
@pytest.mark.parametrize("latent,batch", SHAPES)
def test_three_training_steps(latent, batch, numerics, trainer):
    c = case_of(latent, batch)
    net, model = make(c, trainer, numerics)
    m0, v0 = moments0(c)
    set_moments(model, m0, v0)
    ref = R.CdaeRef64([c["W0"], c["b0"], c["W1"], c["b1"]], c["V"], loss="multinomial" if trainer == "dae" else "mse", lam=0.2, lr=LR)
    w = ref.emb.weight
    ref.uopt.state[w] = {"step": 0, "exp_avg": torch.from_numpy(m0.astype(np.float64)), "exp_avg_sq": torch.from_numpy(v0.astype(np.float64))}
    fp32 = numerics == "fp32"
    batches = list(sampler(c).iter_rows())
    assert [len(rb) for rb in batches] == [hi - lo for lo, hi in c["batches"]] and len(batches) == 3 and len(batches[2]) < batch
    for t, (rb, (lo, hi)) in enumerate(zip(batches, c["batches"])):
        ids = c["ids"][lo:hi]
        assert np.array_equal(host(rb.users), ids)
        before = table(model)
        rbefore = ref.table()[:3]
        dbefore = [ref.dense_state(k) if t else None for k in ("exp_avg", "exp_avg_sq")]
        model._rtx.inject = (dev(c["masks"][t], torch.uint8), None)
        loss = model._fused_step(rb, None, want_loss=True)
        want = ref.train_batch(c["X"][lo:hi], ids, c["masks"][t])
        model._join()
        print("cdae %s %s latent %d batch %d step %d: loss %.9g ref %.9g (rel %.3g)" % (trainer, numerics, latent, batch, t, loss, want, abs(loss - want) / abs(want)))
        if fp32:
            # tests/test_plain_autoencoder.py: MSE loss `<= 1e-6 * abs(ref)`; multinomial + regulariser `<= 1e-5 * abs(want_dae)`
            assert abs(loss - want) <= (1e-5 if trainer == "dae" else 1e-6) * abs(want), (t, loss, want)
        else:
            assert abs(loss - want) < 2e-3 * abs(want), (t, loss, want)       # tests/test_plain_autoencoder.py: bf16 loss `< 2e-3 * abs(ref)`
        after = table(model)
        rV, rm, rv, rstep = ref.table()
        assert model.user_optimizer.state[net.user_factors.weight]["step"] == rstep == t + 1
        touched = np.zeros(R.N_USERS, bool)
        touched[ids[ids >= 0]] = True
        assert 5 <= touched.sum() < R.N_USERS
        for name, got, old in zip(("V", "exp_avg", "exp_avg_sq"), after, before):       # rows outside the batch: to the bit
            assert np.array_equal(bits(got[~touched]), bits(old[~touched])), (name, t)
        for name, got, want_s, old_s in zip(("exp_avg", "exp_avg_sq"), after[1:], (rm, rv), rbefore[1:]):
            err = float(np.max(np.abs(got[touched] - want_s[touched])))
            move = float(np.max(np.abs(want_s[touched] - old_s[touched])))
            scale = float(np.max(np.abs(want_s[touched])))
            print("  user %s: max err %.3g, largest move %.3g, largest value %.3g" % (name, err, move, scale))
            # tests/test_optimizers_gpu.py: state tensors `s_err <= 5e-3 * s_move`, relative to the step's own MOVE of the moment, so a
            # skipped update (error = the move) or a wrong beta or g^2 fails.  It is the project's only end-to-end bound for moments and
            # is held in both numerics: the table's gradient is float32 before the cast in bf16 too.  Measured, worst error / move over
            # every case (profiles/cdae_ulp.txt): float32 5.5e-7 (exp_avg), 4.9e-5 (exp_avg_sq); bf16 3.0e-3 and 4.8e-3 -- 0.60 and
            # 0.96 of the bound
            assert err <= 5e-3 * move, (name, t, err, move)
        dV = np.abs(after[0][touched] - rV[touched])
        print("  user rows: max err %.3g mean %.3g" % (float(dV.max()), float(dV.mean())))
        if fp32:
            assert float(dV.max()) < 5e-6, (t, float(dV.max()))              # tests/test_plain_autoencoder.py: parameters `d < 5e-6`
            if t:       # W / b moments, as ever (tests/test_optimizers_gpu.py: `s_err <= 5e-3 * s_move`)
                for k, old_d in zip(("exp_avg", "exp_avg_sq"), dbefore):
                    for p, want_d, o in zip(net._param_list(), ref.dense_state(k), old_d):
                        assert float(np.max(np.abs(host(model.optimizer.state[p][k]) - want_d))) <= 5e-3 * float(np.max(np.abs(want_d - o)))
        else:
            assert float(dV.max()) < 3.5e-3 and float(dV.mean()) < 2e-4      # tests/test_plain_autoencoder.py: bf16 parameters
        assert net.user_factors.weight.grad is None
    for i, (p, want_p) in enumerate(zip(net._param_list(), ref.params())):
        d = np.abs(host(p) - want_p)
        print("  parameter %d after 3 steps: max %.3g mean %.3g" % (i, float(d.max()), float(d.mean())))
        if fp32:
            assert float(d.max()) < 5e-6, (i, float(d.max()))                # tests/test_plain_autoencoder.py: `d < 5e-6`
        else:
            assert float(d.max()) < 3.5e-3 and float(d.mean()) < 2e-4, (i, float(d.max()), float(d.mean()))
    assert float(model.optimizer.state[net._param_list()[0]]["step"]) in (0.0, 3.0) and model._rtx.adam_step == 3
    never = np.ones(R.N_USERS, bool)
    never[c["ids"][c["ids"] >= 0]] = False
    assert never.sum() == 8
    for got, start in zip(table(model), (c["V"], m0, v0)):
        assert np.array_equal(bits(got[never]), bits(start[never]))


# ------------------------------------------------------------------------------------------------ 4. the row update alone
@pytest.mark.parametrize("latent,ld", [(50, 50), (50, 52), (64, 64), (50, 67), (3, 4)])
@pytest.mark.parametrize("step", [1, 100000])
def test_user_rows_adam_alone(latent, ld, step):
    from rectorch_amd.engine import user_rows_adam
    rng = np.random.default_rng(latent * 100 + ld + step)
    n, batch, ldg = R.N_USERS, 37, latent + 3
    full = [rng.standard_normal((n, ld)).astype(np.float32) * s for s in (0.3, 0.01)] + [(rng.random((n, ld)).astype(np.float32) * 0.02) ** 2]
    ids = rng.permutation(n)[:batch].astype(np.int32)
    ids[[3, 17]] = -1
    ids[5], ids[20], ids[36] = n, 1000, -5
    if 0 not in ids:
        ids[0] = 0
    if n - 1 not in ids:
        ids[1] = n - 1
    assert len(set(ids[(ids >= 0) & (ids < n)])) == ((ids >= 0) & (ids < n)).sum()
    g = (rng.standard_normal((batch, ldg)) * 0.05).astype(np.float32)
    g[2] = 0
    lr, b1, b2, eps = [float(np.float32(v)) for v in (3e-3, 0.9, 0.999, 1e-8)]      # the scalars as the C boundary carries them
    d = [dev(a) for a in full]
    user_rows_adam(d[0][:, :latent], d[1][:, :latent], d[2][:, :latent], dev(ids, torch.int32), dev(g), lr, b1, b2, eps, step, latent=latent)
    got = [host(t) for t in d]
    # bit for bit: the host loop in the header's operation order, float32
    loop = [a.copy() for a in full]
    R.sparse_adam_rows(loop[0][:, :latent], loop[1][:, :latent], loop[2][:, :latent], ids, g[:, :latent], lr, b1, b2, eps, step, dtype=np.float32)
    for name, a, b in zip(("V", "exp_avg", "exp_avg_sq"), got, loop):
        assert np.array_equal(bits(a), bits(b)), (name, float(np.max(np.abs(a - b))))
    # skipped rows and the columns past latent: untouched
    skipped = np.ones(n, bool)
    skipped[ids[(ids >= 0) & (ids < n)]] = False
    assert skipped.sum() == n - batch + 5
    for a, b in zip(got, full):
        assert np.array_equal(bits(a[skipped]), bits(b[skipped])) and np.array_equal(bits(a[:, latent:]), bits(b[:, latent:]))
    # the float64 rule, evaluated at the float32 scalars, within the bound tests/test_optimizers_gpu.py holds one Adam update to
    # (one_update_bound / state_bound: 16 x 2^-24 x the scales of the quantity, its step and the gradient's term)
    rule = [a.astype(np.float64) for a in full]
    R.sparse_adam_rows(rule[0][:, :latent], rule[1][:, :latent], rule[2][:, :latent], ids, g[:, :latent], lr, b1, b2, eps, step)
    G = np.zeros((n, ld))
    ok = (ids >= 0) & (ids < n)
    G[ids[ok], :latent] = np.abs(g[ok, :latent])
    bound_p = 16 * E24 * (np.abs(rule[0]) + np.abs(rule[0] - full[0]) + lr * G)
    worst = float(np.max(np.abs(got[0] - rule[0]) / np.maximum(bound_p, 1e-300)))
    assert np.all(np.abs(got[0] - rule[0]) <= bound_p), worst
    for k, scale in ((1, G), (2, G * G)):
        sb = 16 * E24 * (np.abs(rule[k]) + np.abs(full[k]) + scale)
        assert np.all(np.abs(got[k] - rule[k]) <= sb), k
    print("user_rows_adam latent %d ld %d step %d: worst parameter error / one-update bound %.3f" % (latent, ld, step, worst))


# ------------------------------------------------------------------------------------------------ 5. - 7. routes, epoch, determinism
# The bit-for-bit tests train MultiDAE with lam = 0: with the regulariser on, every Mult-DAE step (with or without a user table) sums
# the squared norms of W with float atomics (adam.hip: k_sumsq), whose order -- and last bit -- is not fixed between two runs.
def run_epoch(c, numerics, route, trainer="dae", seed=5, inject=True):
    from rectorch_amd.engine import RowBatch
    net, model = make(c, trainer, numerics, lam=0.0)
    set_moments(model, *moments0(c))
    smp = sampler(c)
    torch.manual_seed(seed)
    net.train()
    if route == "epoch":
        model.train_epoch(1, smp, verbose=0)
        return state_of(model)
    it = smp.iter_rows() if route == "rows" else iter(smp)
    for t, item in enumerate(it):
        if inject:
            model._rtx.inject = (dev(c["masks"][t], torch.uint8), None)
        if route == "rows":
            assert isinstance(item, RowBatch) and item.users.dtype == torch.int32 and item.users.is_cuda
            loss = model.train_batch(item)
        elif route == "tagged":
            loss = model.train_batch(item[0], item[1])
        else:       # untagged dense tensors, the ids on their own
            lo, hi = c["batches"][t]
            loss = model.train_batch(item[0].clone(), None, users=dev(c["ids"][lo:hi], torch.int32))
        assert np.isfinite(loss)
    return state_of(model)


@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
@pytest.mark.parametrize("latent,batch", SHAPES[:2])
def test_batch_routes_are_bit_equal(latent, batch, numerics):
    c = case_of(latent, batch)
    rows = run_epoch(c, numerics, "rows")
    assert_bit_equal(rows, run_epoch(c, numerics, "tagged"), "tagged")
    assert_bit_equal(rows, run_epoch(c, numerics, "dense"), "dense")
    start = [c["W0"], c["b0"], c["W1"], c["b1"]]
    assert not np.array_equal(rows[0], start[0]) and not np.array_equal(rows[-3], c["V"])


@pytest.mark.parametrize("trainer", ["dae", "ae"])
@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
@pytest.mark.parametrize("latent,batch", SHAPES[:2])
def test_train_epoch_equals_train_batches(latent, batch, numerics, trainer):
    """train_epoch announces batch t + 1 while step t runs and defers the join (bf16): every step must add ITS batch's users"""
    c = case_of(latent, batch)
    epoch = run_epoch(c, numerics, "epoch", trainer, inject=False)
    assert_bit_equal(epoch, run_epoch(c, numerics, "rows", trainer, inject=False), "epoch vs batches")
    # ... and the two runs are one: determinism
    assert_bit_equal(epoch, run_epoch(c, numerics, "epoch", trainer, inject=False), "two epochs from one seed")
    assert not np.array_equal(epoch[-3], c["V"])
    other = run_epoch(c, numerics, "epoch", trainer, seed=6, inject=False)
    assert not np.array_equal(bits(epoch[0]), bits(other[0]))          # (another seed: other dropout draws)


# ------------------------------------------------------------------------------------------------ 8. checkpoint
@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
def test_checkpoint_round_trip(numerics):
    from rectorch_amd.nets import CDAE_net
    from rectorch_amd.models import MultiDAE
    c = case_of(50, 37)
    batches = list(sampler(c).iter_rows())

    def steps(model, ts):
        for t in ts:
            model._rtx.inject = (dev(c["masks"][t], torch.uint8), None)
            model.train_batch(batches[t])
    net, model = make(c, "dae", numerics, lam=0.0)          # (lam = 0: see run_epoch)
    steps(model, [0, 1, 2])
    straight = state_of(model)
    net, model = make(c, "dae", numerics, lam=0.0)
    steps(model, [0, 1])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cdae.pth")
        model.save_model(path, 7)
        ck = torch.load(path, map_location="cpu")
        assert list(ck.keys()) == ["epoch", "state_dict", "optimizer", "user_optimizer"]
        assert "user_factors.weight" in ck["state_dict"] and ck["user_optimizer"]["state"][0]["step"] == 2
        assert len(ck["optimizer"]["param_groups"][0]["params"]) == 4
        fresh = MultiDAE(CDAE_net(R.N_ITEMS, R.N_USERS, 50), lam=0.0, learning_rate=LR, numerics=numerics)
        assert fresh.load_model(path)["epoch"] == 7
        # a MultiDAE_net checkpoint written by the same code has exactly the keys it had
        _, plain = make(c, plain=True)
        plain.save_model(os.path.join(tmp, "dae.pth"), 1)
        assert list(torch.load(os.path.join(tmp, "dae.pth"), map_location="cpu").keys()) == ["epoch", "state_dict", "optimizer"]
    assert fresh._rtx.adam_step == 2
    steps(fresh, [2])
    assert_bit_equal(straight, state_of(fresh), "save / load / third step")
    assert fresh.user_optimizer.state[fresh.network.user_factors.weight]["step"] == 3


def test_a_refused_step_leaves_the_count_and_takes_the_ids_back():
    """a step the engine refuses (a batch of the wrong width) does not advance SparseAdam's step count, and its ids are not left for
    the next call that runs the first layer"""
    from rectorch_amd import _lib
    c = case_of(50, 37)
    net, model = make(c, "dae", "fp32", predict_numerics="fp32")
    x, ids = dev(c["X"][:37]), dev(c["ids"][:37], torch.int32)
    model.train_batch(x, users=ids)
    p = net.user_factors.weight
    assert model.user_optimizer.state[p]["step"] == 1
    before = table(model)
    with pytest.raises(_lib.RtxError, match="n_items"):
        model.train_batch(dev(c["X"][:37, :299]), users=ids)
    assert model.user_optimizer.state[p]["step"] == 1
    for a, b in zip(table(model), before):
        assert np.array_equal(bits(a), bits(b))
    # the training engine's next forward, asked for without ids, adds no user term
    _, plain = make(c, plain=True)
    load(plain.network, dict(c, **{k: host(q) for k, q in zip(("W0", "b0", "W1", "b1"), net._param_list())}))
    assert np.array_equal(host(net._rtx_engines["fp32"].forward(x, training=False)[0]), host(plain.predict(x, remove_train=False)[0]))
    model.train_batch(x, users=ids)
    assert model.user_optimizer.state[p]["step"] == 2


# ------------------------------------------------------------------------------------------------ 9. evaluation
def _close(got, want, tag):
    """the comparison of tests/test_item_item_eval.py: bool arrays equal, float arrays NaN for NaN and within 1e-12"""
    assert set(got) == set(want), tag
    for m in want:
        g, w = np.asarray(got[m]), np.asarray(want[m])
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, m)
        if g.dtype == bool:
            assert np.array_equal(g, w), (tag, m)
        else:
            assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, m)
            ok = ~np.isnan(w)
            assert float(np.max(np.abs(g[ok] - w[ok]))) <= 1e-12, (tag, m)


def test_evaluation_routes():
    import random
    from rectorch_amd.evaluation import _recommend_route, evaluate, metrics_from_lists, one_plus_random, one_plus_random_host
    from rectorch_amd.metrics import Metrics
    c = case_of(50, 37)
    rng = np.random.default_rng(9)
    te = ((rng.random(c["X"].shape) < 0.05) & (c["X"] == 0)).astype(np.float32)
    te[:, 0] = np.where(te.sum(1) == 0, 1.0, te[:, 0])
    te[:, 0] = np.where(c["X"][:, 0] != 0, 0.0, te[:, 0])
    te[:, 1] = np.where(te.sum(1) == 0, 1.0, te[:, 1])
    net, model = make(c, "dae", "fp32")
    for t, rb in enumerate(sampler(c).iter_rows()):          # a trained table
        model.train_batch(rb)
    metrics = ["ndcg@10", "recall@5", "hit@10", "mrr@10"]
    x_all, ids_all = dev(c["X"]), dev(c["ids"], torch.int32)
    with_ids = host(model.predict(x_all, users=ids_all)[0])
    zero_user = host(model.predict(x_all)[0])
    known = c["ids"] >= 0
    assert not np.array_equal(with_ids[known], zero_user[known]) and np.array_equal(with_ids[~known], zero_user[~known])
    for tag, ids, scores in (("ids", "case", with_ids), ("no ids", None, zero_user)):
        smp = sampler(c, ids=ids, te=csr_matrix(te))
        assert smp.resident
        _close(evaluate(model, smp, metrics), Metrics.compute(scores, te, metrics), tag)
        random.seed(4)
        h = one_plus_random_host(model, smp, ["ndcg@10", "hit@10"], r=50)
        random.seed(4)
        d = one_plus_random(model, smp, ["ndcg@10", "hit@10"], r=50)
        for m in h:
            assert np.asarray(d[m]).shape == np.asarray(h[m]).shape and float(np.max(np.abs(np.asarray(d[m], np.float64) - np.asarray(h[m], np.float64)))) <= 1e-12, (tag, m)
        # top-N lists: per batch on the device, against the host lexsort of predict's scores
        assert _recommend_route(model, smp, 10) == "batch"
        items, vals = model.recommend(smp, 10)
        n = scores.shape[1]
        order = np.lexsort((np.broadcast_to(np.arange(n), scores.shape), -scores), axis=1)[:, :10].astype(np.int32)
        assert items.is_cuda and items.dtype == torch.int32 and np.array_equal(host(items), order), tag
        assert np.array_equal(bits(host(vals)), bits(np.take_along_axis(scores, order.astype(np.int64), axis=1)))
        lists = metrics_from_lists(items, csr_matrix(te), metrics)
        _close(lists, evaluate(model, smp, metrics), tag + " lists")


# ------------------------------------------------------------------------------------------------ 10. refusals at the C boundary
def test_c_boundary_refusals():
    from rectorch_amd import _lib
    from rectorch_amd.engine import Engine, Step, make_batch
    L = _lib.lib()
    V = torch.zeros(R.N_USERS, 16, device="cuda")
    m, v = torch.zeros_like(V), torch.zeros_like(V)

    def refused(rc, *needles):
        assert rc == -1, rc                                                 # RTX_EINVAL
        msg = L.rtx_last_error().decode()
        assert all(n in msg for n in needles), msg

    def bind(eng, *ts):
        return L.rtx_engine_bind_users(eng.handle, *[C.c_void_p(t.data_ptr()) if t is not None else None for t in ts], R.N_USERS)
    for args, kw in ((([R.N_ITEMS, 16], [16, R.N_ITEMS], "vae", 0.5, "fp32", 64), {}),
                     (([R.N_ITEMS, 32, 16], [16, 32, R.N_ITEMS], "dae", 0.5, "fp32", 64), {}),
                     (([R.N_ITEMS, 16], [16, 32, R.N_ITEMS], "dae", 0.5, "bf16", 64), {}),
                     (([R.N_ITEMS, 16], [16, R.N_ITEMS], "dae", 0.5, "fp32", 64), {"cond_dim": 3})):
        refused(bind(Engine(*args, **kw), V, m, v), "RTX_DAE or RTX_AE", "n_enc == 1")
    for variant, numerics in (("dae", "fp32"), ("ae", "bf16")):
        c = R.make_case(16)
        eng = Engine([R.N_ITEMS, 16], [16, R.N_ITEMS], variant, 0.5, numerics, 64)
        params = [dev(c[k]) for k in ("W0", "b0", "W1", "b1")]
        grads, m1, m2 = ([torch.zeros_like(p) for p in params] for _ in range(3))
        eng.bind(params, grads, m1, m2)
        refused(bind(eng, V, m, None), "exp_avg and exp_avg_sq come together")
        assert bind(eng, V, m, v) == 0
        start = [p.clone() for p in params]
        refused(L.rtx_engine_set_grad_clip(eng.handle, _lib.RTX_CLIP_NORM2, 1.0), "user table", "RTX_CLIP_NONE")
        refused(L.rtx_engine_set_grad_clip(eng.handle, _lib.RTX_CLIP_VALUE, 1.0), "user table")
        assert L.rtx_engine_set_grad_clip(eng.handle, _lib.RTX_CLIP_NONE, 0.0) == 0
        refused(L.rtx_engine_set_grad_accum(eng.handle, _lib.RTX_ACCUM_FIRST, 0.5), "user table", "RTX_ACCUM_OFF")
        cfg = _lib.DpCfg()
        cfg.rank, cfg.world, cfg.comm_dtype, cfg.emulate = 0, 1, _lib.RTX_FP32, 1
        assert L.rtx_engine_dp_attach(eng.handle, C.byref(cfg)) == -1        # (RTX_AE: refused for its own reason first)
        if variant == "dae":
            assert "user table" in L.rtx_last_error().decode()
        x = dev(c["X"][:8])
        b = make_batch(x, n_items=R.N_ITEMS)
        step = eng._step(inv_batch=1.0 / 8, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=1)
        out, tk = torch.zeros(8, R.N_ITEMS, device="cuda"), C.c_uint64()
        h = torch.zeros(8, 16, device="cuda")
        none, cb, st = None, _lib.LAYER_CB(), None
        refused(L.rtx_engine_train_step_dp(eng.handle, C.byref(b), C.byref(step), none, none, st), "train_step_dp", "rtx_engine_train_step")
        refused(L.rtx_engine_forward_train(eng.handle, C.byref(b), C.byref(step), C.c_void_p(out.data_ptr()), none, none, C.byref(tk), st),
                "forward_train", "rtx_engine_train_step")
        refused(L.rtx_engine_backward(eng.handle, C.byref(b), C.byref(step), C.c_uint64(1), C.c_void_p(out.data_ptr()), C.c_int64(R.N_ITEMS),
                                      none, none, cb, none, st), "backward", "user table")
        refused(L.rtx_engine_encode_train(eng.handle, C.byref(b), C.byref(step), C.c_void_p(h.data_ptr()), none, C.byref(tk), st), "encode_train")
        refused(L.rtx_engine_decode_train(eng.handle, C.c_void_p(h.data_ptr()), 8, C.c_void_p(out.data_ptr()), C.byref(tk), st), "decode_train")
        refused(L.rtx_engine_encode_backward(eng.handle, C.byref(b), C.byref(step), C.c_uint64(1), C.c_void_p(h.data_ptr()), none, cb, none, st),
                "encode_backward")
        refused(L.rtx_engine_decode_backward(eng.handle, 8, C.byref(step), C.c_uint64(1), C.c_void_p(out.data_ptr()), C.c_int64(R.N_ITEMS),
                                             none, cb, none, st), "decode_backward")
        from rectorch_amd.engine import CsrMatrix
        tr = CsrMatrix(csr_matrix(c["X"]))
        rows = torch.arange(8, dtype=torch.int32, device="cuda")
        with pytest.raises(_lib.RtxError, match="evaluate_topk.*user table.*rtx_topk_metrics_ex"):
            eng.evaluate_topk(tr, tr, rows, [0, 8], [5])
        with pytest.raises(_lib.RtxError, match="recommend.*user table.*rtx_topk_items"):
            eng.recommend(tr, rows, [0, 8], 5)
        # a training call with ids but step 0, and one on a table bound without moments
        ids = dev(np.arange(8), torch.int32)
        eng.set_users(ids, 8, 1e-3, 0.9, 0.999, 1e-8, 0)
        loss = torch.zeros(2, device="cuda")
        refused(L.rtx_engine_train_step(eng.handle, C.byref(b), C.byref(step), C.c_void_p(loss.data_ptr()), none, st), "step 0", "step >= 1")
        assert bind(eng, V, None, None) == 0
        eng.set_users(ids, 8, 1e-3, 0.9, 0.999, 1e-8, 1)
        assert L.rtx_engine_train_step(eng.handle, C.byref(b), C.byref(step), C.c_void_p(loss.data_ptr()), none, st) == -4      # RTX_ESTATE
        assert "inference only" in L.rtx_last_error().decode()
        torch.cuda.synchronize()
        # nothing was launched: parameters, table and moments are what they were
        for p, s in zip(params, start):
            assert torch.equal(p, s)
        assert not V.any() and not m.any() and not v.any()
        # set_users without a table
        bare = Engine([R.N_ITEMS, 16], [16, R.N_ITEMS], variant, 0.5, numerics, 64)
        assert L.rtx_engine_set_users(bare.handle, C.c_void_p(ids.data_ptr()), 1e-3, 0.9, 0.999, 1e-8, 1) == -4      # RTX_ESTATE
        assert "rtx_engine_bind_users" in L.rtx_last_error().decode()
    # the stand-alone operator's argument checks
    g = torch.zeros(8, 16, device="cuda")
    refused(L.rtx_user_rows_adam(V.data_ptr(), m.data_ptr(), v.data_ptr(), 16, R.N_USERS, ids.data_ptr(), g.data_ptr(), 16, 8, 16,
                                 1e-3, 0.9, 0.999, 1e-8, 0, None), "step count")
    refused(L.rtx_user_rows_adam(V.data_ptr(), m.data_ptr(), v.data_ptr(), 8, R.N_USERS, ids.data_ptr(), g.data_ptr(), 16, 8, 16,
                                 1e-3, 0.9, 0.999, 1e-8, 1, None), "ld >= latent")
