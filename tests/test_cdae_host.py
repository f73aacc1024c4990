"""CDAE (include/rectorch_hip.h "CDAE"): what needs no GPU -- the header text and the ctypes signatures of the three entry points, the
network class, the sampler's user ids, every refusal, and the float64 judge (tests/cdae_ref64.py) against itself in a second
formulation: the lazy row update written out in numpy against torch.optim.SparseAdam."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

from conftest import ROOT
import cdae_ref64 as R

from rectorch_amd import _lib, nets, parallel
from rectorch_amd.nets import CDAE_net, MultiDAE_net
from rectorch_amd.models import AETrainer, MultiDAE, MultiVAE, VAE
from rectorch_amd.samplers import DataSampler


def header():
    return open(os.path.join(ROOT, "include", "rectorch_hip.h")).read()


# ------------------------------------------------------------------------------------------------ the C boundary
def test_header_and_signatures():
    h = header()
    assert re.search(r"int\s+rtx_engine_bind_users\(rtx_engine\* e, float\* V, float\* exp_avg, float\* exp_avg_sq, int32_t n_users\);", h)
    assert re.search(r"int\s+rtx_engine_set_users\(rtx_engine\* e, const int32_t\* user_ids, float lr, float beta1, float beta2, float eps, "
                     r"int32_t step\);", h)
    assert re.search(r"int\s+rtx_user_rows_adam\(float\* V, float\* exp_avg, float\* exp_avg_sq, int64_t ld, int32_t n_users, "
                     r"const int32_t\* user_ids, const float\* g,\s+int64_t ldg, int32_t batch, int32_t latent, float lr, float beta1, "
                     r"float beta2, float eps, int32_t step, void\* stream\);", h)
    # the definition is text of the header: the formula, the rule and where an fma is not
    for needle in ("tanh( W0 . dropout(normalize(x_b)) + b0 + [u >= 0] . V[u] )", "torch.optim.SparseAdam", "NO fma anywhere",
                   "um = (g - m) * (float)(1 - beta1)", "p' = p - step_size * (m' / (sqrt(v') + eps))", "DISTINCT", "RTX_EINVAL"):
        assert needle in h, needle
    sig = _lib.SIGNATURES
    assert sig["rtx_engine_bind_users"] == (C.c_int, [C.c_void_p] * 4 + [C.c_int32])
    assert sig["rtx_engine_set_users"] == (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_float] * 4 + [C.c_int32])
    res, args = sig["rtx_user_rows_adam"]
    assert res is C.c_int and len(args) == 16 and args[3] is C.c_int64 and args[7] is C.c_int64 and args[-1] is C.c_void_p


# ------------------------------------------------------------------------------------------------ the network
def test_cdae_net_construction():
    assert "CDAE_net" in nets.__all__
    net = CDAE_net(300, 70, latent_size=50, dropout=0.25)
    assert isinstance(net, MultiDAE_net) and net._variant == "dae"
    assert (net.enc_dims, net.dec_dims, net.dropout.p) == ([300, 50], [50, 300], 0.25)
    assert CDAE_net(300, 70).latent_size == 50 and CDAE_net(300, 70).dropout.p == 0.5          # the reference's defaults
    assert list(net.state_dict().keys()) == ["enc_layers.0.weight", "enc_layers.0.bias", "dec_layers.0.weight", "dec_layers.0.bias",
                                             "user_factors.weight"]
    assert isinstance(net.user_factors, torch.nn.Embedding) and net.user_factors.sparse
    assert tuple(net.user_factors.weight.shape) == (70, 50) and not net.user_factors.weight.any()
    # the engine sees W and b only; the table is bound on its own and is not part of the cache key
    pl = net._param_list()
    assert [tuple(p.shape) for p in pl] == [(50, 300), (50,), (300, 50), (300,)]
    assert all(p is not net.user_factors.weight for p in pl)
    assert net._rtx_engine_key("bf16") == MultiDAE_net([50, 300])._rtx_engine_key("bf16") == "bf16"
    assert len(list(net.parameters())) == 5


def test_trainer_optimizers():
    net = CDAE_net(300, 70, 16)
    for model in (MultiDAE(net, learning_rate=2e-3), AETrainer(net, learning_rate=2e-3)):
        held = model.optimizer.param_groups[0]["params"]
        assert len(held) == 4 and all(a is b for a, b in zip(held, net._param_list()))
        uo = model.user_optimizer
        assert type(uo) is torch.optim.SparseAdam and model.user_optimizer is uo
        assert uo.param_groups[0]["params"] == [net.user_factors.weight] and uo.param_groups[0]["lr"] == 2e-3
        g, st = model._user_optim_state()
        assert list(st.keys()) == ["step", "exp_avg", "exp_avg_sq"] and st["step"] == 0           # as SparseAdam's own first step()
        assert st["exp_avg"].shape == net.user_factors.weight.shape and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
        assert net.user_factors.weight.grad is None
    with pytest.raises(AttributeError, match="CDAE_net"):
        MultiDAE(MultiDAE_net([16, 300])).user_optimizer


# ------------------------------------------------------------------------------------------------ the sampler
def small_matrix(n=9, items=20):
    rng = np.random.default_rng(3)
    return csr_matrix((rng.random((n, items)) < 0.3).astype(np.float32))


def test_sampler_user_ids_validation():
    X = small_matrix()
    with pytest.raises(ValueError, match="one id per row"):
        DataSampler(X, device="cpu", user_ids=np.arange(8))
    with pytest.raises(ValueError, match=r"\[-1, 2\^31\)"):
        DataSampler(X, device="cpu", user_ids=np.array([0, 1, 2, 3, 4, 5, 6, 7, -2]))
    with pytest.raises(ValueError, match="user 4 for 2 rows"):
        DataSampler(X, device="cpu", user_ids=np.array([0, 1, 2, 3, 4, 4, 6, 7, 8]))
    with pytest.raises(ValueError, match="int array"):
        DataSampler(X, device="cpu", user_ids=np.linspace(0, 1, 9))
    with pytest.raises(ValueError, match="'rows'"):
        DataSampler(X, device="cpu", user_ids="columns")
    ok = DataSampler(X, device="cpu", user_ids=np.array([-1, 5, 2, -1, 40, 0, -1, 7, 8]))      # -1 may repeat
    assert ok.max_user_id == 40 and ok.user_ids.dtype == np.int32
    assert DataSampler(X, device="cpu", user_ids="rows").max_user_id == 8
    assert DataSampler(X, device="cpu").user_ids is None and DataSampler(X, device="cpu").max_user_id == -1


def test_sampler_cpu_fallback_yields_ids():
    X = small_matrix()
    ids = np.array([-1, 5, 2, -1, 40, 0, -1, 7, 8], np.int32)
    got = [tr._rtx_users for tr, _ in DataSampler(X, None, 4, False, device="cpu", user_ids=ids)]
    assert [g.dtype for g in got] == [torch.int32] * 3
    assert [g.tolist() for g in got] == [[-1, 5, 2, -1], [40, 0, -1, 7], [8]]
    got = [tr._rtx_users.tolist() for tr, _ in DataSampler(X, X, 4, False, device="cpu", user_ids="rows")]
    assert got == [[0, 1, 2, 3], [4, 5, 6, 7], [8]]
    np.random.seed(11)
    order = list(range(9)); np.random.shuffle(order)
    np.random.seed(11)                  # (the sampler draws its permutation when the iteration starts)
    shuffled = [tr._rtx_users.numpy() for tr, _ in DataSampler(X, None, 4, True, device="cpu", user_ids=ids)]
    assert np.concatenate(shuffled).tolist() == ids[order].tolist()
    assert all(not hasattr(tr, "_rtx_users") for tr, _ in DataSampler(X, None, 4, False, device="cpu"))
    from rectorch_amd.engine import batch_users, RowBatch
    tr = next(iter(DataSampler(X, None, 4, False, device="cpu", user_ids=ids)))[0]
    assert batch_users(tr).tolist() == [-1, 5, 2, -1] and batch_users(tr, users=[1, 2, 3, 4]) == [1, 2, 3, 4]
    assert batch_users(torch.zeros(2, 3)) is None
    assert RowBatch(None, None, torch.arange(3), users="u").users == "u" and RowBatch(None, None, torch.arange(3)).users is None


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_what_is_supported():
    x, users = torch.zeros(4, 300), torch.arange(4, dtype=torch.int32)
    for cls in (VAE, MultiVAE):
        with pytest.raises(TypeError, match=r"MultiDAE\(CDAE_net\)"):
            cls(CDAE_net(300, 70, 8))

    def model():
        return MultiDAE(CDAE_net(300, 70, 8))
    m = model()
    with pytest.raises(ValueError, match="user_ids="):
        m.train_batch(x)                                        # no ids with the batch
    m = model(); m.custom_loss = True
    with pytest.raises(NotImplementedError, match="supported for a CDAE_net"):
        m.train_batch(x, users=users)
    m = model(); m.network.differentiable = True
    with pytest.raises(NotImplementedError, match="supported for a CDAE_net"):
        m.train_batch(x, users=users)
    with pytest.raises(NotImplementedError, match="supported: MultiDAE"):
        m.network(x)
    m = model(); m.accumulate_grad_batches = 2
    with pytest.raises(NotImplementedError, match="one batch per update"):
        m.train_batch(x, users=users)
    m = model(); m.clip_grad_norm = 1.0
    with pytest.raises(NotImplementedError, match="no clipping"):
        m.train_batch(x, users=users)
    m = model(); m.clip_grad_value = 0.5
    with pytest.raises(NotImplementedError, match="no clipping"):
        m.train_batch(x, users=users)
    m = model()
    with pytest.raises(NotImplementedError, match="single GPU"):
        parallel.attach(m)
    assert m._rtx.reducer is None
    m = model(); m.user_optimizer = torch.optim.Adam(m.network.user_factors.parameters())
    with pytest.raises(TypeError, match="SparseAdam"):
        m.train_batch(x, users=users)
    m = model(); m.user_optimizer = torch.optim.SparseAdam(m.network.user_factors.parameters(), maximize=True)
    with pytest.raises(ValueError, match="maximize"):
        m.train_batch(x, users=users)
    m = model(); m.user_optimizer = torch.optim.SparseAdam(torch.nn.Embedding(70, 8, sparse=True).parameters())
    with pytest.raises(ValueError, match="net.user_factors.weight"):
        m.train_batch(x, users=users)
    # a loader whose ids the table does not hold
    with pytest.raises(ValueError, match="70 user vectors"):
        model().train_epoch(1, DataSampler(csr_matrix(np.eye(80, 300, dtype=np.float32)), batch_size=40, device="cpu", user_ids="rows"), verbose=0)
    # users= for any other network is an error, not ignored
    with pytest.raises(ValueError, match="CDAE_net"):
        MultiDAE(MultiDAE_net([8, 300])).train_batch(x, users=users)


# ------------------------------------------------------------------------------------------------ the judge against itself
@pytest.mark.parametrize("loss", ["multinomial", "mse"])
def test_ref64_lazy_update_written_out(loss):
    """three steps of CdaeRef64 (torch.optim.SparseAdam) against the numpy rows loop fed with autograd's dense gradient of V"""
    c = R.make_case(50)
    ref = R.CdaeRef64([c["W0"], c["b0"], c["W1"], c["b1"]], c["V"], loss=loss, lr=1e-3, user_lr=3e-3)
    V, m, v = c["V"].astype(np.float64), np.zeros((R.N_USERS, 50)), np.zeros((R.N_USERS, 50))
    for t, (lo, hi) in enumerate(c["batches"]):
        ids, x, mask = c["ids"][lo:hi], c["X"][lo:hi], c["masks"][t]
        # the gradient of V's rows from a dense copy of the same network state
        twin = R.CdaeRef64(ref.params(), V, loss=loss)
        twin.emb = torch.nn.Embedding(R.N_USERS, 50, sparse=False).double()
        with torch.no_grad():
            twin.emb.weight.copy_(torch.from_numpy(V))
        twin.loss(twin.forward(x, ids, mask), x).backward()
        gV = twin.emb.weight.grad.numpy()
        before = (V.copy(), m.copy(), v.copy())
        R.sparse_adam_rows(V, m, v, ids, gV[np.clip(ids, 0, None)], 3e-3, 0.9, 0.999, 1e-8, t + 1)
        ref.train_batch(x, ids, mask)
        rV, rm, rv, step = ref.table()
        assert step == t + 1
        touched = np.zeros(R.N_USERS, bool); touched[ids[ids >= 0]] = True
        for got, want, old in zip((V, m, v), (rV, rm, rv), before):
            assert np.array_equal(got[~touched], old[~touched]) and np.array_equal(want[~touched], old[~touched])
            assert np.allclose(got[touched], want[touched], rtol=1e-12, atol=1e-300)
        moved = np.abs(V[touched] - before[0][touched]).max(axis=1) > 0
        assert moved.sum() >= touched.sum() - 1          # every touched row moved (but the empty row's user: its gradient is zero)
    assert touched.sum() < R.N_USERS


def test_ref64_without_users_is_the_plain_network():
    c = R.make_case(64)
    ref = R.CdaeRef64([c["W0"], c["b0"], c["W1"], c["b1"]], c["V"])
    x = c["X"][:37]
    none = ref.forward(x).detach().numpy()
    minus = ref.forward(x, np.full(37, -1)).detach().numpy()
    far = ref.forward(x, np.full(37, R.N_USERS)).detach().numpy()
    some = ref.forward(x, c["ids"][:37]).detach().numpy()
    assert np.array_equal(none, minus) and np.array_equal(none, far)
    has = c["ids"][:37] >= 0
    assert np.array_equal(some[~has], none[~has]) and not np.array_equal(some[has], none[has])
