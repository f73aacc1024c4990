"""The reference's plain variational autoencoder, VAE(VAE_net(...)) (rectorch/models.py:519-625, rectorch/nets.py:250-353), on
the engine variant RTX_GVAE: raw input rows, z sampled in every mode, sigmoid decoder, loss F.binary_cross_entropy + KLD.

Golden vectors: tests/golden/g15_vae_*.npz, written by tests/golden/make_golden_vae.py from the reference itself; every eps the
reference drew is injected (model._rtx.inject), as the G2 tests do.  The checkpoint the reference's save_model wrote is kept there
as arrays (ck_*) and reassembled into the dictionary torch.load returned for it.
"""
import json
import os
import random
import tempfile

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

from conftest import load_golden, sd_from

CASES = ("deep_bin", "deep_rat_sat", "one_bin")
B = 37


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-30, np.max(np.abs(b))))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


def reference_checkpoint(g):
    """the {'epoch', 'state_dict', 'optimizer'} dictionary the reference's VAE.save_model wrote (make_golden_vae.checkpoint_arrays)"""
    sd = {str(k): torch.from_numpy(np.array(g["ck_sd__%d" % i])) for i, k in enumerate(g["ck_sd_keys"])}
    state = {int(k): {n: torch.from_numpy(np.array(g["ck_opt__%s__%s" % (k, n)])) for n in names}
             for k, names in json.loads(str(g["ck_opt_state"])).items()}
    groups = json.loads(str(g["ck_opt_groups"]))
    for grp in groups:
        grp["betas"] = tuple(grp["betas"])
    return {"epoch": int(g["ck_epoch"]), "state_dict": sd, "optimizer": {"state": state, "param_groups": groups}}


def make_model(g, **kw):
    from rectorch_amd.nets import VAE_net
    from rectorch_amd.models import VAE
    net = VAE_net([int(d) for d in g["c__dec"]], [int(d) for d in g["c__enc"]])
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd_from(g, "c__sd0__").items()})
    return net, VAE(net, **kw)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_variant_mapping():
    from rectorch_amd import _lib
    from rectorch_amd.nets import VAE_net, MultiVAE_net, CMultiVAE_net, SVAE_net, MultiDAE_net
    from rectorch_amd.models import VAE, MultiVAE, CMultiVAE, AETrainer
    assert VAE_net([1, 2], [2, 1])._variant == "gvae"
    assert MultiVAE_net([2, 4])._variant == "vae"
    assert CMultiVAE_net(3, [2, 4])._variant == "vae"
    assert SVAE_net(10, 4, 6, [2, 10], [6, 2])._variant == "vae"
    assert MultiDAE_net([2, 4])._variant == "dae"
    cfg = _lib.make_cfg([300, 64, 16], [16, 64, 300], "gvae", "fp32", 0.0, 64)
    assert cfg.variant == _lib.RTX_GVAE == 2
    assert _lib.make_cfg([4, 2], [2, 4], "vae", "fp32", 0.5, 8).variant == _lib.RTX_VAE
    assert _lib.make_cfg([4, 2], [2, 4], "dae", "fp32", 0.5, 8).variant == _lib.RTX_DAE
    # the model-level variant follows the network: only VAE(VAE_net) is the BCE model
    assert VAE(VAE_net([1, 2], [2, 1]))._variant == "gvae"
    assert VAE(MultiVAE_net([2, 4]))._variant == "vae"
    assert MultiVAE(MultiVAE_net([2, 4]))._variant == "vae"
    assert CMultiVAE(CMultiVAE_net(3, [2, 4]))._variant == "vae"
    assert AETrainer(MultiDAE_net([2, 4]))._variant == "dae"
    assert VAE(VAE_net([1, 2], [2, 1]))._step_scalars() == (1.0, 0.0)
    assert VAE(MultiVAE_net([2, 4]))._step_scalars() == (0.0, 0.0)
    m = VAE(VAE_net([1, 2], [2, 1]))
    assert "_variant" not in str(m)            # a property: the reference-style repr lists instance attributes only
    # the networks' own encode / decode / forward stay as they were
    with pytest.raises(NotImplementedError):
        VAE_net([1, 2]).forward(torch.zeros(1, 2))
    # the loss of another network stays unavailable on VAE
    with pytest.raises(NotImplementedError):
        VAE(MultiVAE_net([2, 4])).loss_function(None, None, None, None)


def test_data_parallel_refuses_generic_vae():
    from rectorch_amd import _lib, parallel
    from rectorch_amd.nets import VAE_net
    from rectorch_amd.models import VAE
    model = VAE(VAE_net([2, 8], [8, 2]))
    with pytest.raises(_lib.RtxError, match="VAE_net"):
        parallel.attach(model, engine="python")
    assert model._rtx.reducer is None


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_fp32_forward_step_and_predict_against_reference(case):
    g = load_golden("g15_vae_" + case)
    x = dev(g["c__x"])
    net, model = make_model(g, numerics="fp32", learning_rate=1e-3)
    # forward with the reference's eps: p, mu, logvar
    eng = net.rtx_engine("fp32", B)
    p, mu, lv = eng.forward(x, training=True, noise=dev(g["c__eps_f"]))
    assert float(np.max(np.abs(p.cpu().numpy() - g["c__p"]))) < 1e-5
    assert rel(mu.cpu(), g["c__mu"]) < 1e-5 and rel(lv.cpu(), g["c__logvar"]) < 1e-5
    if case == "deep_rat_sat":
        assert int((p.cpu().numpy() == 1.0).sum()) > 100          # saturated probabilities, as in the reference
    # loss and every gradient of one backward
    model.keep_grads = True
    model._rtx.inject = (None, dev(g["c__eps_f"]))
    loss = model.train_batch(x)
    assert abs(loss - float(g["c__loss_f"])) <= 1e-6 * abs(float(g["c__loss_f"])), (loss, float(g["c__loss_f"]))
    for i, prm in enumerate(net._param_list()):
        assert rel(prm.grad.cpu(), g["c__grad_%d" % i]) < 1e-5, (case, i, rel(prm.grad.cpu(), g["c__grad_%d" % i]))
    # three Adam steps from the initial parameters with the reference's eps of each step
    net, model = make_model(g, numerics="fp32", learning_rate=1e-3)
    for t in range(3):
        model._rtx.inject = (None, dev(g["c__eps_%d" % t]))
        loss = model.train_batch(x, x)          # (te_batch is ignored, as in the reference)
        ref = float(g["c__loss_%d" % t])
        assert abs(loss - ref) <= 1e-6 * abs(ref), (t, loss, ref)
    for i, prm in enumerate(net._param_list()):
        assert float(np.max(np.abs(prm.detach().cpu().numpy() - g["c__param_%d" % i]))) < 5e-6, (case, i)
    # predict: eval mode, sampled with the reference's eps; with remove_train the stored entries are -inf
    model._rtx.inject = (None, dev(g["c__eps_p"]))
    pk, pmu, plv = model.predict(x, remove_train=False)
    assert float(np.max(np.abs(pk.cpu().numpy() - g["c__pred_keep"]))) < 1e-5
    assert rel(pmu.cpu(), g["c__pred_mu"]) < 1e-5 and rel(plv.cpu(), g["c__pred_logvar"]) < 1e-5
    pr = model.predict(x, remove_train=True)[0].cpu().numpy()
    assert np.array_equal(np.isneginf(pr), g["c__x"] != 0)
    keep = g["c__x"] == 0
    assert np.array_equal(pr[keep], pk.cpu().numpy()[keep])
    assert not net.training


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["deep_bin", "deep_rat_sat"])
def test_bf16_steps_against_reference(case):
    g = load_golden("g15_vae_" + case)
    x = dev(g["c__x"])
    net, model = make_model(g, numerics="bf16", learning_rate=1e-3)
    for t in range(3):
        model._rtx.inject = (None, dev(g["c__eps_%d" % t]))
        loss = model.train_batch(x)
        ref = float(g["c__loss_%d" % t])
        assert abs(loss - ref) < 2e-3 * abs(ref), (t, loss, ref)
    model._join()
    for i, prm in enumerate(net._param_list()):
        d = np.abs(prm.detach().cpu().numpy() - g["c__param_%d" % i])
        # an Adam step moves a parameter by at most ~lr: three steps bound the drift of a sign flip in a bf16 gradient
        assert float(d.max()) < 3.5e-3 and float(d.mean()) < 2e-4, (case, i, float(d.max()), float(d.mean()))


@pytest.mark.gpu
def test_loss_function_and_op_against_reference():
    from rectorch_amd import ops  # noqa: F401  (registers the ops)
    from rectorch_amd.engine import bce_kl_loss
    from rectorch_amd.nets import VAE_net
    from rectorch_amd.models import VAE
    m = load_golden("g15_vae_misc")
    model = VAE(VAE_net([1, 2], [2, 1]))
    args = [dev(m[k]) for k in ("lf_pred", "lf_gt", "lf_mu", "lf_logvar")]      # target 2 included
    loss = model.loss_function(*args)
    assert loss.dim() == 0 and loss.is_cuda
    ref = float(m["lf_loss"])
    assert abs(loss.item() - ref) <= 1e-6 * abs(ref), (loss.item(), ref)
    op = torch.ops.rectorch_hip.bce_kl_loss(*args)
    assert op.item() == loss.item()
    nokl = bce_kl_loss(args[0], args[1])
    assert abs(nokl.item() - float(m["lf_loss_nokl"])) <= 1e-6 * abs(float(m["lf_loss_nokl"]))
    assert torch.ops.rectorch_hip.bce_kl_loss(args[0], args[1], None, None).item() == nokl.item()
    # saturated p == 1.0 (the -100 clamp) and ratings up to 5: the reference's forward loss from its own p / mu / logvar
    for case in CASES:
        g = load_golden("g15_vae_" + case)
        val = model.loss_function(dev(g["c__p"]), dev(g["c__x"]), dev(g["c__mu"]), dev(g["c__logvar"])).item()
        ref = float(g["c__loss_f"])
        assert abs(val - ref) <= 1e-6 * abs(ref), (case, val, ref)


@pytest.mark.gpu
def test_reference_test_VAE_scenario_on_device():
    """reference tests/test_models.py:106-157 on the device, plus the reference-written checkpoint"""
    from rectorch_amd.nets import VAE_net
    from rectorch_amd.models import VAE
    from rectorch_amd.samplers import DataSampler
    net = VAE_net([1, 2], [2, 1])
    model = VAE(net)
    assert model.learning_rate == 1e-3 and isinstance(model.optimizer, torch.optim.Adam)
    assert str(model) == repr(model)
    train = csr_matrix((np.array([1., 1., 1.]), (np.array([0, 0, 1]), np.array([0, 1, 1]))))
    sampler = DataSampler(train, batch_size=1, shuffle=False)
    x = torch.FloatTensor([[1, 1], [2, 2]])
    model.predict(x, True)
    torch.manual_seed(12345)
    out_1 = model.predict(x, False)[0]
    assert out_1.shape == (2, 2) and bool(((out_1 >= 0) & (out_1 <= 1)).all())      # probabilities
    model.train(sampler, num_epochs=10, verbose=4)
    torch.manual_seed(12345)
    out_2 = model.predict(x, False)[0]
    assert not torch.all(out_1.eq(out_2)), "the outputs should be different"
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "vae.pth")
        model.save_model(path, 1)
        model2 = VAE(VAE_net([1, 2], [2, 1]))
        model2.load_model(path)
    torch.manual_seed(12345)
    out_1 = model.predict(x, False)[0]
    torch.manual_seed(12345)
    out_2 = model2.predict(x, False)[0]
    assert torch.all(out_1.eq(out_2)), "the outputs should be the same"
    # the checkpoint the reference's save_model wrote after the same scenario: loads, and scores as the reference did
    m = load_golden("g15_vae_misc")
    model3 = VAE(VAE_net([1, 2], [2, 1]))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reference_vae.pth")
        torch.save(reference_checkpoint(m), path)
        ck = model3.load_model(path)
    assert ck["epoch"] == 10
    assert model3._rtx.adam_step == int(float(ck["optimizer"]["state"][0]["step"])) > 0
    model3._rtx.inject = (None, dev(m["ck_eps"]))
    p = model3.predict(torch.from_numpy(m["ck_x"]), False)[0]
    assert float(np.max(np.abs(p.cpu().numpy() - m["ck_pred_keep"]))) < 1e-5


@pytest.mark.gpu
def test_predict_samples_in_eval_mode():
    g = load_golden("g15_vae_deep_bin")
    net, model = make_model(g, numerics="fp32")
    x = torch.from_numpy(g["c__x"].astype(np.float32))
    torch.manual_seed(3)
    p1, mu1, lv1 = model.predict(x, False)
    torch.manual_seed(3)
    p2, mu2, lv2 = model.predict(x, False)
    assert torch.equal(p1, p2) and torch.equal(mu1, mu2)
    p3, mu3, lv3 = model.predict(x, False)          # the next draw of the generator: another z
    assert not torch.equal(p1, p3)
    assert torch.equal(mu1, mu3) and torch.equal(lv1, lv3)
    assert not net.training


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
def test_resident_rows_equal_dense_step(numerics):
    """ratings 1..5 enter raw: the resident CSR rows, the dense tensor and the reference agree; the sparse first layer stays
    off for this variant even when asked for (k_in_chunks normalises what it streams)"""
    from rectorch_amd.samplers import DataSampler
    g = load_golden("g15_vae_deep_rat_sat")
    X = g["c__x"].astype(np.float32)
    losses, params = [], []
    for route in ("dense", "rows"):
        net, model = make_model(g, numerics=numerics, learning_rate=1e-3)
        eng = net.rtx_engine(numerics, B)
        eng.set_option("sparse_in", 1)
        ls = []
        for t in range(3):
            model._rtx.inject = (None, dev(g["c__eps_%d" % t]))
            if route == "dense":
                ls.append(model.train_batch(torch.from_numpy(X)))
            else:
                (rb,) = list(DataSampler(csr_matrix(X), batch_size=B, shuffle=False).iter_rows())
                ls.append(model._fused_step(rb, None, want_loss=True))
            assert eng.get_option("last_sparse_in") == 0
        model._join()
        losses.append(ls)
        params.append([p.detach().cpu().numpy() for p in net._param_list()])
    assert losses[0] == losses[1], losses
    for a, b in zip(*params):
        assert np.array_equal(a, b)
    if numerics == "fp32":
        for t in range(3):
            assert abs(losses[1][t] - float(g["c__loss_%d" % t])) <= 1e-6 * float(g["c__loss_%d" % t])


def _eval_setup(seed=21):
    from rectorch_amd.nets import VAE_net
    from rectorch_amd.models import VAE
    from rectorch_amd.samplers import DataSampler
    rng = np.random.RandomState(seed)
    U, I, S = 96, 1100, 6
    sat_items = rng.choice(I, S, replace=False)
    tr = (rng.rand(U, I) < 0.05).astype(np.float32)
    te = ((rng.rand(U, I) < 0.03) & (tr == 0)).astype(np.float32)
    te[:, sat_items] = 0.0                         # the tied saturated items are never relevant: tie order cannot matter
    tr[7] = 0.0
    te[5, :3] = 1.0
    tr[5, :3] = 0.0
    te[5, sat_items] = 0.0
    torch.manual_seed(seed)
    net = VAE_net([8, 32, I], [I, 32, 8])
    with torch.no_grad():
        net.dec_layers[-1].bias[torch.as_tensor(sat_items)] = 40.0       # p == 1.0 exactly: a tie at the top of every row
    model = VAE(net)
    smp = DataSampler(csr_matrix(tr), csr_matrix(te), batch_size=40, shuffle=False)
    return model, smp


@pytest.mark.gpu
def test_evaluation_routes_equal_host_loop():
    from rectorch_amd.evaluation import evaluate, evaluate_device, evaluate_host, one_plus_random, one_plus_random_host
    model, smp = _eval_setup()
    assert smp.resident
    metrics = ["ndcg@1", "ndcg@10", "ndcg@1024", "recall@5", "recall@100", "recall@1024", "hit@1", "hit@20", "mrr@10",
               "mrr@1024"]
    torch.manual_seed(11)
    host = evaluate_host(model, smp, metrics)
    for fn in (evaluate, evaluate_device):
        torch.manual_seed(11)
        got = fn(model, smp, metrics)
        for m in metrics:
            a, b = np.asarray(got[m], np.float64), np.asarray(host[m], np.float64)
            assert a.shape == b.shape == (96,), m
            assert np.array_equal(np.isnan(a), np.isnan(b)), m
            ok = ~np.isnan(b)
            assert float(np.max(np.abs(a[ok] - b[ok]))) <= 1e-12, (fn.__name__, m)
    # saturated ties are there: every row's top scores are exactly 1.0
    torch.manual_seed(11)
    rb = next(iter(smp.iter_rows()))
    assert int((model.predict(rb, remove_train=False)[0] == 1.0).sum(dim=1).min()) >= 6
    # the scores are sampled: another seed of torch's generator gives other metrics
    runs = []
    for seed in (11, 12):
        torch.manual_seed(seed)
        runs.append(np.nan_to_num(np.asarray(evaluate(model, smp, ["ndcg@100"])["ndcg@100"], np.float64)))
    assert not np.array_equal(*runs)
    opr_metrics = ["ndcg@10", "recall@5", "hit@10", "mrr@50"]
    random.seed(4)
    torch.manual_seed(13)
    h = one_plus_random_host(model, smp, opr_metrics, r=50)
    random.seed(4)
    torch.manual_seed(13)
    d = one_plus_random(model, smp, opr_metrics, r=50)
    for m in opr_metrics:
        a, b = np.asarray(d[m], np.float64), np.asarray(h[m], np.float64)
        assert a.shape == b.shape and float(np.max(np.abs(a - b))) <= 1e-12, m
