"""The reference's plain autoencoder, AETrainer(MultiDAE_net(...)) (rectorch/models.py:325-516), on the engine variant RTX_AE:
MultiDAE_net's forward (normalised rows, dropout, tanh, raw outputs) trained with torch.nn.MSELoss against the rows as stored.

Golden vectors: tests/golden/g16_ae_*.npz, written by tests/golden/make_golden_ae.py from the reference itself; every keep-mask
the reference drew is injected (model._rtx.inject), as the G4 tests do.  The checkpoint the reference's save_model wrote is kept
there as arrays (ck_*) and reassembled into the dictionary torch.load returned for it.
"""
import ctypes as C
import json
import os
import re
import tempfile

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

from conftest import load_golden, sd_from

CASES = ("deep_rat", "one_bin", "wide_bin")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-30, np.max(np.abs(b))))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


def mask_of(g, name):
    """the keep-mask the reference drew (uint8 [B, n_items] on the device), or None for a network without dropout"""
    if float(g["c__dropout"]) == 0.0:
        return None
    n_items = int(g["c__enc"][0])
    return dev(np.unpackbits(g["c__" + name], axis=1)[:, :n_items], torch.uint8)


def reference_checkpoint(g):
    """the {'epoch', 'state_dict', 'optimizer'} dictionary the reference's save_model wrote (make_golden_ae.checkpoint_arrays)"""
    sd = {str(k): torch.from_numpy(np.array(g["ck_sd__%d" % i])) for i, k in enumerate(g["ck_sd_keys"])}
    state = {int(k): {n: torch.from_numpy(np.array(g["ck_opt__%s__%s" % (k, n)])) for n in names}
             for k, names in json.loads(str(g["ck_opt_state"])).items()}
    groups = json.loads(str(g["ck_opt_groups"]))
    for grp in groups:
        grp["betas"] = tuple(grp["betas"])
    return {"epoch": int(g["ck_epoch"]), "state_dict": sd, "optimizer": {"state": state, "param_groups": groups}}


def make_net(g):
    from rectorch_amd.nets import MultiDAE_net
    net = MultiDAE_net([int(d) for d in g["c__dec"]], [int(d) for d in g["c__enc"]], dropout=float(g["c__dropout"]))
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd_from(g, "c__sd0__").items()})
    return net


def make_model(g, **kw):
    from rectorch_amd.models import AETrainer
    net = make_net(g)
    return net, AETrainer(net, **kw)


def params_of(net):
    return [p.detach().cpu().numpy().copy() for p in net._param_list()]


# ------------------------------------------------------------------------------------------------------------ CPU
def test_variant_constant_and_entry_point():
    from rectorch_amd import _lib
    assert _lib.RTX_AE == 3
    assert _lib.VARIANTS["ae"] == _lib.RTX_AE
    assert _lib.make_cfg([300, 8], [8, 300], "ae", "fp32", 0.5, 64).variant == 3
    assert "rtx_mse_loss" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["rtx_mse_loss"]
    assert restype is C.c_int and len(argtypes) == 6
    header = open(os.path.join(ROOT, "include", "rectorch_hip.h")).read()
    assert re.search(r"#define\s+RTX_AE\s+3\b", header)
    assert re.search(r"int\s+rtx_mse_loss\(const float\* prediction, const float\* ground_truth, int32_t batch, int32_t n_items, "
                     r"float\* loss_out,\s*void\* stream\);", header)


def test_loss_kind_mapping():
    from rectorch_amd.nets import VAE_net, MultiVAE_net, CMultiVAE_net, SVAE_net, MultiDAE_net
    from rectorch_amd.models import AETrainer, VAE, MultiDAE, MultiVAE, CMultiVAE, SVAE
    ae = AETrainer(MultiDAE_net([2, 4]))
    assert ae._loss_kind == "mse" and ae._variant == "dae"
    dae = MultiDAE(MultiDAE_net([2, 4]))
    assert dae._loss_kind == "multinomial" and dae._variant == "dae"
    assert (VAE(VAE_net([1, 2], [2, 1]))._variant, VAE(VAE_net([1, 2], [2, 1]))._loss_kind) == ("gvae", "bce")
    assert (VAE(MultiVAE_net([2, 4]))._variant, VAE(MultiVAE_net([2, 4]))._loss_kind) == ("vae", "multinomial")
    assert (MultiVAE(MultiVAE_net([2, 4]))._variant, MultiVAE(MultiVAE_net([2, 4]))._loss_kind) == ("vae", "multinomial")
    cm = CMultiVAE(CMultiVAE_net(3, [2, 4]))
    assert (cm._variant, cm._loss_kind) == ("vae", "multinomial")
    sv = SVAE(SVAE_net(10, 4, 6, [2, 10], [6, 2]))
    assert (sv._variant, sv._loss_kind) == ("vae", "multinomial")

    class Mine(AETrainer):          # a user's subclass that keeps the base class's loss trains the plain autoencoder too
        pass

    class Other(AETrainer):
        def loss_function(self, prediction, ground_truth):
            return None
    assert Mine(MultiDAE_net([2, 4]))._loss_kind == "mse"
    assert Other(MultiDAE_net([2, 4]))._loss_kind == "multinomial"
    assert "_loss_kind" not in str(ae)         # a property: the reference-style repr lists instance attributes only
    # the loss kind is part of the key of the network's engine cache; forwards share the network's own engine
    net = MultiDAE_net([2, 4])
    assert net._rtx_engine_key("bf16", "mse") != net._rtx_engine_key("bf16", "multinomial") == net._rtx_engine_key("bf16") == "bf16"
    # a network that returns more than the reconstruction cannot be trained with the MSE (the reference fails on the tuple)
    with pytest.raises(NotImplementedError, match="MultiDAE_net"):
        AETrainer(MultiVAE_net([2, 4])).train_batch(torch.zeros(1, 4))


def test_data_parallel_refuses_plain_autoencoder():
    from rectorch_amd import _lib, parallel
    from rectorch_amd.nets import MultiDAE_net
    from rectorch_amd.models import AETrainer
    model = AETrainer(MultiDAE_net([2, 8], [8, 2]))
    with pytest.raises(_lib.RtxError, match="MSE"):
        parallel.attach(model, engine="python")
    assert model._rtx.reducer is None


def test_reference_checkpoint_arrays_reassemble():
    m = load_golden("g16_ae_misc")
    ck = reference_checkpoint(m)
    assert ck["epoch"] == 20
    assert list(ck["state_dict"].keys()) == ["enc_layers.0.weight", "enc_layers.0.bias", "dec_layers.0.weight", "dec_layers.0.bias"]
    assert [tuple(v.shape) for v in ck["state_dict"].values()] == [(1, 2), (1,), (2, 1), (2,)]
    for i, v in enumerate(ck["state_dict"].values()):
        assert v.dtype == torch.float32 and np.array_equal(v.numpy(), m["ck_sd__%d" % i])
    opt = ck["optimizer"]
    assert sorted(opt["state"].keys()) == [0, 1, 2, 3]
    for k, st in opt["state"].items():
        assert list(st.keys()) == ["step", "exp_avg", "exp_avg_sq"]
        assert float(st["step"]) == 40.0                       # 20 epochs x 2 batches
        assert st["exp_avg"].shape == ck["state_dict"][list(ck["state_dict"].keys())[k]].shape
        for n, v in st.items():
            assert np.array_equal(v.numpy(), m["ck_opt__%d__%s" % (k, n)])
    (grp, ) = opt["param_groups"]
    assert grp["lr"] == 1e-3 and grp["betas"] == (0.9, 0.999) and grp["weight_decay"] == 0 and grp["params"] == [0, 1, 2, 3]
    # torch's own optimizer and the network take it
    from rectorch_amd.nets import MultiDAE_net
    net = MultiDAE_net([1, 2], [2, 1], .1)
    net.load_state_dict(ck["state_dict"])
    torch.optim.Adam(net.parameters(), lr=1e-3).load_state_dict(opt)
    assert float(m["lf_loss"]) == 0.25


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_fp32_forward_step_and_predict_against_reference(case):
    g = load_golden("g16_ae_" + case)
    x = dev(g["c__x"])
    net, model = make_model(g, numerics="fp32", learning_rate=1e-3)
    # eval-mode outputs
    y = net.rtx_engine("fp32", x.shape[0]).forward(x, training=False)[0]
    err = float(np.max(np.abs(y.cpu().numpy() - g["c__y_eval"])))
    print("%s eval outputs: max abs %.3g" % (case, err))
    assert err < 1e-5
    # loss and every gradient of one backward, under the reference's keep-mask
    model.keep_grads = True
    model._rtx.inject = (mask_of(g, "mask_f"), None)
    loss = model.train_batch(x)
    ref = float(g["c__loss_f"])
    print("%s loss %.9g reference %.9g (rel %.3g)" % (case, loss, ref, abs(loss - ref) / abs(ref)))
    assert abs(loss - ref) <= 1e-6 * abs(ref), (loss, ref)
    for i, prm in enumerate(net._param_list()):
        r = rel(prm.grad.cpu(), g["c__grad_%d" % i])
        print("%s gradient %d: rel %.3g" % (case, i, r))
        assert r < 1e-5, (case, i, r)
    assert net._rtx_engines[("fp32", "mse")].variant == "ae"
    # three Adam steps from the initial parameters with the reference's keep-mask of each step
    net, model = make_model(g, numerics="fp32", learning_rate=1e-3)
    for t in range(3):
        model._rtx.inject = (mask_of(g, "mask_%d" % t), None)
        loss = model.train_batch(x, x)          # (te_batch is ignored, as in the reference)
        ref = float(g["c__loss_%d" % t])
        print("%s step %d loss %.9g reference %.9g (rel %.3g)" % (case, t, loss, ref, abs(loss - ref) / abs(ref)))
        assert abs(loss - ref) <= 1e-6 * abs(ref), (t, loss, ref)
    for i, prm in enumerate(net._param_list()):
        d = float(np.max(np.abs(prm.detach().cpu().numpy() - g["c__param_%d" % i])))
        print("%s parameter %d after 3 steps: max abs %.3g" % (case, i, d))
        assert d < 5e-6, (case, i, d)
    # predict: eval mode; with remove_train the stored entries are -inf
    model._rtx.inject = None
    pk = model.predict(x, remove_train=False)
    assert isinstance(pk, tuple) and len(pk) == 1
    pk = pk[0].cpu().numpy()
    assert float(np.max(np.abs(pk - g["c__pred_keep"]))) < 1e-5
    pr = model.predict(x, remove_train=True)[0].cpu().numpy()
    assert np.array_equal(np.isneginf(pr), g["c__x"] != 0)
    keep = g["c__x"] == 0
    assert np.array_equal(pr[keep], pk[keep])
    assert not net.training


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["deep_rat", "one_bin"])
def test_bf16_steps_against_reference(case):
    g = load_golden("g16_ae_" + case)
    x = dev(g["c__x"])
    net, model = make_model(g, numerics="bf16", learning_rate=1e-3)
    for t in range(3):
        model._rtx.inject = (mask_of(g, "mask_%d" % t), None)
        loss = model.train_batch(x)
        ref = float(g["c__loss_%d" % t])
        print("%s bf16 step %d loss %.9g reference %.9g (rel %.3g)" % (case, t, loss, ref, abs(loss - ref) / abs(ref)))
        assert abs(loss - ref) < 2e-3 * abs(ref), (t, loss, ref)
    model._join()
    for i, prm in enumerate(net._param_list()):
        d = np.abs(prm.detach().cpu().numpy() - g["c__param_%d" % i])
        print("%s bf16 parameter %d after 3 steps: max %.3g mean %.3g" % (case, i, float(d.max()), float(d.mean())))
        # an Adam step moves a parameter by at most ~lr: three steps bound the drift of a sign flip in a bf16 gradient
        assert float(d.max()) < 3.5e-3 and float(d.mean()) < 2e-4, (case, i, float(d.max()), float(d.mean()))


@pytest.mark.gpu
def test_loss_function_and_op_against_reference():
    from rectorch_amd import _lib, ops  # noqa: F401  (registers the ops)
    from rectorch_amd.engine import mse_loss
    from rectorch_amd.nets import MultiDAE_net
    from rectorch_amd.models import AETrainer
    m = load_golden("g16_ae_misc")
    model = AETrainer(MultiDAE_net([1, 2], [2, 1], .1))
    pred, gt = dev(m["lf_pred"]), dev(m["lf_gt"])      # a target of 2 included
    loss = model.loss_function(pred, gt)
    assert loss.dim() == 0 and loss.is_cuda
    ref = float(m["lf_loss"])
    assert abs(loss.item() - ref) <= 1e-6 * abs(ref), (loss.item(), ref)
    op = torch.ops.rectorch_hip.mse_loss(pred, gt)
    assert op.dim() == 0 and op.item() == loss.item()
    # each case's eval outputs against its stored rows (ratings up to 5; 301 and 4133 columns: rows of any alignment)
    for case in CASES:
        g = load_golden("g16_ae_" + case)
        y, x = dev(g["c__y_eval"]), dev(g["c__x"])
        want = float(np.mean((g["c__x"].astype(np.float64) - g["c__y_eval"].astype(np.float64)) ** 2))
        val = model.loss_function(y, x)
        print("%s mse %.9g float64 %.9g (rel %.3g)" % (case, val.item(), want, abs(val.item() - want) / want))
        assert abs(val.item() - want) <= 1e-6 * want, (case, val.item(), want)
        assert torch.ops.rectorch_hip.mse_loss(y, x).item() == val.item() == mse_loss(y, x).item()
    # the training forward's outputs give the reference's training loss
    g = load_golden("g16_ae_deep_rat")
    val = model.loss_function(dev(g["c__y_f"]), dev(g["c__x"])).item()
    assert abs(val - float(g["c__loss_f"])) <= 1e-6 * float(g["c__loss_f"])
    with pytest.raises(_lib.RtxError):
        model.loss_function(torch.zeros(0, 4), torch.zeros(0, 4))
    with pytest.raises(_lib.RtxError):
        model.loss_function(torch.zeros(2, 4), torch.zeros(2, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["wide_bin", "deep_rat"])
def test_loss_grads_padding_and_determinism(case, numerics):
    """rtx_engine_loss_grads with RTX_STEP_KEEP_GRADS: a batch below the padded batch and 301 / 4133 columns below the padded
    width (the second chunk of wide_bin is 37 columns wide): were a padded row or column of d loss / d logits not zero, the weight
    gradients would carry it.  Two identical runs give the same bits: loss, gradients and, after three steps, parameters."""
    from rectorch_amd import _lib
    g = load_golden("g16_ae_" + case)
    x = dev(g["c__x"])
    B = x.shape[0]
    runs = []
    for _ in range(2):
        net, model = make_model(g, numerics=numerics, learning_rate=1e-3)
        st, _, m, v = model._ensure_train_state()
        eng = net.rtx_engine(numerics, B, train_buffers=(st.grads, m, v), loss="mse")
        assert eng.variant == "ae"
        step = eng._step(mask=mask_of(g, "mask_f"), inv_batch=1.0 / B, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=1,
                         lam=0.3, beta=0.7,                      # both ignored by this variant
                         flags=_lib.RTX_STEP_KEEP_GRADS)
        eng.loss_grads(x, None, step, st.loss_buf[0:1], st.loss_buf[1:2])
        torch.cuda.synchronize()
        loss = float(st.loss_buf[0].item())
        grads = [t.detach().cpu().numpy().copy() for t in st.grads]
        ref = float(g["c__loss_f"])
        tol_l, tol_g = (1e-6, 1e-5) if numerics == "fp32" else (2e-3, None)
        assert abs(loss - ref) <= tol_l * abs(ref), (loss, ref)
        for i, gr in enumerate(grads):
            assert np.isfinite(gr).all()
            if tol_g is not None:
                assert rel(gr, g["c__grad_%d" % i]) < tol_g, (case, i, rel(gr, g["c__grad_%d" % i]))
        assert np.array_equal(params_of(net)[0], sd_from(g, "c__sd0__")["enc_layers.0.weight"])     # no optimizer ran
        losses = []
        for t in range(3):
            model._rtx.inject = (mask_of(g, "mask_%d" % t), None)
            losses.append(model.train_batch(x))
        model._join()
        runs.append((loss, grads, losses, params_of(net)))
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2], (runs[0][0], runs[1][0], runs[0][2], runs[1][2])
    for a, b in zip(runs[0][1] + runs[0][3], runs[1][1] + runs[1][3]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
def test_resident_rows_equal_dense_step(numerics):
    """ratings 1..5 are the loss target as stored: the resident CSR rows, the dense tensor and the reference agree"""
    from rectorch_amd.samplers import DataSampler
    g = load_golden("g16_ae_deep_rat")
    X = g["c__x"].astype(np.float32)
    B = X.shape[0]
    losses, params = [], []
    for route in ("dense", "rows"):
        net, model = make_model(g, numerics=numerics, learning_rate=1e-3)
        ls = []
        for t in range(3):
            model._rtx.inject = (mask_of(g, "mask_%d" % t), None)
            if route == "dense":
                ls.append(model.train_batch(torch.from_numpy(X)))
            else:
                (rb,) = list(DataSampler(csr_matrix(X), batch_size=B, shuffle=False).iter_rows())
                ls.append(model._fused_step(rb, None, want_loss=True))
        model._join()
        losses.append(ls)
        params.append(params_of(net))
    assert losses[0] == losses[1], losses
    for a, b in zip(*params):
        assert np.array_equal(a, b)
    if numerics == "fp32":
        for t in range(3):
            assert abs(losses[1][t] - float(g["c__loss_%d" % t])) <= 1e-6 * float(g["c__loss_%d" % t])


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
def test_train_epoch_on_resident_sampler_equals_train_batches(numerics):
    """two batches (19 + 18 users) through train_epoch -- the second announced to the engine while the first runs, the join
    between them deferred (bf16) -- end with the parameters of the same two train_batch calls; the dropout seeds come from torch's
    generator in the same order on both routes"""
    from rectorch_amd.samplers import DataSampler
    g = load_golden("g16_ae_deep_rat")
    X = g["c__x"].astype(np.float32)
    res = []
    for route in ("epoch", "batches"):
        net, model = make_model(g, numerics=numerics, learning_rate=1e-3)
        smp = DataSampler(csr_matrix(X), batch_size=19, shuffle=False)
        assert smp.resident and len(smp) == 2
        torch.manual_seed(5)
        if route == "epoch":
            model.train_epoch(1, smp, verbose=0)          # (its closing log line reads and clears the engine's loss sum)
        else:
            net.train()
            losses = [model.train_batch(torch.from_numpy(X[:19])), model.train_batch(torch.from_numpy(X[19:]), torch.from_numpy(X[19:]))]
            assert all(np.isfinite(l) and l > 0 for l in losses), losses
        model._join()
        assert model._rtx.adam_step == 2
        res.append(params_of(net))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert not np.array_equal(res[0][0], sd_from(g, "c__sd0__")["enc_layers.0.weight"])


def _eval_setup(seed=31):
    from rectorch_amd.nets import MultiDAE_net
    from rectorch_amd.models import AETrainer
    from rectorch_amd.samplers import DataSampler
    rng = np.random.RandomState(seed)
    U, I = 50, 301
    tr = (rng.rand(U, I) < 0.08).astype(np.float32) * rng.randint(1, 6, size=(U, I)).astype(np.float32)
    te = ((rng.rand(U, I) < 0.05) & (tr == 0)).astype(np.float32)
    tr[3] = 0.0                                    # a user without history
    te[:, 0] = np.where(te.sum(1) == 0, 1.0, te[:, 0])
    torch.manual_seed(seed)
    model = AETrainer(MultiDAE_net([16, 64, I], dropout=0.5), numerics="fp32", predict_numerics="fp32")
    smp = DataSampler(csr_matrix(tr), csr_matrix(te), batch_size=16, shuffle=False)
    return model, smp, tr


@pytest.mark.gpu
def test_evaluation_and_recommend_routes_equal_host_loop():
    from rectorch_amd.evaluation import _recommend_route, evaluate, evaluate_host, recommend_host
    model, smp, tr = _eval_setup()
    assert smp.resident
    (rb,) = list(type(smp)(csr_matrix(tr), batch_size=50, shuffle=False).iter_rows())
    for _ in range(2):                             # a trained model: two MSE steps
        model._fused_step(rb, None, want_loss=False)
    metrics = ["ndcg@10", "recall@5", "hit@10", "mrr@10"]
    host = evaluate_host(model, smp, metrics)
    got = evaluate(model, smp, metrics)
    for m in metrics:
        a, b = np.asarray(got[m], np.float64), np.asarray(host[m], np.float64)
        assert a.shape == b.shape == (50,), m
        assert np.array_equal(np.isnan(a), np.isnan(b)), m
        ok = ~np.isnan(b)
        assert float(np.max(np.abs(a[ok] - b[ok]))) <= 1e-12, m
    # top-N lists: the whole loader in one engine call, against predict + a host sort
    assert _recommend_route(model, smp, 10) == "engine"
    want = recommend_host(model, smp, 10)
    items, scores = model.recommend(smp, 10)
    assert items.is_cuda and items.dtype == torch.int32 and items.shape == (50, 10)
    assert torch.equal(items.cpu(), want[0].cpu())
    assert torch.equal(scores.cpu().view(torch.int32), want[1].cpu().view(torch.int32))
    seen = np.take_along_axis(tr, items.cpu().numpy().astype(np.int64), axis=1)
    assert (seen == 0).all()


@pytest.mark.gpu
def test_one_plus_random_save_and_load():
    """the inherited pieces: one_plus_random on the device, save_model / load_model, and the reference-written checkpoint"""
    import random
    from rectorch_amd.evaluation import one_plus_random, one_plus_random_host
    from rectorch_amd.nets import MultiDAE_net
    from rectorch_amd.models import AETrainer
    model, smp, tr = _eval_setup()
    opr_metrics = ["ndcg@10", "hit@10"]
    random.seed(4)
    h = one_plus_random_host(model, smp, opr_metrics, r=50)
    random.seed(4)
    d = one_plus_random(model, smp, opr_metrics, r=50)
    for m in opr_metrics:
        a, b = np.asarray(d[m], np.float64), np.asarray(h[m], np.float64)
        assert a.shape == b.shape and float(np.max(np.abs(a - b))) <= 1e-12, m
    x = torch.from_numpy(tr[:8])
    model.train_batch(x)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ae.pth")
        model.save_model(path, 1)
        model2 = AETrainer(MultiDAE_net([16, 64, 301], dropout=0.5), numerics="fp32")
        ck = model2.load_model(path)
    assert ck["epoch"] == 1 and model2._rtx.adam_step == 1
    assert torch.equal(model.predict(x, False)[0], model2.predict(x, False)[0])
    # the checkpoint the reference's save_model wrote after its test_AETrainer scenario: loads, and scores as the reference did
    m = load_golden("g16_ae_misc")
    model3 = AETrainer(MultiDAE_net([1, 2], [2, 1], .1))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "reference_ae.pth")
        torch.save(reference_checkpoint(m), path)
        ck = model3.load_model(path)
    assert ck["epoch"] == 20 and model3._rtx.adam_step == 40
    p = model3.predict(torch.from_numpy(m["ck_x"]), False)[0]
    assert float(np.max(np.abs(p.cpu().numpy() - m["ck_pred_keep"]))) < 1e-5
    model3.train_batch(torch.from_numpy(m["ck_x"]))           # training resumes from the loaded optimizer state
    assert model3._rtx.adam_step == 41


@pytest.mark.gpu
def test_mse_and_multinomial_trainers_stay_apart():
    """MultiDAE and AETrainer on copies of one initial state take one step each: the first optimises the multinomial loss + its
    norm regulariser, the second the MSE, and on ONE shared network they never share a training engine."""
    from rectorch_amd.models import AETrainer, MultiDAE
    g = load_golden("g16_ae_one_bin")          # no dropout: the training forward is the eval forward
    x = dev(g["c__x"])
    B = x.shape[0]
    net_d, net_a = make_net(g), make_net(g)
    dae = MultiDAE(net_d, lam=0.2, numerics="fp32")
    ae = AETrainer(net_a, numerics="fp32")
    y0 = net_d.rtx_engine("fp32", B).forward(x, training=False)[0]
    want_dae = dae.loss_function(y0, x).item()
    want_ae = ae.loss_function(y0, x).item()
    l_dae = dae.train_batch(x)
    l_ae = ae.train_batch(x)
    # float32 sums of 300 terms per row in another order than the stand-alone operators', and 1 / (B I) rounded once more in the
    # step: a few 1e-7 each, bounded by 2e-6; the multinomial loss adds its log-sum-exp and the regulariser: 1e-5
    assert abs(l_dae - want_dae) <= 1e-5 * abs(want_dae), (l_dae, want_dae)
    assert abs(l_ae - want_ae) <= 2e-6 * abs(want_ae), (l_ae, want_ae)
    assert abs(l_ae - float(g["c__loss_0"])) <= 1e-6 * float(g["c__loss_0"])
    assert abs(l_dae - l_ae) > 0.5 * abs(l_ae)                    # two different objectives, on different scales
    assert list(net_d._rtx_engines.keys()) == ["fp32"] and net_d._rtx_engines["fp32"].variant == "dae"
    assert net_a._rtx_engines[("fp32", "mse")].variant == "ae"
    assert not np.array_equal(params_of(net_d)[0], params_of(net_a)[0])
    # one network, two trainers
    net = make_net(g)
    dae, ae = MultiDAE(net, lam=0.2, numerics="fp32"), AETrainer(net, numerics="fp32")
    for _ in range(2):
        l1 = dae.train_batch(x)
        e_dae = net._rtx_engines["fp32"]
        l2 = ae.train_batch(x)
        e_ae = net._rtx_engines[("fp32", "mse")]
        assert e_dae is not e_ae and e_dae.handle.value != e_ae.handle.value and (e_dae.variant, e_ae.variant) == ("dae", "ae")
        assert net._rtx_engines["fp32"] is e_dae
    # each saw the other's update: the second MSE loss is computed on parameters both trainers moved
    y = net.rtx_engine("fp32", B).forward(x, training=False)[0]
    assert np.isfinite(l1) and np.isfinite(l2) and torch.isfinite(y).all()
    # predictions run on the network's own engine: one forward for both trainers
    assert torch.equal(dae.predict(x, False)[0], ae.predict(x, False)[0])
    assert set(net._rtx_engines.keys()) == {"fp32", ("fp32", "mse")}


@pytest.mark.gpu
def test_engine_refusals():
    from rectorch_amd import _lib
    from rectorch_amd.engine import Engine
    with pytest.raises(_lib.RtxError, match=r"error -1: .*RTX_AE"):
        Engine([300, 8], [8, 300], "ae", 0.5, "fp32", 64, cond_dim=2)
    eng = Engine([300, 8], [8, 300], "ae", 0.5, "fp32", 64)
    cfg = _lib.DpCfg()
    cfg.rank, cfg.world, cfg.comm_dtype, cfg.emulate = 0, 1, _lib.RTX_FP32, 1
    assert _lib.lib().rtx_engine_dp_attach(eng.handle, C.byref(cfg)) == -1            # RTX_EINVAL
    assert b"RTX_AE" in _lib.lib().rtx_last_error()
    assert _lib.lib().rtx_abi_version() == 8
