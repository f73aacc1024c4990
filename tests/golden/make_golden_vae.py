#!/usr/bin/env python
"""Generate the plain-VAE golden vectors (g15) by IMPORTING the reference (makgyver/rectorch), as make_golden.py does.

Run from the repo root:   python tests/golden/make_golden_vae.py

Writes tests/golden/g15_vae_<case>.npz (one file per case, each below 1 MiB) and tests/golden/g15_vae_misc.npz.  The misc file
also holds the checkpoint the reference's VAE.save_model writes after its tests/test_models.py::test_VAE scenario, as plain
arrays (ck_*: epoch, every state_dict tensor, the optimizer's param_groups as JSON and every optimizer state tensor), not as a
pickle: tests/test_generic_vae.py reassembles the dictionary torch.load returns for that file and checks here that the
reassembly is exact.

Model: VAE(VAE_net(dec_dims, enc_dims)) (reference models.py:519-625, nets.py:250-353): raw input, tanh hidden layers,
mu | logvar, z = mu + eps * exp(logvar / 2) drawn in every mode, sigmoid decoder, loss F.binary_cross_entropy(p, x) + KLD.
The eps of every forward pass is captured from the reference's own RNG (torch.randn_like under a fixed seed: VAE_net draws
nothing else), so the device run can inject it.

Cases (B = 37 users):
  deep_bin      enc [300, 64, 16] / dec [16, 64, 300], binary rows, one empty row
  deep_rat_sat  the same shapes, ratings 1..5, one empty row, last decoder bias uniform in [-30, 30]: saturated p == 1.0,
                the -100 clamp of log1p(-p) and the zero gradient where p (1 - p) == 0
  one_bin       enc [300, 8] / dec [8, 300] (one layer each), binary rows, one empty row
Per case: the initial parameters, forward p / mu / logvar with eps_f, the loss and every gradient of one backward, 3 Adam
steps (lr 1e-3) with eps_0..2 (the loss of each, the parameters after the third), predict under eps_p without remove_train
(with remove_train the same scores, -inf at the stored entries of x).
Global: loss_function on the reference test's tensors (pred = sigmoid(ones), gt = [[1, 1], [2, 1]], mu / logvar of encode(gt)).

Targets above one.  The reference trains on the rows as stored (ratings 1..5 included) and its test calls loss_function with a
target of 2, but the torch this script runs under refuses F.binary_cross_entropy targets outside [0, 1] on the CPU.  For such
targets only, the reference's F.binary_cross_entropy call is served by torch's own decomposition of the operator
(torch._decomp.decompositions.binary_cross_entropy / binary_cross_entropy_backward: the same element formula with the -100
clamps, and the backward (p - x) / max(p (1 - p), 1e-12) / numel of the native kernel) wrapped in an autograd Function;
targets inside [0, 1] go to the native operator unchanged.
"""
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True          # keep the reference tree pristine
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools", "ref_standins"))
sys.path.insert(0, "/root/reference")

import numpy as np                       # noqa: E402
import torch                             # noqa: E402
from scipy.sparse import csr_matrix      # noqa: E402

from rectorch.nets import VAE_net        # noqa: E402
from rectorch.models import VAE          # noqa: E402
from rectorch.samplers import DataSampler  # noqa: E402

B, LR = 37, 1e-3


class _BceDecomp(torch.autograd.Function):
    """F.binary_cross_entropy (mean) as torch's decomposition computes it, forward and backward, without the range check"""
    @staticmethod
    def forward(ctx, p, x):
        from torch._decomp import decompositions as dec
        ctx.save_for_backward(p, x)
        return dec.binary_cross_entropy(p, x)

    @staticmethod
    def backward(ctx, g):
        from torch._decomp import decompositions as dec
        p, x = ctx.saved_tensors
        return dec.binary_cross_entropy_backward(g, p, x), None


_native_bce = torch.nn.functional.binary_cross_entropy


def _bce(input, target, *args, **kwargs):
    if args or kwargs or bool(((target >= 0) & (target <= 1)).all()):
        return _native_bce(input, target, *args, **kwargs)
    return _BceDecomp.apply(input, target)


torch.nn.functional.binary_cross_entropy = _bce      # (what rectorch.models' F.binary_cross_entropy resolves to)


def eps_for(seed, shape):
    """what VAE_net._reparameterize draws after torch.manual_seed(seed): torch.randn_like(std) on a float32 [B, Z] tensor"""
    torch.manual_seed(seed)
    return torch.randn(shape)


def params(net):
    return [p.detach().numpy().copy() for p in net.parameters()]


def put_params(out, prefix, net):
    for k, v in net.state_dict().items():
        out["%s__%s" % (prefix, k.replace(".", "__"))] = v.numpy().copy()


def run_case(name, enc, dec, X, init_seed, sat_bias=False):
    torch.manual_seed(init_seed)
    net = VAE_net(list(dec), list(enc))
    if sat_bias:
        with torch.no_grad():
            g = torch.Generator().manual_seed(init_seed + 1)
            net.dec_layers[-1].bias.copy_(torch.rand(net.dec_layers[-1].bias.shape, generator=g) * 60.0 - 30.0)
    model = VAE(net, learning_rate=LR)
    out = {}
    pre = "c"
    out[pre + "__enc"] = np.array(enc, np.int32)
    out[pre + "__dec"] = np.array(dec, np.int32)
    out[pre + "__x"] = X.astype(np.uint8)
    put_params(out, pre + "__sd0", net)
    x = torch.from_numpy(X.astype(np.float32))
    Z = enc[-1]
    # forward + loss + one backward, eps captured
    ef = eps_for(1000 + init_seed, (B, Z))
    torch.manual_seed(1000 + init_seed)
    net.train()
    p, mu, lv = net(x)
    z = mu + ef * torch.exp(0.5 * lv)
    assert torch.equal(net.decode(z), p), "eps capture does not reproduce the reference's draw"
    loss = model.loss_function(p, x, mu, lv)
    net.zero_grad()
    loss.backward()
    out[pre + "__eps_f"] = ef.numpy()
    out[pre + "__p"] = p.detach().numpy()
    out[pre + "__mu"] = mu.detach().numpy()
    out[pre + "__logvar"] = lv.detach().numpy()
    out[pre + "__loss_f"] = np.float32(loss.item())
    for i, prm in enumerate(net.parameters()):
        out[pre + "__grad_%d" % i] = prm.grad.numpy().copy()
    net.zero_grad()
    # 3 Adam steps through the reference's train_batch
    for t in range(3):
        seed = 2000 + 10 * init_seed + t
        out[pre + "__eps_%d" % t] = eps_for(seed, (B, Z)).numpy()
        torch.manual_seed(seed)
        out[pre + "__loss_%d" % t] = np.float32(model.train_batch(x))
    for i, v in enumerate(params(net)):
        out[pre + "__param_%d" % i] = v
    # predict: eval mode, still sampled
    seed = 3000 + init_seed
    out[pre + "__eps_p"] = eps_for(seed, (B, Z)).numpy()
    torch.manual_seed(seed)
    pr, pmu, plv = model.predict(x, True)
    torch.manual_seed(seed)
    pk = model.predict(x, False)[0]
    assert torch.equal(torch.where(x != 0, torch.full_like(pk, -np.inf), pk), pr)
    out[pre + "__pred_keep"] = pk.numpy()
    out[pre + "__pred_mu"] = pmu.numpy()
    out[pre + "__pred_logvar"] = plv.numpy()
    np.savez_compressed(os.path.join(HERE, "g15_vae_%s.npz" % name), **out)
    return out


def checkpoint_arrays(ck):
    """the checkpoint dictionary {'epoch', 'state_dict', 'optimizer'} of AETrainer.save_model as npz-storable arrays"""
    out = {"ck_epoch": np.int64(ck["epoch"]), "ck_sd_keys": np.array(list(ck["state_dict"].keys()))}
    for i, v in enumerate(ck["state_dict"].values()):
        out["ck_sd__%d" % i] = v.numpy().copy()
    opt = ck["optimizer"]
    out["ck_opt_groups"] = np.array(json.dumps(opt["param_groups"]))
    out["ck_opt_state"] = np.array(json.dumps({str(k): list(v.keys()) for k, v in opt["state"].items()}))
    for k, st in opt["state"].items():
        for name, v in st.items():
            out["ck_opt__%s__%s" % (k, name)] = v.numpy().copy()
    return out


def checkpoint_from_arrays(g):
    """the inverse of checkpoint_arrays (tests/test_generic_vae.py does the same)"""
    sd = {str(k): torch.from_numpy(np.array(g["ck_sd__%d" % i])) for i, k in enumerate(g["ck_sd_keys"])}
    state = {int(k): {n: torch.from_numpy(np.array(g["ck_opt__%s__%s" % (k, n)])) for n in names}
             for k, names in json.loads(str(g["ck_opt_state"])).items()}
    groups = json.loads(str(g["ck_opt_groups"]))
    for grp in groups:
        grp["betas"] = tuple(grp["betas"])          # (a tuple in torch.optim.Adam's state_dict; JSON keeps lists)
    return {"epoch": int(g["ck_epoch"]), "state_dict": sd, "optimizer": {"state": state, "param_groups": groups}}


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return a == b


def main():
    rng = np.random.RandomState(15)
    I = 300
    Xb = (rng.rand(B, I) < 0.08).astype(np.float64)
    Xb[4] = 0.0
    Xr = ((rng.rand(B, I) < 0.1) * rng.randint(1, 6, size=(B, I))).astype(np.float64)
    Xr[11] = 0.0
    run_case("deep_bin", [I, 64, 16], [16, 64, I], Xb, 1)
    sat = run_case("deep_rat_sat", [I, 64, 16], [16, 64, I], Xr, 2, sat_bias=True)["c__p"]
    assert (sat == 1.0).sum() > 100, "the saturated case must saturate"
    run_case("one_bin", [I, 8], [8, I], Xb, 3)
    out = {}

    # the reference test's loss_function tensors (tests/test_models.py:121-127)
    torch.manual_seed(7)
    net = VAE_net([1, 2], [2, 1])
    model = VAE(net)
    gt = torch.FloatTensor([[1, 1], [2, 1]])
    mu, logvar = model.network.encode(gt)
    pred = torch.sigmoid(torch.FloatTensor([[1, 1], [1, 1]]))
    out["lf_pred"] = pred.numpy()
    out["lf_gt"] = gt.numpy()
    out["lf_mu"] = mu.detach().numpy()
    out["lf_logvar"] = logvar.detach().numpy()
    out["lf_loss"] = np.float32(model.loss_function(pred, gt, mu, logvar).item())
    out["lf_loss_nokl"] = np.float32(torch.nn.functional.binary_cross_entropy(pred, gt).item())

    # the reference test's scenario (tests/test_models.py:129-157): 10 epochs on the 2 x 2 sampler, then save_model
    torch.manual_seed(8)
    net = VAE_net([1, 2], [2, 1])
    model = VAE(net)
    train = csr_matrix((np.array([1., 1., 1.]), (np.array([0, 0, 1]), np.array([0, 1, 1]))))
    model.train(DataSampler(train, batch_size=1, shuffle=False), num_epochs=10, verbose=0)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "vae.pth")
        model.save_model(path, 10)
        ck = torch.load(path)
    arrays = checkpoint_arrays(ck)
    assert _same(checkpoint_from_arrays(arrays), ck), "the checkpoint does not survive its array form"
    out.update(arrays)
    xck = torch.FloatTensor([[1, 1], [2, 2]])
    out["ck_x"] = xck.numpy()
    out["ck_eps"] = eps_for(9, (2, 1)).numpy()
    torch.manual_seed(9)
    out["ck_pred_keep"] = model.predict(xck, False)[0].numpy()
    np.savez_compressed(os.path.join(HERE, "g15_vae_misc.npz"), **out)
    print("wrote g15_vae_{deep_bin,deep_rat_sat,one_bin,misc}.npz")


if __name__ == "__main__":
    main()
