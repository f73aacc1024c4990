#!/usr/bin/env python
"""Generate the plain-autoencoder golden vectors (g16) by IMPORTING the reference (makgyver/rectorch), as make_golden.py and
make_golden_vae.py do.

Run on the CPU from the repo root:   python tests/golden/make_golden_ae.py
(the reference checkout is looked for where RECTORCH_REFERENCE points, by default where make_golden.py looks)

Writes tests/golden/g16_ae_<case>.npz (one file per case, each below 1 MiB) and tests/golden/g16_ae_misc.npz.  The misc file also
holds the checkpoint the reference's AETrainer.save_model writes after its tests/test_models.py::test_AETrainer scenario, as
plain arrays (ck_*, the layout of g15_vae_misc.npz), not as a pickle: tests/test_plain_autoencoder.py reassembles the dictionary
torch.load returns for that file, and this script checks that the reassembly is exact.

Model: AETrainer(MultiDAE_net(dec_dims, enc_dims, dropout)) (reference models.py:325-516, nets.py:175-247): L2-normalised
input, dropout in training, tanh on every layer but the decoder's last, raw outputs; loss torch.nn.MSELoss()(x, y) against the
rows as stored (ratings included).  The keep-mask of every training forward is captured by seeded replay, as make_golden.py
does for G4: torch.manual_seed(s) then F.dropout(ones) is what MultiDAE_net.forward draws, so the device run can inject it.

Cases:
  deep_rat   B = 37, enc [301, 64, 16] / dec [16, 64, 301], dropout 0.5, ratings 1..5, one empty row
  one_bin    B = 37, enc [300, 8] / dec [8, 300] (one layer each), dropout 0, binary rows, one empty row
  wide_bin   B = 5, enc [4133, 4] / dec [4, 4133], dropout 0, binary rows: two 4096-column chunks of the loss kernel, the second
             37 columns wide; stored entries in both chunks, at columns 4095 and 4096 among them
Per case: the initial parameters, the eval-mode outputs, the loss and every gradient of one training backward (mask_f), 3 Adam
steps (lr 1e-3) with mask_0..2 (the loss of each, the parameters after the third), predict without remove_train (with
remove_train the same scores, -inf at the stored entries of x: checked here).
Global (misc): loss_function on the reference test's tensors (pred = ones, gt = [[1, 1], [2, 1]]: 0.25) and the reference
test's scenario (20 epochs on the 2 x 2 sampler, save_model, predict of [[1, 1], [2, 2]]).
"""
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True          # keep the reference tree pristine
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools", "ref_standins"))
sys.path.insert(0, os.environ.get("RECTORCH_REFERENCE", "/root/reference"))

import numpy as np                       # noqa: E402
import torch                             # noqa: E402
import torch.nn.functional as F          # noqa: E402
from scipy.sparse import csr_matrix      # noqa: E402

from rectorch.nets import MultiDAE_net   # noqa: E402
from rectorch.models import AETrainer    # noqa: E402
from rectorch.samplers import DataSampler  # noqa: E402

LR = 1e-3


def mask_for(seed, shape, p):
    """the keep-mask MultiDAE_net.encode draws after torch.manual_seed(seed): nn.Dropout(p) on a float32 [B, I] tensor"""
    torch.manual_seed(seed)
    return (F.dropout(torch.ones(shape), p, True) != 0).numpy().astype(np.uint8)


def params(net):
    return [p.detach().numpy().copy() for p in net.parameters()]


def put_params(out, prefix, net):
    for k, v in net.state_dict().items():
        out["%s__%s" % (prefix, k.replace(".", "__"))] = v.numpy().copy()


def run_case(name, enc, dec, X, dropout, init_seed):
    B, I = X.shape
    torch.manual_seed(init_seed)
    net = MultiDAE_net(list(dec), list(enc), dropout)
    model = AETrainer(net, learning_rate=LR)
    out = {}
    pre = "c"
    out[pre + "__enc"] = np.array(enc, np.int32)
    out[pre + "__dec"] = np.array(dec, np.int32)
    out[pre + "__dropout"] = np.float64(dropout)
    out[pre + "__x"] = X.astype(np.uint8)
    put_params(out, pre + "__sd0", net)
    x = torch.from_numpy(X.astype(np.float32))
    # eval-mode outputs
    net.eval()
    with torch.no_grad():
        out[pre + "__y_eval"] = net(x).numpy().copy()
    # one training forward + loss + backward, keep-mask captured
    seed = 1000 + init_seed
    mf = mask_for(seed, (B, I), dropout)
    out[pre + "__mask_f"] = np.packbits(mf, axis=1)
    net.train()
    torch.manual_seed(seed)
    y = net(x)
    h = F.normalize(x) * torch.from_numpy(mf.astype(np.float32)) / (1.0 - dropout)
    for layer in net.enc_layers:
        h = torch.tanh(layer(h))
    assert torch.equal(net.decode(h), y), "mask capture does not reproduce the reference's draw"
    loss = model.loss_function(y, x)
    net.zero_grad()
    loss.backward()
    out[pre + "__y_f"] = y.detach().numpy()
    out[pre + "__loss_f"] = np.float32(loss.item())
    for i, prm in enumerate(net.parameters()):
        out[pre + "__grad_%d" % i] = prm.grad.numpy().copy()
    net.zero_grad()
    # 3 Adam steps through the reference's train_batch
    for t in range(3):
        seed = 2000 + 10 * init_seed + t
        out[pre + "__mask_%d" % t] = np.packbits(mask_for(seed, (B, I), dropout), axis=1)
        torch.manual_seed(seed)
        out[pre + "__loss_%d" % t] = np.float32(model.train_batch(x))
    for i, v in enumerate(params(net)):
        out[pre + "__param_%d" % i] = v
    # predict: eval mode, nothing drawn
    pr = model.predict(x, True)[0]
    pk = model.predict(x, False)[0]
    assert torch.equal(torch.where(x != 0, torch.full_like(pk, -np.inf), pk), pr)
    out[pre + "__pred_keep"] = pk.numpy()
    path = os.path.join(HERE, "g16_ae_%s.npz" % name)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
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
    """the inverse of checkpoint_arrays (tests/test_plain_autoencoder.py does the same)"""
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
    rng = np.random.RandomState(16)
    B = 37
    Xr = ((rng.rand(B, 301) < 0.1) * rng.randint(1, 6, size=(B, 301))).astype(np.float64)
    Xr[11] = 0.0
    Xr[0, 300] = 4.0                      # a stored entry in the masked tail group of the row
    Xb = (rng.rand(B, 300) < 0.08).astype(np.float64)
    Xb[4] = 0.0
    Xw = (rng.rand(5, 4133) < 0.02).astype(np.float64)
    Xw[1, 4095] = Xw[1, 4096] = 1.0       # the last column of the first chunk, the first of the second
    Xw[2, 4132] = 1.0                     # the last item
    Xw[3, 4096:] = 0.0                    # a row with nothing in the second chunk
    assert Xw[:, :4096].any() and Xw[:, 4096:].any()
    run_case("deep_rat", [301, 64, 16], [16, 64, 301], Xr, 0.5, 1)
    run_case("one_bin", [300, 8], [8, 300], Xb, 0.0, 2)
    run_case("wide_bin", [4133, 4], [4, 4133], Xw, 0.0, 3)
    out = {}

    # the reference test's loss_function tensors (tests/test_models.py:71-73): a target of 2
    model = AETrainer(MultiDAE_net([1, 2], [2, 1], .1))
    gt = torch.FloatTensor([[1, 1], [2, 1]])
    pred = torch.FloatTensor([[1, 1], [1, 1]])
    out["lf_pred"] = pred.numpy()
    out["lf_gt"] = gt.numpy()
    out["lf_loss"] = np.float32(model.loss_function(pred, gt).item())
    assert out["lf_loss"] == np.float32(0.25)

    # the reference test's scenario (tests/test_models.py:75-102): 20 epochs on the 2 x 2 sampler, then save_model
    torch.manual_seed(8)
    net = MultiDAE_net([1, 2], [2, 1], .1)
    model = AETrainer(net)
    train = csr_matrix((np.array([1., 1., 1.]), (np.array([0, 0, 1]), np.array([0, 1, 1]))))
    model.train(DataSampler(train, batch_size=1, shuffle=False), num_epochs=20, verbose=0)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ae.pth")
        model.save_model(path, 20)
        ck = torch.load(path)
    arrays = checkpoint_arrays(ck)
    assert _same(checkpoint_from_arrays(arrays), ck), "the checkpoint does not survive its array form"
    out.update(arrays)
    xck = torch.FloatTensor([[1, 1], [2, 2]])
    out["ck_x"] = xck.numpy()
    out["ck_pred_keep"] = model.predict(xck, False)[0].numpy()
    np.savez_compressed(os.path.join(HERE, "g16_ae_misc.npz"), **out)
    print("wrote g16_ae_{deep_rat,one_bin,wide_bin,misc}.npz")


if __name__ == "__main__":
    main()
