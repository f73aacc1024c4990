"""GPU (-m gpu): a loss computed outside the engine -- ``net.differentiable`` and ``model.custom_loss`` over
``rtx_engine_forward_train`` / ``rtx_engine_backward``.

1. the reference's own losses, written in torch and sent through the custom route, reproduce the reference's recorded steps under
   the tolerances the fused route's tests of the same fixtures use;
2. losses the engine does not have, against the float64 restatement of tests/test_custom_loss_host.py on the same injected draws:
   float32 gradients within rel() < 2e-4 (the project's bound for them); bf16 gradients at most twice as far from float64 as the
   EXISTING fused step's are for its built-in loss (one more float32 rounding of the output gradient in front of the same bf16
   rounding), both numbers printed;
3. bare networks under ``torch.optim.SGD``;  4. autograd semantics and the ticket;  5. the fused route is untouched.
"""
import subprocess

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

from conftest import load_golden, sd_from, params_in_order
from test_custom_loss_host import build_extgrad, forward64, kld, multinomial_kl, params64, rel

pytestmark = pytest.mark.gpu


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


@pytest.fixture(scope="module", autouse=True)
def _require_native_path():
    from rectorch_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()


def test_native_driver_extgrad():
    """tests/native/test_extgrad.cpp: rtx_launch_import_dout and the external d mu / d logvar of both VAE-head backward kernels
    against float64, element by element, poisoned outputs, bit-checked padding"""
    out = subprocess.run([build_extgrad(always=False)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout and "host reference only" not in out.stdout


# =================================================================================================== 1. the reference's own losses
def _counting(cls, loss):
    """a subclass of ``cls`` whose loss_function is ``loss`` (torch ops on the device tensors) and counts its calls"""
    class Custom(cls):
        def loss_function(self, *args):
            self.calls = getattr(self, "calls", 0) + 1
            return loss(self, *args)
    Custom.__name__ = "Custom" + cls.__name__
    return Custom


def _ref_mvae_loss(self, recon_x, x, mu, logvar, beta=1.0):
    return multinomial_kl(recon_x, x, mu, logvar, beta)


def _ref_mdae_loss(self, recon_x, x):
    l2_reg = 0
    for W in self.network.parameters():          # through torch: this term's gradient reaches p.grad without the engine
        l2_reg = l2_reg + W.norm(2)
    return multinomial_kl(recon_x, x) + self.lam * l2_reg


class _Bce(torch.autograd.Function):
    """``F.binary_cross_entropy(p, x)`` (mean) as the reference's CPU path computes it, forward and backward: the logarithms clamped
    at -100, d / dp = (p - x) / max(p (1 - p), 1e-12) / n.  Written out because torch's DEVICE kernel asserts 0 <= x <= 1 and traps on
    the rating targets of the G15 fixtures (the reference trains on the host, where there is no such check)."""

    @staticmethod
    def forward(ctx, p, x):
        ctx.save_for_backward(p, x)
        return ((x - 1) * torch.log1p(-p).clamp_min(-100.0) - x * torch.log(p).clamp_min(-100.0)).mean()

    @staticmethod
    def backward(ctx, g):
        p, x = ctx.saved_tensors
        return g * (p - x) / (p * (1 - p)).clamp_min(1e-12) / p.numel(), None


def _ref_vae_loss(self, recon_x, x, mu, logvar):
    return _Bce.apply(recon_x, x) + kld(mu, logvar)


def _ref_mse_loss(self, prediction, ground_truth):
    return torch.nn.MSELoss()(ground_truth, prediction)


def _load(net, sd):
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return net


def _check_step(g, t, net, model, keys, moments=True):
    sd_t, _ = params_in_order(sd_from(g, "sd_%d__" % t))
    for k, prm, ref in zip(keys, net._param_list(), sd_t):
        kk = k.replace(".", "__")
        assert rel(prm.grad.cpu(), g["grad_%d__%s" % (t, kk)]) < 2e-4, (t, k)
        assert float(np.max(np.abs(prm.detach().cpu().numpy() - ref))) < 5e-6, (t, k)
        st = model.optimizer.state[prm]
        assert int(float(st["step"])) == t + 1
        if moments:
            assert rel(st["exp_avg"].cpu(), g["exp_avg_%d__%s" % (t, kk)]) < 2e-4
            assert rel(st["exp_avg_sq"].cpu(), g["exp_avg_sq_%d__%s" % (t, kk)]) < 4e-4


@pytest.mark.parametrize("name", ["g2_mvae_train_step_small", "g2b_mvae_train_step_te", "g2c_mvae_train_step_deep"])
def test_reference_mvae_loss_through_the_custom_route(name):
    """tolerances of test_gpu_parity.test_g2_train_steps_fp32"""
    from rectorch_amd.nets import MultiVAE_net
    from rectorch_amd.models import MultiVAE
    g = load_golden(name)
    enc, dec = [int(v) for v in g["enc_dims"]], [int(v) for v in g["dec_dims"]]
    beta, anneal, p, lr = [float(v) for v in g["meta"]]
    net = _load(MultiVAE_net(list(dec), list(enc), dropout=p), sd_from(g, "sd0__"))
    model = _counting(MultiVAE, _ref_mvae_loss)(net, beta=beta, anneal_steps=int(anneal), learning_rate=lr, numerics="fp32")
    model.custom_loss = True
    _, keys = params_in_order(sd_from(g, "sd0__"))
    steps = g["xs"].shape[0]
    for t in range(steps):
        model._rtx.inject = (dev(g["mask_%d" % t], torch.uint8), dev(g["eps_%d" % t]))
        gt = torch.from_numpy(g["gts"][t]) if "gts" in g else None
        loss = model.train_batch(torch.from_numpy(g["xs"][t]), gt)
        assert isinstance(loss, float)
        assert abs(loss - float(g["loss_%d" % t])) < 1e-5 * abs(float(g["loss_%d" % t])), (t, loss)
        _check_step(g, t, net, model, keys)
    assert model.gradient_updates == float(g["gradient_updates"])
    assert model.calls == steps


def test_reference_mdae_loss_through_the_custom_route():
    """G4, tolerances of test_gpu_parity.test_g4_dae_train_steps_fp32 (gradients and moments: G2's); lam * sum ||W||_2 is written
    over self.network.parameters(), so its gradient reaches the parameters through torch and the engine's Adam gets lam = 0"""
    from rectorch_amd.nets import MultiDAE_net
    from rectorch_amd.models import MultiDAE
    g = load_golden("g4_mdae_train_step_small")
    enc, dec = [int(v) for v in g["enc_dims"]], [int(v) for v in g["dec_dims"]]
    lam, wd, p, lr = [float(v) for v in g["meta"]]
    net = _load(MultiDAE_net(list(dec), list(enc), dropout=p), sd_from(g, "sd0__"))
    model = _counting(MultiDAE, _ref_mdae_loss)(net, lam=lam, learning_rate=lr, numerics="fp32")
    model.custom_loss = True
    _, keys = params_in_order(sd_from(g, "sd0__"))
    for t in range(3):
        model._rtx.inject = (dev(g["mask_%d" % t], torch.uint8), None)
        loss = model.train_batch(torch.from_numpy(g["xs"][t]))
        assert abs(loss - float(g["loss_%d" % t])) < 1e-5 * abs(float(g["loss_%d" % t]))
        _check_step(g, t, net, model, keys, moments=("exp_avg_%d__enc_layers__0__weight" % t) in g)
    assert model.calls == 3


def test_reference_cmvae_loss_through_the_custom_route():
    """G11, tolerances of test_gpu_parity.test_g11_cmvae_train_steps_fp32"""
    from rectorch_amd.nets import CMultiVAE_net
    from rectorch_amd.models import CMultiVAE
    g = load_golden("g11_cmvae_train_steps")
    enc, dec = [int(v) for v in g["enc_dims"]], [int(v) for v in g["dec_dims"]]
    beta, anneal, p, lr = [float(v) for v in g["meta"]]
    cond = g["xs"].shape[2] - enc[0]
    net = _load(CMultiVAE_net(cond, list(dec), list(enc), dropout=p), sd_from(g, "sd0__"))
    model = _counting(CMultiVAE, _ref_mvae_loss)(net, beta=beta, anneal_steps=int(anneal), learning_rate=lr, numerics="fp32")
    model.custom_loss = True
    _, keys = params_in_order(sd_from(g, "sd0__"))
    steps = g["xs"].shape[0]
    for t in range(steps):
        model._rtx.inject = (dev(g["mask_%d" % t], torch.uint8), dev(g["eps_%d" % t]))
        loss = model.train_batch(torch.from_numpy(g["xs"][t]), torch.from_numpy(g["gts"][t]))
        assert abs(loss - float(g["loss_%d" % t])) < 1e-5 * abs(float(g["loss_%d" % t])), (t, loss)
        _check_step(g, t, net, model, keys, moments=("exp_avg_%d__enc_layers__0__weight" % t) in g)
    assert model.gradient_updates == float(g["gradient_updates"])
    assert model.calls == steps


@pytest.mark.parametrize("case", ["deep_bin", "deep_rat_sat", "one_bin"])
def test_reference_vae_loss_through_the_custom_route(case):
    """G15, tolerances of test_generic_vae.test_fp32_forward_step_and_predict_against_reference"""
    from rectorch_amd.nets import VAE_net
    from rectorch_amd.models import VAE
    g = load_golden("g15_vae_" + case)
    x = dev(g["c__x"])

    def make():
        net = _load(VAE_net([int(d) for d in g["c__dec"]], [int(d) for d in g["c__enc"]]), sd_from(g, "c__sd0__"))
        model = _counting(VAE, _ref_vae_loss)(net, numerics="fp32", learning_rate=1e-3)
        model.custom_loss = True
        return net, model
    net, model = make()
    model._rtx.inject = (None, dev(g["c__eps_f"]))
    loss = model.train_batch(x)
    print("%s loss %.9g reference %.9g" % (case, loss, float(g["c__loss_f"])))
    assert abs(loss - float(g["c__loss_f"])) <= 1e-6 * abs(float(g["c__loss_f"])), (loss, float(g["c__loss_f"]))
    for i, prm in enumerate(net._param_list()):
        r = rel(prm.grad.cpu(), g["c__grad_%d" % i])
        print("%s gradient %d: rel %.3g" % (case, i, r))
        assert r < 1e-5, (case, i, r)
    net, model = make()
    for t in range(3):
        model._rtx.inject = (None, dev(g["c__eps_%d" % t]))
        loss = model.train_batch(x, x)
        ref = float(g["c__loss_%d" % t])
        assert abs(loss - ref) <= 1e-6 * abs(ref), (t, loss, ref)
    for i, prm in enumerate(net._param_list()):
        assert float(np.max(np.abs(prm.detach().cpu().numpy() - g["c__param_%d" % i]))) < 5e-6, (case, i)
    assert model.calls == 3


@pytest.mark.parametrize("case", ["deep_rat", "one_bin", "wide_bin"])
def test_reference_mse_loss_through_the_custom_route(case):
    """G16, tolerances of test_plain_autoencoder.test_fp32_forward_step_and_predict_against_reference"""
    from rectorch_amd.nets import MultiDAE_net
    from rectorch_amd.models import AETrainer
    g = load_golden("g16_ae_" + case)
    x = dev(g["c__x"])
    n_items = int(g["c__enc"][0])

    def mask_of(name):
        if float(g["c__dropout"]) == 0.0:
            return None
        return dev(np.unpackbits(g["c__" + name], axis=1)[:, :n_items], torch.uint8)

    def make():
        net = _load(MultiDAE_net([int(d) for d in g["c__dec"]], [int(d) for d in g["c__enc"]], dropout=float(g["c__dropout"])),
                    sd_from(g, "c__sd0__"))
        model = _counting(AETrainer, _ref_mse_loss)(net, numerics="fp32", learning_rate=1e-3)
        assert model._loss_kind == "multinomial"          # untouched: the fused step of such a subclass is not the route taken here
        model.custom_loss = True
        return net, model
    net, model = make()
    model._rtx.inject = (mask_of("mask_f"), None)
    loss = model.train_batch(x)
    ref = float(g["c__loss_f"])
    print("%s loss %.9g reference %.9g" % (case, loss, ref))
    assert abs(loss - ref) <= 1e-6 * abs(ref), (loss, ref)
    for i, prm in enumerate(net._param_list()):
        r = rel(prm.grad.cpu(), g["c__grad_%d" % i])
        print("%s gradient %d: rel %.3g" % (case, i, r))
        assert r < 1e-5, (case, i, r)
    net, model = make()
    for t in range(3):
        model._rtx.inject = (mask_of("mask_%d" % t), None)
        loss = model.train_batch(x, x)
        ref = float(g["c__loss_%d" % t])
        assert abs(loss - ref) <= 1e-6 * abs(ref), (t, loss, ref)
    for i, prm in enumerate(net._param_list()):
        assert float(np.max(np.abs(prm.detach().cpu().numpy() - g["c__param_%d" % i]))) < 5e-6, (case, i)
    assert model.calls == 3


# =================================================================================================== 2. losses the engine does not have
# G2c's network, and one whose hidden and head layers take the one-launch kernels, whose batch needs padding and whose width is odd
SHAPES = {"g2c": ([77, 21, 13, 5], [5, 9, 77], 7), "wide": ([4133, 256, 64], [64, 256, 4133], 37)}
VARIANTS = ("vae", "dae", "gvae", "cond")
COND, P_DROP, BETA = 5, 0.5, 0.2


def build_net(variant, shape, seed=3):
    from rectorch_amd.nets import MultiVAE_net, MultiDAE_net, VAE_net, CMultiVAE_net
    from rectorch_amd.utils.hashinit import hash_state_dict
    enc, dec, _ = SHAPES[shape]
    cond = COND if variant == "cond" else 0
    sd = hash_state_dict([enc[0] + cond] + list(enc[1:]), dec, "dae" if variant == "dae" else "vae", seed, 0.3)
    if variant == "vae":
        net = MultiVAE_net(list(dec), list(enc), dropout=P_DROP)
    elif variant == "dae":
        net = MultiDAE_net(list(dec), list(enc), dropout=P_DROP)
    elif variant == "gvae":
        net = VAE_net(list(dec), list(enc))
    else:
        net = CMultiVAE_net(COND, list(dec), list(enc), dropout=P_DROP)
    return _load(net, sd).to("cuda"), sd


def make_data(variant, shape, seed=0):
    """(input rows, target rows, keep-mask or None, eps or None) as numpy arrays"""
    enc, _, B = SHAPES[shape]
    I, Z = enc[0], enc[-1]
    rng = np.random.RandomState(seed)
    x = (rng.rand(B, I) < (0.3 if I < 100 else 0.03)).astype(np.float32)
    x[np.arange(B), rng.randint(0, I, B)] = 1.0          # no empty row
    xin, gt = x, x
    if variant == "cond":
        onehot = np.zeros((B, COND), np.float32)
        onehot[np.arange(B), np.arange(B) % COND] = 1.0
        xin = np.hstack([x, onehot])
        gt = x * (rng.rand(B, I) < 0.7).astype(np.float32)
    keep = None if variant == "gvae" else (rng.rand(B, I) >= P_DROP).astype(np.uint8)
    eps = None if variant == "dae" else rng.randn(B, Z).astype(np.float32)
    return xin, gt, keep, eps


def linear_loss(shape):
    """(out W).sum() + (mu a).sum() + (logvar b).sum(): the gradient handed to the engine is exactly W, a, b"""
    enc, _, B = SHAPES[shape]
    rng = np.random.RandomState(5)
    W, a, b = [torch.from_numpy(rng.randn(B, n).astype(np.float32)) for n in (enc[0], enc[-1], enc[-1])]

    def loss(out, gt, mu, logvar):
        total = (out * W.to(out)).sum()
        if mu is not None:
            total = total + (mu * a.to(mu)).sum() + (logvar * b.to(logvar)).sum()
        return total
    return loss


def focal_loss(out, gt, mu, logvar):
    """focal-weighted log-softmax NLL + 0.3 ||mu||_1"""
    lp = torch.log_softmax(out, 1)
    total = -(((1 - lp.exp()) ** 2) * lp * gt).sum(-1).mean()
    if mu is not None:
        total = total + 0.3 * mu.abs().sum()
    return total


def builtin_loss(variant):
    """the loss the fused step of this variant has built in, in torch ops"""
    if variant == "dae":
        return lambda out, gt, mu, logvar: multinomial_kl(out, gt)
    if variant == "gvae":
        return lambda out, gt, mu, logvar: _Bce.apply(out, gt) + kld(mu, logvar)
    return lambda out, gt, mu, logvar: multinomial_kl(out, gt, mu, logvar, BETA)


def reference_grads(variant, shape, sd, data, loss):
    """the float64 restatement's loss and gradients, parameter order"""
    enc, _, _ = SHAPES[shape]
    xin, gt, keep, eps = data
    ps, _ = params64(sd)
    out, mu, logvar = forward64(ps, len(enc) - 1, "vae" if variant == "cond" else variant, torch.from_numpy(xin),
                                None if keep is None else torch.from_numpy(keep), None if eps is None else torch.from_numpy(eps),
                                0.0 if variant == "gvae" else P_DROP, COND if variant == "cond" else 0)
    value = loss(out, torch.from_numpy(gt).double(), mu, logvar)
    value.backward()
    return value.item(), [p.grad.numpy() for p in ps]


def device_grads(net, variant, data, numerics, loss):
    """the differentiable route's loss and gradients under the same injected draws"""
    xin, gt, keep, eps = data
    net.train()
    for p in net.parameters():
        p.grad = None
    res = net._differentiable_forward(dev(xin), numerics=numerics, mask=dev(keep, torch.uint8), noise=dev(eps))
    out, mu, logvar = (res, None, None) if variant == "dae" else res
    assert out.grad_fn is not None and out.dtype == torch.float32
    value = loss(out, dev(gt), mu, logvar)
    value.backward()
    return value.item(), [p.grad.cpu().numpy() for p in net._param_list()]


@pytest.mark.parametrize("which", ["linear", "focal"])
@pytest.mark.parametrize("shape", ["g2c", "wide"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_custom_losses_fp32_against_float64(variant, shape, which):
    loss = linear_loss(shape) if which == "linear" else focal_loss
    net, sd = build_net(variant, shape)
    data = make_data(variant, shape)
    want, ref = reference_grads(variant, shape, sd, data, loss)
    got, grads = device_grads(net, variant, data, "fp32", loss)
    print("%s %s %s: loss %.9g, float64 %.9g" % (variant, shape, which, got, want))
    _, keys = params_in_order(sd)
    for k, gdev, gref in zip(keys, grads, ref):
        r = rel(gdev, gref)
        print("  %-24s rel %.3g" % (k, r))
        assert r < 2e-4, (variant, shape, which, k, r)


@pytest.mark.parametrize("shape", ["g2c", "wide"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_custom_route_bf16_no_worse_than_twice_the_fused_step(variant, shape):
    """self-calibrating: the error of the EXISTING fused bf16 step's gradients (keep_grads) against the float64 restatement of its
    built-in loss, and the custom route's error for the same loss written in torch, same shape, same draws; per tensor the second
    is at most twice the first.  Measured on an MI355X: worst ratio 1.48, every pair in profiles/custom_loss_bf16_pairs.txt
    (DESIGN.md section 9.1)."""
    from rectorch_amd.models import MultiVAE, MultiDAE, VAE, CMultiVAE
    loss = builtin_loss(variant)
    data = make_data(variant, shape)
    xin, gt, keep, eps = data
    net, sd = build_net(variant, shape)
    _, ref = reference_grads(variant, shape, sd, data, loss)
    # the fused step
    if variant == "dae":
        model = MultiDAE(net, lam=0.0, numerics="bf16")
    elif variant == "gvae":
        model = VAE(net, numerics="bf16")
    elif variant == "vae":
        model = MultiVAE(net, beta=BETA, numerics="bf16")
    else:
        model = CMultiVAE(net, beta=BETA, numerics="bf16")
    model.keep_grads = True
    model._rtx.inject = (dev(keep, torch.uint8), dev(eps))
    if variant in ("dae", "gvae"):
        model.train_batch(dev(xin))
    else:
        model.train_batch(dev(xin), dev(gt))
    fused = [p.grad.cpu().numpy().copy() for p in net._param_list()]
    # the custom route, from the same initial parameters
    net2, _ = build_net(variant, shape)
    _, custom = device_grads(net2, variant, data, "bf16", loss)
    _, keys = params_in_order(sd)
    bad = []
    for k, gf, gc, gref in zip(keys, fused, custom, ref):
        ef, ec = rel(gf, gref), rel(gc, gref)
        print("%s %s %-24s fused %.3g custom %.3g" % (variant, shape, k, ef, ec))
        if not ec <= 2.0 * ef:
            bad.append((k, ef, ec))
    assert not bad, bad


# =================================================================================================== 3. bare networks, a torch optimizer
def _sgd_reference(sd, enc, batches, seeds, lr):
    """three SGD steps of the float64 restatement with the engine's own draws for the given seeds (oracle/philox_oracle.py)"""
    from oracle import philox_oracle
    ps, _ = params64(sd)
    for x, seed in zip(batches, seeds):
        B, I = x.shape
        keep = torch.from_numpy(philox_oracle.dropout_mask(seed, 0, B, I, np.float32(P_DROP)).astype(np.uint8))
        eps = torch.from_numpy(philox_oracle.noise(seed, 0, B, enc[-1]))
        out, mu, logvar = forward64(ps, len(enc) - 1, "vae", torch.from_numpy(x), keep, eps, P_DROP)
        loss = focal_loss(out, torch.from_numpy(x).double(), mu, logvar)
        grads = torch.autograd.grad(loss, ps)
        with torch.no_grad():
            for p, g in zip(ps, grads):
                p -= lr * g
    return [p.detach().numpy() for p in ps]


@pytest.mark.parametrize("source", ["dense", "rows"])
def test_bare_network_with_torch_sgd(source):
    """net.differentiable = True, torch.optim.SGD, three steps on G2c's network: parameters within 5e-6 absolute (G2's parameter
    bound) of the restatement -- which also shows that the compute copies are refreshed after a foreign optimizer's step"""
    from rectorch_amd.nets import draw_seed
    from rectorch_amd.samplers import DataSampler
    enc, _, B = SHAPES["g2c"]
    lr = 0.05
    net, sd = build_net("vae", "g2c")
    rng = np.random.RandomState(9)
    dense = (rng.rand(3 * B, enc[0]) < 0.3).astype(np.float32)
    dense[np.arange(3 * B), rng.randint(0, enc[0], 3 * B)] = 1.0
    batches = [dense[i * B:(i + 1) * B] for i in range(3)]
    torch.manual_seed(77)
    seeds = [draw_seed() for _ in range(3)]
    want = _sgd_reference(sd, enc, batches, seeds, lr)
    net.differentiable = True
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=lr)
    if source == "rows":
        inputs = list(DataSampler(csr_matrix(dense), batch_size=B, shuffle=False).iter_rows())
    else:
        inputs = [dev(b) for b in batches]
    torch.manual_seed(77)
    for x, b in zip(inputs, batches):
        opt.zero_grad()
        out, mu, logvar = net(x)
        assert out.grad_fn is not None
        focal_loss(out, dev(b), mu, logvar).backward()
        opt.step()
    for p, w in zip(net._param_list(), want):
        d = float(np.max(np.abs(p.detach().cpu().numpy() - w)))
        assert d < 5e-6, d
    moved = max(float(np.max(np.abs(w - np.array(v)))) for w, v in zip(want, params_in_order(sd)[0]))
    assert moved > 1e-3          # the three steps did move the parameters


# =================================================================================================== 4. autograd semantics
def _seeded_backward(net, x, seed):
    torch.manual_seed(seed)
    out, mu, logvar = net(x)
    ((out ** 2).sum() + (mu * logvar).sum()).backward()
    return out, mu, logvar


def test_grad_is_set_then_accumulated():
    net, _ = build_net("vae", "g2c")
    x = dev(make_data("vae", "g2c")[0])
    net.differentiable = True
    net.train()
    assert all(p.grad is None for p in net.parameters())
    out, mu, logvar = _seeded_backward(net, x, 5)
    assert out.grad_fn is not None and mu.grad_fn is not None and logvar.grad_fn is not None
    first = [p.grad.clone() for p in net._param_list()]
    assert all(float(g.abs().max()) > 0 for g in first)
    bufs = net._diff_buffers()[0]
    assert all(p.grad.data_ptr() != b.data_ptr() for p, b in zip(net._param_list(), bufs))     # p.grad never aliases the engine's buffers
    _seeded_backward(net, x, 5)                          # the same seeded forward again, no zero_grad
    for p, g in zip(net._param_list(), first):
        assert torch.equal(p.grad, 2 * g)


def test_forward_is_unchanged_where_the_route_is_off():
    net, _ = build_net("vae", "g2c")
    x = dev(make_data("vae", "g2c")[0])
    net.train()
    torch.manual_seed(3)
    plain = net(x)                                       # today's training forward
    assert all(t.grad_fn is None for t in plain)
    net.differentiable = True
    torch.manual_seed(3)
    with torch.no_grad():
        off = net(x)
    assert all(t.grad_fn is None for t in off) and all(torch.equal(a, b) for a, b in zip(plain, off))
    torch.manual_seed(3)
    on = net(x)
    assert all(t.grad_fn is not None for t in on) and all(torch.equal(a, b.detach()) for a, b in zip(plain, on))     # the same draws
    net.differentiable = False
    net.eval()
    ev = net(x)
    net.differentiable = True
    ev2 = net(x)
    assert all(t.grad_fn is None for t in ev2) and all(torch.equal(a, b) for a, b in zip(ev, ev2))
    with pytest.raises(ValueError, match="requires_grad"):
        net.train()
        net(x.clone().requires_grad_())


def test_generic_vae_net_methods_run_on_the_engine():
    net, _ = build_net("gvae", "g2c")
    x = dev(make_data("gvae", "g2c")[0])
    net.eval()
    mu, logvar = net.encode(x)
    torch.manual_seed(1)
    p, mu2, logvar2 = net(x)
    assert torch.equal(mu, mu2) and torch.equal(logvar, logvar2)
    assert float(p.min()) >= 0.0 and float(p.max()) <= 1.0
    q = net.decode(mu)
    assert q.shape == p.shape and float(q.min()) >= 0.0 and float(q.max()) <= 1.0
    net.differentiable = True
    net.train()
    out, _, _ = net(x)
    assert out.grad_fn is not None


def test_stale_ticket_raises_and_leaves_the_engine_usable():
    net, _ = build_net("vae", "g2c")
    xa = dev(make_data("vae", "g2c", seed=0)[0])
    xb = dev(make_data("vae", "g2c", seed=1)[0])
    net.differentiable = True
    net.train()
    torch.manual_seed(1)
    out_a, _, _ = net(xa)
    torch.manual_seed(2)
    out_b, mu_b, logvar_b = net(xb)                      # overwrites A's activations
    with pytest.raises(RuntimeError, match="stale ticket"):
        out_a.sum().backward()
    assert all(p.grad is None for p in net.parameters())          # nothing ran, nothing was handed to autograd
    ((out_b ** 2).sum() + (mu_b * logvar_b).sum()).backward()     # B's ticket is still good
    fresh, _ = build_net("vae", "g2c")
    fresh.differentiable = True
    fresh.train()
    _seeded_backward(fresh, xb, 2)
    for p, q in zip(net._param_list(), fresh._param_list()):
        assert torch.equal(p.grad, q.grad)


def test_predict_between_two_custom_steps_changes_nothing():
    from rectorch_amd.models import MultiVAE
    x = dev(make_data("vae", "g2c")[0])

    def run(with_predict):
        net, _ = build_net("vae", "g2c")
        model = _counting(MultiVAE, _ref_mvae_loss)(net, beta=BETA, numerics="fp32")
        model.custom_loss = True
        torch.manual_seed(11)
        model.train_batch(x)
        if with_predict:
            model.predict(x)
        torch.manual_seed(12)
        model.train_batch(x)
        return [p.detach().clone() for p in net._param_list()]
    for a, b in zip(run(False), run(True)):
        assert torch.equal(a, b)


def test_custom_loss_on_resident_samplers():
    """train_epoch's resident branch: the input stays row numbers, the loss gets the dense rows (rtx_csr_gather_dense) -- also for
    the conditioned resident sampler, whose slots are CSR handles like any other"""
    from rectorch_amd.models import MultiVAE, CMultiVAE
    from rectorch_amd.samplers import DataSampler, ConditionedDataSampler
    enc, _, B = SHAPES["g2c"]
    rng = np.random.RandomState(2)
    dense = (rng.rand(3 * B, enc[0]) < 0.3).astype(np.float32)
    dense[np.arange(3 * B), rng.randint(0, enc[0], 3 * B)] = 1.0
    seen = []

    def loss(self, recon_x, x, mu, logvar, beta=1.0):
        seen.append(tuple(x.shape))
        assert recon_x.grad_fn is not None and x.is_cuda and recon_x.shape == x.shape
        return multinomial_kl(recon_x, x, mu, logvar, beta)
    net, _ = build_net("vae", "g2c")
    model = _counting(MultiVAE, loss)(net, beta=BETA, numerics="fp32")
    model.custom_loss = True
    before = [p.detach().clone() for p in net._param_list()]
    model.train_epoch(1, DataSampler(csr_matrix(dense), batch_size=B, shuffle=False))
    assert model.calls == 3 and seen == [(B, enc[0])] * 3
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, net._param_list()))
    seen.clear()
    cnet, _ = build_net("cond", "g2c")
    cmodel = _counting(CMultiVAE, loss)(cnet, beta=BETA, numerics="fp32")
    cmodel.custom_loss = True
    iid2cids = {i: sorted({int(i % COND), int((i * 7) % COND)}) for i in range(enc[0])}
    sampler = ConditionedDataSampler(iid2cids, COND, csr_matrix(dense), None, batch_size=16, shuffle=False, resident=True)
    cmodel.train_epoch(1, sampler)
    assert cmodel.calls == len(seen) > 0 and all(s[1] == enc[0] for s in seen)


# =================================================================================================== 5. the fused route is untouched
def test_fused_route_shares_no_state_with_the_custom_route():
    """two seeded bf16 train_batch steps of MultiVAE at [4133, 256, 64]: bit-identical parameters whether or not a custom step ran,
    on a different model object, in between"""
    from rectorch_amd.models import MultiVAE
    x = dev(make_data("vae", "wide")[0])

    def run(custom_between):
        net, _ = build_net("vae", "wide")
        model = MultiVAE(net, beta=BETA, numerics="bf16")
        assert model.custom_loss is False
        torch.manual_seed(21)
        model.train_batch(x)
        if custom_between:
            other_net, _ = build_net("vae", "wide", seed=4)
            other = _counting(MultiVAE, _ref_mvae_loss)(other_net, beta=BETA, numerics="bf16")
            other.custom_loss = True
            other.train_batch(x)
            assert other.calls == 1
        torch.manual_seed(22)
        model.train_batch(x)
        torch.cuda.synchronize()
        return [p.detach().clone() for p in net._param_list()]
    for a, b in zip(run(False), run(True)):
        assert torch.equal(a, b)
