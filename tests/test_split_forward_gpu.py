"""GPU (-m gpu): differentiable ``encode`` / ``_reparameterize`` / ``decode`` over the engine's two halves
(``rtx_engine_encode_train`` / ``encode_backward`` / ``decode_train`` / ``decode_backward``, ``rtx_reparam`` / ``rtx_reparam_grad``).

1. ``decode(_reparameterize(*encode(x)))`` equals ``net(x)`` of the differentiable route to the bit, same injected draws;
2. float32 gradients of the composed forward -- every parameter and ``d z`` -- against float64 autograd of the restatement
   (tests/test_split_forward_host.py, which ties it to ``forward64``): rel() < 2e-4, the project's bound for these gradients;
3. bf16 gradients: per tensor at most twice as far from float64 as the existing ``net(x)`` route's in the same run (one more float32
   rounding of ``d z`` and of ``d mu`` / ``d logvar``), every pair printed (profiles/split_forward_bf16_pairs.txt);
4. the draws of ``engine.reparameterize``;  5. several samples per user through one decode;  6. the tickets of the two halves;
7. a model on a network with a composed ``forward`` reproduces the reference's recorded steps;  8. nothing changes with the switch off.
"""
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_golden, sd_from, params_in_order
from test_custom_loss_host import kld, params64, rel
from test_custom_loss_gpu import (SHAPES, VARIANTS, COND, P_DROP, BETA, build_net, builtin_loss, dev, focal_loss, _check_step, _counting,
                                  _load, _ref_mvae_loss)
from test_split_forward_host import build_halves, decode64, encode64, reparam64

pytestmark = pytest.mark.gpu

# the shapes of tests/test_custom_loss_gpu.py, and G2c's network at B = 1
CASES = {"g2c": ("g2c", SHAPES["g2c"][2]), "wide": ("wide", SHAPES["wide"][2]), "g2c_b1": ("g2c", 1)}


@pytest.fixture(scope="module", autouse=True)
def _require_native_path():
    from rectorch_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()


def test_native_driver_halves():
    """tests/native/test_halves.cpp: the d z export, the d h import, rtx_reparam / rtx_reparam_grad and k_vae_bwd without a slab against
    float64, element by element, poisoned outputs, bit-checked padding"""
    out = subprocess.run([build_halves(always=False)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout and "host reference only" not in out.stdout


# =================================================================================================== data, the composed forward
def make_data(variant, case, seed=0):
    """tests/test_custom_loss_gpu.make_data at this case's batch size: (input rows, target rows, keep-mask or None, eps or None)"""
    shape, B = CASES[case]
    enc = SHAPES[shape][0]
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


def composed(net, variant, x, keep, eps):
    """the reference's forward written from its three pieces: ``(out, mu, logvar, z)`` (``mu`` / ``logvar`` None for "dae", ``z`` = h)"""
    if variant == "dae":
        z = net.encode(x, _mask=keep)
        return net.decode(z), None, None, z
    mu, logvar = net.encode(x) if variant == "gvae" else net.encode(x, _mask=keep)
    z = net._reparameterize(mu, logvar, _noise=eps)
    return net.decode(z), mu, logvar, z


def linear_loss(case):
    """(out W).sum() + (mu a).sum() + (logvar b).sum(): the gradient handed to the engine is exactly W, a, b"""
    shape, B = CASES[case]
    enc = SHAPES[shape][0]
    rng = np.random.RandomState(5)
    W, a, b = [torch.from_numpy(rng.randn(B, n).astype(np.float32)) for n in (enc[0], enc[-1], enc[-1])]

    def loss(out, gt, mu, logvar):
        total = (out * W.to(out)).sum()
        if mu is not None:
            total = total + (mu * a.to(mu)).sum() + (logvar * b.to(logvar)).sum()
        return total
    return loss


def z_term(case, rows=None):
    """a term on z itself: (z c).sum() + ||z||^2 / 4"""
    shape, B = CASES[case]
    c = torch.from_numpy(np.random.RandomState(6).randn(rows or B, SHAPES[shape][0][-1]).astype(np.float32))
    return lambda z: (z * c.to(z)).sum() + 0.25 * (z ** 2).sum()


def reference_grads(variant, case, sd, data, loss, zloss=None):
    """float64: the loss of the composed restatement, the parameters' gradients in parameter order, and d z"""
    enc = SHAPES[CASES[case][0]][0]
    xin, gt, keep, eps = data
    ps, _ = params64(sd)
    v = "vae" if variant == "cond" else variant
    a, b = encode64(ps, len(enc) - 1, v, torch.from_numpy(xin), None if keep is None else torch.from_numpy(keep),
                    0.0 if variant == "gvae" else P_DROP, COND if variant == "cond" else 0)
    z = a if variant == "dae" else reparam64(a, b, torch.from_numpy(eps))
    z.retain_grad()
    out = decode64(ps, len(enc) - 1, v, z)
    value = loss(out, torch.from_numpy(gt).double(), None if variant == "dae" else a, b)
    if zloss is not None:
        value = value + zloss(z)
    value.backward()
    return value.item(), [p.grad.numpy() for p in ps], z.grad.numpy()


def device_grads(net, variant, data, numerics, loss, zloss=None, route="composed"):
    """the same on the device: the composed forward, or (route "whole", no z term) the existing ``net(x)`` Function"""
    xin, gt, keep, eps = data
    net.train()
    net.differentiable = numerics
    for p in net.parameters():
        p.grad = None
    keep, eps = dev(keep, torch.uint8), dev(eps)
    z = None
    if route == "whole":
        res = net._differentiable_forward(dev(xin), numerics=numerics, mask=keep, noise=eps)
        out, mu, logvar = (res, None, None) if variant == "dae" else res
    else:
        out, mu, logvar, z = composed(net, variant, dev(xin), keep, eps)
        z.retain_grad()
    assert out.grad_fn is not None and out.dtype == torch.float32
    value = loss(out, dev(gt), mu, logvar)
    if zloss is not None:
        value = value + zloss(z)
    value.backward()
    return value.item(), [p.grad.cpu().numpy() for p in net._param_list()], None if z is None or z.grad is None else z.grad.cpu().numpy()


# =================================================================================================== 1. forward equals net(x)
@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("variant", VARIANTS)
def test_composed_forward_equals_the_whole_forward_to_the_bit(variant, case, numerics):
    net, _ = build_net(variant, CASES[case][0])
    xin, _, keep, eps = make_data(variant, case)
    x, keep, eps = dev(xin), dev(keep, torch.uint8), dev(eps)
    net.train()
    net.differentiable = numerics
    res = net._differentiable_forward(x, numerics=numerics, mask=keep, noise=eps)
    whole = (res, None, None) if variant == "dae" else res
    whole = [None if t is None else t.detach().clone() for t in whole]
    out, mu, logvar, z = composed(net, variant, x, keep, eps)
    assert out.grad_fn is not None and z.grad_fn is not None
    assert torch.equal(out.detach(), whole[0])
    if variant != "dae":
        assert mu.grad_fn is not None and logvar.grad_fn is not None
        assert torch.equal(mu.detach(), whole[1]) and torch.equal(logvar.detach(), whole[2])


# =================================================================================================== 2. fp32 gradients against float64
@pytest.mark.parametrize("which", ["linear", "focal"])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("variant", VARIANTS)
def test_composed_gradients_fp32_against_float64(variant, case, which):
    loss = linear_loss(case) if which == "linear" else focal_loss
    net, sd = build_net(variant, CASES[case][0])
    data = make_data(variant, case)
    want, ref, ref_dz = reference_grads(variant, case, sd, data, loss, z_term(case))
    got, grads, dz = device_grads(net, variant, data, "fp32", loss, z_term(case))
    print("%s %s %s: loss %.9g, float64 %.9g" % (variant, case, which, got, want))
    _, keys = params_in_order(sd)
    for k, gdev, gref in list(zip(keys, grads, ref)) + [("d z", dz, ref_dz)]:
        r = rel(gdev, gref)
        print("  %-24s rel %.3g" % (k, r))
        assert r < 2e-4, (variant, case, which, k, r)


# =================================================================================================== 3. bf16 against the existing route
@pytest.mark.parametrize("shape", ["g2c", "wide"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_composed_route_bf16_no_worse_than_twice_the_whole_route(variant, shape):
    """self-calibrating: per tensor, the composed route's error against float64 and the error of the existing ``net(x)`` Function for
    the same loss (the variant's built-in one, written in torch) on the same draws, in the same run; the first is at most twice the
    second.  Measured on an MI355X: every pair in profiles/split_forward_bf16_pairs.txt."""
    loss = builtin_loss(variant)
    data = make_data(variant, shape)
    net, sd = build_net(variant, shape)
    _, ref, _ = reference_grads(variant, shape, sd, data, loss)
    _, whole, _ = device_grads(net, variant, data, "bf16", loss, route="whole")
    net2, _ = build_net(variant, shape)
    _, split, _ = device_grads(net2, variant, data, "bf16", loss)
    _, keys = params_in_order(sd)
    bad = []
    for k, gw, gs, gref in zip(keys, whole, split, ref):
        ew, es = rel(gw, gref), rel(gs, gref)
        print("%s %s %-24s whole %.3g composed %.3g" % (variant, shape, k, ew, es))
        if not es <= 2.0 * ew:
            bad.append((k, ew, es))
    assert not bad, bad


# =================================================================================================== 4. the draws of reparameterize
def test_reparameterize_draws_the_reference_normals():
    """mu = 0, logvar = 0: z is the draw itself, element (b, j) at index b latent + j of oracle/philox_oracle.py under the tolerance of
    tests/test_philox_draws.py; the custom op and an injected noise give the same operator"""
    from rectorch_amd import engine, ops          # noqa: F401  (ops registers torch.ops.rectorch_hip)
    from test_philox_draws import SEED, TOL, TOL_EXACT, _normal_errors
    seed = SEED & (2 ** 63 - 1)
    for n, Z in ((1, 1), (7, 5), (37, 64), (111, 64)):
        zero = torch.zeros(n, Z, device="cuda")
        z = engine.reparameterize(zero, zero, seed=seed)
        e_all, e_exact = _normal_errors(z.cpu().numpy().reshape(-1), seed, 0, np.arange(n * Z))
        print("reparameterize [%d, %d]: worst draw error %.3g (u1 exact: %.3g)" % (n, Z, e_all, e_exact))
        assert e_all <= TOL and e_exact <= TOL_EXACT
        assert torch.equal(torch.ops.rectorch_hip.reparameterize(zero, zero, seed, None), z)
        mu, logvar = torch.randn(n, Z, device="cuda"), torch.randn(n, Z, device="cuda")
        assert torch.equal(engine.reparameterize(mu, logvar, noise=z), engine.reparameterize(mu, logvar, seed=seed))


# =================================================================================================== 5. several samples per user
@pytest.mark.parametrize("shape", ["g2c", "wide"])
def test_three_samples_per_user_through_one_decode(shape):
    """K = 3: mu / logvar repeated, one _reparameterize and ONE decode of 3 B rows; float32 gradients against float64"""
    K = 3
    enc, _, B = SHAPES[shape]
    net, sd = build_net("vae", shape)
    xin, gt, keep, _ = make_data("vae", shape)
    eps = np.random.RandomState(8).randn(K * B, enc[-1]).astype(np.float32)
    zloss = z_term(shape, K * B)

    def total(out, gt3, mu, logvar, z):
        return focal_loss(out, gt3, None, None) + BETA * kld(mu, logvar) + zloss(z)
    ps, keys = params64(sd)
    mu, logvar = encode64(ps, len(enc) - 1, "vae", torch.from_numpy(xin), torch.from_numpy(keep), P_DROP)
    z = reparam64(mu.repeat(K, 1), logvar.repeat(K, 1), torch.from_numpy(eps))
    total(decode64(ps, len(enc) - 1, "vae", z), torch.from_numpy(gt).double().repeat(K, 1), mu, logvar, z).backward()
    net.train()
    net.differentiable = "fp32"
    dmu, dlogvar = net.encode(dev(xin), _mask=dev(keep, torch.uint8))
    dz = net._reparameterize(dmu.repeat(K, 1), dlogvar.repeat(K, 1), _noise=dev(eps))
    out = net.decode(dz)
    assert out.shape == (K * B, enc[0])
    total(out, dev(gt).repeat(K, 1), dmu, dlogvar, dz).backward()
    for k, p, p64 in zip(keys, net._param_list(), ps):
        r = rel(p.grad.cpu().numpy(), p64.grad.numpy())
        print("%s K=3 %-24s rel %.3g" % (shape, k, r))
        assert r < 2e-4, (shape, k, r)


# =================================================================================================== 6. tickets
def _composed_backward(net, x, keep, eps):
    out, mu, logvar, z = composed(net, "vae", x, keep, eps)
    ((out ** 2).sum() + (mu * logvar).sum() + z.sum()).backward()


def test_tickets_of_the_two_halves():
    net, _ = build_net("vae", "g2c")
    xa, _, keep, eps = make_data("vae", "g2c", seed=0)
    xb = make_data("vae", "g2c", seed=1)[0]
    xa, xb, keep, eps = dev(xa), dev(xb), dev(keep, torch.uint8), dev(eps)
    net.differentiable = True
    net.train()
    # a second encode before the backward of the first
    mu_a, logvar_a = net.encode(xa, _mask=keep)
    net.encode(xb, _mask=keep)
    with pytest.raises(RuntimeError, match="encode_backward: stale ticket"):
        (mu_a * logvar_a).sum().backward()
    assert all(p.grad is None for p in net.parameters())          # nothing ran, nothing was handed to autograd
    # a prediction between decode and backward
    mu, logvar = net.encode(xa, _mask=keep)
    out = net.decode(net._reparameterize(mu, logvar, _noise=eps))
    net.eval()
    net(xa)
    net.train()
    with pytest.raises(RuntimeError, match="decode_backward: stale ticket"):
        out.sum().backward()
    assert all(p.grad is None for p in net.parameters())
    # the whole-forward ticket goes stale on an encode
    whole, _, _ = net._differentiable_forward(xa, mask=keep, noise=eps)
    net.encode(xb, _mask=keep)
    with pytest.raises(RuntimeError, match="backward: stale ticket"):
        whole.sum().backward()
    assert all(p.grad is None for p in net.parameters())
    # encode -> decode -> backward in autograd's order (decode's backward, the sampling's, encode's): the engine trains as a fresh one
    _composed_backward(net, xa, keep, eps)
    fresh, _ = build_net("vae", "g2c")
    fresh.differentiable = True
    fresh.train()
    _composed_backward(fresh, xa, keep, eps)
    for p, q in zip(net._param_list(), fresh._param_list()):
        assert p.grad is not None and float(p.grad.abs().max()) > 0 and torch.equal(p.grad, q.grad)


# =================================================================================================== 7. model level
def test_model_on_a_network_with_a_composed_forward_reproduces_the_reference_steps():
    """G2 through MultiVAE on a MultiVAE_net subclass whose forward is decode(_reparameterize(*encode(x))), the reference's loss in
    torch: tolerances of tests/test_custom_loss_gpu.test_reference_mvae_loss_through_the_custom_route"""
    from rectorch_amd.nets import MultiVAE_net
    from rectorch_amd.models import MultiVAE

    class Composed(MultiVAE_net):
        forwards = 0

        def forward(self, x):
            self.forwards += 1
            mu, logvar = self.encode(x)
            return self.decode(self._reparameterize(mu, logvar)), mu, logvar

    g = load_golden("g2_mvae_train_step_small")
    enc, dec = [int(v) for v in g["enc_dims"]], [int(v) for v in g["dec_dims"]]
    beta, anneal, p, lr = [float(v) for v in g["meta"]]
    net = _load(Composed(list(dec), list(enc), dropout=p), sd_from(g, "sd0__"))
    model = _counting(MultiVAE, _ref_mvae_loss)(net, beta=beta, anneal_steps=int(anneal), learning_rate=lr, numerics="fp32")
    model.custom_loss = True
    _, keys = params_in_order(sd_from(g, "sd0__"))
    steps = g["xs"].shape[0]
    for t in range(steps):
        model._rtx.inject = (dev(g["mask_%d" % t], torch.uint8), dev(g["eps_%d" % t]))
        gt = torch.from_numpy(g["gts"][t]) if "gts" in g else None
        loss = model.train_batch(torch.from_numpy(g["xs"][t]), gt)
        assert abs(loss - float(g["loss_%d" % t])) < 1e-5 * abs(float(g["loss_%d" % t])), (t, loss)
        _check_step(g, t, net, model, keys)
        assert net.forwards == t + 1 and model.calls == t + 1
    assert model.gradient_updates == float(g["gradient_updates"])
    assert net.differentiable is False and not hasattr(net, "_rtx_trainer")


# =================================================================================================== 8. the switch off
def test_nothing_changes_with_the_switch_off():
    """encode / decode / forward (eval, and seeded training mode) and the parameters after three fused bf16 steps, from a fresh network
    that never sets the switch and from one that ran a composed forward and backward first and switched it off again: bit-equal"""
    from rectorch_amd.models import MultiVAE
    xin, _, keep, eps = make_data("vae", "wide")
    x, keep, eps = dev(xin), dev(keep, torch.uint8), dev(eps)

    def run(split_first):
        net, _ = build_net("vae", "wide")
        if split_first:
            net.differentiable = "bf16"
            net.train()
            _composed_backward(net, x, keep, eps)
            for p in net.parameters():
                p.grad = None
            net.differentiable = False
        got = []
        for train in (False, True):
            net.train(train)
            torch.manual_seed(31)
            mu, logvar = net.encode(x)
            got += [mu, logvar, net.decode(mu)] + list(net(x))
        assert all(t.grad_fn is None for t in got)
        with pytest.raises(NotImplementedError):
            net._reparameterize(mu, logvar)
        model = MultiVAE(net, beta=BETA, numerics="bf16")
        for t in range(3):
            torch.manual_seed(40 + t)
            model.train_batch(x)
        torch.cuda.synchronize()
        return got + [p.detach().clone() for p in net._param_list()]
    for a, b in zip(run(False), run(True)):
        assert torch.equal(a, b)
