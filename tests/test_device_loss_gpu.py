"""GPU (-m gpu): the package's loss operators are differentiable -- ``rtx_*_loss_grad`` under ``engine.multinomial_loss``,
``bce_kl_loss``, ``mse_loss``, ``sum_l2_norms``, the models' ``loss_function`` and ``torch.ops.rectorch_hip.*_loss``.

0. the native driver: every route of the four launchers against float64, element by element;
1. subclasses whose ``loss_function`` is ``super().loss_function(...)`` reproduce the reference's recorded steps through the custom
   route, under the tolerances tests/test_custom_loss_gpu.py applies to the torch-written losses on the same fixtures;
2. the common override -- the package's loss plus a term of the user's -- against the float64 restatement of the FULL loss;
3. the same in bf16: at most twice as far from float64 as the fused step is for its built-in loss, both numbers printed;
4. autograd semantics;  5. the stand-alone operators against torch's float64 autograd;  6. the fused step is untouched.
"""
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_golden, sd_from, params_in_order
import test_custom_loss_gpu as cl
from test_custom_loss_host import forward64, kld, multinomial_kl, params64, rel
from test_device_loss_host import build_loss_grad

pytestmark = pytest.mark.gpu
dev = cl.dev


@pytest.fixture(scope="module", autouse=True)
def _require_native_path():
    from rectorch_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()


def test_native_driver_loss_grad():
    """tests/native/test_loss_grad.cpp on the device: poisoned and guarded outputs, float64 bounds of tests/native/test_loss.cpp, row
    losses bit-equal to the launchers without gradients, a second launch bit-equal to the first"""
    out = subprocess.run([build_loss_grad(always=False)], capture_output=True, text=True, timeout=600)
    print(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout and "host reference only" not in out.stdout


# =================================================================================================== 1. super().loss_function(...)
def _through_super(cls):
    class Custom(cls):
        def loss_function(self, *args):
            self.calls = getattr(self, "calls", 0) + 1
            return super().loss_function(*args)
    Custom.__name__ = "Custom" + cls.__name__
    return Custom


@pytest.mark.parametrize("name", ["g2_mvae_train_step_small", "g2b_mvae_train_step_te", "g2c_mvae_train_step_deep"])
def test_mvae_steps_through_super(name):
    from rectorch_amd.nets import MultiVAE_net
    from rectorch_amd.models import MultiVAE
    g = load_golden(name)
    enc, dec = [int(v) for v in g["enc_dims"]], [int(v) for v in g["dec_dims"]]
    beta, anneal, p, lr = [float(v) for v in g["meta"]]
    net = cl._load(MultiVAE_net(list(dec), list(enc), dropout=p), sd_from(g, "sd0__"))
    model = _through_super(MultiVAE)(net, beta=beta, anneal_steps=int(anneal), learning_rate=lr, numerics="fp32")
    model.custom_loss = True
    _, keys = params_in_order(sd_from(g, "sd0__"))
    steps = g["xs"].shape[0]
    for t in range(steps):
        model._rtx.inject = (dev(g["mask_%d" % t], torch.uint8), dev(g["eps_%d" % t]))
        gt = torch.from_numpy(g["gts"][t]) if "gts" in g else None
        loss = model.train_batch(torch.from_numpy(g["xs"][t]), gt)
        assert abs(loss - float(g["loss_%d" % t])) < 1e-5 * abs(float(g["loss_%d" % t])), (t, loss)
        cl._check_step(g, t, net, model, keys)
    assert model.gradient_updates == float(g["gradient_updates"])
    assert model.calls == steps


def test_mdae_steps_through_super():
    """G4, the regulariser included: MultiDAE.loss_function hands the parameters themselves to sum_l2_norms, so lam * W / ||W||
    reaches p.grad through torch and the engine's Adam gets lam = 0"""
    from rectorch_amd.nets import MultiDAE_net
    from rectorch_amd.models import MultiDAE
    g = load_golden("g4_mdae_train_step_small")
    enc, dec = [int(v) for v in g["enc_dims"]], [int(v) for v in g["dec_dims"]]
    lam, wd, p, lr = [float(v) for v in g["meta"]]
    net = cl._load(MultiDAE_net(list(dec), list(enc), dropout=p), sd_from(g, "sd0__"))
    model = _through_super(MultiDAE)(net, lam=lam, learning_rate=lr, numerics="fp32")
    model.custom_loss = True
    _, keys = params_in_order(sd_from(g, "sd0__"))
    for t in range(3):
        model._rtx.inject = (dev(g["mask_%d" % t], torch.uint8), None)
        loss = model.train_batch(torch.from_numpy(g["xs"][t]))
        assert abs(loss - float(g["loss_%d" % t])) < 1e-5 * abs(float(g["loss_%d" % t]))
        cl._check_step(g, t, net, model, keys, moments=("exp_avg_%d__enc_layers__0__weight" % t) in g)
    assert model.calls == 3


def test_cmvae_steps_through_super():
    from rectorch_amd.nets import CMultiVAE_net
    from rectorch_amd.models import CMultiVAE
    g = load_golden("g11_cmvae_train_steps")
    enc, dec = [int(v) for v in g["enc_dims"]], [int(v) for v in g["dec_dims"]]
    beta, anneal, p, lr = [float(v) for v in g["meta"]]
    cond = g["xs"].shape[2] - enc[0]
    net = cl._load(CMultiVAE_net(cond, list(dec), list(enc), dropout=p), sd_from(g, "sd0__"))
    model = _through_super(CMultiVAE)(net, beta=beta, anneal_steps=int(anneal), learning_rate=lr, numerics="fp32")
    model.custom_loss = True
    _, keys = params_in_order(sd_from(g, "sd0__"))
    steps = g["xs"].shape[0]
    for t in range(steps):
        model._rtx.inject = (dev(g["mask_%d" % t], torch.uint8), dev(g["eps_%d" % t]))
        loss = model.train_batch(torch.from_numpy(g["xs"][t]), torch.from_numpy(g["gts"][t]))
        assert abs(loss - float(g["loss_%d" % t])) < 1e-5 * abs(float(g["loss_%d" % t])), (t, loss)
        cl._check_step(g, t, net, model, keys, moments=("exp_avg_%d__enc_layers__0__weight" % t) in g)
    assert model.gradient_updates == float(g["gradient_updates"])
    assert model.calls == steps


def _one_step_then_three(g, make, inject, case):
    """the G15 / G16 protocol of tests/test_custom_loss_gpu.py: one step's loss (1e-6) and gradients (1e-5), then three steps' losses
    and the parameters after them (5e-6)"""
    x = dev(g["c__x"])
    net, model = make()
    inject(model, "f")
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
        inject(model, str(t))
        loss = model.train_batch(x, x)
        ref = float(g["c__loss_%d" % t])
        assert abs(loss - ref) <= 1e-6 * abs(ref), (t, loss, ref)
    for i, prm in enumerate(net._param_list()):
        assert float(np.max(np.abs(prm.detach().cpu().numpy() - g["c__param_%d" % i]))) < 5e-6, (case, i)
    assert model.calls == 3


@pytest.mark.parametrize("case", ["deep_bin", "deep_rat_sat", "one_bin"])
def test_vae_steps_through_super(case):
    """G15: rating targets and saturated probabilities included (p == 1.0: the gradient's clamp, then the sigmoid's exact zero)"""
    from rectorch_amd.nets import VAE_net
    from rectorch_amd.models import VAE
    g = load_golden("g15_vae_" + case)

    def make():
        net = cl._load(VAE_net([int(d) for d in g["c__dec"]], [int(d) for d in g["c__enc"]]), sd_from(g, "c__sd0__"))
        model = _through_super(VAE)(net, numerics="fp32", learning_rate=1e-3)
        model.custom_loss = True
        return net, model

    def inject(model, which):
        model._rtx.inject = (None, dev(g["c__eps_" + which]))
    _one_step_then_three(g, make, inject, case)


@pytest.mark.parametrize("case", ["deep_rat", "one_bin", "wide_bin"])
def test_ae_steps_through_super(case):
    from rectorch_amd.nets import MultiDAE_net
    from rectorch_amd.models import AETrainer
    g = load_golden("g16_ae_" + case)
    n_items = int(g["c__enc"][0])

    def make():
        net = cl._load(MultiDAE_net([int(d) for d in g["c__dec"]], [int(d) for d in g["c__enc"]], dropout=float(g["c__dropout"])),
                       sd_from(g, "c__sd0__"))
        model = _through_super(AETrainer)(net, numerics="fp32", learning_rate=1e-3)
        model.custom_loss = True
        return net, model

    def inject(model, which):
        mask = None
        if float(g["c__dropout"]) != 0.0:
            mask = dev(np.unpackbits(g["c__mask_" + which], axis=1)[:, :n_items], torch.uint8)
        model._rtx.inject = (mask, None)
    _one_step_then_three(g, make, inject, case)


# =================================================================================================== 2. the common override
def _extended(cls):
    class Extended(cls):
        def loss_function(self, recon_x, x, mu, logvar, beta=1.0):
            return super().loss_function(recon_x, x, mu, logvar, beta) + 0.1 * mu.pow(2).mean()
    return Extended


def _full_loss(beta):
    return lambda out, gt, mu, logvar: multinomial_kl(out, gt, mu, logvar, beta) + 0.1 * mu.pow(2).mean()


def test_package_loss_plus_own_term_trains_on_the_full_loss():
    """G2's network and first batch, fp32: every parameter gradient of super().loss_function(...) + 0.1 mean(mu^2) within
    rel() < 2e-4 of the float64 restatement of the FULL loss (without a backward of the package's loss these are the gradients of the
    extra term alone)"""
    from rectorch_amd.nets import MultiVAE_net
    from rectorch_amd.models import MultiVAE
    g = load_golden("g2_mvae_train_step_small")
    enc, dec = [int(v) for v in g["enc_dims"]], [int(v) for v in g["dec_dims"]]
    beta, anneal, p, lr = [float(v) for v in g["meta"]]
    sd = sd_from(g, "sd0__")
    x = torch.from_numpy(g["xs"][0])
    gt = torch.from_numpy(g["gts"][0]) if "gts" in g else x
    ps, keys = params64(sd)
    out, mu, logvar = forward64(ps, len(enc) - 1, "vae", x, torch.from_numpy(g["mask_0"]), torch.from_numpy(g["eps_0"]), p)
    want = _full_loss(float(g["anneal_beta_0"]))(out, gt.double(), mu, logvar)
    want.backward()
    net = cl._load(MultiVAE_net(list(dec), list(enc), dropout=p), sd)
    model = _extended(MultiVAE)(net, beta=beta, anneal_steps=int(anneal), learning_rate=lr, numerics="fp32")
    model.custom_loss = True
    model._rtx.inject = (dev(g["mask_0"], torch.uint8), dev(g["eps_0"]))
    loss = model.train_batch(x, gt if "gts" in g else None)
    print("loss %.9g, float64 %.9g" % (loss, want.item()))
    assert abs(loss - want.item()) < 1e-5 * abs(want.item())
    for k, prm, ref in zip(keys, net._param_list(), ps):
        r = rel(prm.grad.cpu(), ref.grad)
        print("  %-24s rel %.3g" % (k, r))
        assert r < 2e-4, (k, r)


# =================================================================================================== 3. bf16
@pytest.mark.parametrize("shape", ["g2c", "wide"])
def test_bf16_no_worse_than_twice_the_fused_step(shape):
    """the bound of test_custom_loss_gpu.test_custom_route_bf16_no_worse_than_twice_the_fused_step: the fused bf16 step's gradient
    error against the float64 restatement of its built-in loss, and the error of the custom route under
    super().loss_function(...) + 0.1 mean(mu^2) against the float64 restatement of THAT loss -- same network, same draws; per tensor
    the second is at most twice the first"""
    from rectorch_amd.models import MultiVAE
    data = cl.make_data("vae", shape)
    xin, gt, keep, eps = data
    net, sd = cl.build_net("vae", shape)
    _, ref_builtin = cl.reference_grads("vae", shape, sd, data, cl.builtin_loss("vae"))
    _, ref_full = cl.reference_grads("vae", shape, sd, data, _full_loss(cl.BETA))
    model = MultiVAE(net, beta=cl.BETA, numerics="bf16")
    model.keep_grads = True
    model._rtx.inject = (dev(keep, torch.uint8), dev(eps))
    model.train_batch(dev(xin), dev(gt))
    fused = [p.grad.cpu().numpy().copy() for p in net._param_list()]
    net2, _ = cl.build_net("vae", shape)
    model2 = _extended(MultiVAE)(net2, beta=cl.BETA, numerics="bf16")
    model2.custom_loss = True
    model2._rtx.inject = (dev(keep, torch.uint8), dev(eps))
    model2.train_batch(dev(xin), dev(gt))
    custom = [p.grad.cpu().numpy().copy() for p in net2._param_list()]
    _, keys = params_in_order(sd)
    bad = []
    for k, gf, gc, rb, rf in zip(keys, fused, custom, ref_builtin, ref_full):
        ef, ec = rel(gf, rb), rel(gc, rf)
        print("%s %-24s fused %.3g  super() + own term %.3g" % (shape, k, ef, ec))
        if not ec <= 2.0 * ef:
            bad.append((k, ef, ec))
    assert not bad, bad


# =================================================================================================== 4. autograd semantics
B, I, Z = 3, 257, 5


def _operands(seed=0, probabilities=False):
    rng = np.random.RandomState(seed)
    y = rng.randn(B, I).astype(np.float32)
    if probabilities:
        y = (1.0 / (1.0 + np.exp(-y))).astype(np.float32)
    x = (rng.rand(B, I) < 0.1).astype(np.float32) * rng.choice([1.0, 3.5], (B, I)).astype(np.float32)
    if probabilities:
        x = np.minimum(x, 1.0)
    return y, x, rng.randn(B, Z).astype(np.float32), rng.randn(B, Z).astype(np.float32)


def _leaves(*arrays, dtype=torch.float32):
    return [dev(a, dtype).requires_grad_() for a in arrays]


def test_scaling_and_accumulation():
    from rectorch_amd.engine import multinomial_loss
    y, x, mu, lv = _operands()
    a = _leaves(y, mu, lv)
    multinomial_loss(a[0], dev(x), a[1], a[2], 0.3).backward()
    b = _leaves(y, mu, lv)
    (3 * multinomial_loss(b[0], dev(x), b[1], b[2], 0.3)).backward()
    for p, q in zip(a, b):
        assert float(p.grad.abs().max()) > 0
        assert torch.allclose(q.grad, 3 * p.grad, rtol=1e-6, atol=0)
    c = _leaves(y, mu, lv)
    first = multinomial_loss(c[0], dev(x), c[1], c[2], 0.3)
    second = multinomial_loss(c[0], dev(x), c[1], c[2], 0.3)        # two losses from one set of leaves
    first.backward()
    second.backward()
    for p, q in zip(a, c):
        assert torch.equal(q.grad, 2 * p.grad)


def test_value_is_the_plain_operators_to_the_bit():
    from rectorch_amd import engine
    y, x, mu, lv = _operands()
    p, xb, _, _ = _operands(1, probabilities=True)
    params = [dev(np.random.RandomState(t).randn(*s).astype(np.float32)) for t, s in enumerate([(7, 5), (5,), (300, 13)])]
    calls = [
        (engine.multinomial_loss, (dev(y), dev(x), dev(mu), dev(lv), 0.3), (0, 2, 3)),
        (engine.multinomial_loss, (dev(y), dev(x)), (0,)),
        (engine.bce_kl_loss, (dev(p), dev(xb), dev(mu), dev(lv)), (0, 2, 3)),
        (engine.bce_kl_loss, (dev(p), dev(xb)), (0,)),
        (engine.mse_loss, (dev(y), dev(x)), (0,)),
        (lambda *ts: engine.sum_l2_norms(list(ts)), tuple(params), (0, 1, 2)),
    ]
    for fn, args, diff in calls:
        with torch.no_grad():
            plain = fn(*args)
        enabled = fn(*args)                              # grad mode on, nothing requires grad: today's path
        assert plain.grad_fn is None and enabled.grad_fn is None and torch.equal(plain, enabled)
        leaves = [a.clone().requires_grad_() if i in diff else a for i, a in enumerate(args)]
        with torch.no_grad():
            off = fn(*leaves)                            # operands require grad, grad mode off
        assert off.grad_fn is None and torch.equal(off, plain)
        on = fn(*leaves)
        assert on.grad_fn is not None and on.dtype == torch.float32 and on.dim() == 0
        assert torch.equal(on.detach(), plain), (fn, on.item(), plain.item())
        again = fn(*leaves)
        assert torch.equal(again.detach(), on.detach())


def test_target_requiring_grad_raises():
    from rectorch_amd import engine
    y, x, mu, lv = _operands()
    with pytest.raises(ValueError, match=r"\bx requires grad"):
        engine.multinomial_loss(dev(y).requires_grad_(), dev(x).requires_grad_(), dev(mu), dev(lv), 0.3)
    with pytest.raises(ValueError, match=r"\bx requires grad"):
        engine.bce_kl_loss(dev(y).sigmoid().requires_grad_(), dev(x).requires_grad_())
    with pytest.raises(ValueError, match="ground_truth requires grad"):
        engine.mse_loss(dev(y).requires_grad_(), dev(x).requires_grad_())


def test_gradients_reach_operands_of_other_dtype_and_layout():
    from rectorch_amd.engine import multinomial_loss, mse_loss
    y, x, mu, lv = _operands()
    base = dev(y).requires_grad_()
    multinomial_loss(base, dev(x)).backward()
    y64 = dev(y, torch.float64).requires_grad_()
    multinomial_loss(y64, dev(x)).backward()
    assert y64.grad.dtype == torch.float64 and y64.grad.shape == (B, I)
    assert torch.equal(y64.grad, base.grad.double())
    yt = dev(np.ascontiguousarray(y.T)).requires_grad_()          # [I, B]: its transpose is a non-contiguous [B, I]
    multinomial_loss(yt.t(), dev(x)).backward()
    assert yt.grad.shape == (I, B) and torch.equal(yt.grad.t(), base.grad)
    wide = dev(np.hstack([y, y])).requires_grad_()                # a column slice: rows strided
    mse_loss(wide[:, :I], dev(x)).backward()
    plain = dev(y).requires_grad_()
    mse_loss(plain, dev(x)).backward()
    assert torch.equal(wide.grad[:, :I], plain.grad) and float(wide.grad[:, I:].abs().max()) == 0.0


def test_ops_are_differentiable_like_the_engine_functions():
    from rectorch_amd import engine
    import rectorch_amd.ops  # noqa: F401
    y, x, mu, lv = _operands()
    p, xb, _, _ = _operands(1, probabilities=True)
    pairs = [
        (lambda a, m, l: engine.multinomial_loss(a, dev(x), m, l, 0.3),
         lambda a, m, l: torch.ops.rectorch_hip.multinomial_loss(a, dev(x), m, l, 0.3), (y, mu, lv)),
        (lambda a, m, l: engine.bce_kl_loss(a, dev(xb), m, l),
         lambda a, m, l: torch.ops.rectorch_hip.bce_kl_loss(a, dev(xb), m, l), (p, mu, lv)),
        (lambda a: engine.mse_loss(a, dev(x)), lambda a: torch.ops.rectorch_hip.mse_loss(a, dev(x)), (y,)),
    ]
    for fn, op, arrays in pairs:
        a, b = _leaves(*arrays), _leaves(*arrays)
        va, vb = fn(*a), op(*b)
        assert vb.grad_fn is not None and torch.equal(va.detach(), vb.detach())
        va.backward()
        vb.backward()
        for s, t in zip(a, b):
            assert torch.equal(s.grad, t.grad)
        with torch.no_grad():
            assert op(*b).grad_fn is None
    assert torch.ops.rectorch_hip.mse_loss(dev(y), dev(x)).grad_fn is None


# =================================================================================================== 5. against torch's float64 autograd
def test_operators_against_float64_autograd():
    """B = 3, I = 257, Z = 5: the four operators' gradients within rel() < 2e-4 of torch's float64 CPU autograd of the reference's
    formulas (BCE: ``_Bce`` of tests/test_custom_loss_gpu.py, which takes rating targets)"""
    from rectorch_amd import engine
    y, x, mu, lv = _operands()
    p, _, _, _ = _operands(1, probabilities=True)
    p[0, :4] = [0.0, 1.0, 0.0, 1.0]                     # both clamps ...
    xr = x.copy()
    xr[0, :4] = [0.0, 0.0, 3.5, 1.0]                    # ... against a rating too

    def check(name, device_fn, host_fn, arrays):
        a = _leaves(*arrays)
        h = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in arrays]
        got, want = device_fn(*a), host_fn(*h)
        got.backward()
        want.backward()
        print("%s: %.9g, float64 %.9g" % (name, got.item(), want.item()))
        assert abs(got.item() - want.item()) <= 1e-5 * abs(want.item())
        for i, (s, t) in enumerate(zip(a, h)):
            r = rel(s.grad.cpu(), t.grad)
            print("  operand %d: rel %.3g" % (i, r))
            assert r < 2e-4, (name, i, r)
    x64 = torch.from_numpy(x).double()
    check("multinomial + 0.3 KL", lambda a, m, l: engine.multinomial_loss(a, dev(x), m, l, 0.3),
          lambda a, m, l: multinomial_kl(a, x64, m, l, 0.3), (y, mu, lv))
    check("multinomial", lambda a: engine.multinomial_loss(a, dev(x)), lambda a: multinomial_kl(a, x64), (y,))
    check("BCE + KL", lambda a, m, l: engine.bce_kl_loss(a, dev(xr), m, l),
          lambda a, m, l: cl._Bce.apply(a, torch.from_numpy(xr).double()) + kld(m, l), (p, mu, lv))
    check("MSE", lambda a: engine.mse_loss(a, dev(x)), lambda a: torch.nn.MSELoss()(x64, a), (y,))
    ws = [np.random.RandomState(t).randn(*s).astype(np.float32) for t, s in enumerate([(7, 5), (5,), (300, 13)])] + [np.zeros((4, 3), np.float32)]
    check("sum of norms", lambda *t: engine.sum_l2_norms(list(t)), lambda *t: sum(w.norm(2) for w in t), ws)


# =================================================================================================== 6. the fused step is untouched
def test_fused_step_is_unchanged_by_a_differentiable_loss_call():
    from rectorch_amd.models import MultiVAE
    x = dev(cl.make_data("vae", "g2c")[0])
    y, t, mu, lv = _operands()

    def run(call_between):
        net, _ = cl.build_net("vae", "g2c")
        model = MultiVAE(net, beta=cl.BETA, numerics="bf16")
        torch.manual_seed(21)
        model.train_batch(x)
        if call_between:
            a = _leaves(y, mu, lv)
            model.loss_function(a[0], dev(t), a[1], a[2], 0.3).backward()
            assert float(a[0].grad.abs().max()) > 0
        torch.manual_seed(22)
        model.train_batch(x)
        torch.cuda.synchronize()
        return [p.detach().clone() for p in net._param_list()]
    for a, b in zip(run(False), run(True)):
        assert torch.equal(a, b)
