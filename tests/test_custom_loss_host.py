"""CPU: the host side of the custom-loss route (``net.differentiable``, ``model.custom_loss``, ``rtx_engine_forward_train`` /
``rtx_engine_backward``) -- defaults, the binding of the two C calls, the errors that need no device -- and the float64
restatement of the networks' training forward that tests/test_custom_loss_gpu.py measures the device against, pinned here to the
reference's own recorded gradients."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, sd_from, params_in_order


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-30, np.max(np.abs(b))))


# ------------------------------------------------------------------------------------------------ the float64 restatement
def forward64(params, n_enc, variant, x, keep=None, eps=None, p=0.0, cond_dim=0):
    """The training forward of SURVEY Appendix B in float64 torch ops on the host, with the draws injected: ``params`` = [W, b, ...]
    (float64, encoder first), ``keep`` the dropout keep-mask over the item columns, ``eps`` the N(0, 1) draws.  ``variant``:
    "vae" / "dae" (normalised, dropped-out input; a conditioned input's last ``cond_dim`` columns pass raw) or "gvae" (raw input,
    sigmoid output).  Returns ``(out, mu, logvar)`` (``mu`` / ``logvar`` None for "dae")."""
    h = x.to(torch.float64)
    if variant != "gvae":
        items, cond = h[:, :h.shape[1] - cond_dim], h[:, h.shape[1] - cond_dim:]
        items = items / items.norm(dim=1, keepdim=True).clamp_min(1e-12)
        if keep is not None:
            items = items * keep.to(torch.float64) / (1.0 - p)
        h = torch.cat([items, cond], 1)
    layers = [(params[2 * i], params[2 * i + 1]) for i in range(len(params) // 2)]
    mu = logvar = None
    for i, (W, b) in enumerate(layers):
        h = h @ W.T + b
        if i == n_enc - 1 and variant != "dae":
            mu, logvar = h[:, :h.shape[1] // 2], h[:, h.shape[1] // 2:]
            h = mu + eps.to(torch.float64) * torch.exp(0.5 * logvar)
        elif i < len(layers) - 1:
            h = torch.tanh(h)
    return (torch.sigmoid(h) if variant == "gvae" else h), mu, logvar


def kld(mu, logvar):
    return -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))


def multinomial_kl(recon, gt, mu=None, logvar=None, beta=0.0):
    """the reference's MultiVAE / MultiDAE likelihood term (+ beta KLD) in torch ops, any float type"""
    nll = -torch.mean(torch.sum(torch.log_softmax(recon, 1) * gt, -1))
    return nll if mu is None else nll + beta * kld(mu, logvar)


def params64(sd):
    vals, keys = params_in_order(sd)
    return [torch.tensor(np.array(v), dtype=torch.float64, requires_grad=True) for v in vals], keys


@pytest.mark.parametrize("name", ["g2_mvae_train_step_small", "g2b_mvae_train_step_te", "g2c_mvae_train_step_deep"])
def test_restatement_reproduces_the_reference_step(name):
    """step 0 of the G2 fixtures: the restatement's loss within 1e-5 relative and its gradients within rel() < 2e-4 of the reference's
    recorded ones -- the bounds tests/test_gpu_parity.py states for the same quantities (measured: loss <= 7e-8, gradients
    <= 3.8e-7)"""
    g = load_golden(name)
    enc = [int(v) for v in g["enc_dims"]]
    beta, anneal, p, _ = [float(v) for v in g["meta"]]
    ps, keys = params64(sd_from(g, "sd0__"))
    x = torch.from_numpy(g["xs"][0])
    gt = torch.from_numpy(g["gts"][0]).double() if "gts" in g else x.double()
    out, mu, logvar = forward64(ps, len(enc) - 1, "vae", x, torch.from_numpy(g["mask_0"]), torch.from_numpy(g["eps_0"]), p)
    loss = multinomial_kl(out, gt, mu, logvar, float(g["anneal_beta_0"]))
    loss.backward()
    want = float(g["loss_0"])
    print(name, "loss rel. error %.2e" % (abs(loss.item() - want) / abs(want)))
    assert abs(loss.item() - want) < 1e-5 * abs(want)
    assert rel(out.detach(), g["logits_0"]) < 1e-5
    worst = 0.0
    for k, prm in zip(keys, ps):
        r = rel(prm.grad, g["grad_0__%s" % k.replace(".", "__")])
        worst = max(worst, r)
        assert r < 2e-4, (k, r)
    print(name, "max gradient rel() %.2e" % worst)


# ------------------------------------------------------------------------------------------------ defaults
def test_defaults_and_loss_kinds():
    from rectorch_amd.models import AETrainer, MultiDAE, MultiVAE, CMultiVAE, VAE
    from rectorch_amd.nets import MultiDAE_net, MultiVAE_net, CMultiVAE_net, VAE_net

    class Other(AETrainer):
        def loss_function(self, prediction, ground_truth):
            return None

    models = [(AETrainer(MultiDAE_net([2, 4])), "mse"), (Other(MultiDAE_net([2, 4])), "multinomial"),
              (MultiDAE(MultiDAE_net([2, 4])), "multinomial"), (MultiVAE(MultiVAE_net([2, 4])), "multinomial"),
              (CMultiVAE(CMultiVAE_net(3, [2, 4])), "multinomial"), (VAE(VAE_net([1, 2], [2, 1])), "bce"),
              (VAE(MultiVAE_net([2, 4])), "multinomial")]
    for m, kind in models:
        assert m.custom_loss is False
        assert m.network.differentiable is False
        assert m._loss_kind == kind, type(m).__name__
        m.custom_loss = True                      # an attribute like keep_grads: the loss kind of the fused step is untouched
        assert m._loss_kind == kind
    net = MultiVAE_net([2, 4])
    assert not net._diff_active()
    net.differentiable = True
    assert net._diff_active() and net._diff_numerics() == "fp32"
    net.differentiable = "bf16"
    assert net._diff_numerics() == "bf16"
    net.eval()
    assert not net._diff_active()
    net.train()
    with torch.no_grad():
        assert not net._diff_active()
    net.differentiable = "fp16"
    with pytest.raises(ValueError):
        net._diff_numerics()


# ------------------------------------------------------------------------------------------------ the C calls
def _header_args(name):
    text = open(os.path.join(ROOT, "include", "rectorch_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, re.S)
    assert m, "%s is not declared in include/rectorch_hip.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _kind(c_arg):
    if "rtx_layer_cb" in c_arg:
        return "callback"
    if "*" in c_arg:
        return "pointer"
    for t in ("uint64_t", "int64_t", "int32_t"):
        if re.search(r"\b%s\b" % t, c_arg):
            return t
    raise AssertionError("unexpected argument '%s'" % c_arg)


def _ctypes_kind(t):
    import ctypes as C
    from rectorch_amd import _lib
    if t is _lib.LAYER_CB:
        return "callback"
    if t is C.c_void_p or t is C.c_char_p or isinstance(t, type(C.POINTER(C.c_int))):
        return "pointer"
    return {C.c_uint64: "uint64_t", C.c_int64: "int64_t", C.c_int32: "int32_t"}[t]


@pytest.mark.parametrize("name", ["rtx_engine_forward_train", "rtx_engine_backward"])
def test_new_symbols_declared_and_bound_alike(name):
    import ctypes as C
    from rectorch_amd import _lib
    args = _header_args(name)
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int
    assert [_kind(a) for a in args] == [_ctypes_kind(t) for t in argtypes], (args, argtypes)
    names = [re.sub(r"[\*\s]", "", a.split()[-1]) for a in args]
    want = {"rtx_engine_forward_train": ["e", "batch", "step", "out", "mu", "logvar", "ticket", "stream"],
            "rtx_engine_backward": ["e", "batch", "step", "ticket", "d_out", "ld", "d_mu", "d_logvar", "cb", "user", "stream"]}[name]
    assert names == want


# ------------------------------------------------------------------------------------------------ errors that need no device
def test_custom_loss_with_a_package_loss_raises_before_any_gpu_call():
    from rectorch_amd.models import AETrainer, MultiDAE, MultiVAE, VAE
    from rectorch_amd.nets import MultiDAE_net, MultiVAE_net, VAE_net
    x = torch.zeros(3, 4)
    for m in (AETrainer(MultiDAE_net([2, 4])), MultiDAE(MultiDAE_net([2, 4])), MultiVAE(MultiVAE_net([2, 4])), VAE(VAE_net([2, 4]))):
        m.custom_loss = True
        with pytest.raises(ValueError, match="loss_function"):
            m.train_batch(x)

    class Mine(MultiVAE):
        def loss_function(self, recon_x, x, mu, logvar, beta=1.0):
            return recon_x.sum()

    from rectorch_amd.evaluation import _method_is_ours
    assert not _method_is_ours(Mine(MultiVAE_net([2, 4])), "loss_function")
    m = MultiVAE(MultiVAE_net([2, 4]))
    m.loss_function = lambda *a: None            # an instance attribute is the user's too
    assert not _method_is_ours(m, "loss_function")


def test_input_requiring_grad_raises_before_any_gpu_call():
    from rectorch_amd.nets import MultiDAE_net, MultiVAE_net
    for net in (MultiVAE_net([2, 4]), MultiDAE_net([2, 4])):
        net.differentiable = True
        net.train()
        with pytest.raises(ValueError, match="requires_grad"):
            net(torch.zeros(3, 4, requires_grad=True))


def test_data_parallel_plan_refuses_custom_loss():
    from rectorch_amd import _lib
    from rectorch_amd.models import MultiVAE
    from rectorch_amd.nets import MultiVAE_net

    class Mine(MultiVAE):
        def loss_function(self, recon_x, x, mu, logvar, beta=1.0):
            return recon_x.sum()

    m = Mine(MultiVAE_net([2, 4]))
    m.custom_loss = True
    m._rtx.reducer = object()
    with pytest.raises(_lib.RtxError, match="data-parallel"):
        m.train_batch(torch.zeros(3, 4))


# ------------------------------------------------------------------------------------------------ the native driver's host mode
def build_extgrad(always=True):
    """the driver's path; built by its makefile -- ``always=False``: only where it does not exist yet (as tests/test_gpu_parity.py
    treats the other native drivers: the build step made it)"""
    path = os.path.join(ROOT, "build", "native", "test_extgrad")
    if always or not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), "-f", "extgrad.mk"])
    return path


def test_native_driver_host_mode():
    """tests/native/test_extgrad.cpp --host: its case generator and float64 reference against a second formulation, no HIP call"""
    out = subprocess.run([build_extgrad(), "--host"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout and "host reference only" in out.stdout
