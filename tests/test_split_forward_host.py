"""CPU: the host side of the differentiable ``encode`` / ``_reparameterize`` / ``decode`` (``rtx_engine_encode_train`` /
``encode_backward`` / ``decode_train`` / ``decode_backward``, ``rtx_reparam`` / ``rtx_reparam_grad``) -- the binding of the six C
calls, the ABI number, what stays as it was with the switch off, the errors that need no device -- and the float64 restatement of
the three pieces, which tests/test_split_forward_gpu.py measures the device against, tied here to ``forward64`` of
tests/test_custom_loss_host.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_custom_loss_host import _ctypes_kind, _header_args, _kind, forward64


# ------------------------------------------------------------------------------------------------ the float64 restatement
def encode64(params, n_enc, variant, x, keep=None, p=0.0, cond_dim=0):
    """layers [0, n_enc) of ``forward64``: ``(mu, logvar)`` for "vae" / "gvae", ``(h, None)`` for "dae" """
    h = x.to(torch.float64)
    if variant != "gvae":
        items, cond = h[:, :h.shape[1] - cond_dim], h[:, h.shape[1] - cond_dim:]
        items = items / items.norm(dim=1, keepdim=True).clamp_min(1e-12)
        if keep is not None:
            items = items * keep.to(torch.float64) / (1.0 - p)
        h = torch.cat([items, cond], 1)
    for i in range(n_enc):
        h = h @ params[2 * i].T + params[2 * i + 1]
        if i < n_enc - 1 or variant == "dae":
            h = torch.tanh(h)
    if variant == "dae":
        return h, None
    return h[:, :h.shape[1] // 2], h[:, h.shape[1] // 2:]


def reparam64(mu, logvar, eps):
    return mu + eps.to(torch.float64) * torch.exp(0.5 * logvar)


def decode64(params, n_enc, variant, z):
    """layers [n_enc, n_layers) of ``forward64``"""
    n_layers = len(params) // 2
    h = z
    for i in range(n_enc, n_layers):
        h = h @ params[2 * i].T + params[2 * i + 1]
        if i < n_layers - 1:
            h = torch.tanh(h)
    return torch.sigmoid(h) if variant == "gvae" else h


@pytest.mark.parametrize("variant", ["vae", "dae", "gvae", "cond"])
def test_the_three_pieces_compose_to_forward64_exactly(variant):
    rng = np.random.RandomState(4)
    cond = 3 if variant == "cond" else 0
    enc = [19 + cond, 11, 7, 4]
    dec = [4, 6, 19]
    widths = enc[:-1] + [enc[-1] * (1 if variant == "dae" else 2)]
    dims = list(zip(widths[:-1], widths[1:])) + list(zip(dec[:-1], dec[1:]))
    params = []
    for d_in, d_out in dims:
        params += [torch.from_numpy(rng.randn(d_out, d_in) * 0.4), torch.from_numpy(rng.randn(d_out) * 0.3)]
    B = 5
    x = torch.from_numpy((rng.rand(B, enc[0]) < 0.4).astype(np.float32))
    x[:, 0] = 1.0
    keep = None if variant == "gvae" else torch.from_numpy((rng.rand(B, 19) >= 0.5).astype(np.uint8))
    eps = None if variant == "dae" else torch.from_numpy(rng.randn(B, 4).astype(np.float32))
    v = "vae" if variant == "cond" else variant
    p = 0.0 if variant == "gvae" else 0.5
    out, mu, logvar = forward64(params, 3, v, x, keep, eps, p, cond)
    a, b = encode64(params, 3, v, x, keep, p, cond)
    z = a if variant == "dae" else reparam64(a, b, eps)
    out2 = decode64(params, 3, v, z)
    assert torch.equal(out, out2)
    if variant != "dae":
        assert torch.equal(mu, a) and torch.equal(logvar, b)


# ------------------------------------------------------------------------------------------------ the C calls
NEW = {"rtx_engine_encode_train": ["e", "batch", "step", "out0", "out1", "ticket", "stream"],
       "rtx_engine_encode_backward": ["e", "batch", "step", "ticket", "d_out0", "d_out1", "cb", "user", "stream"],
       "rtx_engine_decode_train": ["e", "z", "n", "out", "ticket", "stream"],
       "rtx_engine_decode_backward": ["e", "n", "step", "ticket", "d_out", "ld", "d_z", "cb", "user", "stream"],
       "rtx_reparam": ["mu", "logvar", "n", "latent", "eps_in", "seed", "offset", "z", "eps_out", "stream"],
       "rtx_reparam_grad": ["d_z", "logvar", "eps", "n", "latent", "d_mu", "d_logvar", "stream"]}


@pytest.mark.parametrize("name", sorted(NEW))
def test_new_symbols_declared_and_bound_alike(name):
    from rectorch_amd import _lib
    args = _header_args(name)
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int
    assert [_kind(a) for a in args] == [_ctypes_kind(t) for t in argtypes], (args, argtypes)
    assert [re.sub(r"[\*\s]", "", a.split()[-1]) for a in args] == NEW[name]


def test_abi_version_is_still_8():
    from rectorch_amd import _lib
    assert _lib.lib().rtx_abi_version() == 8
    text = open(os.path.join(ROOT, "rectorch_amd", "csrc", "engine.hip")).read()
    assert re.search(r"rtx_abi_version\(void\)\s*\{\s*return 8;", text)


# ------------------------------------------------------------------------------------------------ the switch off; errors without a device
def test_reparameterize_in_training_with_the_switch_off_still_raises():
    from rectorch_amd.nets import MultiVAE_net, CMultiVAE_net
    for net in (MultiVAE_net([2, 4]), CMultiVAE_net(3, [2, 4])):
        assert net.differentiable is False and net.training
        mu = torch.zeros(3, 2)
        with pytest.raises(NotImplementedError, match="sampling outside forward"):
            net._reparameterize(mu, mu)
        net.eval()
        assert net._reparameterize(mu, mu) is mu
        net.differentiable = True
        assert net._reparameterize(mu, mu) is mu          # eval: mu, with the switch on too


def test_svae_net_keeps_raising():
    from rectorch_amd.nets import SVAE_net
    net = SVAE_net(9, 4, 6, [3, 5, 9], [6, 5, 3])
    net.differentiable = True
    z = torch.zeros(2, 3)
    for call in (lambda: net.encode(torch.zeros(2, 9)), lambda: net.decode(z), lambda: net._reparameterize(z, z)):
        with pytest.raises(NotImplementedError):
            call()


def test_input_requiring_grad_raises_before_any_gpu_call():
    from rectorch_amd.nets import MultiDAE_net, MultiVAE_net
    for net in (MultiVAE_net([2, 4]), MultiDAE_net([2, 4])):
        net.differentiable = True
        net.train()
        with pytest.raises(ValueError, match="requires_grad"):
            net.encode(torch.zeros(3, 4, requires_grad=True))


def test_a_forward_of_the_users_own_is_told_apart():
    from rectorch_amd.evaluation import _method_is_ours
    from rectorch_amd.nets import MultiDAE_net, MultiVAE_net, CMultiVAE_net, VAE_net

    class Composed(MultiVAE_net):
        def forward(self, x):
            mu, logvar = self.encode(x)
            return self.decode(self._reparameterize(mu, logvar)), mu, logvar

    for net in (MultiVAE_net([2, 4]), MultiDAE_net([2, 4]), CMultiVAE_net(3, [2, 4]), VAE_net([2, 4])):
        assert _method_is_ours(net, "forward")
    assert not _method_is_ours(Composed([2, 4]), "forward")
    net = MultiVAE_net([2, 4])
    net.forward = lambda x: None                 # an instance attribute is the user's too
    assert not _method_is_ours(net, "forward")


# ------------------------------------------------------------------------------------------------ the native driver's host mode
def build_halves(always=True):
    """the driver's path; built by its makefile -- ``always=False``: only where it does not exist yet (the build step made it)"""
    path = os.path.join(ROOT, "build", "native", "test_halves")
    if always or not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), "-f", "halves.mk"])
    return path


def test_native_driver_host_mode():
    """tests/native/test_halves.cpp --host: its case generators and float64 references against a second formulation, no HIP call"""
    out = subprocess.run([build_halves(), "--host"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout and "host reference only" in out.stdout
