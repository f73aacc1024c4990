"""CPU: the host side of the differentiable device losses (``rtx_multinomial_loss_grad``, ``rtx_bce_kl_loss_grad``,
``rtx_mse_loss_grad``, ``rtx_sum_l2_norms_grad``) -- the binding of the four C calls, the errors that need no device, and the native
driver's host mode (its case generator and float64 references against central differences)."""
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from test_custom_loss_host import _ctypes_kind, _header_args, _kind

ENTRIES = {
    "rtx_multinomial_loss_grad": ["recon", "x", "batch", "n_items", "mu", "logvar", "latent", "beta", "loss_out", "d_recon", "d_mu",
                                  "d_logvar", "stream"],
    "rtx_bce_kl_loss_grad": ["recon", "x", "batch", "n_items", "mu", "logvar", "latent", "loss_out", "d_recon", "d_mu", "d_logvar",
                             "stream"],
    "rtx_mse_loss_grad": ["prediction", "ground_truth", "batch", "n_items", "loss_out", "d_prediction", "stream"],
    "rtx_sum_l2_norms_grad": ["tensors", "sizes", "n", "out", "grads", "stream"],
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_new_entries_declared_and_bound_alike(name):
    """header and ctypes table agree argument by argument, and each entry is the one without ``_grad`` plus its gradient outputs"""
    import ctypes as C
    from rectorch_amd import _lib
    args = _header_args(name)
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int

    def kind(a):
        return "float" if re.match(r"float \w+$", a) else _kind(a)

    def ckind(t):
        return "float" if t is C.c_float else _ctypes_kind(t)
    assert [kind(a) for a in args] == [ckind(t) for t in argtypes], (args, argtypes)
    names = [re.sub(r"[\*\s]", "", a.split()[-1]) for a in args]
    assert names == ENTRIES[name]
    plain = [re.sub(r"[\*\s]", "", a.split()[-1]) for a in _header_args(name[:-len("_grad")])]
    assert [n for n in names if not n.startswith("d_") and n != "grads"] == plain
    assert _lib.SIGNATURES[name[:-len("_grad")]][1] == [t for t, n in zip(argtypes, names) if not n.startswith("d_") and n != "grads"]


def test_target_requiring_grad_raises_before_any_gpu_call():
    from rectorch_amd import engine
    y = torch.zeros(3, 4, requires_grad=True)
    x = torch.zeros(3, 4, requires_grad=True)
    with pytest.raises(ValueError, match=r"\bx requires grad"):
        engine.multinomial_loss(y, x)
    with pytest.raises(ValueError, match=r"\bx requires grad"):
        engine.bce_kl_loss(y, x)
    with pytest.raises(ValueError, match="ground_truth requires grad"):
        engine.mse_loss(y, x)


def test_custom_step_still_refuses_a_loss_that_is_not_overridden():
    from rectorch_amd.models import MultiVAE
    from rectorch_amd.nets import MultiVAE_net
    m = MultiVAE(MultiVAE_net([2, 4]))
    m.custom_loss = True
    with pytest.raises(ValueError, match="loss_function"):
        m.train_batch(torch.zeros(3, 4))


def build_loss_grad(always=True):
    """the native driver's path; built by its makefile -- ``always=False``: only where it does not exist yet (the build step made it)"""
    path = os.path.join(ROOT, "build", "native", "test_loss_grad")
    if always or not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), "-f", "lossgrad.mk"])
    return path


def test_native_driver_host_mode():
    """tests/native/test_loss_grad.cpp --host: the case generator's promises (a row without a target, logits of +-80, rating targets,
    p = 0 and 1 against every target kind) and the float64 gradients against central differences of the float64 loss; no HIP call"""
    out = subprocess.run([build_loss_grad(), "--host"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout and "host reference only" in out.stdout


def test_build_step_makes_the_driver():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "lossgrad.mk" in text
