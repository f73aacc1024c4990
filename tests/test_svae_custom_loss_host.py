"""CPU: the host side of SVAE's custom-loss route (``SVAE_net.differentiable``, ``SVAE.custom_loss``, ``rtx_svae_forward_train`` /
``rtx_svae_backward`` / ``rtx_svae_apply_adam``) -- the binding of the three C calls, the errors that need no device -- and the
float64 torch restatement of ``SVAE_net`` that tests/test_svae_custom_loss_gpu.py measures the device against, pinned here to
oracle/svae_oracle.py (itself pinned to the reference's recorded steps by tests/golden/g12_svae_*.npz)."""
import re

import numpy as np
import pytest
import torch

from test_custom_loss_host import _ctypes_kind, _header_args, _kind, rel

I, E, H, L, D = 120, 24, 32, 8, 40          # the dimensions of tests/test_svae_routes.py


# ------------------------------------------------------------------------------------------------ the float64 restatement
class Svae64(torch.nn.Module):
    """``SVAE_net`` (reference nets.py:624-693) in float64 torch modules on the host, eps injected: embedding -> ``nn.GRU`` -> tanh
    MLP encoder with a linear ``mu | logvar`` head -> ``z = mu + eps exp(logvar / 2)`` (always sampled) -> tanh MLP decoder with a
    linear output.  ``sd``: a state dict with the reference's keys (numpy or torch values)."""

    def __init__(self, sd):
        super().__init__()
        sd = {k: torch.as_tensor(np.array(v), dtype=torch.float64) for k, v in sd.items()}
        n_items, embed = sd["item_embed.weight"].shape
        rnn = sd["gru.weight_hh_l0"].shape[1]
        self.item_embed = torch.nn.Embedding(n_items, embed)
        self.gru = torch.nn.GRU(embed, rnn, batch_first=True, num_layers=1)
        for part in ("enc_layers", "dec_layers"):
            n = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith(part + "."))
            shapes = [sd["%s.%d.weight" % (part, i)].shape for i in range(n)]
            setattr(self, part, torch.nn.ModuleList([torch.nn.Linear(s[1], s[0]) for s in shapes]))
        self.double()
        self.load_state_dict(sd)
        self.keys = ["%s.%d.%s" % (part, i, kind) for part in ("enc_layers", "dec_layers") for i in range(len(getattr(self, part)))
                     for kind in ("weight", "bias")]
        self.keys += ["item_embed.weight", "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0"]

    def param_list(self):
        """the parameters in the engine's order (``SVAE_net._param_list``, ``SvaeOracle.keys``)"""
        named = dict(self.named_parameters())
        return [named[k] for k in self.keys]

    def forward(self, items, eps):
        """``items``: the T item ids of ONE sequence; ``eps``: [T, latent].  Returns ``(logits [T, n_items], mu, logvar)``."""
        items = torch.as_tensor(np.asarray(items), dtype=torch.long).view(1, -1)
        h = self.gru(self.item_embed(items))[0][0]
        for i, layer in enumerate(self.enc_layers):
            h = layer(h)
            if i != len(self.enc_layers) - 1:
                h = torch.tanh(h)
        Z = h.shape[1] // 2
        mu, logvar = h[:, :Z], h[:, Z:]
        h = mu + torch.as_tensor(np.asarray(eps), dtype=torch.float64) * torch.exp(0.5 * logvar)
        for i, layer in enumerate(self.dec_layers):
            h = layer(h)
            if i != len(self.dec_layers) - 1:
                h = torch.tanh(h)
        return h, mu, logvar

    def grads(self):
        """{key: gradient as numpy} after a backward (a parameter the loss did not reach: zeros)"""
        return {k: (np.zeros(tuple(p.shape)) if p.grad is None else p.grad.numpy().copy()) for k, p in zip(self.keys, self.param_list())}


def svae_loss(recon_x, x, mu, logvar, beta=1.0):
    """the reference's SVAE loss (models.py:1622-1626) in torch ops, any float type: ``recon_x`` [1, T, n_items], ``x`` the target,
    [1, T, n_items] or flattened to [1, T * n_items] as ``train_batch`` hands it over -- the normaliser is ``sum(x[0, :n_items])``"""
    n_items = recon_x.shape[2]
    nll = -(torch.log_softmax(recon_x, -1) * x.view(recon_x.shape)).sum()
    d = float(x[0, :n_items].sum())
    kl = -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=-1))
    return nll / d + beta * kl


def make_sd(R, seed, n_items=I, embed=E, hidden=H, latent=L, dec_hidden=D):
    """a state dict of ``SVAE_net`` at the test dimensions, as numpy arrays, from torch's seeded initialisation"""
    from rectorch_amd.nets import SVAE_net
    torch.manual_seed(seed)
    net = SVAE_net(n_items=n_items, embed_size=embed, rnn_size=R, dec_dims=[latent, dec_hidden, n_items], enc_dims=[R, hidden, latent])
    return {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}


def make_sequence(rng, T, n_items=I, latent=L, n_targets=3, distinct=False):
    """(items with one item repeated where T > 1, multi-hot targets [T, n_items], eps [T, latent])"""
    items = rng.choice(n_items, size=T, replace=False) if distinct else rng.randint(0, n_items, size=T)
    if T > 1 and not distinct:
        items[-1] = items[0]
    y = np.zeros((T, n_items))
    for t in range(T):
        y[t, rng.choice(n_items, size=n_targets, replace=False)] = 1.0
    return items, y, rng.randn(T, latent).astype(np.float32)


@pytest.mark.parametrize("T", [1, 2, 9])
def test_restatement_reproduces_the_oracle(T):
    """R = 3, one item repeated in the sequence: the loss and every gradient of SvaeOracle.loss_and_grads within 1e-9 relative"""
    from oracle.svae_oracle import SvaeOracle
    sd = make_sd(3, seed=40 + T)
    rng = np.random.RandomState(T)
    items, y, eps = make_sequence(rng, T)
    if T > 1:
        assert len(set(items.tolist())) < T
    beta = 0.2
    orc = SvaeOracle(sd, n_enc=2, n_dec=2, beta=beta)
    want, grads, logits, mu, lv = orc.loss_and_grads(items, y, eps.astype(np.float64), beta, likelihood_d=float(y[0].sum()))
    net = Svae64(sd)
    assert net.keys == orc.keys
    out, m, l = net(items, eps)
    loss = svae_loss(out[None], torch.from_numpy(y).view(1, -1), m, l, beta)
    loss.backward()
    assert abs(loss.item() - want) < 1e-9 * abs(want), (loss.item(), want)
    assert rel(out.detach(), logits) < 1e-9 and rel(m.detach(), mu) < 1e-9 and rel(l.detach(), lv) < 1e-9
    got = net.grads()
    for k in orc.keys:
        r = rel(got[k], grads[k])
        print("T=%d %-22s rel %.2e" % (T, k, r))
        assert r < 1e-9, (k, r)


# ------------------------------------------------------------------------------------------------ the C calls
WANT_ARGS = {
    "rtx_svae_forward_train": ["s", "items", "total_steps", "seq_ptr", "n_seq", "eps_noise", "seed", "offset", "logits_out", "mu", "logvar",
                               "ticket", "stream"],
    "rtx_svae_backward": ["s", "items", "total_steps", "seq_ptr", "n_seq", "ticket", "d_logits", "ld", "d_mu", "d_logvar", "stream"],
    "rtx_svae_apply_adam": ["s", "step", "stream"],
}


@pytest.mark.parametrize("name", sorted(WANT_ARGS))
def test_new_symbols_declared_and_bound_alike(name):
    import ctypes as C
    from rectorch_amd import _lib
    args = _header_args(name)
    assert name in _lib.SIGNATURES, "%s is missing from _lib.SIGNATURES" % name
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int
    assert [_kind(a) for a in args] == [_ctypes_kind(t) for t in argtypes], (args, argtypes)
    assert [re.sub(r"[\*\s]", "", a.split()[-1]) for a in args] == WANT_ARGS[name]


# ------------------------------------------------------------------------------------------------ errors that need no device
def _net(R=3):
    from rectorch_amd.nets import SVAE_net
    return SVAE_net(n_items=12, embed_size=4, rnn_size=R, dec_dims=[2, 5, 12], enc_dims=[R, 5, 2])


def test_defaults():
    from rectorch_amd.models import SVAE
    net = _net()
    model = SVAE(net)
    assert model.custom_loss is False and net.differentiable is False and not net._diff_active()
    net.differentiable = True
    assert net._diff_active()
    net.eval()
    assert not net._diff_active()


def test_custom_loss_with_the_package_loss_raises_before_any_gpu_call():
    from rectorch_amd.models import SVAE
    model = SVAE(_net())
    model.custom_loss = True
    with pytest.raises(ValueError, match="loss_function"):
        model.train_batch(torch.tensor([[1, 2, 3]]), torch.zeros(1, 3, 12))


def test_custom_loss_refuses_a_pack_before_any_gpu_call():
    from rectorch_amd.engine import SvaePack
    from rectorch_amd.models import SVAE

    class Mine(SVAE):
        def loss_function(self, recon_x, x, mu, logvar, beta=1.0):
            return recon_x.sum()

    model = Mine(_net())
    model.custom_loss = True
    pack = SvaePack([[1, 2], [3]], [[[4], [5]], [[6]]], device="cpu")
    with pytest.raises(NotImplementedError, match="pack"):
        model.train_batch(pack, pack)
