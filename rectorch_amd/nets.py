"""Network classes of the Mult-VAE / Mult-DAE path with the reference's API (rectorch/nets.py), computed
by librectorch_hip on an MI355X.

The classes are ``torch.nn.Module`` s holding ordinary ``nn.Linear`` parameters (same ``state_dict`` keys
and shapes as the reference: ``enc_layers.{i}.weight/bias``, ``dec_layers.{i}.weight/bias``, so reference
checkpoints load), but ``encode`` / ``decode`` / ``forward`` do not run torch kernels: they hand the
parameters' device pointers to the HIP engine.  By default these methods are forward-only (no autograd graph) and training
goes through :class:`rectorch_amd.models.MultiVAE` / ``MultiDAE``, which use the engine's fused forward+loss+backward+Adam
step.  With ``net.differentiable`` set, ``net(x)`` in training mode is a ``torch.autograd.Function`` over the engine's
training forward and its backward chain (``rtx_engine_forward_train`` / ``rtx_engine_backward``): the outputs carry a
``grad_fn``, ``loss.backward()`` fills ``p.grad``, and any torch loss and optimizer train the network -- the reference's
``forward -> loss_function -> loss.backward() -> optimizer.step()``.  The inputs are constants (no ``d / dx``) and the Functions
are once-differentiable.  The same switch makes the three documented pieces differentiable on their own -- ``encode`` and
``decode`` over the engine's two halves (``rtx_engine_encode_train`` / ``encode_backward``, ``rtx_engine_decode_train`` /
``decode_backward``), ``_reparameterize`` over ``rtx_reparam`` -- so a subclass may compose its own ``forward`` from them with any
sampling in between.  One encode and one decode per backward: a second one makes the first one's ticket stale (stack several views
or samples as ONE batch).  :class:`SVAE_net` has ``net(x)`` alone, over its own engine (``rtx_svae_forward_train`` /
``rtx_svae_backward``).

Reference: AE_net nets.py:22-96, MultiDAE_net :175-247, VAE_net :250-353, MultiVAE_net :356-417.
"""
import logging

import torch
from torch import nn
from torch.nn.init import xavier_uniform_ as xavier_init
from torch.nn.init import normal_ as normal_init

from torch.autograd.function import once_differentiable

from . import _lib
from .engine import Engine

__all__ = ['AE_net', 'MultiDAE_net', 'CDAE_net', 'VAE_net', 'MultiVAE_net', 'CMultiVAE_net', 'SVAE_net']

logger = logging.getLogger(__name__)

DEFAULT_MAX_BATCH = 512


def draw_seed():
    """One 63-bit Philox seed per stochastic call, drawn from torch's global CPU generator: like the
    reference, ``torch.manual_seed(s)`` makes dropout masks and eps reproducible (tests/test_nets.py:56-74:
    encode and forward under the same seed give the same mu/logvar)."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


class _EngineTrainForward(torch.autograd.Function):
    """``net(x)`` of a differentiable network: ``forward`` is ``rtx_engine_forward_train`` (the activations stay in the engine,
    named by a ticket), ``backward`` is ``rtx_engine_backward`` from autograd's gradients of the outputs; the parameters'
    gradients leave the engine's bound buffers as copies, so that autograd sets or accumulates ``p.grad`` by its own rules."""

    @staticmethod
    def forward(ctx, net, eng, key, x, step, alive, grads, *params):
        out, mu, logvar, ticket, batch, keep = eng.forward_train(x, step)
        ctx.rtx = (net, eng, key, step, ticket, batch, (keep, alive, x), grads)
        ctx.set_materialize_grads(False)
        if mu is None:
            return out
        return out, mu, logvar

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_mu=None, g_logvar=None):
        net, eng, key, step, ticket, batch, _alive, grads = ctx.rtx
        if net._rtx_engines.get(key) is not eng or eng._bound is None or eng._bound[1] is not grads:
            raise RuntimeError("backward: stale ticket %d: the network's engine was rebuilt (a larger batch arrived) or bound to other "
                               "training buffers after this forward; run the forward again" % ticket)
        if g_out is None:
            g_out = torch.zeros((batch.batch, eng.n_items), dtype=torch.float32, device=grads[0].device)
        if (g_mu is None) != (g_logvar is None):
            ref = g_mu if g_mu is not None else g_logvar
            g_mu = torch.zeros_like(ref) if g_mu is None else g_mu
            g_logvar = torch.zeros_like(ref) if g_logvar is None else g_logvar
        eng.backward(batch, step, ticket, g_out, g_mu, g_logvar)       # (a stale ticket: RtxError, a RuntimeError, nothing enqueued)
        return (None,) * 7 + _param_grads(net, grads)


def _param_grads(net, grads):
    """what a Function hands autograd for its parameters: copies of the engine's gradient buffers -- or nothing inside a trainer's
    accumulation window (``net._rtx_accum``), where those buffers ARE the accumulators and the engine has just added into them"""
    if getattr(net, "_rtx_accum", False):
        return (None,) * len(grads)
    return tuple(g.clone() for g in grads)


def _engine_is_stale(net, eng, key, grads):
    """the engine a Function's forward ran on is no longer the network's, or no longer writes the gradient buffers it returns"""
    return net._rtx_engines.get(key) is not eng or eng._bound is None or eng._bound[1] is not grads


class _EngineEncode(torch.autograd.Function):
    """``net.encode(x)`` of a differentiable network: ``rtx_engine_encode_train`` forward, ``rtx_engine_encode_backward`` from
    autograd's gradients of ``(mu, logvar)`` or ``h``; built like :class:`_EngineTrainForward`, with the encoder layers' parameters
    alone as operands -- it returns copies of THEIR gradients only."""

    @staticmethod
    def forward(ctx, net, eng, key, x, step, alive, grads, *params):
        o0, o1, ticket, batch, keep = eng.encode_train(x, step)
        ctx.rtx = (net, eng, key, step, ticket, batch, (keep, alive, x), grads, len(params))
        ctx.set_materialize_grads(False)
        return o0 if o1 is None else (o0, o1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g0, g1=None):
        net, eng, key, step, ticket, batch, _alive, grads, n_params = ctx.rtx
        if _engine_is_stale(net, eng, key, grads):
            raise RuntimeError("encode_backward: stale ticket %d: the network's engine was rebuilt (a larger batch arrived) or bound to "
                               "other training buffers after this encode; run the forward again" % ticket)
        vae = eng.variant in ("vae", "gvae")
        zeros = lambda: torch.zeros((batch.batch, eng.latent), dtype=torch.float32, device=grads[0].device)
        g0 = zeros() if g0 is None else g0
        g1 = (zeros() if g1 is None else g1) if vae else None
        eng.encode_backward(batch, step, ticket, g0, g1)               # (a stale ticket: RtxError, a RuntimeError, nothing enqueued)
        return (None,) * 7 + _param_grads(net, grads[:n_params])


class _EngineDecode(torch.autograd.Function):
    """``net.decode(z)`` of a differentiable network: ``rtx_engine_decode_train`` forward, ``rtx_engine_decode_backward`` from
    autograd's gradient of the output: copies of the decoder layers' gradients, and ``d loss / d z`` when ``z`` requires grad."""

    @staticmethod
    def forward(ctx, net, eng, key, z, grads, *params):
        out, ticket = eng.decode_train(z)
        ctx.rtx = (net, eng, key, ticket, z.shape[0], grads, len(params))
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        net, eng, key, ticket, n, grads, n_params = ctx.rtx
        if _engine_is_stale(net, eng, key, grads):
            raise RuntimeError("decode_backward: stale ticket %d: the network's engine was rebuilt (a larger batch arrived) or bound to "
                               "other training buffers after this decode; run the forward again" % ticket)
        if g_out is None:
            g_out = torch.zeros((n, eng.n_items), dtype=torch.float32, device=grads[0].device)
        d_z = eng.decode_backward(n, ticket, g_out, want_dz=ctx.needs_input_grad[3])
        return (None, None, None, d_z, None) + _param_grads(net, grads[len(grads) - n_params:])


class _SvaeTrainForward(torch.autograd.Function):
    """:class:`_EngineTrainForward` for :class:`SVAE_net`: ``rtx_svae_forward_train`` / ``rtx_svae_backward``.  The outputs are the
    rows of all time steps: ``(logits [T, n_items], mu [T, latent], logvar [T, latent])``."""

    @staticmethod
    def forward(ctx, net, eng, x, step, alive, grads, *params):
        logits, mu, logvar, ticket, seqs = eng.forward_train(x, step)
        ctx.rtx = (net, eng, ticket, seqs, (alive, step), grads)
        ctx.set_materialize_grads(False)
        return logits, mu, logvar

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_mu, g_logvar):
        net, eng, ticket, seqs, _alive, grads = ctx.rtx
        if net._svae_engine is not eng or len(eng._keep) < 2 or eng._keep[1] is not grads:
            raise RuntimeError("backward: stale ticket %d: the network's engine was rebuilt (a longer sequence arrived) or bound to other "
                               "training buffers after this forward; run the forward again" % ticket)
        eng.backward(seqs, ticket, g_out, g_mu, g_logvar)       # (a stale ticket: RtxError, a RuntimeError, nothing enqueued)
        return (None,) * 6 + tuple(g.clone() for g in grads)


class AE_net(nn.Module):
    r"""Abstract Autoencoder network (reference nets.py:22-96).

    Parameters
    ----------
    dec_dims : list of int
        Decoder dimensions, ``dec_dims[0]`` latent size ... ``dec_dims[-1]`` input size.
    enc_dims : list of int or None
        Encoder dimensions; if it evaluates to False, ``enc_dims = dec_dims[::-1]``.
    """
    _variant = None

    def __init__(self, dec_dims, enc_dims=None):
        super(AE_net, self).__init__()
        if enc_dims:
            self.enc_dims = enc_dims
        else:
            self.enc_dims = dec_dims[::-1]
        self.dec_dims = dec_dims
        self._rtx_engines = {}
        self._rtx_shadow_versions = {}
        self._rtx_masters_stale = False     # data parallel, sharded optimizer: this rank's float32 masters hold only ITS rows
        # False: net(x) is forward-only.  True (= "fp32"), "fp32" or "bf16": in training mode with grad mode on, net(x) goes through
        # the engine of that numerics mode as an autograd Function -- outputs with a grad_fn, loss.backward() fills p.grad -- and so
        # do encode(x), decode(z) and _reparameterize(mu, logvar) on their own, for a forward a subclass composes from them
        self.differentiable = False
        self._rtx_diff_bufs = None          # (gradient buffers the engine writes, stand-in Adam moments): never p.grad itself

    def encode(self, x):
        raise NotImplementedError()

    def decode(self, z):
        raise NotImplementedError()

    def forward(self, x):
        z = self.encode(x)
        return self.decode(z)

    def init_weights(self):
        raise NotImplementedError()

    # ---- HIP engine plumbing (not part of the reference API) -------------------------------------
    def _param_list(self):
        ps = []
        for layer in list(self.enc_layers) + list(self.dec_layers):
            ps += [layer.weight, layer.bias]
        return ps

    def _param_version(self):
        return tuple((p.data_ptr(), p._version) for p in self._param_list())

    def _device(self):
        p = next(self.parameters())
        if not p.is_cuda:
            _lib.require_gpu()
            raise _lib.RtxError("the network's parameters are on %s; move it to the MI355X first (net.to('cuda')): "
                                "rectorch_amd has no CPU compute path" % p.device)
        return p.device

    @staticmethod
    def _rtx_engine_key(numerics, loss=None):
        """key of the engine cache: the numerics mode alone for the network's own training loss (and for every forward), the
        pair (numerics, loss) for a trainer with another loss -- ``AETrainer``'s "mse" on a :class:`MultiDAE_net`"""
        return numerics if loss in (None, "multinomial", "bce") else (numerics, loss)

    def rtx_engine(self, numerics="fp32", max_batch=DEFAULT_MAX_BATCH, train_buffers=None, loss=None):
        """The engine of this network for a numerics mode ("fp32": exact-f32 MFMA, parity mode; "bf16":
        bf16 MFMA with f32 accumulation).  Rebuilt when a larger batch arrives, re-bound when the parameter
        storage changes, shadows refreshed when the parameters were modified by anyone but the engine.
        ``loss="mse"`` (a :class:`MultiDAE_net` only): the training engine of the plain autoencoder, the engine variant
        ``RTX_AE`` -- an engine of its own, never the one that trains the multinomial loss."""
        self._device()
        variant = self._variant
        if loss == "mse":
            if variant != "dae":
                raise NotImplementedError("the MSE autoencoder step runs on a MultiDAE_net; %s has no such engine" % type(self).__name__)
            variant = "ae"
        key = self._rtx_engine_key(numerics, loss)
        eng = self._rtx_engines.get(key)
        if getattr(self, "_rtx_masters_stale", False) and (
                eng is None or eng.max_batch < max_batch or self._rtx_shadow_versions.get(key) != self._param_version()):
            # building an engine or refreshing its compute copies reads the float32 masters, of which this rank holds current
            # values only for its own rows of the sharded matrices: wrong weights with no error otherwise
            raise _lib.RtxError("sharded optimizer: an engine (%s numerics, batch %d) would be rebuilt from float32 masters whose "
                                "rows of other ranks are stale; call model.consolidate() on EVERY rank first" % (numerics, max_batch))
        if eng is None or eng.max_batch < max_batch:
            if eng is not None:
                # the engine that is let go may hold the optimizer state of its last deferred steps tile-major: back into the tensors
                # on this stream, before its successor reads them
                eng.join()
            mb = max(max_batch, DEFAULT_MAX_BATCH if eng is None else eng.max_batch)
            dropout = getattr(self, "dropout", None)        # (VAE_net has none: p = 0)
            eng = Engine(self.enc_dims, self.dec_dims, variant, 0.0 if dropout is None else dropout.p, numerics, mb,
                         cond_dim=getattr(self, "cond_dim", 0))
            self._rtx_engines[key] = eng
            self._rtx_shadow_versions.pop(key, None)
        params = [p.data for p in self._param_list()]
        pkey = tuple(t.data_ptr() for t in params)
        tkey = None if train_buffers is None else tuple(t.data_ptr() for ts in train_buffers for t in ts)
        if getattr(eng, "param_key", None) != pkey or (tkey is not None and getattr(eng, "train_key", None) != tkey):
            eng.join()      # (the tensors bound so far get their optimizer state back before the engine lets go of them)
            if train_buffers is not None:
                eng.bind(params, *train_buffers)
            else:
                eng.bind(params)
            eng.param_key, eng.train_key = pkey, tkey
            self._rtx_shadow_versions.pop(key, None)
        ver = self._param_version()
        if self._rtx_shadow_versions.get(key) != ver:
            eng.sync_shadows()
            self._rtx_shadow_versions[key] = ver
        return eng

    def _rtx_mark_updated(self, numerics):
        """Called by the trainer after an engine-side Adam step: that engine's shadows are fresh, every other
        engine's are stale (the master parameters changed under them).  ``numerics``: that engine's cache key."""
        ver = self._param_version()
        for k in list(self._rtx_shadow_versions):
            if k != numerics:
                self._rtx_shadow_versions.pop(k)
        self._rtx_shadow_versions[numerics] = ver

    def _as_input(self, x):
        from .engine import RowBatch, tagged_rows
        if isinstance(x, RowBatch) or tagged_rows(x) is not None:
            return x
        dev = self._device()
        return x.reshape(x.shape[0], -1).to(dev, torch.float32).contiguous()

    # ---- autograd through the engine (net.differentiable) ------------------------------------------
    def _diff_numerics(self):
        d = self.differentiable
        if d is True:
            return "fp32"
        if d in ("fp32", "bf16"):
            return d
        raise ValueError("net.differentiable must be False, True, 'fp32' or 'bf16', got %r" % (d,))

    def _diff_active(self):
        return bool(self.differentiable) and self.training and torch.is_grad_enabled()

    def _diff_buffers(self):
        """the gradient buffers the differentiable route binds its engine to, and zero stand-ins for the Adam moments the engine's
        binding wants (a trainer passes its optimizer's).  Buffers of their own: were they ``p.grad``, autograd's accumulation
        of what ``backward`` returns would double or drop a term."""
        params = self._param_list()
        b = self._rtx_diff_bufs
        if b is None or b[0][0].device != params[0].device or [g.shape for g in b[0]] != [p.shape for p in params]:
            b = self._rtx_diff_bufs = ([torch.zeros_like(p.data) for p in params], None)
        return b

    def _diff_moments(self):
        grads, mom = self._diff_buffers()
        if mom is None:
            mom = ([torch.zeros_like(g) for g in grads], [torch.zeros_like(g) for g in grads])
            self._rtx_diff_bufs = (grads, mom)
        return mom

    def _differentiable_forward(self, x, numerics=None, mask=None, noise=None, moments=None):
        """``net(x)`` as an autograd Function over the engine (see the module docstring).  ``numerics`` / ``moments``: a trainer's
        own mode and its optimizer's ``(exp_avg, exp_avg_sq)`` lists; ``mask`` / ``noise``: injected draws (parity tests)."""
        from .engine import RowBatch
        if isinstance(x, torch.Tensor) and x.requires_grad:
            raise ValueError("the differentiable route treats its input as a constant (no d / dx): x.requires_grad is set")
        numerics = numerics or self._diff_numerics()
        x = self._as_input(x)
        B = len(x) if isinstance(x, RowBatch) else x.shape[0]
        grads = self._diff_buffers()[0]
        m, v = moments if moments is not None else self._diff_moments()
        eng = self.rtx_engine(numerics, B, train_buffers=(grads, m, v))
        step = eng._step(seed=draw_seed(), mask=mask, noise=noise)
        return _EngineTrainForward.apply(self, eng, self._rtx_engine_key(numerics), x, step, (mask, noise), grads, *self._param_list())

    def _diff_engine(self, n, numerics=None, moments=None):
        """``(cache key, gradient buffers, engine)`` of the differentiable route for a batch of ``n`` rows.  A trainer that runs the
        network's own ``forward`` announces its numerics through ``differentiable`` and its moments through ``_rtx_trainer``."""
        numerics = numerics or self._diff_numerics()
        grads = self._diff_buffers()[0]
        m, v = moments or getattr(self, "_rtx_trainer", {}).get("moments") or self._diff_moments()
        return self._rtx_engine_key(numerics), grads, self.rtx_engine(numerics, n, train_buffers=(grads, m, v))

    def _injected(self, what):
        """the draw a trainer injects into the pieces of a composed forward (parity tests): "mask" or "noise" """
        return getattr(self, "_rtx_trainer", {}).get(what)

    def _differentiable_encode(self, x, numerics=None, mask=None, moments=None):
        """``net.encode(x)`` as an autograd Function over the engine's encoder half: ``(mu, logvar)`` or ``h`` with a ``grad_fn``.
        Arguments as :meth:`_differentiable_forward`."""
        from .engine import RowBatch
        if isinstance(x, torch.Tensor) and x.requires_grad:
            raise ValueError("the differentiable route treats its input as a constant (no d / dx): x.requires_grad is set")
        x = self._as_input(x)
        B = len(x) if isinstance(x, RowBatch) else x.shape[0]
        key, grads, eng = self._diff_engine(B, numerics, moments)
        mask = mask if mask is not None else self._injected("mask")
        step = eng._step(seed=draw_seed(), mask=mask)
        return _EngineEncode.apply(self, eng, key, x, step, mask, grads, *self._param_list()[:2 * len(self.enc_layers)])

    def _differentiable_decode(self, z, numerics=None, moments=None):
        """``net.decode(z)`` as an autograd Function over the engine's decoder half; ``z`` may require grad"""
        z = z.to(self._device(), torch.float32)
        key, grads, eng = self._diff_engine(z.shape[0], numerics, moments)
        return _EngineDecode.apply(self, eng, key, z, grads, *self._param_list()[2 * len(self.enc_layers):])

    def _init_linear(self):
        for layer in self.enc_layers:
            xavier_init(layer.weight)
            normal_init(layer.bias)
        for layer in self.dec_layers:
            xavier_init(layer.weight)
            normal_init(layer.bias)


class MultiDAE_net(AE_net):
    r"""Denoising Autoencoder network for collaborative filtering (reference nets.py:175-247):
    L2-normalise -> dropout -> tanh(Linear) on every encoder layer; decoder tanh on all but the last layer.
    """
    _variant = "dae"

    def __init__(self, dec_dims, enc_dims=None, dropout=0.5):
        super(MultiDAE_net, self).__init__(dec_dims, enc_dims)
        self.dropout = nn.Dropout(dropout)
        self.enc_layers = nn.ModuleList(
            [nn.Linear(d_in, d_out) for d_in, d_out in zip(self.enc_dims[:-1], self.enc_dims[1:])])
        self.dec_layers = nn.ModuleList(
            [nn.Linear(d_in, d_out) for d_in, d_out in zip(self.dec_dims[:-1], self.dec_dims[1:])])
        self.init_weights()

    def encode(self, x, _mask=None):
        if self._diff_active():
            return self._differentiable_encode(x, mask=_mask)
        x = self._as_input(x)
        eng = self.rtx_engine("fp32", x.shape[0])
        h, _ = eng.encode(x, training=self.training, seed=draw_seed() if self.training else 0)
        return h

    def decode(self, z):
        if self._diff_active():
            return self._differentiable_decode(z)
        eng = self.rtx_engine("fp32", z.shape[0])
        return eng.decode(z.to(self._device()))

    def forward(self, x):
        if self._diff_active():
            return self._differentiable_forward(x)
        x = self._as_input(x)
        eng = self.rtx_engine("fp32", x.shape[0])
        logits, _, _ = eng.forward(x, training=self.training, seed=draw_seed() if self.training else 0)
        return logits

    def init_weights(self):
        r"""xavier_uniform weights, N(0,1) biases (reference nets.py:235-247)."""
        self._init_linear()


class CDAE_net(MultiDAE_net):
    r"""Collaborative Denoising Auto-Encoder network (Wu, DuBois, Zheng, Ester, WSDM 2016), with the signature of the reference's
    ``CDAE_net`` (nets.py:100-172).  The reference's class is not exported and marked unchecked, so the definition is this package's
    (include/rectorch_hip.h, "CDAE"): a :class:`MultiDAE_net` with one layer on each side plus one vector per training user added
    in front of the hidden activation,

    .. math:: h = \tanh(W_0\,\mathrm{dropout}(\mathrm{normalize}(x_b)) + b_0 + [u \ge 0]\,V_u), \qquad out = W_1 h + b_1 .

    ``user_factors`` is an ``nn.Embedding(n_users, latent_size, sparse=True)``, zero-initialised: an untrained user, an id of -1
    and a call without ids all give :class:`MultiDAE_net`'s forward exactly.  ``encode`` and ``forward`` take the ids as a second
    argument (``users``: an int tensor, one id per row; ids outside ``[0, n_users)`` count as -1).

    Train it with :class:`rectorch_amd.models.MultiDAE` (multinomial likelihood + the norm regulariser over W and b, not over V) or
    :class:`rectorch_amd.models.AETrainer` (MSE) on a ``DataSampler(..., user_ids=...)``.  ``W, b`` follow ``model.optimizer``;
    the table follows ``model.user_optimizer``, a ``torch.optim.SparseAdam``, on the rows of each batch, inside the step's
    backward kernel -- ``user_factors.weight.grad`` stays ``None``.  ``net.differentiable`` (the autograd route) is not available.
    """

    def __init__(self, n_items, n_users, latent_size=50, dropout=0.5):
        super(CDAE_net, self).__init__([latent_size, n_items], [n_items, latent_size], dropout)
        self.n_items, self.n_users, self.latent_size = int(n_items), int(n_users), int(latent_size)
        self.user_factors = nn.Embedding(self.n_users, self.latent_size, sparse=True)
        nn.init.zeros_(self.user_factors.weight)
        self._rtx_user_moments = None       # (exp_avg, exp_avg_sq) of the trainer's SparseAdam, for the training engine

    def _dense_parameters(self):
        """what ``model.optimizer`` and the regulariser see: W and b, not the user table"""
        return self._param_list()

    def _diff_active(self):
        if self.differentiable:
            raise NotImplementedError("CDAE_net has no differentiable route (net.differentiable / custom_loss = True): the user "
                                      "table's gradient never leaves the backward kernel; supported: MultiDAE(CDAE_net) and "
                                      "AETrainer(CDAE_net) with their built-in losses")
        return False

    def rtx_engine(self, numerics="fp32", max_batch=DEFAULT_MAX_BATCH, train_buffers=None, loss=None):
        """:meth:`AE_net.rtx_engine`, with the user table bound to the engine (the table is not part of the parameter list or of
        the cache key; a training engine also gets the moments the trainer left in ``_rtx_user_moments``)"""
        eng = super(CDAE_net, self).rtx_engine(numerics, max_batch, train_buffers, loss)
        V = self.user_factors.weight.data
        keep = getattr(eng, "_users_keep", None)
        if train_buffers is not None and self._rtx_user_moments is not None:
            eng.bind_users(V, *self._rtx_user_moments)
        elif keep is None or keep[0].data_ptr() != V.data_ptr():
            eng.bind_users(V)           # (a forward needs no moments; a binding that already names this table stays)
        return eng

    def _users_for(self, eng, x, users):
        from .engine import batch_users
        eng.set_users(batch_users(x, users), batch=None)

    def encode(self, x, users=None, _mask=None):
        self._diff_active()
        x = self._as_input(x)
        eng = self.rtx_engine("fp32", len(x) if not isinstance(x, torch.Tensor) else x.shape[0])
        self._users_for(eng, x, users)
        h, _ = eng.encode(x, training=self.training, seed=draw_seed() if self.training else 0, mask=_mask)
        return h

    def forward(self, x, users=None):
        self._diff_active()
        x = self._as_input(x)
        eng = self.rtx_engine("fp32", len(x) if not isinstance(x, torch.Tensor) else x.shape[0])
        self._users_for(eng, x, users)
        logits, _, _ = eng.forward(x, training=self.training, seed=draw_seed() if self.training else 0)
        return logits


class VAE_net(AE_net):
    r"""Variational Autoencoder network (reference nets.py:250-353): builds the layers (the last encoder layer
    emits mean and log-variance) and initialises them.

    On the device this is the engine variant ``"gvae"`` (``RTX_GVAE``): the input rows enter raw (no normalisation,
    no dropout), tanh hidden layers, ``z = mu + eps * exp(logvar / 2)`` sampled in every mode (the reference's
    ``_reparameterize`` has no eval branch), a sigmoid output, and the BCE + KL loss of :class:`rectorch_amd.models.VAE`.
    That model trains and scores it; the network's own ``encode`` (``(mu, logvar)``), ``decode`` (sigmoid probabilities) and
    ``forward`` (``(probabilities, mu, logvar)``, one seed from torch's generator per call) run on the same engine
    (``rtx_engine_encode`` / ``decode`` / ``forward``) once the network is on the device; a network still on the host, and
    :class:`SVAE_net`, which has an engine of its own, keep raising ``NotImplementedError``.  With ``differentiable`` set,
    ``forward`` in training mode carries a ``grad_fn`` (the gradient handed back is taken w.r.t. the probabilities)."""
    _variant = "gvae"

    def __init__(self, dec_dims, enc_dims=None):
        super(VAE_net, self).__init__(dec_dims, enc_dims)
        temp_dims = self.enc_dims[:-1] + [self.enc_dims[-1] * 2]
        self.enc_layers = nn.ModuleList(
            [nn.Linear(d_in, d_out) for d_in, d_out in zip(temp_dims[:-1], temp_dims[1:])])
        self.dec_layers = nn.ModuleList(
            [nn.Linear(d_in, d_out) for d_in, d_out in zip(self.dec_dims[:-1], self.dec_dims[1:])])
        self.init_weights()

    def _own_engine(self, n):
        if self._variant != "gvae":
            raise NotImplementedError("%s has an engine of its own; VAE_net's encode / decode do not apply to it" % type(self).__name__)
        if not next(self.parameters()).is_cuda:
            raise NotImplementedError("VAE_net computes through its engine (RTX_GVAE) on the MI355X only and this network is on the "
                                      "host: move it to the device first (net.to('cuda'))")
        return self.rtx_engine("fp32", n)

    def encode(self, x):
        eng = self._own_engine(x.shape[0])
        if self._diff_active():
            return self._differentiable_encode(x)
        return eng.encode(self._as_input(x))

    def _reparameterize(self, mu, var, _noise=None):
        """``mu + eps * exp(var / 2)``, sampled in every mode as the reference's is (nets.py:317-320; ``var`` is the log-variance):
        one seed from torch's generator per call, the head's own draws and arithmetic (``rtx_reparam``), differentiable with
        respect to ``mu`` and ``var``."""
        from .engine import reparameterize
        self._own_engine(mu.shape[0])
        noise = _noise if _noise is not None else self._injected("noise")
        return reparameterize(mu, var, seed=draw_seed(), noise=noise)

    def decode(self, z):
        eng = self._own_engine(z.shape[0])
        if self._diff_active():
            return self._differentiable_decode(z)
        return eng.decode(z.to(self._device()))

    def forward(self, x):
        eng = self._own_engine(len(x))
        if self._diff_active():
            return self._differentiable_forward(x)
        # z is sampled in every mode (_reparameterize has no eval branch): one seed per call, as VAE.predict draws it
        return eng.forward(self._as_input(x), training=self.training, seed=draw_seed())

    def init_weights(self):
        r"""xavier_uniform weights, N(0,1) biases (reference nets.py:341-353)."""
        self._init_linear()


class MultiVAE_net(VAE_net):
    r"""Variational Autoencoder network for collaborative filtering (reference nets.py:356-417):
    ``encode`` = L2-normalise -> dropout (training) -> tanh(Linear) ... -> Linear -> (mu, logvar);
    ``_reparameterize`` samples in training, returns mu in eval; ``decode`` = tanh(Linear) ... -> Linear.
    """
    _variant = "vae"

    def __init__(self, dec_dims, enc_dims=None, dropout=0.5):
        super(MultiVAE_net, self).__init__(dec_dims, enc_dims)
        self.dropout = nn.Dropout(dropout)

    def encode(self, x, _mask=None):
        if self._diff_active():
            return self._differentiable_encode(x, mask=_mask)
        x = self._as_input(x)
        eng = self.rtx_engine("fp32", x.shape[0])
        return eng.encode(x, training=self.training, seed=draw_seed() if self.training else 0)

    def _reparameterize(self, mu, logvar, _noise=None):
        if self.training:
            if not self.differentiable:
                raise NotImplementedError("sampling outside forward() is not exposed; call net(x) in training mode")
            # one seed per call; the fused head's draws and arithmetic on a [B, latent] tensor (rtx_reparam), differentiable
            from .engine import reparameterize
            noise = _noise if _noise is not None else self._injected("noise")
            return reparameterize(mu, logvar, seed=draw_seed(), noise=noise)
        return mu

    def decode(self, z):
        if self._diff_active():
            return self._differentiable_decode(z)
        eng = self.rtx_engine("fp32", z.shape[0])
        return eng.decode(z.to(self._device()))

    def forward(self, x):
        if self._diff_active():
            return self._differentiable_forward(x)
        x = self._as_input(x)
        eng = self.rtx_engine("fp32", x.shape[0])
        return eng.forward(x, training=self.training, seed=draw_seed() if self.training else 0)


class CMultiVAE_net(MultiVAE_net):
    r"""Conditioned Variational Autoencoder network for collaborative filtering (reference nets.py:420-480).

    The input rows are ``[items | condition one-hot]``: the item part is L2-normalised and dropped out, the
    ``cond_dim`` condition columns are concatenated raw, so the first encoder layer is
    ``Linear(n_items + cond_dim, ...)``.  On the device this is the same engine with ``rtx_cfg.cond_dim`` set: the
    gather kernel leaves the trailing columns unscaled and the first GEMM simply has a longer K.
    """

    def __init__(self, cond_dim, dec_dims, enc_dims=None, dropout=0.5):
        super(CMultiVAE_net, self).__init__(dec_dims, enc_dims, dropout)
        self.cond_dim = cond_dim

        temp_dims = self.enc_dims[:-1] + [self.enc_dims[-1] * 2]
        temp_dims[0] += self.cond_dim
        self.enc_layers = nn.ModuleList(
            [nn.Linear(d_in, d_out) for d_in, d_out in zip(temp_dims[:-1], temp_dims[1:])])

        self.dec_layers = nn.ModuleList(
            [nn.Linear(d_in, d_out) for d_in, d_out in zip(self.dec_dims[:-1], self.dec_dims[1:])])
        self.init_weights()


class SVAE_net(VAE_net):
    """Sequential Variational Autoencoder network (reference nets.py:624-693): item embedding -> one-layer GRU
    (batch_first) -> the VAE head of :class:`VAE_net` (tanh hidden layers, linear ``mu | logvar``; **always** sampled,
    in eval too, because ``_reparameterize`` is the base class's) -> tanh MLP decoder with a linear output.

    The ``nn.Embedding`` / ``nn.GRU`` / ``nn.Linear`` modules hold the parameters (same ``state_dict`` keys as the
    reference: ``enc_layers.*``, ``dec_layers.*``, ``item_embed.weight``, ``gru.weight_ih_l0`` ...); the computation is
    the ``rtx_svae`` engine of librectorch_hip.

    Parameters
    ----------
    n_items : :obj:`int`
        Number of items.
    embed_size : :obj:`int`
        Size of the embedding for the items.
    rnn_size : :obj:`int`
        Size of the recurrent layer of the GRU part of the network.
    dec_dims, enc_dims : :obj:`list` of :obj:`int`
        See :class:`AE_net` (``enc_dims[0]`` must be ``rnn_size``).
    """
    _variant = "vae"

    def __init__(self, n_items, embed_size, rnn_size, dec_dims, enc_dims):
        super(SVAE_net, self).__init__(dec_dims, enc_dims)
        self.enc_dims = enc_dims
        self.dec_dims = dec_dims
        self.n_items = n_items
        self.embed_size = embed_size
        self.rnn_size = rnn_size
        self.item_embed = nn.Embedding(n_items, embed_size)
        self.gru = nn.GRU(embed_size, rnn_size, batch_first=True, num_layers=1)
        self.init_weights()
        self._svae_engine = None

    def init_weights(self):
        r"""xavier_normal weights for the encoder / decoder layers, biases left at their defaults (reference
        nets.py:689-693)."""
        for layer in self.enc_layers:
            nn.init.xavier_normal_(layer.weight)
        for layer in self.dec_layers:
            nn.init.xavier_normal_(layer.weight)

    def _param_list(self):
        # the order of SVAE_net.parameters(): the MLPs are registered by VAE_net.__init__, then embedding and GRU
        ps = []
        for layer in list(self.enc_layers) + list(self.dec_layers):
            ps += [layer.weight, layer.bias]
        return ps + [self.item_embed.weight, self.gru.weight_ih_l0, self.gru.weight_hh_l0, self.gru.bias_ih_l0,
                     self.gru.bias_hh_l0]

    def svae_engine(self, seq_len=1, train_buffers=None):
        """The ``rtx_svae`` engine of this network, grown when a longer sequence arrives and re-bound when the parameter
        (or training-buffer) storage changes.  There are no compute copies: the kernels read the parameters in place."""
        from .engine import SvaeEngine
        self._device()
        eng = self._svae_engine
        if eng is None or eng.max_len < seq_len:
            eng = SvaeEngine(self.n_items, self.embed_size, self.rnn_size, self.enc_dims, self.dec_dims,
                             max_len=max(256, 2 * int(seq_len)))
            if getattr(self, "svae_numerics", "fp32") == "bf16":     # set by SVAE(..., numerics="bf16")
                eng.set_option("gemm_bf16", 1)
            self._svae_engine = eng
        params = [p.data for p in self._param_list()]
        pkey = tuple(t.data_ptr() for t in params)
        tkey = None if train_buffers is None else tuple(t.data_ptr() for ts in train_buffers for t in ts)
        if getattr(eng, "param_key", None) != pkey or (tkey is not None and getattr(eng, "train_key", None) != tkey):
            if train_buffers is not None:
                eng.bind(params, *train_buffers)
            else:
                eng.bind(params)
            eng.param_key, eng.train_key = pkey, tkey
        return eng

    def _rtx_mark_updated(self, numerics):
        pass

    def _differentiable_forward(self, x, noise=None, moments=None):
        """``net(x)`` as an autograd Function over the ``rtx_svae`` engine (``rtx_svae_forward_train`` / ``rtx_svae_backward``) at the
        network's own arithmetic (``svae_numerics``): ``(logits [T, n_items], mu, logvar)`` of all rows.  ``x``: a ``[1, T]`` sequence
        or a :class:`rectorch_amd.engine.SvaePack` / ``SvaeEvalPack``; ``noise``: injected draws ``[T, latent]`` (parity tests);
        ``moments``: a trainer's ``(exp_avg, exp_avg_sq)`` lists."""
        T = x.n_steps if hasattr(x, "seq_ptr") else int(x.numel())
        grads = self._diff_buffers()[0]
        m, v = moments if moments is not None else self._diff_moments()
        eng = self.svae_engine(T, train_buffers=(grads, m, v))
        if noise is not None:
            noise = noise.to(grads[0].device, torch.float32).contiguous()
            if noise.numel() < T * eng.latent:
                raise _lib.RtxError("the injected noise must hold [%d, %d] draws, got %s" % (T, eng.latent, tuple(noise.shape)))
        step = _lib.Step()
        step.seed, step.offset = draw_seed() & (2 ** 64 - 1), 0
        step.eps_noise = None if noise is None else noise.data_ptr()
        return _SvaeTrainForward.apply(self, eng, x, step, noise, grads, *self._param_list())

    def forward(self, x):
        """``x``: LongTensor [1, T].  Returns ``(dec_out [1, T, n_items], mu [T, latent], logvar [T, latent])``.  With
        ``differentiable`` set, in training mode with grad mode on, the three carry a ``grad_fn`` (see :class:`AE_net`)."""
        if self._diff_active():
            self._diff_numerics()       # (validates the switch; the arithmetic is the engine's own, ``svae_numerics``)
            la, mu, logvar = self._differentiable_forward(x)
            return la.view(x.shape[0], x.shape[1], -1), mu, logvar
        la, _, mu, logvar = self.svae_engine(x.numel()).forward(x, seed=draw_seed())
        return la.view(x.shape[0], x.shape[1], -1), mu, logvar
