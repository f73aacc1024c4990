r"""Trainer classes of the Mult-VAE / Mult-DAE path with the reference's API (rectorch/models.py), running
on the MI355X engine.

Same class hierarchy and signatures as the reference: ``RecSysModel`` (models.py:70-161) ->
``TorchNNTrainer`` (:164-322) -> ``AETrainer`` (:325-516) -> ``VAE`` (:519-625) -> ``MultiVAE`` (:709-908), and
``MultiDAE`` (:628-706).  What changes is underneath: ``train_batch`` is ONE call into librectorch_hip
(gather -> forward -> multinomial/KL loss -> backward -> fused Adam, all hand-written HIP), ``predict`` is the
HIP forward, and ``train_epoch`` feeds row numbers of a device-resident CSR instead of dense host batches and
reads the loss back only at the logging boundaries.  ``model.optimizer`` is still a ``torch.optim`` object (Adam by default;
Adam / AdamW with decoupled decay, SGD, Adagrad and RMSprop train too: :func:`optimizer_spec`) whose ``state`` tensors ARE the
buffers the fused optimizer kernel updates, so checkpoints round-trip with the reference's layout (``epoch``, ``state_dict``,
``optimizer``, ``gradient_updates``).
"""
import logging
import os
import time

from collections import namedtuple

import numpy as np
import torch
import torch.optim as optim

from . import _lib
from .engine import AdmmSolver, CsrMatrix, EaseSolver, KnnSolver, WmfSolver, RowBatch, SvaeEvalPack, SvaePack, SvaeTarget, batch_users, bce_kl_loss, mse_loss, multinomial_loss, tagged_rows
from .evaluation import ValidFunc, evaluate
from .samplers import DataSampler, is_resident_conditioned

__all__ = ['RecSysModel', 'TorchNNTrainer', 'AETrainer', 'VAE', 'MultiVAE', 'MultiDAE', 'CMultiVAE', 'EASE', 'ADMM_Slim', 'ItemKNN', 'WMF', 'SVAE']

logger = logging.getLogger(__name__)

# What the device step needs to know of ``model.optimizer``: the rule (``kind`` / ``flags`` / the four scalars of ``rtx_optim``;
# lr, eps, weight_decay and betas are read from the param group at every step), and the state keys of the kernel's two state
# slots (``None``: the rule keeps no tensor there) with whether torch keeps a ``step`` tensor for it.
OptimSpec = namedtuple("OptimSpec", "kind flags momentum dampening alpha lr_decay m_key v_key keeps_step")

_SUPPORTED_OPTIMIZERS = ("torch.optim.Adam (coupled or decoupled weight decay), AdamW, SGD (momentum, dampening, nesterov, "
                         "weight_decay), Adagrad (lr_decay, eps, weight_decay, initial_accumulator_value) and RMSprop (alpha, eps, "
                         "momentum, weight_decay); one param group holding exactly the network's parameters; no amsgrad, maximize, "
                         "centered, capturable or differentiable")


def optimizer_spec(optimizer, params=None):
    """The :class:`OptimSpec` of a torch optimizer, or ``TypeError`` (a class the device step has no rule for: anything but
    exactly ``Adam``, ``AdamW``, ``SGD``, ``Adagrad``, ``RMSprop`` -- a subclass may override ``step``) / ``ValueError`` (an option
    it does not implement).  Nothing is approximated: what is not supported raises, before any launch.  ``params``: the network's
    parameter list, which the optimizer's one param group must hold exactly."""
    kinds = {optim.Adam: _lib.RTX_OPTIM_ADAM, optim.AdamW: _lib.RTX_OPTIM_ADAM, optim.SGD: _lib.RTX_OPTIM_SGD,
             optim.Adagrad: _lib.RTX_OPTIM_ADAGRAD, optim.RMSprop: _lib.RTX_OPTIM_RMSPROP}
    if type(optimizer) not in kinds:
        raise TypeError("model.optimizer is a %s.%s: the device step has no update rule for it (a subclass may change step()); supported: %s"
                        % (type(optimizer).__module__, type(optimizer).__name__, _SUPPORTED_OPTIMIZERS))
    if len(optimizer.param_groups) != 1:
        raise ValueError("model.optimizer has %d param groups; supported: %s" % (len(optimizer.param_groups), _SUPPORTED_OPTIMIZERS))
    g = optimizer.param_groups[0]
    if params is not None:
        held = g['params']
        if len(held) != len(params) or set(map(id, held)) != set(map(id, params)):
            raise ValueError("model.optimizer's param group holds %d tensors that are not exactly the network's %d parameters; "
                             "supported: %s" % (len(held), len(params), _SUPPORTED_OPTIMIZERS))
    for opt in ("amsgrad", "maximize", "centered", "capturable", "differentiable"):
        if g.get(opt, False):
            raise ValueError("model.optimizer has %s=True, which the device step does not implement; supported: %s" % (opt, _SUPPORTED_OPTIMIZERS))
    kind = kinds[type(optimizer)]
    if kind == _lib.RTX_OPTIM_ADAM:
        flags = _lib.RTX_OPTIM_DECOUPLED if g.get('decoupled_weight_decay', False) else 0
        return OptimSpec(kind, flags, 0.0, 0.0, 0.0, 0.0, 'exp_avg', 'exp_avg_sq', True)
    if kind == _lib.RTX_OPTIM_SGD:
        mom = float(g['momentum'])
        flags = _lib.RTX_OPTIM_NESTEROV if g['nesterov'] else 0
        return OptimSpec(kind, flags, mom, float(g['dampening']), 0.0, 0.0, 'momentum_buffer' if mom != 0 else None, None, False)
    if kind == _lib.RTX_OPTIM_ADAGRAD:
        return OptimSpec(kind, 0, 0.0, 0.0, 0.0, float(g['lr_decay']), None, 'sum', True)
    mom = float(g['momentum'])
    return OptimSpec(kind, 0, mom, 0.0, float(g['alpha']), 0.0, 'momentum_buffer' if mom != 0 else None, 'square_avg', True)


_SUPPORTED_CLIPPING = ("model.clip_grad_norm = None or a number >= 0 (float('inf') reports the norm and clips nothing) with "
                       "model.clip_grad_norm_type 2.0 or float('inf'), as torch.nn.utils.clip_grad_norm_ with error_if_nonfinite=False; "
                       "or model.clip_grad_value = None or a number >= 0, as clip_grad_value_; one of the two at a time; single GPU")


def grad_clip_spec(model):
    """``(mode, bound)`` of ``rtx_engine_set_grad_clip`` for the model's clip attributes (``clip_grad_norm``,
    ``clip_grad_norm_type``, ``clip_grad_value``; read at every step, as ``lr`` is), or ``ValueError`` for what the device does not
    implement.  Nothing is approximated: what is not supported raises, before any launch."""
    norm, value = getattr(model, "clip_grad_norm", None), getattr(model, "clip_grad_value", None)
    if norm is not None and value is not None:
        raise ValueError("model.clip_grad_norm and model.clip_grad_value are both set; supported: %s" % _SUPPORTED_CLIPPING)
    if getattr(model, "clip_grad_error_if_nonfinite", False):
        raise ValueError("error_if_nonfinite=True is not implemented (the norm stays on the device); supported: %s" % _SUPPORTED_CLIPPING)
    for name, bound in (("clip_grad_norm", norm), ("clip_grad_value", value)):
        if bound is not None and not float(bound) >= 0.0:
            raise ValueError("model.%s = %r is not a number >= 0; supported: %s" % (name, bound, _SUPPORTED_CLIPPING))
    if norm is not None:
        norm_type = float(getattr(model, "clip_grad_norm_type", 2.0))
        if norm_type == 2.0:
            return _lib.RTX_CLIP_NORM2, float(norm)
        if norm_type == float("inf"):
            return _lib.RTX_CLIP_NORMINF, float(norm)
        raise ValueError("model.clip_grad_norm_type = %r is not implemented; supported: %s" % (norm_type, _SUPPORTED_CLIPPING))
    if value is not None:
        return _lib.RTX_CLIP_VALUE, float(value)
    return _lib.RTX_CLIP_NONE, 0.0


_SUPPORTED_ACCUM = ("supported: model.accumulate_grad_batches = an int >= 1 on AETrainer, VAE, MultiDAE, MultiVAE and CMultiVAE with their "
                    "built-in losses or custom_loss = True, float32 or bf16 numerics, any supported optimizer and clipping, single GPU; "
                    "SVAE batches by packs and data-parallel plans by ranks instead")


_ACCUM_REBUILT = ("a micro-batch of %d rows arrived in the middle of an accumulation window and needs a larger engine than the one "
                  "that holds the window; put the largest micro-batch first, or call model.apply_accumulated() before it")


def accum_spec(k):
    """``model.accumulate_grad_batches`` as the int it must be (``ValueError`` otherwise): micro-batches per optimizer update"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError("model.accumulate_grad_batches = %r; %s" % (k, _SUPPORTED_ACCUM))
    return int(k)


def _step_scalars_of(spec, g):
    """(lr, beta1, beta2, eps, weight_decay) of a param group for ``rtx_step`` (read at every step: lr schedulers work)"""
    b1, b2 = g['betas'] if spec.kind == _lib.RTX_OPTIM_ADAM else (0.0, 0.0)
    return dict(lr=float(g['lr']), beta1=float(b1), beta2=float(b2), eps=float(g.get('eps', 0.0)), weight_decay=float(g['weight_decay']))


class RecSysModel():
    r"""Abstract base class that any Recommendation model must inherit from (reference models.py:70-161)."""
    def train(self, train_data, **kwargs):
        raise NotImplementedError()

    def predict(self, x, *args, **kwargs):
        raise NotImplementedError()

    def save_model(self, filepath, *args, **kwargs):
        raise NotImplementedError()

    def load_model(self, filepath, *args, **kwargs):
        raise NotImplementedError()


class _RtxState:
    """Private per-trainer state of the HIP path (kept in one object with a short repr because the
    reference's ``__str__`` prints every attribute of the model)."""
    def __init__(self):
        self.flat_grads = None
        self.grads = None
        self.layer_ranges = None
        self.tensor_offsets = None
        self.adam_step = 0
        self.spec = None          # OptimSpec of model.optimizer as of the last _ensure_optim_state
        self.optim = None         # the optimizer object adam_step counts the updates of (a new model.optimizer starts at its own count)
        self.sgd_first = False    # SGD with momentum: the buffers were created here and no update has filled them yet
        self.loss_buf = None      # [0] = last loss, [1] = running sum since the last read-back
        self.pending_seed = None  # the dropout seed drawn one step early for a batch announced to the engine
        self.reducer = None       # data parallel: rectorch_amd.parallel.GradAllReducer
        self.masters_sharded = False   # sharded optimizer: the float32 master rows of other ranks are stale until gathered
        self.norm_engine = None   # the engine whose last optimizer step computed a gradient norm (model.last_grad_norm), else None
        self.inject = None        # parity tests: (dropout keep-mask, eps) captured from the reference's RNG
        self.accum_pending = 0    # gradient accumulation: micro-steps in the open window
        self.accum_k = 1          # ... its accumulate_grad_batches, read at its first micro-step
        self.accum_engine = None  # ... the engine whose bound gradient buffers hold it
        self.accum_scalars = None # ... (beta, lam) of the window
        self.accum_custom = False # ... opened on the custom-loss route

    def __repr__(self):
        return "<MI355X engine state>"


class TorchNNTrainer(RecSysModel):
    r"""Abstract class representing a neural network-based model (reference models.py:164-322).

    Parameters
    ----------
    net : :class:`torch.nn.Module`
        The neural network architecture (a :mod:`rectorch_amd.nets` network).
    learning_rate : :obj:`float` [optional]
        The learning rate for the optimizer, by default 1e-3.

    Attributes
    ----------
    network, learning_rate, optimizer, device : as in the reference.  ``device`` is the HIP device: a
        network still on the host is moved to the MI355X at construction (this package has no CPU compute
        path); without any HIP device the object can be built, saved and loaded but not run.
    """
    def __init__(self, net, learning_rate=1e-3):
        self.network = net
        self.learning_rate = learning_rate
        self.optimizer = None #to be initialized in the sub-classes

        if not next(self.network.parameters()).is_cuda and torch.cuda.is_available():
            logger.info("moving the network to the MI355X (rectorch_amd computes only on the HIP device)")
            self.network.to(torch.device("cuda"))
        if next(self.network.parameters()).is_cuda:
            self.device = torch.device("cuda")
        else:
            self.device = torch.device("cpu")

    def loss_function(self, prediction, ground_truth, *args, **kwargs):
        raise NotImplementedError()

    def train(self, train_data, *args, **kwargs):
        raise NotImplementedError()

    def train_epoch(self, epoch, train_data, *args, **kwargs):
        raise NotImplementedError()

    def train_batch(self, epoch, tr_batch, te_batch, *args, **kwargs):
        raise NotImplementedError()

    def predict(self, x, *args, **kwargs):
        raise NotImplementedError()

    def __str__(self):
        # "ClassName(\n  attr = value,\n  ...\n)" with multi-line values indented under their attribute -- the layout of
        # the reference's repr (models.py:313-322), which its users read in logs
        fields = []
        for name, value in vars(self).items():
            first, *rest = str(value).split("\n")
            fields.append("  %s = %s" % (name, "\n".join([first] + ["  " + ln for ln in rest])))
        return "%s(\n%s\n)" % (type(self).__name__, ",\n".join(fields))

    __repr__ = __str__


def _with_next(it):
    """(item, next item or None) over an iterator: one batch of look-ahead for the engine's prefetch"""
    it = iter(it)
    try:
        cur = next(it)
    except StopIteration:
        return
    for nxt in it:
        yield cur, nxt
        cur = nxt
    yield cur, None


class _EpochLog:
    """The reference's progress lines for one epoch (models.py:401-422): every ``max(10, n_batches // 10**verbose)``
    batches ``| epoch e | i/n batches | ms/batch t | loss l |`` with the mean loss of that stretch, at the end
    ``| epoch e | loss L | total time: Ts |`` with the mean over all batches.  One implementation for every trainer."""
    def __init__(self, epoch, n_batches, verbose):
        self.epoch, self.n_batches = epoch, n_batches
        self.every = max(10, n_batches // 10 ** verbose)
        self.t_epoch = self.t_stretch = time.time()
        self.total = 0.0
        self.seen = 0           # batches actually consumed (a sampler's __len__ may be approximate: SVAE packs under shuffle)

    def due(self, n_done):
        return n_done % self.every == 0

    def stretch(self, n_done, loss_sum):
        """close a stretch of ``every`` batches whose losses sum to ``loss_sum``"""
        now = time.time()
        logger.info('| epoch %d | %d/%d batches | ms/batch %.2f | loss %.2f |', self.epoch, n_done, self.n_batches,
                    (now - self.t_stretch) * 1000 / self.every, loss_sum / self.every)
        self.total += loss_sum
        self.seen = n_done
        self.t_stretch = time.time()

    def finish(self, tail_loss_sum, n_done=None):
        n = n_done if n_done is not None else self.n_batches
        logger.info("| epoch %d | loss %.4f | total time: %.2fs |", self.epoch,
                    (self.total + tail_loss_sum) / max(n, 1), time.time() - self.t_epoch)


def _validate(model, epoch, valid_data, valid_metric, valid_func):
    """one validation pass + the reference's log line; returns the mean of the metric (models.py:389-398, 881-889)"""
    assert valid_metric is not None, \
        "In case of validation 'valid_metric' must be provided"
    per_user = valid_func(model, valid_data, valid_metric)
    mean = np.mean(per_user)
    logger.info('| epoch %d | %s %.3f (%.4f) |', epoch, valid_metric, mean, np.std(per_user) / np.sqrt(len(per_user)))
    return mean


class AETrainer(TorchNNTrainer):
    r"""Base class for Autoencoder-based models (reference models.py:325-516).  Holds the Adam optimizer, the
    epoch loop, prediction and checkpointing shared by :class:`MultiDAE` and :class:`MultiVAE`.

    The class is concrete, as in the reference: ``AETrainer(MultiDAE_net(...))`` is the plain (denoising) autoencoder trained
    with ``torch.nn.MSELoss`` against the raw input rows.  On the device that is the engine variant ``RTX_AE``: the forward of
    :class:`rectorch_amd.nets.MultiDAE_net` and a fused MSE loss + gradient kernel.  A subclass that keeps this class's
    ``loss_function`` trains the same way; data parallelism is not available for it.

    Extra keyword arguments (not in the reference): ``numerics`` = arithmetic of the training step
    ("bf16": bf16 MFMA operands, f32 accumulation, f32 master weights and Adam; "fp32": exact-f32 MFMA) and
    ``predict_numerics`` (default "fp32", the parity mode: logits within 1e-5 of the reference's CPU path).
    """
    _variant = "dae"
    _uses_te = False     # train_batch ignores te_batch (reference models.py:444-445)

    def __init__(self, ae_net, learning_rate=1e-3, numerics="bf16", predict_numerics="fp32"):
        super(AETrainer, self).__init__(ae_net, learning_rate)
        from .nets import CDAE_net
        self._is_cdae = isinstance(ae_net, CDAE_net)    # the network has a user table (its own optimizer, ids with every batch)
        self.optimizer = optim.Adam(self._net_parameters(), lr=learning_rate)
        # CDAE_net only: the optimizer of the user table, created on demand (the property ``user_optimizer``)
        self._user_optimizer = None
        self.numerics = numerics
        self.predict_numerics = predict_numerics
        # the single-GPU bf16 step runs Adam inside the weight-gradient kernels (dw_adam.hip), so the gradients never
        # reach HBM and p.grad is NOT refreshed; set True to also store them (4 B/param).  float32 numerics and the
        # data-parallel step always store them.
        self.keep_grads = False
        # train_batch returns THIS step's loss as a float (reference models.py:835).  True: the float comes from the engine's host
        # mailbox (rtx_engine_wait_loss: the host spins on a step count in coherent host memory while the step's remaining
        # kernels keep running); False: ``loss.item()``, which drains the stream like the reference does.
        self.loss_mailbox = True
        # train_epoch / callers of _fused_step(next_x=...) announce the next batch to the engine, which gathers it on its side
        # stream under the current step's last weight kernel (rtx_engine_set_next_batch); False: every step gathers for itself
        self.prefetch_batches = True
        # True: train_batch / train_epoch do what the reference's train_batch does with a subclass's OWN loss_function -- the
        # engine's training forward with a grad_fn (nets.py: the differentiable route, at self.numerics), self.loss_function(...)
        # in torch, loss.backward() through the engine's backward chain, Adam (rtx_engine_apply_adam) on p.grad.  False: the fused
        # step with the built-in loss that _loss_kind names, whatever loss_function says.  Single GPU only.
        self.custom_loss = False
        # Gradient clipping between the backward pass and the optimizer, on the device (torch.nn.utils.clip_grad_norm_ /
        # clip_grad_value_ in front of optimizer.step(); read at every step, so they can be scheduled): clip_grad_norm = max_norm of
        # the global norm of type clip_grad_norm_type (2.0 or float('inf')), or clip_grad_value = the element-wise bound.  What is
        # clipped is the gradient of loss_function, Mult-DAE's regulariser term included and weight decay not.  One stated difference
        # to torch: p.grad keeps the UNCLIPPED gradient the step stored (without the regulariser term, as with keep_grads); torch
        # would have scaled it in place.  With either set the bf16 step stores its gradients too (p.grad is refreshed every step):
        # a global norm needs every gradient before any parameter moves, so the step takes the unfused schedule.
        self.clip_grad_norm = None
        self.clip_grad_norm_type = 2.0
        self.clip_grad_value = None
        # Gradient accumulation on the device: with k = accumulate_grad_batches > 1 every train_batch call is a micro-step --
        # forward, loss, backward, the gradient added into p.grad with weight 1 / k (the weight-gradient kernels' accumulating
        # epilogue) -- and every k-th call also clips (if set) and runs model.optimizer's rule: torch's
        # ``(loss / k).backward()`` k times, ``clip_grad_*``, ``optimizer.step()``.  train_batch returns the micro-batch's own,
        # unscaled loss.  Once per window: the optimizer's step count, MultiVAE.gradient_updates (one beta per window), weight decay,
        # Mult-DAE's regulariser gradient.  Read at the first micro-step of a window; changing it inside one raises.
        # ``apply_accumulated()`` applies a partial window, ``pending_micro_batches`` counts the open one.  Single GPU.  With custom_loss = True the user's loss is not divided: the package applies 1 / k.
        self.accumulate_grad_batches = 1
        self._rtx = _RtxState()

    # ------------------------------------------------------------------------------ CDAE's user table
    def _net_parameters(self):
        """the parameters ``model.optimizer`` updates and the regulariser sees: all of them, but for a CDAE_net's user table"""
        dense = getattr(self.network, "_dense_parameters", None)
        return self.network.parameters() if dense is None else dense()

    @property
    def user_optimizer(self):
        """CDAE_net only: the optimizer of ``net.user_factors`` -- a ``torch.optim.SparseAdam`` over
        ``net.user_factors.parameters()``, created on first use with the model's learning rate; assign another SparseAdam to
        replace it.  The device step applies its rule (``torch.optim._functional.sparse_adam``) to the rows of each batch inside
        the backward kernel; its state lives in ``user_optimizer.state[p]`` under torch's keys (``step``, ``exp_avg``,
        ``exp_avg_sq``), created as its own first ``step()`` would; ``lr``, ``betas`` and ``eps`` are read at every step, so
        schedulers work.  ``net.user_factors.weight.grad`` stays ``None``: the gradient is consumed where it is produced and
        never stored (as clipping leaves the unclipped gradient in ``p.grad``, a stated difference to torch)."""
        if not self._is_cdae:
            raise AttributeError("user_optimizer belongs to a CDAE_net; the network is a %s" % type(self.network).__name__)
        if self._user_optimizer is None:
            self._user_optimizer = optim.SparseAdam(self.network.user_factors.parameters(), lr=self.learning_rate)
        return self._user_optimizer

    @user_optimizer.setter
    def user_optimizer(self, value):
        self._user_optimizer = value

    _CDAE_SUPPORTED = ("supported for a CDAE_net: MultiDAE / AETrainer with their built-in loss, float32 or bf16 numerics, any "
                       "supported model.optimizer for W and b, model.user_optimizer = a torch.optim.SparseAdam (maximize=False) "
                       "over net.user_factors.parameters(), one batch per update, no clipping, single GPU")

    def _cdae_refusals(self):
        """what a CDAE_net does not train with, before anything is launched"""
        if self.custom_loss or self.network.differentiable:
            raise NotImplementedError("custom_loss = True / net.differentiable: the user table's gradient never leaves the backward "
                                      "kernel, so there is no autograd route; " + self._CDAE_SUPPORTED)
        if accum_spec(self.accumulate_grad_batches) > 1:
            raise NotImplementedError("accumulate_grad_batches = %d: the user rows are updated inside every backward pass; %s"
                                      % (self.accumulate_grad_batches, self._CDAE_SUPPORTED))
        if grad_clip_spec(self)[0] != _lib.RTX_CLIP_NONE:
            raise NotImplementedError("clip_grad_norm / clip_grad_value: the user table's gradient is never stored and cannot enter a "
                                      "norm; " + self._CDAE_SUPPORTED)
        if self._rtx.reducer is not None:
            raise NotImplementedError("a data-parallel plan is attached: the user rows are updated in place, there is no gradient "
                                      "to exchange; " + self._CDAE_SUPPORTED)

    def _user_optim_state(self):
        """``(group, state)`` of ``model.user_optimizer`` for the device step: checked, and with what SparseAdam's own first
        ``step()`` creates (``step = 0`` and two zero tensors); the network learns where the moments are"""
        net, opt = self.network, self.user_optimizer
        p = net.user_factors.weight
        if type(opt) is not optim.SparseAdam:
            raise TypeError("model.user_optimizer is a %s.%s: the device step has SparseAdam's rule only; %s"
                            % (type(opt).__module__, type(opt).__name__, self._CDAE_SUPPORTED))
        if len(opt.param_groups) != 1 or len(opt.param_groups[0]['params']) != 1 or opt.param_groups[0]['params'][0] is not p:
            raise ValueError("model.user_optimizer must hold one param group with exactly net.user_factors.weight; " + self._CDAE_SUPPORTED)
        g = opt.param_groups[0]
        if g.get('maximize', False):
            raise ValueError("model.user_optimizer has maximize=True, which the device step does not implement; " + self._CDAE_SUPPORTED)
        state = opt.state[p]
        if len(state) == 0:
            state['step'] = 0
            state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        for k in ('exp_avg', 'exp_avg_sq'):
            t = state[k]
            if t.device != p.device or t.dtype != p.dtype or not t.is_contiguous():
                state[k] = t.to(device=p.device, dtype=p.dtype).contiguous()
        net._rtx_user_moments = (state['exp_avg'], state['exp_avg_sq'])
        return g, state

    # ------------------------------------------------------------------------------------------ loss
    @property
    def _loss_kind(self):
        """the training loss of the fused step: "mse" for this class and for every subclass that keeps its ``loss_function``
        (the engine variant ``RTX_AE``), else the loss of the network's own engine variant.  Apart from ``_variant``, which names
        the layer layout and forward; part of the key of the network's engine cache."""
        if type(self).loss_function is AETrainer.loss_function:
            return "mse"
        return "bce" if self._variant == "gvae" else "multinomial"

    def loss_function(self, prediction, ground_truth):
        r"""Mean squared error ``torch.nn.MSELoss()(ground_truth, prediction)`` (reference models.py:347-377) on the HIP
        device; returns a 0-dim tensor."""
        return mse_loss(prediction, ground_truth)

    # ------------------------------------------------------------------------------------- training
    def train(self,
              train_data,
              valid_data=None,
              valid_metric=None,
              valid_func=ValidFunc(evaluate),
              num_epochs=100,
              verbose=1):
        r"""Training of a neural network-based model (reference models.py:379-398): ``num_epochs`` epochs, each followed
        by a validation pass when ``valid_data`` is given; Ctrl-C ends training early with a warning."""
        try:
            for epoch in range(1, num_epochs + 1):
                self.train_epoch(epoch, train_data, verbose)
                if valid_data is not None:
                    self.consolidate()          # (data parallel, sharded optimizer: every rank runs train() and gets here)
                    _validate(self, epoch, valid_data, valid_metric, valid_func)
        except KeyboardInterrupt:
            logger.warning('Handled KeyboardInterrupt: exiting from training early')

    def train_epoch(self, epoch, train_loader, verbose=1):
        r"""Training of a single epoch (reference models.py:401-422): same progress lines.  With a device-resident
        :class:`DataSampler` the batches are row numbers, steps are enqueued back to back and the loss is read from the
        device only where a progress line needs it (the engine keeps a running sum)."""
        self.network.train()
        if self._is_cdae and getattr(train_loader, "max_user_id", -1) >= self.network.n_users:
            raise ValueError("the loader's user ids reach %d, the CDAE_net has %d user vectors (ids 0 .. %d; -1 marks a user without one)"
                             % (train_loader.max_user_id, self.network.n_users, self.network.n_users - 1))
        log = _EpochLog(epoch, len(train_loader), verbose)
        resident = isinstance(train_loader, DataSampler) and train_loader.resident
        if is_resident_conditioned(train_loader):
            # batches built on the device into a ring of CSR pairs (samplers.py): the same back-to-back steps; batch j + 1 is built,
            # on this stream, before step j is enqueued -- the ring is sized for exactly that look-ahead (csrc/cond_rows.hip)
            if self._rtx.reducer is not None:
                raise _lib.RtxError("a resident conditioned sampler cannot be trained under a data-parallel plan: its batches live in "
                                    "a ring of device buffers that the plan's row slices do not know; use resident=False")
            resident = True
        pending = 0.0                       # host path: losses of the current stretch
        done = 0
        def shaped(item):
            return item if self._uses_te or item.te is None else RowBatch(item.tr, None, item.rows, users=item.users)
        for done, (item, nxt) in enumerate(_with_next(train_loader.iter_rows()) if resident else ((i, None) for i in train_loader), 1):
            if resident:
                # (the batch after this one is announced to the engine: it is gathered under this step's last weight kernel)
                # (no wait for the engine's side stream between two steps: the next step resolves the join in its first kernel)
                self._fused_step(shaped(item), None, want_loss=False, next_x=None if nxt is None else shaped(nxt), defer_join=True)
            else:
                data, gt = item
                pending += self.train_batch(data, gt)
            if log.due(done):
                log.stretch(done, self._read_loss_sum() if resident else pending)
                pending = 0.0
        self.apply_accumulated()            # (accumulate_grad_batches > 1: a partial last window is applied; no gradient crosses an epoch)
        log.finish(self._read_loss_sum() if resident else pending, done)

    def train_batch(self, tr_batch, te_batch=None, users=None):
        r"""Training of a single batch (reference models.py:424-447): the loss target is the batch itself
        (``te_batch`` is ignored, as in the reference).  Returns the loss as a Python float.  ``users`` (CDAE_net only): the
        batch's user ids, one per row, when the batch does not carry them (a ``DataSampler(user_ids=...)`` batch does)."""
        return self._fused_step(tr_batch, None, want_loss=True, users=users)

    # ---------------------------------------------------------------------------- the fused HIP step
    def _step_scalars(self):
        """(beta, lam) of this update; sub-classes fill them."""
        return 0.0, 0.0

    def _after_step(self):
        pass

    def _ensure_train_state(self):
        st = self._rtx
        params = self.network._param_list()
        if st.grads is None or st.flat_grads.device != params[0].device:
            optimizer_spec(self.optimizer, params)      # (an optimizer the step has no rule for raises before anything is allocated)
            # one flat gradient buffer (one RCCL all-reduce region per layer); p.grad are views into it
            # a weight matrix's region holds its rows padded to a multiple of 128 (zeros), so that a data-parallel
            # reduce-scatter can cut it into equal, row-aligned blocks for any power-of-two number of ranks
            offs, total = [], 0
            for p in params:
                offs.append(total)
                n = p.numel() if p.dim() == 1 else ((p.shape[0] + 1 + 127) // 128 * 128) * p.shape[1]
                total += (n + 63) // 64 * 64
            st.flat_grads = torch.zeros(total, dtype=torch.float32, device=params[0].device)
            st.grads = [st.flat_grads[o:o + p.numel()].view(p.shape) for o, p in zip(offs, params)]
            st.layer_ranges = [(offs[2 * l], offs[2 * l + 1] + params[2 * l + 1].numel()) for l in range(len(params) // 2)]
            st.tensor_offsets = offs
            for p, g in zip(params, st.grads):
                p.grad = g
            st.loss_buf = torch.zeros(2, dtype=torch.float32, device=params[0].device)
        m, v = self._ensure_optim_state(params)[1:]
        return st, params, m, v

    def _ensure_optim_state(self, params):
        """``model.optimizer`` for the device step: ``(spec, m, v)`` -- its :class:`OptimSpec` (raises for what the step does not
        implement) and the tensors of the kernel's two state slots, one per parameter, after creating in ``optimizer.state``
        exactly what the optimizer's own first ``step()`` would (Adam: ``step``, ``exp_avg``, ``exp_avg_sq``; SGD with momentum:
        ``momentum_buffer``, without: nothing; Adagrad: ``step`` and ``sum``, which torch creates at construction; RMSprop:
        ``step``, ``square_avg`` and, with momentum, ``momentum_buffer``).  A slot the rule does not keep gets the parameter
        itself as a stand-in: the binding wants a pointer, the kernel never follows it."""
        st = self._rtx
        opt = self.optimizer
        spec = st.spec = optimizer_spec(opt, params)
        if st.optim is not opt:             # a new optimizer counts its own updates (state['step'] of a loaded one, below)
            st.optim, st.adam_step, st.sgd_first = opt, 0, False
        keys = [k for k in (spec.m_key, spec.v_key) if k is not None]
        for i, p in enumerate(params):
            if not keys and not spec.keeps_step:
                break                       # (plain SGD: torch never touches optimizer.state)
            state = opt.state[p]
            if spec.keeps_step and 'step' not in state:
                state['step'] = torch.tensor(0.0, dtype=torch.float32)
            for k in keys:
                t = state.get(k)
                if t is None:
                    if spec.kind == _lib.RTX_OPTIM_ADAGRAD:
                        state[k] = torch.full_like(p, float(opt.param_groups[0]['initial_accumulator_value']), memory_format=torch.preserve_format)
                    else:
                        state[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    if spec.kind == _lib.RTX_OPTIM_SGD:
                        st.sgd_first = True     # torch's first step clones the gradient into the buffer: the kernel does (RTX_OPTIM_FIRST)
                elif t.device != p.device or t.dtype != p.dtype or not t.is_contiguous():
                    # (Adagrad's sum is made where the parameters were when the optimizer was constructed)
                    state[k] = t.to(device=p.device, dtype=p.dtype).contiguous()
            if i == 0 and spec.keeps_step:
                st.adam_step = max(st.adam_step, int(float(state['step'])))
        m = [opt.state[p][spec.m_key] if spec.m_key else p.data for p in params]
        v = [opt.state[p][spec.v_key] if spec.v_key else p.data for p in params]
        return spec, m, v

    def _optim_step(self, eng, spec, count=True):
        """the optimizer side of ONE device step on ``eng``: tells the engine the rule when it is not the one it runs (an engine
        starts with plain Adam), counts the update, returns the ``rtx_step`` optimizer fields"""
        st = self._rtx
        flags = spec.flags | (_lib.RTX_OPTIM_FIRST if spec.kind == _lib.RTX_OPTIM_SGD and spec.m_key and st.sgd_first else 0)
        key = (spec.kind, flags, spec.momentum, spec.dampening, spec.alpha, spec.lr_decay)
        if getattr(eng, "_optim_key", (_lib.RTX_OPTIM_ADAM, 0, 0.0, 0.0, 0.0, 0.0)) != key:
            if st.reducer is not None and key[:2] != (_lib.RTX_OPTIM_ADAM, 0):
                raise _lib.RtxError("data parallel trains with torch.optim.Adam (coupled weight decay) only; model.optimizer is a %s"
                                    % type(self.optimizer).__name__)
            eng.set_optimizer(*key)
            eng._optim_key = key
        clip = grad_clip_spec(self)
        if getattr(eng, "_clip_key", (_lib.RTX_CLIP_NONE, 0.0)) != clip:
            eng.set_grad_clip(*clip)
            eng._clip_key = clip
        st.norm_engine = eng if clip[0] in (_lib.RTX_CLIP_NORM2, _lib.RTX_CLIP_NORMINF) else None
        if not count:       # a micro-step that only accumulates: the count of the update its window ends with
            return dict(_step_scalars_of(spec, self.optimizer.param_groups[0]), step=st.adam_step + 1)
        st.adam_step += 1
        return dict(_step_scalars_of(spec, self.optimizer.param_groups[0]), step=st.adam_step)

    def _check_clip(self):
        """the clip attributes, before anything of a step is launched: ``ValueError`` for what is not implemented, and no clipping
        under a data-parallel plan (the norm of the reduced gradient needs every bucket before the first optimizer pass)"""
        clip = grad_clip_spec(self)
        if clip[0] != _lib.RTX_CLIP_NONE and self._rtx.reducer is not None:
            raise _lib.RtxError("gradient clipping is not available under a data-parallel plan: the bucketed exchange has no global "
                                "gradient norm; unset model.clip_grad_norm / model.clip_grad_value")
        return clip

    @property
    def last_grad_norm(self):
        """The total gradient norm of the last training step as a float -- what ``clip_grad_norm_`` returns -- or ``None`` when
        that step had no norm mode set.  Fetched from the engine's host mailbox on access, not in ``train_batch``."""
        eng = self._rtx.norm_engine
        if eng is None:
            return None
        return eng.wait_grad_norm(self._rtx.adam_step)[0]

    def _optim_stepped(self, spec, write_step=False):
        """behind a device step: SGD's first update is done; ``state['step']`` where asked for; and what torch's own ``step``
        wrapper records for ``torch.optim.lr_scheduler`` (its "scheduler before optimizer.step()" warning stays quiet)"""
        st = self._rtx
        st.sgd_first = False
        self.optimizer._opt_called = True
        if write_step and spec.keeps_step:
            for p in self.network._param_list():
                self.optimizer.state[p]['step'] = torch.tensor(float(st.adam_step), dtype=torch.float32)

    # ------------------------------------------------------------------- a subclass's own loss_function
    def _custom_loss_call(self, outputs, x, gt, beta):
        """``self.loss_function`` with the reference's argument list for this class (models.py:441-442): ``(recon, gt)``"""
        return self.loss_function(outputs, gt)

    def _require_own_loss(self):
        """``custom_loss`` with one of the package's own ``loss_function``s, not overridden at all: the fused step is the route"""
        from .evaluation import _method_is_ours
        if _method_is_ours(self, "loss_function"):
            raise ValueError("custom_loss = True needs a loss_function of your own: %s.loss_function is this package's -- the fused "
                             "step (custom_loss = False) trains with that loss; an override may call super().loss_function(...), "
                             "which is differentiable" % type(self).__name__)

    def _custom_step(self, x, target, want_loss=True, accum=False):
        """One training step with ``custom_loss`` set: the reference's ``train_batch`` (models.py:424-447, 817-835).  ``x`` /
        ``target`` as for :meth:`_fused_step`; a resident sampler's row numbers stay row numbers for the engine, the dense
        tensors ``loss_function`` gets are gathered on the device (``rtx_csr_gather_dense``).  A network whose ``forward`` is the
        user's own (a subclass composing ``encode`` / ``_reparameterize`` / ``decode``) is run through that ``forward``; the
        package's networks take the whole-forward Function.
        ``accum``: a micro-step of an accumulation window (``accumulate_grad_batches`` = k > 1).  ``loss.backward()`` runs on the
        user's unscaled loss with the engine's accumulating epilogues set (weight 1 / k), so the engine's gradient buffers are the
        accumulators; the Functions hand autograd no parameter gradients then, and what the loss reaches the parameters with through
        torch alone (``p.grad`` after the backward) is added to the accumulators with the same weight.  The k-th micro-step copies the
        accumulators to ``p.grad`` and runs the optimizer."""
        self._require_own_loss()
        self._check_clip()
        st = self._rtx
        if st.reducer is not None:
            raise _lib.RtxError("custom_loss = True is not available under a data-parallel plan: the route has no gradient exchange")
        _lib.require_gpu()
        net = self.network
        params = net._param_list()
        spec, m, v = self._ensure_optim_state(params)
        if st.loss_buf is None:
            st.loss_buf = torch.zeros(2, dtype=torch.float32, device=params[0].device)
        if not isinstance(x, RowBatch):
            x = net._as_input(x)
        if target is not None and not isinstance(target, RowBatch):
            target = net._as_input(target)

        def dense(t, te=False):
            rb = t if isinstance(t, RowBatch) else None
            if rb is None:
                return t
            return (rb.te if te and rb.te is not None else rb.tr).gather_dense(rb.rows)
        x_dense = dense(x)
        if target is not None:
            gt = dense(target)
        elif isinstance(x, RowBatch) and x.te is not None:
            gt = dense(x, te=True)
        else:
            gt = x_dense
        inj = st.inject or (None, None)
        first = st.accum_pending == 0
        if accum and first:
            st.accum_k, st.accum_scalars, st.accum_custom = self._accum_window(), (self._step_scalars()[0], 0.0), True
        beta = st.accum_scalars[0] if accum else self._step_scalars()[0]
        from .evaluation import _method_is_ours
        with torch.enable_grad():
            if _method_is_ours(net, "forward"):
                outputs = net._differentiable_forward(x, numerics=self.numerics, mask=inj[0], noise=inj[1], moments=(m, v))
            else:
                # a forward of the user's own, composed from encode / _reparameterize / decode (the reference's second extension
                # point): net(x) itself, with the pieces differentiable at this model's numerics for the call
                was = net.differentiable
                net.differentiable = self.numerics
                net._rtx_trainer = {"moments": (m, v), "mask": inj[0], "noise": inj[1]}
                try:
                    outputs = net(x)
                finally:
                    net.differentiable = was
                    del net._rtx_trainer
                if not any(isinstance(t, torch.Tensor) and t.requires_grad for t in (outputs if isinstance(outputs, (tuple, list)) else (outputs,))):
                    raise _lib.RtxError("custom_loss: %s.forward returned nothing that carries a grad_fn -- the network must be in "
                                        "training mode (net.train()) and build its outputs from encode / _reparameterize / decode"
                                        % type(net).__name__)
            loss = self._custom_loss_call(outputs, x_dense, gt, beta)
        for p in params:                      # optimizer.zero_grad(): buffers that exist are kept (they may be views of one flat one)
            if p.grad is not None:
                p.grad.detach_()
                p.grad.zero_()
        B = len(x) if isinstance(x, RowBatch) else x.shape[0]
        grads = net._diff_buffers()[0]
        if accum:
            eng = net._rtx_engines.get(net._rtx_engine_key(self.numerics))      # the engine the forward ran on
            if first:
                st.accum_engine = eng
            elif eng is not st.accum_engine:
                self._accum_abandon()
                raise _lib.RtxError(_ACCUM_REBUILT % B)
            k = st.accum_k
            eng.set_grad_accum(_lib.RTX_ACCUM_FIRST if first else _lib.RTX_ACCUM_ADD, 1.0 / k)
            net._rtx_accum = True
            try:
                loss.backward()
            finally:
                net._rtx_accum = False
                eng.set_grad_accum(_lib.RTX_ACCUM_OFF)          # (the mode holds for this backward pass alone)
            for gbuf, p in zip(grads, params):                  # terms that reach the parameters through torch, unscaled
                if p.grad is not None:
                    gbuf.add_(p.grad, alpha=1.0 / k)
            loss = loss.detach().to(torch.float32)
            st.loss_buf[0] = loss
            st.loss_buf[1] += loss
            if st.accum_pending + 1 == k:
                self._accum_apply_custom()
            else:
                st.accum_pending += 1
            return loss.item() if want_loss else None
        loss.backward()
        # optimizer.step(): the engine's Adam reads its bound gradient buffers -- p.grad (the engine's gradients plus whatever the
        # loss reaches the parameters with through torch) goes there first
        eng = net.rtx_engine(self.numerics, B, train_buffers=(grads, m, v))
        for gbuf, p in zip(grads, params):
            if p.grad is None:
                gbuf.zero_()
            else:
                gbuf.copy_(p.grad)
        step = eng._step(lam=0.0, **self._optim_step(eng, spec))
        eng.apply_adam(step)
        self._optim_stepped(spec, write_step=True)
        net._rtx_mark_updated(net._rtx_engine_key(self.numerics))
        self._after_step()
        loss = loss.detach().to(torch.float32)
        st.loss_buf[0] = loss
        st.loss_buf[1] += loss
        return loss.item() if want_loss else None

    def _fused_step(self, x, target, want_loss=True, next_x=None, next_target=None, defer_join=False, users=None):
        """``users`` (CDAE_net only): the batch's user ids when they do not come with ``x`` (:func:`rectorch_amd.engine.batch_users`).
        ``next_x`` (optional, a :class:`RowBatch`): the batch of the NEXT ``_fused_step`` call.  The engine gathers it on its
        side stream under this step's last weight kernel, so that step starts with the first-layer product (single GPU, bf16).
        Its dropout seed is drawn now and kept for that step: the sequence of draws from torch's generator is unchanged.
        ``defer_join`` (epoch loops only): the step does not make the stream wait for the engine's side stream at its end
        (``RTX_STEP_DEFER_JOIN``); the next step resolves the join inside its first kernel.  The caller must not read parameters,
        optimizer state or the loss buffers before its next ``_fused_step`` / engine call or ``self._join()``."""
        cdae = self._is_cdae
        if cdae:
            self._cdae_refusals()
            users = batch_users(x, users)
            if users is None:
                raise ValueError("training a CDAE_net needs the batch's user ids: build the loader with DataSampler(..., user_ids='rows') "
                                 "(or user_ids=<one id per row>), or pass train_batch(tr, te, users=<int tensor, one id per row>)")
            user_group, user_state = self._user_optim_state()
        elif users is not None:
            raise ValueError("users= belongs to a CDAE_net; the network is a %s" % type(self.network).__name__)
        if self._accum_window() > 1:
            return self._accum_micro_step(x, target, want_loss)
        if self.custom_loss:
            return self._custom_step(x, target, want_loss)
        loss_kind = self._loss_kind
        if loss_kind == "mse" and getattr(self.network, "_variant", None) != "dae":
            # (the reference fails here too: its MSELoss gets the tuple a VAE network's forward returns)
            raise NotImplementedError("AETrainer's MSE step runs on a MultiDAE_net; %s returns more than the reconstruction -- use "
                                      "the trainer of that network" % type(self.network).__name__)
        self._check_clip()
        _lib.require_gpu()
        st, params, m, v = self._ensure_train_state()
        spec = st.spec
        if not isinstance(x, RowBatch):
            x = self.network._as_input(x)
            if target is not None:
                target = self.network._as_input(target)
        B = len(x) if isinstance(x, RowBatch) else x.shape[0]
        eng = self.network.rtx_engine(self.numerics, B, train_buffers=(st.grads, m, v), loss=loss_kind)
        beta, lam = self._step_scalars()
        opt_scalars = self._optim_step(eng, spec)
        if cdae:
            # the ids of THIS batch, consumed by the train_step below (a batch announced through next_x brings item rows only)
            # (SparseAdam's step count moves once the step is enqueued; a step the engine refuses leaves the count and takes the ids back)
            eng.set_users(users, batch=B, lr=user_group['lr'], beta1=user_group['betas'][0], beta2=user_group['betas'][1],
                          eps=user_group['eps'], step=int(user_state['step']) + 1)
        from .nets import draw_seed
        red = st.reducer
        if red is not None and self._variant == "gvae":
            raise _lib.RtxError("data parallel is not available for VAE(VAE_net): the engine has no data-parallel step for it")
        if red is not None and loss_kind == "mse":
            raise _lib.RtxError("data parallel is not available for AETrainer's MSE loss: the engine has no data-parallel step for it")
        native = red is not None and getattr(red, "native", False)
        # (python-driven reducer) data parallel, bf16 numerics and bf16 exchange with the optimizer behind each bucket: the weight-gradient kernels write
        # the bf16 images the all-reduce sends directly (no float32 gradient store, no cast pass); p.grad is not filled then
        direct16 = (red is not None and not native and self.numerics == "bf16" and red.flat16 is not None and red.on_device and
                    getattr(red, "bucket_adam", False) and getattr(red, "allow_direct16", True) and not self.keep_grads)
        if red is not None and not native:
            red.direct16 = direct16
            eng.bind_grads16(red.grads16_ptrs() if direct16 else None)
        inj = self._rtx.inject or (None, None)     # (keep-mask uint8 [B, n_items], eps [B, latent]) for parity tests
        seed = st.pending_seed if st.pending_seed is not None else draw_seed()     # (drawn one step early for an announced batch)
        st.pending_seed = None
        if (next_x is not None and (red is None or native) and self.numerics == "bf16" and self._rtx.inject is None and self.prefetch_batches
                and isinstance(next_x, RowBatch)):
            st.pending_seed = draw_seed()
            # (data parallel, engine-scheduled: the gather rides behind bucket A on the engine's side stream; the dropout stream of a rank is
            #  keyed by its rank, as the step itself keys it)
            eng.set_next_batch(next_x, next_target, seed=st.pending_seed, offset=0 if red is None else red.rank)
        step = eng._step(seed=seed, offset=0 if red is None else red.rank, mask=inj[0], noise=inj[1],
                         beta=float(beta), lam=float(lam),
                         # (a rank's slice made by parallel.shard_batch knows the global batch: no collective, no host sync)
                         inv_batch=1.0 / (B if red is None else (getattr(x, "global_len", None) or red.global_batch(B))),
                         flags=(_lib.RTX_STEP_KEEP_GRADS if self.keep_grads else 0) |
                               (_lib.RTX_STEP_DEFER_JOIN if defer_join and (red is None or native) and not want_loss and self.numerics == "bf16" else 0) |
                               (_lib.RTX_STEP_GRADS_BF16 if direct16 else 0) |
                               # data parallel: the (rank-independent) DAE regulariser enters the summed loss once
                               (_lib.RTX_STEP_NO_REG_IN_LOSS if red is not None and red.rank != 0 else 0),
                         **opt_scalars)
        loss_out, loss_acc = st.loss_buf[0:1], st.loss_buf[1:2]
        mailbox = red is None and want_loss and self.loss_mailbox
        if mailbox and not getattr(eng, "_mailbox", False):
            eng.loss_mailbox(True)
        if red is None:
            try:
                eng.train_step(x, target, step, loss_out, loss_acc)
            except Exception:
                if cdae:
                    eng.set_users(None)
                raise
            if cdae:
                user_state['step'] += 1
        elif native:
            # the engine schedules the whole data-parallel step (rectorch_amd/parallel.py NativePlan): ONE call
            if getattr(eng, "_dp_plan", None) is not red:
                eng.dp_attach(red)                   # (a rebuilt engine -- a larger batch arrived -- attaches again)
            red.error = None                         # (a stale failure of an earlier step must not be re-raised for this one)
            try:
                eng.train_step_dp(x, target, step, loss_out, loss_acc)
            except _lib.RtxError:
                if getattr(red, "error", None) is not None:
                    raise red.error                  # a collective issued through torch.distributed failed: its own message
                raise
            if eng._dp_any_sharded and red.transport != "emulate":   # what the ENGINE shards, not what the plan asked for
                st.masters_sharded = True
                self.network._rtx_masters_stale = True
        else:
            if getattr(red, "bucket_adam", False):
                g16 = red.grads16_ptrs()
                red.adam = lambda lo, hi: eng.apply_adam_layers(step, lo, hi, g16)
                if getattr(red, "sharded", False):
                    # sharded optimizer: this rank updates only its rows of the big matrices, then the compute copies
                    # are all-gathered in place (rectorch_amd/parallel.py)
                    red.adam_rows = lambda layer, lo, hi: eng.apply_adam_rows(
                        step, layer, lo, hi, True,
                        None if g16 is None else g16[2 * layer], None if g16 is None else g16[2 * layer + 1])
                    red.shadow = eng.shadow_tensor
                    st.masters_sharded = True
                    self.network._rtx_masters_stale = True
            else:
                red.adam = None
            eng.loss_grads(x, target, step, loss_out, loss_acc, layer_cb=red.on_layer)
            red.wait()
            if red.adam is None:
                eng.apply_adam(step)
            red.adam = None
        self.network._rtx_mark_updated(self.network._rtx_engine_key(self.numerics, loss_kind))
        self._optim_stepped(spec)
        self._after_step()
        if want_loss:
            if red is not None:
                return red.reduce_scalar(st.loss_buf[0:1].clone())
            if mailbox:
                # THIS step's loss (reference models.py:835 `return loss.item()`) from the engine's host mailbox: the weight-gradient
                # + Adam kernels behind the loss keep running while the host returns and enqueues the next step
                return eng.wait_loss(st.adam_step)
            return st.loss_buf[0].item()       # the reference's per-step loss.item() sync
        return None

    # ------------------------------------------------------------------------------- gradient accumulation
    @property
    def pending_micro_batches(self):
        """micro-steps in the open accumulation window (0: none is open)"""
        return self._rtx.accum_pending

    def _accum_window(self):
        """``accumulate_grad_batches`` of the current window: the attribute, checked, at a window's first micro-step; inside a
        window the value it was opened with -- a different one raises before anything is launched"""
        st = self._rtx
        k = accum_spec(self.accumulate_grad_batches)
        if st.accum_pending and k != st.accum_k:
            raise _lib.RtxError("model.accumulate_grad_batches changed from %d to %d with %d micro-batches of a window accumulated; "
                                "change it between windows, or call model.apply_accumulated() first" % (st.accum_k, k, st.accum_pending))
        return k

    def _accum_refusals(self):
        """what gradient accumulation does not cover, before anything is launched"""
        if self._rtx.reducer is not None:
            raise _lib.RtxError("accumulate_grad_batches > 1 is not available under a data-parallel plan: the accumulators are one "
                                "device's float32 gradient buffers; %s" % _SUPPORTED_ACCUM)

    def _accum_micro_step(self, x, target, want_loss=True):
        """One micro-step of an accumulation window of ``k = accumulate_grad_batches`` calls: forward, loss and backward on the
        current stream (``rtx_engine_loss_grads``) with the weight-gradient kernels adding ``g / k`` into ``p.grad``; the k-th
        call runs the same schedule inside ``rtx_engine_train_step``, followed by clipping and the optimizer reading ``p.grad``.
        Per window: one optimizer step count, one ``(beta, lam)``; per micro-step: its own dropout seed and its own loss."""
        self._accum_refusals()
        if self.custom_loss != self._rtx.accum_custom and self._rtx.accum_pending:
            raise _lib.RtxError("model.custom_loss changed inside an accumulation window; call model.apply_accumulated() first")
        if self.custom_loss:
            return self._custom_step(x, target, want_loss, accum=True)
        loss_kind = self._loss_kind
        if loss_kind == "mse" and getattr(self.network, "_variant", None) != "dae":
            raise NotImplementedError("AETrainer's MSE step runs on a MultiDAE_net; %s returns more than the reconstruction -- use "
                                      "the trainer of that network" % type(self.network).__name__)
        self._check_clip()
        _lib.require_gpu()
        st, params, m, v = self._ensure_train_state()
        spec = st.spec
        if not isinstance(x, RowBatch):
            x = self.network._as_input(x)
            if target is not None:
                target = self.network._as_input(target)
        B = len(x) if isinstance(x, RowBatch) else x.shape[0]
        first = st.accum_pending == 0
        if not first and B > st.accum_engine.max_batch:
            # (a batch above the engine's max_batch would rebuild it; the new handle would know nothing of the open window.  Refused
            #  BEFORE the network builds that engine: the old one stays the cached one, and apply_accumulated() leaves it current)
            raise _lib.RtxError(_ACCUM_REBUILT % B)
        eng = self.network.rtx_engine(self.numerics, B, train_buffers=(st.grads, m, v), loss=loss_kind)
        if first:
            st.accum_k, st.accum_engine, st.accum_scalars, st.accum_custom = self._accum_window(), eng, self._step_scalars(), False
        elif eng is not st.accum_engine:        # (rebuilt for any other reason: nothing of the window can be trusted)
            self._accum_abandon()
            raise _lib.RtxError(_ACCUM_REBUILT % B)
        k = st.accum_k
        last = st.accum_pending + 1 == k
        beta, lam = st.accum_scalars
        opt_scalars = self._optim_step(eng, spec, count=last)
        from .nets import draw_seed
        inj = st.inject or (None, None)
        seed = st.pending_seed if st.pending_seed is not None else draw_seed()
        st.pending_seed = None
        step = eng._step(seed=seed, offset=0, mask=inj[0], noise=inj[1], beta=float(beta), lam=float(lam), inv_batch=1.0 / B, flags=0,
                         **opt_scalars)
        loss_out, loss_acc = st.loss_buf[0:1], st.loss_buf[1:2]
        mailbox = want_loss and self.loss_mailbox
        if mailbox and not getattr(eng, "_mailbox", False):
            eng.loss_mailbox(True)
        eng.set_grad_accum(_lib.RTX_ACCUM_FIRST if first else _lib.RTX_ACCUM_ADD, 1.0 / k)
        if last:
            eng.train_step(x, target, step, loss_out, loss_acc)      # (with a mode set: the unfused schedule, reading the accumulators)
            self._accum_closed(spec, loss_kind)
        else:
            eng.loss_grads(x, target, step, loss_out, loss_acc)
            st.accum_pending += 1
        if want_loss:
            # (every loss reduction has a mailbox ticket of its own: this is THIS micro-batch's loss, whatever the shared step count)
            return eng.wait_loss(opt_scalars["step"]) if mailbox else st.loss_buf[0].item()
        return None

    def _accum_abandon(self):
        """drop the open window (its engine is gone): the next micro-step opens a new one"""
        st = self._rtx
        st.accum_pending, st.accum_engine, st.accum_scalars = 0, None, None

    def _accum_apply_custom(self):
        """the update of a custom-loss window: the accumulators (the engine's bound gradient buffers) become ``p.grad``, then clip
        and rule on them"""
        st, net = self._rtx, self.network
        eng = st.accum_engine
        spec = self._ensure_optim_state(net._param_list())[0]
        for gbuf, p in zip(net._diff_buffers()[0], net._param_list()):
            if p.grad is None:
                p.grad = gbuf.clone()
            else:
                p.grad.copy_(gbuf)
        step = eng._step(lam=0.0, **self._optim_step(eng, spec))
        eng.apply_adam(step)
        st.accum_pending, st.accum_engine, st.accum_scalars = 0, None, None
        self._optim_stepped(spec, write_step=True)
        net._rtx_mark_updated(net._rtx_engine_key(self.numerics))
        self._after_step()

    def _accum_closed(self, spec, loss_kind):
        st = self._rtx
        st.accum_pending, st.accum_engine, st.accum_scalars = 0, None, None
        self.network._rtx_mark_updated(self.network._rtx_engine_key(self.numerics, loss_kind))
        self._optim_stepped(spec)
        self._after_step()

    def apply_accumulated(self):
        """Apply the open accumulation window now: clipping (if set) and ``model.optimizer``'s rule on what ``p.grad`` holds -- with
        j < k micro-steps the sum of j terms of weight 1 / k, what torch's loop leaves when it stops early and steps.  Returns
        False, and launches nothing, when no window is open."""
        st = self._rtx
        if st.accum_pending == 0:
            return False
        self._check_clip()
        if st.accum_custom:
            self._accum_apply_custom()
            return True
        eng = st.accum_engine
        spec = self._ensure_optim_state(self.network._param_list())[0]
        beta, lam = st.accum_scalars
        # (Mult-DAE's regulariser is part of every micro-step's loss: j of k terms of weight 1 / k of its gradient, formed at the update)
        lam = lam * st.accum_pending / st.accum_k
        step = eng._step(beta=float(beta), lam=float(lam), **self._optim_step(eng, spec))
        eng.apply_adam(step)        # (norm / clip, then the rule, on the accumulators; Mult-DAE's regulariser term from the norms the
        self._accum_closed(spec, self._loss_kind)   #  last micro-step computed: no parameter has moved since)
        return True

    def _require_closed_window(self, what):
        if self._rtx.accum_pending:
            raise _lib.RtxError("%s() with %d of %d micro-batches of a gradient accumulation window accumulated: the checkpoint would "
                                "drop them; call model.apply_accumulated() first (train_epoch does at the end of every epoch)"
                                % (what, self._rtx.accum_pending, self._rtx.accum_k))

    def _join(self):
        """order the current stream behind everything the engines' side streams still carry (steps run with ``defer_join``)"""
        for eng in getattr(self.network, "_rtx_engines", {}).values():
            eng.join()

    def _read_loss_sum(self):
        self._join()
        st = self._rtx
        if st.reducer is not None:
            s = st.reducer.reduce_scalar(st.loss_buf[1:2].clone())
        else:
            s = st.loss_buf[1].item()
        st.loss_buf[1].zero_()
        return s

    # ----------------------------------------------------------------------------------- prediction
    def _predict_engine(self, n):
        """what every prediction starts with: the checks, eval mode and the engine of the predict numerics for batches of ``n`` rows
        (``evaluate_device`` does this ONCE per loader instead of once per batch)"""
        _lib.require_gpu()
        self._join()         # (an epoch interrupted between two deferred-join steps: order this stream behind the side streams first)
        if self._rtx.masters_sharded and self.predict_numerics != self.numerics:
            # that engine's compute copies come from the float32 masters, of which this rank holds only its rows
            raise _lib.RtxError("sharded optimizer: the float32 master rows of the other ranks are stale on this rank; call "
                                "model.consolidate() on EVERY rank (it is a collective) before predict() in another numerics "
                                "mode than the training one")
        self.network.eval()
        return self.network.rtx_engine(self.predict_numerics, n)

    def _predict_tuple(self, x, remove_train, users=None):
        x_in = self.network._as_input(x)
        n = len(x_in) if isinstance(x_in, RowBatch) else x_in.shape[0]
        eng = self._predict_engine(n)
        if self._is_cdae:
            # the ids that come with the batch, or none: the zero user vector (whichever route below scores the batch consumes them)
            eng.set_users(batch_users(x, users), batch=n)
        elif users is not None:
            raise ValueError("users= belongs to a CDAE_net; the network is a %s" % type(self.network).__name__)
        # VAE(VAE_net) samples z in eval mode too (the reference's VAE_net._reparameterize has no eval branch): one seed from
        # torch's generator per call, so that torch.manual_seed makes a prediction repeatable; the others draw nothing
        gvae = self._variant == "gvae"
        seed = 0
        if gvae:
            from .nets import draw_seed
            seed = draw_seed()
        noise = self._rtx.inject[1] if gvae and self._rtx.inject is not None else None     # (parity tests: the reference's eps)
        if not isinstance(x_in, RowBatch) and tagged_rows(x_in) is None and noise is None:
            # dense input: through the PyTorch-ROCm custom op (torch.ops.rectorch_hip.*, rectorch_amd/ops.py)
            from . import ops  # noqa: F401  (registers the ops)
            if self._variant in ("vae", "gvae"):
                return torch.ops.rectorch_hip.mvae_forward(eng.op_handle, x_in, False, bool(remove_train), seed)
            return (torch.ops.rectorch_hip.mdae_forward(eng.op_handle, x_in, False, bool(remove_train), 0), None, None)
        return eng.forward(x_in, training=False, remove_train=remove_train, seed=seed, noise=noise)

    def predict(self, x, remove_train=True, users=None):
        r"""Perform the prediction using a trained Autoencoder (reference models.py:449-473).  Returns the
        1-tuple ``(recon_x,)``; with ``remove_train`` the items of ``x`` are scored :math:`-\infty`.
        ``users`` (CDAE_net only): the rows' user ids when the batch does not carry them.  A CDAE_net scored WITHOUT ids (or
        with -1) uses the zero user vector: that is fold-in of users the fit never saw."""
        recon_x, _, _ = self._predict_tuple(x, remove_train, users)
        return (recon_x, )

    def recommend(self, loader, k=100, remove_train=True):
        r"""The ``k`` best items of every user of ``loader`` and their scores, on the device:
        :func:`rectorch_amd.evaluation.recommend` with this model (``(items int32, scores)`` of shape ``[users, min(k, n_items)]``
        in loader order)."""
        from .evaluation import recommend
        return recommend(self, loader, k=k, remove_train=remove_train)

    # -------------------------------------------------------------------------------- checkpointing
    def consolidate(self):
        """Data parallel with the sharded optimizer: every rank holds current float32 master rows (and Adam moments) only for
        its own shard of the big matrices.  COLLECTIVE -- call it on EVERY rank -- before anything reads parameters from the
        host side: checkpoints, ``state_dict()``, ``predict`` in another numerics mode, a larger batch (the engine is rebuilt
        from the masters).  ``train()`` does so before each validation pass; ``save_model`` / ``predict`` raise when called with
        stale rows.  A no-op without the sharded optimizer."""
        self._gather_sharded_state()

    def _gather_sharded_state(self):
        st = self._rtx
        if st.reducer is None or not st.masters_sharded:
            return
        params = self.network._param_list()
        if getattr(st.reducer, "native", False):
            def tensors_n(layer):
                p = params[2 * layer]
                state = self.optimizer.state[p]
                return [p.data, state['exp_avg'], state['exp_avg_sq']]
            torch.cuda.current_stream().synchronize()
            eng = self.network._rtx_engines[self.numerics]
            st.reducer.gather_state(eng, tensors_n, len(params) // 2)
            st.masters_sharded = False
            self.network._rtx_masters_stale = False
            keep = self.network._rtx_shadow_versions.get(self.numerics)
            self.network._rtx_shadow_versions.clear()     # compute copies of the other numerics modes: refresh from the masters
            if keep is not None:
                # p.data was rewritten in place (version counters moved) with the values the training engine's compute copies
                # already hold: that engine's copies stay valid
                self.network._rtx_shadow_versions[self.numerics] = self.network._param_version()
            return

        def tensors(layer):
            p = params[2 * layer]
            state = self.optimizer.state[p]
            return [p.data, state['exp_avg'], state['exp_avg_sq']]
        st.reducer.wait()
        st.reducer.gather_state(tensors)
        st.masters_sharded = False
        self.network._rtx_masters_stale = False
        self.network._rtx_shadow_versions.clear()     # compute copies of the other numerics modes: refresh from the masters

    def _require_consolidated(self, what):
        if self._rtx.masters_sharded:
            raise _lib.RtxError("sharded optimizer: %s() needs the float32 master rows of every rank; call model.consolidate() "
                                "on EVERY rank first (it is a collective -- a rank-0-only checkpoint would deadlock inside it)" % what)

    def _sync_optimizer_state(self):
        """write the step count the fused Adam kernel is at into torch.optim.Adam's state"""
        self._join()         # (checkpoints read parameters and moments through torch: behind the engines' side streams)
        for p in self.network.parameters():
            state = self.optimizer.state.get(p)
            if state is not None and 'step' in state:
                state['step'] = torch.tensor(float(self._rtx.adam_step), dtype=torch.float32)

    def save_model(self, filepath, cur_epoch):
        r"""Save the model to file (reference models.py:475-489): ``epoch``, ``state_dict``, ``optimizer``."""
        self._require_consolidated("save_model")
        self._require_closed_window("save_model")
        self._sync_optimizer_state()
        state = {'epoch': cur_epoch,
                 'state_dict': self.network.state_dict(),
                 'optimizer': self.optimizer.state_dict()
                }
        if self._is_cdae:       # (one more key, for this network only)
            state['user_optimizer'] = self.user_optimizer.state_dict()
        self._save_checkpoint(filepath, state)

    def _save_checkpoint(self, filepath, state):
        logger.info("Saving model checkpoint to %s...", filepath)
        torch.save(state, filepath)
        logger.info("Model checkpoint saved!")

    def load_model(self, filepath):
        r"""Load the model from file (reference models.py:496-516); returns the checkpoint dictionary."""
        assert os.path.isfile(filepath), "The checkpoint file %s does not exist." %filepath
        logger.info("Loading model checkpoint from %s...", filepath)
        checkpoint = torch.load(filepath, map_location=self.device)
        self._join()         # (nothing of an open deferred step may land in the tensors after the checkpoint's values)
        self.network.load_state_dict(checkpoint['state_dict'])
        self.optimizer.load_state_dict(checkpoint['optimizer'])
        if self._is_cdae and 'user_optimizer' in checkpoint:
            self.user_optimizer.load_state_dict(checkpoint['user_optimizer'])
        steps = [int(float(s['step'])) for s in self.optimizer.state.values() if 'step' in s]
        self._rtx.adam_step = steps[0] if steps else 0
        logger.info("Model checkpoint loaded!")
        return checkpoint


class VAE(AETrainer):
    r"""Standard Variational Autoencoder (reference models.py:519-625) and the plumbing its subclasses share: ``predict``
    returns ``(recon_x, mu, logvar)``.

    With the reference's plain :class:`rectorch_amd.nets.VAE_net` this is the whole model on the device: ``train_batch``
    is one fused step (raw input rows, z sampled, sigmoid decoder, loss ``F.binary_cross_entropy(p, x) + KLD`` with the
    input as target, backward and Adam; ``te_batch`` is ignored as in the reference), ``loss_function`` the same loss on
    dense tensors, and ``predict`` returns the sigmoid probabilities, sampled in eval mode too with one seed drawn from
    torch's generator per call.  Data parallelism is not available for it."""

    def __init__(self, vae_net, *args, **kwargs):
        from .nets import CDAE_net
        if isinstance(vae_net, CDAE_net):
            raise TypeError("%s cannot train a CDAE_net: it has no mean / log-variance head; supported: MultiDAE(CDAE_net) "
                            "(multinomial likelihood) and AETrainer(CDAE_net) (MSE)" % type(self).__name__)
        super(VAE, self).__init__(vae_net, *args, **kwargs)

    @property
    def _variant(self):
        # VAE_net is an engine variant of its own (RTX_GVAE); with any other network this class stays the MultiVAE plumbing
        return "gvae" if getattr(self.network, "_variant", None) == "gvae" else "vae"

    def loss_function(self, recon_x, x, mu, logvar):
        r"""``F.binary_cross_entropy(recon_x, x) + KLD`` (reference models.py:533-583) on the HIP device, ``recon_x`` being the
        sigmoid probabilities; returns a 0-dim tensor."""
        if self._variant != "gvae":
            raise NotImplementedError("the generic BCE VAE loss belongs to VAE(VAE_net); use MultiVAE for this network")
        return bce_kl_loss(recon_x, x, mu, logvar)

    def _custom_loss_call(self, outputs, x, gt, beta):
        """``(recon_x, x, mu, logvar)`` with the input batch as target (reference models.py:588-589)"""
        recon, mu, logvar = outputs
        return self.loss_function(recon, x, mu, logvar)

    def _step_scalars(self):
        if self._variant == "gvae":
            return 1.0, 0.0            # BCE + KLD: the KL term at weight one, no annealing (the engine enforces it too)
        return super()._step_scalars()

    def predict(self, x, remove_train=True):
        r"""Perform the prediction using a trained Variational Autoencoder (reference models.py:594-625).
        Returns ``(recon_x, mu, logvar)``; with ``remove_train`` the items of ``x`` are scored
        :math:`-\infty`."""
        return self._predict_tuple(x, remove_train)


class MultiDAE(AETrainer):
    r"""Denoising Autoencoder with multinomial likelihood for collaborative filtering (reference
    models.py:628-706): Adam with (coupled) ``weight_decay=0.001``; loss = multinomial NLL +
    :math:`\lambda \sum_W \lVert W \rVert_2`.

    Parameters
    ----------
    mdae_net : :class:`rectorch_amd.nets.MultiDAE_net`
    lam : :obj:`float` [optional]
        The regularization hyper-parameter, by default 0.2.
    learning_rate : :obj:`float` [optional]
        By default 1e-3.
    """
    _variant = "dae"

    def __init__(self,
                 mdae_net,
                 lam=0.2,
                 learning_rate=1e-3,
                 numerics="bf16",
                 predict_numerics="fp32"):
        super(MultiDAE, self).__init__(mdae_net, learning_rate, numerics, predict_numerics)
        self.optimizer = optim.Adam(self._net_parameters(),
                                    lr=self.learning_rate,
                                    weight_decay=0.001)
        self.lam = lam

    def loss_function(self, recon_x, x):
        r"""Multinomial likelihood denoising autoencoder loss (reference models.py:662-706), on the HIP
        device; returns a 0-dim tensor.  Where ``recon_x`` requires grad the result is differentiable, and the regulariser is
        taken over the parameters themselves: its gradient reaches ``p.grad`` through torch."""
        from .engine import sum_l2_norms
        nll = multinomial_loss(recon_x, x)
        params = list(self._net_parameters())
        if not (torch.is_grad_enabled() and recon_x.requires_grad):
            params = [p.data for p in params]
        return nll + self.lam * sum_l2_norms(params)

    def _step_scalars(self):
        return 0.0, self.lam


class MultiVAE(VAE):
    r"""Variational Autoencoder for collaborative Filtering (reference models.py:709-908).

    Parameters
    ----------
    mvae_net : :class:`rectorch_amd.nets.MultiVAE_net`
    beta : :obj:`float` [optional]
        The :math:`\beta` hyper-parameter of Multi-VAE, by default 1.0.
    anneal_steps : :obj:`int` [optional]
        Number of annealing steps for reaching the target value ``beta``, by default 0 (no annealing).
    learning_rate : :obj:`float` [optional]
        By default 1e-3.

    Attributes
    ----------
    anneal_steps, annealing, gradient_updates (a float, as in the reference), beta.
    """
    _uses_te = True      # the loss target is te_batch when given (reference models.py:819-822)

    def __init__(self,
                 mvae_net,
                 beta=1.,
                 anneal_steps=0,
                 learning_rate=1e-3,
                 numerics="bf16",
                 predict_numerics="fp32"):
        super(MultiVAE, self).__init__(mvae_net, learning_rate, numerics, predict_numerics)
        self.optimizer = optim.Adam(self.network.parameters(),
                                    lr=learning_rate,
                                    weight_decay=0.0)
        self.anneal_steps = anneal_steps
        self.annealing = anneal_steps > 0
        self.gradient_updates = 0.
        self.beta = beta

    def loss_function(self, recon_x, x, mu, logvar, beta=1.0):
        r"""VAE for collaborative filtering loss function (reference models.py:776-815):
        multinomial NLL + ``beta`` * KL, on the HIP device; returns a 0-dim tensor."""
        return multinomial_loss(recon_x, x, mu, logvar, beta)

    def _custom_loss_call(self, outputs, x, gt, beta):
        """``(recon_x, gt, mu, logvar, anneal_beta)``: the target is ``te_batch`` when given (reference models.py:819-831)"""
        recon, mu, logvar = outputs
        return self.loss_function(recon, gt, mu, logvar, beta)

    def _step_scalars(self):
        if self.annealing:
            anneal_beta = min(self.beta, 1. * self.gradient_updates / self.anneal_steps)
        else:
            anneal_beta = self.beta
        return anneal_beta, 0.0

    def _after_step(self):
        self.gradient_updates += 1.

    def train_batch(self, tr_batch, te_batch=None):
        r"""Training of a single batch (reference models.py:817-835): the encoder input is ``tr_batch``, the
        loss target ``te_batch`` when given, the KL weight is annealed with ``gradient_updates``."""
        return self._fused_step(tr_batch, te_batch, want_loss=True)

    def train(self,
              train_data,
              valid_data=None,
              valid_metric=None,
              valid_func=ValidFunc(evaluate),
              num_epochs=200,
              best_path="chkpt_best.pth",
              verbose=1):
        r"""Training procedure for Multi-VAE (reference models.py:837-895): per epoch ``train_epoch``, then -- when
        ``valid_data`` is truthy, as in the reference -- validation with ``valid_func`` and a checkpoint to ``best_path``
        whenever the mean of ``valid_metric`` improves on the best so far (metrics are assumed non-negative)."""
        best = -1.
        try:
            for epoch in range(1, num_epochs + 1):
                self.train_epoch(epoch, train_data, verbose)
                if valid_data:
                    self.consolidate()          # (data parallel, sharded optimizer: every rank runs train() and gets here)
                    score = _validate(self, epoch, valid_data, valid_metric, valid_func)
                    if score > best:
                        self.save_model(best_path, epoch)
                        best = score
        except KeyboardInterrupt:
            logger.warning('Handled KeyboardInterrupt: exiting from training early')

    def save_model(self, filepath, cur_epoch):
        r"""Save the model to file (reference models.py:897-903): adds ``gradient_updates``."""
        self._require_consolidated("save_model")
        self._require_closed_window("save_model")
        self._sync_optimizer_state()
        state = {'epoch': cur_epoch,
                 'state_dict': self.network.state_dict(),
                 'optimizer': self.optimizer.state_dict(),
                 'gradient_updates': self.gradient_updates
                }
        self._save_checkpoint(filepath, state)

    def load_model(self, filepath):
        r"""Load the model from file and restore ``gradient_updates`` (reference models.py:905-908)."""
        checkpoint = super().load_model(filepath)
        self.gradient_updates = checkpoint['gradient_updates']
        return checkpoint


class CMultiVAE(MultiVAE):
    r"""Conditioned Variational Autoencoder for collaborative filtering (reference models.py:911-956).

    Same training procedure as :class:`MultiVAE`; the network is a :class:`rectorch_amd.nets.CMultiVAE_net` and the
    sampler a :class:`rectorch_amd.samplers.ConditionedDataSampler`, whose batches are ``[items | condition]`` rows
    with the condition-filtered rows as loss target.  ``predict`` masks the *item* columns of ``x`` only
    (``x[:, :-cond_dim].nonzero()``, reference models.py:952-953) -- the engine bounds the mask at ``n_items``.
    """
    def __init__(self,
                 cmvae_net,
                 beta=1.,
                 anneal_steps=0,
                 learning_rate=1e-3,
                 numerics="bf16",
                 predict_numerics="fp32"):
        super(CMultiVAE, self).__init__(cmvae_net,
                                        beta=beta,
                                        anneal_steps=anneal_steps,
                                        learning_rate=learning_rate,
                                        numerics=numerics,
                                        predict_numerics=predict_numerics)

    def predict(self, x, remove_train=True):
        return self._predict_tuple(x, remove_train)


class _FoldInModel(RecSysModel):
    r"""What the models share that are fitted once on the device and then scored by multiplying users' sparse rows by something
    resident in HBM (EASE, ADMM_Slim, ItemKNN, WMF).  ``_solver`` is that resident model -- a solver of :mod:`rectorch_amd.engine`
    whose ``scores`` folds rows in -- or ``None`` before ``train`` / ``load_model``.  A subclass adds ``train`` and ``predict``, the
    save file's two hooks (:meth:`_state`, :meth:`_set_state`) and the two parts of its ``__str__`` (:meth:`_str_head`,
    :meth:`_str_size`)."""
    _solver = None

    def _require_solver(self, what):
        if self._solver is None:
            raise RuntimeError("%s.%s called before train / load_model" % (type(self).__name__, what))
        return self._solver

    def _fold_in(self, rows, what):
        """``(solver, rows as a resident CsrMatrix)`` for the fold-in methods"""
        solver = self._require_solver(what)
        X = rows if isinstance(rows, CsrMatrix) else CsrMatrix(rows)
        if X.shape[1] != solver.n_items:
            raise ValueError("rows have %d columns, the model has %d items" % (X.shape[1], solver.n_items))
        return solver, X

    @staticmethod
    def _lists(n, n_items, k, chunk, score_chunk, excl, predict_chunk):
        """The chunk loop behind ``recommend`` / ``recommend_rows``, whatever the scores come from.  ``score_chunk(lo, hi, out)``: the
        score rows of users ``lo .. hi`` as a float64 device tensor (written into ``out``, nothing masked) -- they go into ONE scratch
        buffer, chunk after chunk, and the float64 selection kernel ranks them with the resident ``excl`` (nullable; row b = user b) as
        its exclusion: the ``[users, n_items]`` matrix exists neither on the host nor whole on the device.  ``score_chunk`` None (a
        loaded score matrix) or ``k`` above the kernel's 1024: ``predict_chunk(lo, hi)`` -- a host array, masked by its maker -- and a
        host sort, in the same chunks."""
        from .engine import topk_items, TOPK_ITEMS_MAX
        from .evaluation import _lexsort_topk
        if score_chunk is None or int(k) > TOPK_ITEMS_MAX:
            parts = [_lexsort_topk(predict_chunk(lo, min(lo + chunk, n)), k) for lo in range(0, n, chunk)]
            dev = "cuda" if torch.cuda.is_available() else "cpu"
            if not parts:
                return torch.empty((0, 0), dtype=torch.int32, device=dev), torch.empty((0, 0), dtype=torch.float64, device=dev)
            return (torch.from_numpy(np.concatenate([p[0] for p in parts])).to(dev),
                    torch.from_numpy(np.concatenate([p[1] for p in parts])).to(dev))
        kk = min(int(k), n_items)
        items = torch.empty((n, kk), dtype=torch.int32, device="cuda")
        vals = torch.empty((n, kk), dtype=torch.float64, device="cuda")
        scratch = torch.empty((min(chunk, max(n, 1)), n_items), dtype=torch.float64, device="cuda")
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            scores = score_chunk(lo, hi, scratch[:hi - lo])
            rows = torch.arange(lo, hi, dtype=torch.int32, device="cuda") if excl is not None else None
            topk_items(scores, k, excl, rows, out=(items[lo:hi], vals[lo:hi]))
        return items, vals

    def recommend(self, ids_te_users, test_tr, k=100, remove_train=True):
        r"""The ``k`` best items of the given users and their scores, on the device: ``(items, scores)``, device tensors of
        shape ``[users, min(k, n_items)]`` (int32 / float64), score descending, item id ascending among equal scores.

        Parameters
        ----------
        ids_te_users : array_like
            List of the test user indexes.
        test_tr : :class:`scipy.sparse.csr_matrix`
            Training portion of the test users.
        k : :obj:`int` [optional]
            Length of the lists, by default 100.
        remove_train : :obj:`bool` [optional]
            Whether the items in ``test_tr`` rank as :math:`-\infty`, by default True.
        """
        return self._recommend(ids_te_users, test_tr, k, remove_train)

    def _recommend(self, ids_te_users, test_tr, k, remove_train, chunk=1024):
        """``recommend``: the users' rows of the TRAINING matrix times the model (the solver's ``scores`` without a mask), ``test_tr``
        as the exclusion, through :meth:`_lists`."""
        if int(k) < 1:
            raise ValueError("recommend: k must be >= 1, got %s" % (k,))
        solver = self._require_solver("recommend")
        from .engine import TOPK_ITEMS_MAX
        ids_host = np.asarray(ids_te_users)
        ids = torch.as_tensor(ids_te_users, dtype=torch.int32).to("cuda").contiguous()
        n, n_items = int(ids.numel()), solver.n_items
        excl = None
        if remove_train and int(k) <= TOPK_ITEMS_MAX:
            if test_tr.shape[0] != n or test_tr.shape[1] != n_items:
                raise ValueError("mask matrix has shape %s, expected (%d, %d)" % (test_tr.shape, n, n_items))
            excl = CsrMatrix(test_tr)
        return self._lists(n, n_items, k, chunk, lambda lo, hi, out: solver.scores(ids[lo:hi], None, out=out), excl,
                           lambda lo, hi: self.predict(ids_host[lo:hi], test_tr[lo:hi], remove_train=remove_train)[0])   # k above 1024

    def score_rows(self, rows, remove_train=True, as_tensor=False):
        r"""Fold-in: the scores of ANY users over the model's items, :math:`S = \mathbf{R} \cdot \mathbf{B}` for the rows
        :math:`\mathbf{R}` given -- users the fit never saw included.  (``predict`` looks the users up in the training matrix;
        where ``rows`` are rows of it, both give the same bits.)  ``ADMM_Slim`` with ``item_bias`` adds the bias term of its fit.

        Parameters
        ----------
        rows : :class:`scipy.sparse.csr_matrix` or :class:`rectorch_amd.engine.CsrMatrix`
            One row per user over the model's ``n_items`` items.
        remove_train : :obj:`bool` [optional]
            Whether to set the scores of the items stored in ``rows`` to :math:`-\infty`, by default True.
        as_tensor : :obj:`bool` [optional]
            Return the float64 device tensor instead of copying it to a numpy array, by default False.

        Raises ``RuntimeError`` before ``train`` and on a model restored by ``load_model`` (it holds the training users' score
        matrix, not the item-item matrix), ``ValueError`` when ``rows`` has another width.
        """
        solver, X = self._fold_in(rows, "score_rows")
        ids = torch.arange(X.shape[0], dtype=torch.int32, device="cuda")
        pred = solver.scores(ids, X if remove_train else None, X=X)
        return pred if as_tensor else pred.cpu().numpy()

    def recommend_rows(self, rows, k=100, remove_train=True):
        r"""The ``k`` best items of ANY users (fold-in, see ``score_rows``) and their scores, on the device: ``(items,
        scores)``, device tensors ``[users, min(k, n_items)]`` (int32 / float64), score descending, item id ascending among equal
        scores; with ``remove_train`` the items stored in ``rows`` rank as :math:`-\infty`.  The chunk loop of ``recommend``."""
        return self._recommend_rows(rows, k, remove_train)

    def _recommend_rows(self, rows, k, remove_train, chunk=1024):
        if int(k) < 1:
            raise ValueError("recommend_rows: k must be >= 1, got %s" % (k,))
        solver, X = self._fold_in(rows, "recommend_rows")
        n = X.shape[0]
        ids = torch.arange(n, dtype=torch.int32, device="cuda")

        def score_chunk(lo, hi, out):
            return solver.scores(ids[lo:hi], None, out=out, X=X)

        def predict_chunk(lo, hi):                    # k above the kernel's 1024: masked on the device, sorted on the host
            return solver.scores(ids[lo:hi], X if remove_train else None, X=X, mask_rows=ids[lo:hi]).cpu().numpy()

        return self._lists(n, solver.n_items, k, chunk, score_chunk, X if remove_train else None, predict_chunk)

    def _state(self):
        """the dictionary ``save_model`` writes"""
        raise NotImplementedError()

    def _set_state(self, state):
        """takes what :meth:`_state` returned, read back from a file"""
        raise NotImplementedError()

    def save_model(self, filepath):
        state = self._state()
        logger.info("Saving %s model to %s...", type(self).__name__, filepath)
        np.save(filepath, state)
        logger.info("Model saved!")

    def load_model(self, filepath):
        assert os.path.isfile(filepath), "The model file %s does not exist." %filepath
        logger.info("Loading %s model from %s...", type(self).__name__, filepath)
        state = np.load(filepath, allow_pickle=True)[()]
        self._set_state(state)
        logger.info("Model loaded!")
        return state

    def _str_head(self):
        """``Class(hyper-parameters`` -- no closing bracket"""
        raise NotImplementedError()

    def _str_size(self):
        """what follows ``model size=`` for a fitted or loaded model, else None"""
        raise NotImplementedError()

    def __str__(self):
        size = self._str_size()
        return self._str_head() + (", model size=%s)" % size if size else ") - not trained yet!")

    def __repr__(self):
        return str(self)


class _ScoreMatrixModel(_FoldInModel):
    r"""The two models of the reference whose ``model`` is the training users' score matrix (EASE, ADMM_Slim).  Here the item-item
    matrix stays in HBM and ``predict`` multiplies the requested users' training rows by it on the device; ``model`` is materialised
    on the host only when it is read (``save_model`` does, to keep the file format).  A model restored by ``load_model`` holds that
    host matrix alone: ``predict`` and ``recommend`` are look-ups in it, as in the reference, and fold-in is refused."""
    _model = None      # host score matrix: only after ``model`` was read or ``load_model``

    def _score_matrix(self):
        """Every training user's score row of the device-resident model, as a host float64 matrix."""
        solver = self._solver
        n_users = solver.train.shape[0]
        out = np.empty((n_users, solver.n_items), dtype=np.float64)
        step = 8192
        for lo in range(0, n_users, step):
            hi = min(lo + step, n_users)
            out[lo:hi] = solver.scores(torch.arange(lo, hi, dtype=torch.int32)).cpu().numpy()
        return out

    @property
    def model(self):
        """The reference's score matrix -- EASE: **S** = X B; ADMM_Slim: X C (+ b with ``item_bias``) -- as a :class:`numpy.ndarray`
        (``None`` before training)."""
        if self._model is None and self._solver is not None:
            self._model = self._score_matrix()
        return self._model

    @model.setter
    def model(self, value):
        self._model = value
        self._solver = None

    def predict(self, ids_te_users, test_tr, remove_train=True, as_tensor=False):
        r"""Prediction, :math:`S_{u}=\mathbf{X}_{u,:} \cdot \mathbf{B}` (EASE: reference models.py:1028-1057; ADMM_Slim:
        models.py:1524-1529, with :math:`\mathbf{C}` and the item-bias row).

        Parameters
        ----------
        ids_te_users : array_like
            List of the test user indexes.
        test_tr : :class:`scipy.sparse.csr_matrix`
            Training portion of the test users.
        remove_train : :obj:`bool` [optional]
            Whether to set the scores of the items in ``test_tr`` to :math:`-\infty`, by default True.
        as_tensor : :obj:`bool` [optional]
            Return the float64 device tensor instead of copying it to a numpy array, by default False.

        Returns
        -------
        pred, : :obj:`tuple` with a single element
            The items' score (on the columns) for each user (on the rows).
        """
        if self._model is not None and self._solver is None:
            pred = self._model[ids_te_users, :]         # a loaded score matrix is a pure look-up, as in the reference
            if remove_train:
                pred[test_tr.nonzero()] = -np.inf
            return (torch.from_numpy(pred).to("cuda"), ) if as_tensor else (pred, )
        solver = self._require_solver("predict")
        mask = CsrMatrix(test_tr) if remove_train else None
        pred = solver.scores(ids_te_users, mask)
        return (pred, ) if as_tensor else (pred.cpu().numpy(), )

    def _recommend(self, ids_te_users, test_tr, k, remove_train, chunk=1024):
        if self._solver is not None or self._model is None or int(k) < 1:
            return super()._recommend(ids_te_users, test_tr, k, remove_train, chunk)
        ids_host = np.asarray(ids_te_users)             # a loaded score matrix: ``predict`` is a host look-up, sorted on the host
        return self._lists(len(ids_host), self._model.shape[1], k, chunk, None, None,
                           lambda lo, hi: self.predict(ids_host[lo:hi], test_tr[lo:hi], remove_train=remove_train)[0])

    def _fold_in(self, rows, what):
        if self._solver is None:    # a loaded host score matrix is no item-item matrix to multiply new rows by: as before ``train``
            raise RuntimeError("%s.%s needs the item-item matrix of a trained model: call train first (a model restored by load_model "
                               "holds only the training users' score matrix)" % (type(self).__name__, what))
        return super()._fold_in(rows, what)

    def _str_size(self):
        shape = self._solver.train.shape if self._solver is not None else self._model.shape if self._model is not None else None
        return None if shape is None else "(%d, %d)" % tuple(shape)


class EASE(_ScoreMatrixModel):
    r"""Embarrassingly Shallow AutoEncoder (reference rectorch/models.py:959-1069) solved on the MI355X.

    Same constructor, attributes and methods as the reference.  ``train`` computes the closed form
    :math:`B = P / (-\operatorname{diag} P),\ P = (X^\top X + \lambda I)^{-1},\ B_{ii} = 0` in float64 on the
    device (``rtx_ease_fit``: MFMA Gram matrix, blocked Cholesky, triangular inverse) and keeps ``B`` in HBM;
    ``predict`` multiplies the requested users' training rows by ``B`` on the device instead of looking them up
    in a materialised ``n_users x n_items`` score matrix.  ``model`` -- the reference's score matrix
    ``X B`` -- is materialised on the host only when it is read (``save_model`` does, to keep the file format).

    Parameters
    ----------
    lam : :obj:`float` [optional]
        The regularization hyper-parameter, by default 100.
    """
    def __init__(self, lam=100.):
        self.lam = lam

    def train(self, train_data):
        """Training of the EASE model (reference models.py:1006-1026).

        Parameters
        ----------
        train_data : :class:`scipy.sparse.csr_matrix`
            The training data.
        """
        logger.info("EASE - start tarining (lam=%.4f)", self.lam)
        self._model = None
        self._solver = EaseSolver(train_data, self.lam)
        logger.info("EASE - training complete")

    def _state(self):
        return {'lambda': self.lam,
                'model': self.model
               }

    def _set_state(self, state):
        self.lam = state["lambda"]
        self.model = state["model"]

    def _str_head(self):
        return "EASE(lambda=%.4f" % self.lam


class ADMM_Slim(_ScoreMatrixModel):
    r"""ADMM SLIM (reference rectorch/models.py:1389-1577) solved on the MI355X.

    Same constructor, attributes and methods as the reference.  ``train`` runs the reference's algorithm in float64 on the
    device (``rtx_admm_fit``): :math:`P = (X^\top X + (\lambda_2 + \rho) I)^{-1}` by EASE's pipeline, then
    ``num_iter`` ADMM iterations, each one MFMA GEMM :math:`P (\rho C - \Gamma)` with the element-wise steps fused into
    it; ``C`` stays in HBM.  ``predict`` multiplies the requested users' training rows by ``C`` on the device (plus the
    item-bias row with ``item_bias``) instead of looking them up in a materialised ``n_users x n_items`` score matrix.
    ``model`` -- the reference's score matrix -- is materialised on the host only when it is read (``save_model`` does,
    to keep the file format).

    Parameters
    ----------
    lambda1 : :obj:`float` [optional]
        Elastic net regularization hyper-parameters :math:`\lambda_1`, by default 5.
    lambda2 : :obj:`float` [optional]
        Elastic net regularization hyper-parameters :math:`\lambda_2`, by default 1e3.
    rho : :obj:`float` [optional]
        The penalty hyper-parameter :math:`\rho>0` that applies to :math:`\|B-C\|^2_F`, by default 1e5.
    nn_constr : :obj:`bool` [optional]
        Whether to keep the non-negativity constraint, by default ``True``.
    l1_penalty : :obj:`bool` [optional]
        Whether to keep the L1 penalty, by default ``True``.
    item_bias : :obj:`bool` [optional]
        Whether to model the item biases, by default ``False``.
    """
    def __init__(self,
                 lambda1=5.,
                 lambda2=1e3,
                 rho=1e5,
                 nn_constr=True,
                 l1_penalty=True,
                 item_bias=False):
        self.lambda1 = lambda1
        self.lambda2 = lambda2
        self.rho = rho
        self.nn_constr = nn_constr
        self.l1_penalty = l1_penalty
        self.item_bias = item_bias

    def train(self, train_data, num_iter=50, verbose=1):
        r"""Training of ADMM SLIM (reference models.py:1464-1522).

        Parameters
        ----------
        train_data : :class:`scipy.sparse.csr_matrix`
            The training data.
        num_iter : :obj:`int` [optional]
            Maximum number of training iterations, by default 50. This argument has no effect
            if both :attr:`nn_constr` and :attr:`l1_penalty` are set to ``False``.
        verbose : :obj:`int` [optional]
            The level of verbosity of the logging, by default 1.
        """
        self._model = None
        self._solver = None
        iterate = self.nn_constr or self.l1_penalty
        self._solver = AdmmSolver(train_data, self.lambda1, self.lambda2, self.rho, self.nn_constr, self.l1_penalty,
                                  self.item_bias, num_iter if iterate else 0)
        logger.info("ADMM_Slim - linear kernel computed")
        logger.info("ADMM_Slim - inverse of XtX computed")
        if iterate and num_iter > 0:
            log_delay = max(5, num_iter // (10 * verbose))
            for j in range(log_delay - 1, num_iter, log_delay):
                logger.info("| iteration %d/%d |", j + 1, num_iter)

    def _state(self):
        return {'lambda1': self.lambda1,
                'lambda2': self.lambda2,
                'rho' : self.rho,
                'model': self.model,
                'nn_constr' : self.nn_constr,
                'l1_penalty' : self.l1_penalty,
                'item_bias' : self.item_bias
               }

    def _set_state(self, state):
        self.lambda1 = state["lambda1"]
        self.lambda2 = state["lambda2"]
        self.rho = state["rho"]
        self.nn_constr = state["nn_constr"]
        self.l1_penalty = state["l1_penalty"]
        self.item_bias = state["item_bias"]
        self.model = state["model"]

    def _str_head(self):
        # "lamdba2" sic: the reference's spelling
        return ("ADMM_Slim(lambda1=%.4f, lamdba2=%.4f, rho=%.4f, non_negativity=%s, L1_penalty=%s, item_bias=%s"
                % (self.lambda1, self.lambda2, self.rho, self.nn_constr, self.l1_penalty, self.item_bias))


class ItemKNN(_FoldInModel):
    r"""Item-based k-nearest-neighbour top-N model, fitted and scored on the MI355X in float64.  (The reference has no ItemKNN;
    ``include/rectorch_hip.h`` holds the definition.)

    :math:`G = X^\top X`; for :math:`i \ne j` with :math:`G_{ij} > 0` the similarity is cosine,
    :math:`S_{ij} = G_{ij} / (\sqrt{G_{ii}} \sqrt{G_{jj}} + shrink)`, or jaccard, :math:`S_{ij} = G_{ij} / (G_{ii} + G_{jj} - G_{ij} +
    shrink)` (binary data only).  Every item :math:`j` keeps its ``k`` most similar items :math:`N_k(j)` (similarity descending, item
    id ascending among equal similarities); :math:`W_{ij} = S_{ij}` for :math:`i \in N_k(j)`, divided by the sum of the list's
    similarities with ``normalize``; scores are :math:`X W`.  ``W`` stays in HBM as a sparse matrix; the ``W`` property copies it
    to a :class:`scipy.sparse.csr_matrix` (rows = source items) on first read.

    Parameters
    ----------
    k : :obj:`int` [optional]
        Neighbours per item, 1 to 1024, by default 100.
    shrink : :obj:`float` [optional]
        The shrinkage term of the denominator, finite and >= 0, by default 0.
    similarity : :obj:`str` [optional]
        ``"cosine"`` or ``"jaccard"``, by default ``"cosine"``.
    normalize : :obj:`bool` [optional]
        Divide every item's neighbour weights by their sum, by default False.
    """
    def __init__(self, k=100, shrink=0.0, similarity="cosine", normalize=False):
        self._check_args(k, shrink, similarity)
        self.k = int(k)
        self.shrink = float(shrink)
        self.similarity = similarity
        self.normalize = bool(normalize)
        self._W = None          # host copy of W: only after ``W`` was read or ``load_model``

    @staticmethod
    def _check_args(k, shrink, similarity):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= _lib.KNN_MAX_K:
            raise ValueError("ItemKNN: k = %r is not supported; supported: an integer in [1, %d] (the device selection's limit)"
                             % (k, _lib.KNN_MAX_K))
        try:
            ok = np.isfinite(float(shrink)) and float(shrink) >= 0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("ItemKNN: shrink = %r is not supported; supported: a finite number >= 0" % (shrink,))
        if similarity not in _lib.KNN_SIMILARITIES:
            raise ValueError("ItemKNN: similarity = %r is not supported; supported: %s"
                             % (similarity, ", ".join("'%s'" % s for s in sorted(_lib.KNN_SIMILARITIES))))

    @property
    def W(self):
        """The item-item matrix as a float64 :class:`scipy.sparse.csr_matrix` ``[n_items, n_items]``, row = source item ``i``, column
        = scored item ``j`` (``None`` before training)."""
        if self._W is None and self._solver is not None:
            from scipy.sparse import csr_matrix
            indptr, indices, values = (t.cpu().numpy() for t in self._solver.weights())
            n = self._solver.n_items
            self._W = csr_matrix((values, indices, indptr), shape=(n, n))
        return self._W

    def train(self, train_data):
        """Fit on the training matrix (``rtx_knn_fit``).

        Parameters
        ----------
        train_data : :class:`scipy.sparse.csr_matrix`
            The training data (jaccard: binary).
        """
        logger.info("ItemKNN - start training (k=%d, shrink=%.4f, %s)", self.k, self.shrink, self.similarity)
        self._W = None
        self._solver = KnnSolver(train_data, self.k, self.shrink, self.similarity, self.normalize)
        logger.info("ItemKNN - training complete")

    def _require_train(self, what):
        solver = self._require_solver(what)
        if solver.train is None:
            raise RuntimeError("ItemKNN.%s looks users up in the training matrix, which a model restored by load_model does not hold: "
                               "pass the users' rows to score_rows / recommend_rows instead" % what)
        return solver

    def predict(self, ids_te_users, test_tr, remove_train=True, as_tensor=False):
        r"""Scores of training users, :math:`S_{u}=\mathbf{X}_{u,:} \cdot \mathbf{W}`; arguments and result as ``EASE.predict``.
        A model restored by ``load_model`` has no training matrix to look the users up in: ``RuntimeError`` (use ``score_rows``)."""
        solver = self._require_train("predict")
        mask = CsrMatrix(test_tr) if remove_train else None
        pred = solver.scores(ids_te_users, mask)
        return (pred, ) if as_tensor else (pred.cpu().numpy(), )

    def recommend(self, ids_te_users, test_tr, k=100, remove_train=True):
        """As :meth:`_FoldInModel.recommend`; refused like ``predict`` on a model restored by ``load_model``."""
        self._require_train("recommend")
        return self._recommend(ids_te_users, test_tr, k, remove_train)

    def _state(self):
        return {'k': self.k,
                'shrink': self.shrink,
                'similarity': self.similarity,
                'normalize': self.normalize,
                'W': self.W
               }

    def _set_state(self, state):
        self._check_args(state["k"], state["shrink"], state["similarity"])
        self.k = int(state["k"])
        self.shrink = float(state["shrink"])
        self.similarity = state["similarity"]
        self.normalize = bool(state["normalize"])
        self._W = state["W"].tocsr().astype(np.float64)
        self._solver = KnnSolver.from_csr(self._W)

    def _str_head(self):
        return "ItemKNN(k=%d, shrink=%.4f, similarity=%s, normalize=%s" % (self.k, self.shrink, self.similarity, self.normalize)

    def _str_size(self):
        s = self._solver
        return None if s is None else "(%d, %d), nnz=%d" % (s.n_items, s.n_items, s.nnz)


class WMF(_FoldInModel):
    r"""Weighted matrix factorisation for implicit feedback by alternating least squares (Hu, Koren, Volinsky 2008), fitted and
    scored on the MI355X in float64.  (The reference has no WMF; ``include/rectorch_hip.h`` holds the definition.)

    Confidence :math:`c_{ui} = 1 + \alpha r_{ui}` on the stored entries :math:`r_{ui} > 0`, preference 1 there and 0 elsewhere.  With
    item factors :math:`Y` a user's vector solves :math:`(Y^\top Y + \sum_{i \in I_u} \alpha r_{ui}\, y_i y_i^\top + \lambda I)\, x_u =
    \sum_{i \in I_u} (1 + \alpha r_{ui})\, y_i`; the item half-sweep is the same on the transposed matrix.  One iteration is a user
    half-sweep, then an item half-sweep.  Scores are :math:`x_u \cdot y_j`, and the vector of ANY user -- seen by the fit or not --
    is one such solve against the final item factors (fold-in), which is how every scoring method of this class obtains it.

    Parameters
    ----------
    factors : :obj:`int` [optional]
        Number of latent factors, 1 to 128, by default 64.
    alpha : :obj:`float` [optional]
        The confidence weight, finite and >= 0, by default 40.
    lam : :obj:`float` [optional]
        The regularisation, finite and > 0, by default 1.
    num_iter : :obj:`int` [optional]
        ALS iterations, >= 0, by default 15.
    seed : :obj:`int` [optional]
        Seed of the initial item factors, ``numpy.random.RandomState(seed).normal(0, 0.01, (n_items, factors))``, by default 98765.
    """
    def __init__(self, factors=64, alpha=40.0, lam=1.0, num_iter=15, seed=98765):
        self._check_args(factors, alpha, lam, num_iter)
        self.factors = int(factors)
        self.alpha = float(alpha)
        self.lam = float(lam)
        self.num_iter = int(num_iter)
        self.seed = seed
        self._Y = None          # host copies of the factor tables: only after they were read or ``load_model``
        self._U = None

    @staticmethod
    def _check_args(factors, alpha, lam, num_iter):
        if isinstance(factors, bool) or not isinstance(factors, (int, np.integer)) or not 1 <= int(factors) <= _lib.WMF_MAX_FACTORS:
            raise ValueError("WMF: factors = %r is not supported; supported: an integer in [1, %d] (the device solve's limit)"
                             % (factors, _lib.WMF_MAX_FACTORS))

        def number(v):
            try:
                return float(v) if np.isfinite(float(v)) else None
            except (TypeError, ValueError):
                return None
        if number(alpha) is None or number(alpha) < 0:
            raise ValueError("WMF: alpha = %r is not supported; supported: a finite number >= 0" % (alpha,))
        if number(lam) is None or number(lam) <= 0:
            raise ValueError("WMF: lam = %r is not supported; supported: a finite number > 0" % (lam,))
        if isinstance(num_iter, bool) or not isinstance(num_iter, (int, np.integer)) or int(num_iter) < 0:
            raise ValueError("WMF: num_iter = %r is not supported; supported: an integer >= 0" % (num_iter,))

    def train(self, train_data, verbose=1):
        """Fit on the training matrix (``rtx_wmf_fit``): ``num_iter`` iterations from the seeded initial item factors, drawn on the
        host in float64.

        Parameters
        ----------
        train_data : :class:`scipy.sparse.csr_matrix`
            The training data, users x items, stored values > 0.
        verbose : :obj:`int` [optional]
            The level of verbosity of the logging, by default 1.
        """
        logger.info("WMF - start training (factors=%d, alpha=%.4f, lam=%.4f, %d iterations)", self.factors, self.alpha, self.lam, self.num_iter)
        self._Y = self._U = None
        self._solver = None
        Y0 = np.random.RandomState(self.seed).normal(0, 0.01, (train_data.shape[1], self.factors))
        self._solver = WmfSolver(train_data, Y0, self.alpha, self.lam, self.num_iter)
        if verbose:
            t = self._solver.timings()
            logger.info("WMF - training complete (%.1f ms: Gram %.1f, user half %.1f, item half %.1f)", t["fit_ms"], t["gram_ms"],
                        t["user_ms"], t["item_ms"])

    @property
    def item_factors(self):
        """The item factors as a float64 :class:`numpy.ndarray` ``[n_items, factors]`` (``None`` before training)."""
        if self._Y is None and self._solver is not None:
            self._Y = self._solver.factors("items").cpu().numpy()
        return self._Y

    @property
    def user_factors(self):
        """The user factors of the last user half-sweep, ``[n_users, factors]`` (``None`` before training and for a model loaded
        from a file that stored none)."""
        if self._U is None and self._solver is not None and self._solver.n_users:
            self._U = self._solver.factors("users").cpu().numpy()
        return self._U

    def _check_users(self, ids_te_users, test_tr, what):
        self._require_solver(what)
        if len(np.asarray(ids_te_users)) != test_tr.shape[0]:
            raise ValueError("WMF.%s: %d user ids for %d rows of test_tr" % (what, len(np.asarray(ids_te_users)), test_tr.shape[0]))

    def predict(self, ids_te_users, test_tr, remove_train=True, as_tensor=False):
        r"""Scores of the given users; arguments and result as ``EASE.predict``.  Row ``b`` of ``test_tr`` is the history of user
        ``ids_te_users[b]``, and the prediction is the FOLD-IN of that row -- one user solve against the item factors, then
        :math:`x_u \cdot y_j` -- so it equals ``score_rows(test_tr)`` to the bit, whether or not the fit saw the user; the ids only
        have to match ``test_tr`` in number."""
        self._check_users(ids_te_users, test_tr, "predict")
        return (_FoldInModel.score_rows(self, test_tr, remove_train, as_tensor), )

    def recommend(self, ids_te_users, test_tr, k=100, remove_train=True):
        """As :meth:`_FoldInModel.recommend`, by fold-in of ``test_tr`` like ``predict``."""
        self._check_users(ids_te_users, test_tr, "recommend")
        return self._recommend_rows(test_tr, k, remove_train)

    def _state(self):
        return {'factors': self.factors,
                'alpha': self.alpha,
                'lam': self.lam,
                'num_iter': self.num_iter,
                'seed': self.seed,
                'item_factors': self.item_factors,
                'user_factors': self.user_factors
               }

    def _set_state(self, state):
        self._check_args(state["factors"], state["alpha"], state["lam"], state["num_iter"])
        Y = np.ascontiguousarray(state["item_factors"], dtype=np.float64)
        if Y.ndim != 2 or Y.shape[1] != int(state["factors"]):
            raise ValueError("WMF.load_model: the item factors have shape %s, expected (n_items, %d)" % (Y.shape, int(state["factors"])))
        self.factors = int(state["factors"])
        self.alpha = float(state["alpha"])
        self.lam = float(state["lam"])
        self.num_iter = int(state["num_iter"])
        self.seed = state["seed"]
        self._Y = Y
        self._U = None if state["user_factors"] is None else np.ascontiguousarray(state["user_factors"], dtype=np.float64)
        self._solver = WmfSolver.from_factors(Y, self.alpha, self.lam)

    def _str_head(self):
        return "WMF(factors=%d, alpha=%.4f, lambda=%.4f, num_iter=%d" % (self.factors, self.alpha, self.lam, self.num_iter)

    def _str_size(self):
        return None if self._solver is None else "(%d, %d)" % (self._solver.n_items, self.factors)


# the two list methods with the chunk size as an argument: tests/test_recommend_models.py and tests/test_item_item_eval.py pass a small
# one, to see several fills of the scratch buffer
def _recommend_item_item(model, ids_te_users, test_tr, k, remove_train, chunk=1024):
    return model._recommend(ids_te_users, test_tr, k, remove_train, chunk)


def _recommend_rows_item_item(model, rows, k, remove_train, chunk=1024):
    return model._recommend_rows(rows, k, remove_train, chunk)


class SVAE(MultiVAE):
    r"""Sequential Variational Autoencoders for Collaborative Filtering (reference models.py:1581-1635).

    One user sequence per optimizer step, as in the reference (several with ``SVAE_Sampler(pack=N)``, which is not: one
    Adam step for the mean loss of a pack of users): ``train_batch(x, y)`` with ``x`` the LongTensor
    ``[1, T]`` of the user's items and ``y`` the multi-hot targets ``[1, T, n_items]`` yielded by
    :class:`rectorch_amd.samplers.SVAE_Sampler` (or its compact :class:`rectorch_amd.engine.SvaeTarget`).  The whole
    step -- embedding, GRU, VAE head, decoder, loss, back-propagation through time, Adam with ``weight_decay=5e-3`` --
    is one call into librectorch_hip (``rtx_svae_train_step``), in float32.  A subclass with a ``loss_function`` of its own sets
    ``custom_loss = True`` and is trained with it (:meth:`_custom_step`: ``rtx_svae_forward_train`` -> the loss in torch ->
    ``rtx_svae_backward`` -> ``rtx_svae_apply_adam``), one ``[1, T]`` sequence per step.

    Parameters
    ----------
    svae_net : :class:`rectorch_amd.nets.SVAE_net`
    beta, anneal_steps, learning_rate
        As in :class:`MultiVAE`.
    numerics : "fp32" (default: the reference's arithmetic) or "bf16" -- every matrix product of the model with bf16 operands and
        float32 accumulation on the bf16 MFMA (what ``BASELINE.json`` ``configs[4]`` names); the GRU recurrences, the losses,
        the master weights and Adam stay float32.  Not in the reference's signature.
    """
    def __init__(self,
                 svae_net,
                 beta=1.,
                 anneal_steps=0,
                 learning_rate=1e-3,
                 numerics="fp32"):
        if numerics not in ("fp32", "bf16"):
            raise ValueError("numerics must be 'fp32' or 'bf16', got %r" % (numerics,))
        if getattr(svae_net, "_svae_engine", None) is not None and getattr(svae_net, "svae_numerics", "fp32") != numerics:
            svae_net._svae_engine = None          # built for the other arithmetic: rebuilt on first use
        svae_net.svae_numerics = numerics
        super(SVAE, self).__init__(svae_net,
                                   beta=beta,
                                   anneal_steps=anneal_steps,
                                   learning_rate=learning_rate,
                                   numerics="fp32",
                                   predict_numerics="fp32")
        self.optimizer = optim.Adam(self.network.parameters(),
                                    lr=learning_rate,
                                    weight_decay=5e-3)

    def loss_function(self, recon_x, x, mu, logvar, beta=1.0):
        r"""SVAE loss (reference models.py:1622-1626): :math:`\sum_t \mathrm{NLL}_t / d + \beta \cdot
        \mathrm{mean}_t \mathrm{KL}_t` with :math:`d` = ``sum(x[0, :n_items])`` -- all the ones of a ``[1, T, n_items]``
        target, but only those of the first time step when the target arrives flattened, as it does from
        ``train_batch``.  Computed by the HIP multinomial-loss kernel on the ``T`` rows."""
        T, n_items = recon_x.shape[1], recon_x.shape[2]
        d = float(torch.sum(x[0, :n_items]))
        y = x.reshape(T, n_items).to(recon_x.device, torch.float32)
        scale = T / d
        return scale * multinomial_loss(recon_x.reshape(T, n_items), y, mu, logvar, beta / scale)

    def train_batch(self, tr_batch, te_batch=None):
        r"""Training of a single sequence (reference models.py:817-835 with the SVAE loss and optimizer)."""
        if accum_spec(self.accumulate_grad_batches) > 1:
            raise _lib.RtxError("SVAE has no gradient accumulation: its packs are the batching it has (SVAE_Sampler's pack size); "
                                "%s" % _SUPPORTED_ACCUM)
        if self.custom_loss:
            return self._custom_step(tr_batch, te_batch)
        self._check_clip()
        _lib.require_gpu()
        if te_batch is None:
            raise ValueError("SVAE.train_batch needs the target sequence (SVAE_Sampler yields it)")
        st, params, m, v = self._ensure_train_state()
        pack = tr_batch if isinstance(tr_batch, SvaePack) else None
        T = pack.n_steps if pack is not None else int(tr_batch.numel())
        eng = self.network.svae_engine(T, train_buffers=(st.grads, m, v))
        if self.loss_mailbox and not getattr(eng, "_mailbox", False):
            eng.loss_mailbox(True)
        if pack is not None:
            d = 1.0           # every user's own normaliser travels with the pack's rows
        elif isinstance(te_batch, SvaeTarget):
            d = te_batch.d
        else:
            # the reference flattens the target to [1, T * n_items] before loss_function reads x[0, :n_items]
            d = float(te_batch.reshape(te_batch.shape[0], -1)[0, :eng.n_items].sum())
        if self.annealing:
            anneal_beta = min(self.beta, 1. * self.gradient_updates / self.anneal_steps)
        else:
            anneal_beta = self.beta
        spec = st.spec
        o = self._optim_step(eng, spec)
        from .nets import draw_seed
        noise = self._rtx.inject[1] if self._rtx.inject else None     # parity tests: eps captured from the reference's RNG
        step = _lib.Step()
        step.beta, step.lam = float(anneal_beta), 0.0
        step.inv_batch = (1.0 / d) if d != 0 else float("inf")
        step.lr, step.beta1, step.beta2 = o['lr'], o['beta1'], o['beta2']
        step.eps, step.weight_decay = o['eps'], o['weight_decay']
        step.step, step.flags = o['step'], 0
        step.seed, step.offset = draw_seed() & (2 ** 64 - 1), 0
        step.dropout_mask = None
        step.eps_noise = None if noise is None else noise.data_ptr()
        if pack is not None:
            # SVAE_Sampler(pack=N): ONE optimizer step for the mean of the pack's per-user losses (not in the reference)
            eng.train_pack(pack, step, anneal_beta, st.loss_buf[0:1], st.loss_buf[1:2])
        else:
            eng.train_step(tr_batch, te_batch, step, st.loss_buf[0:1], st.loss_buf[1:2])
        self._optim_stepped(spec)
        self.gradient_updates += 1.
        if getattr(eng, "_mailbox", False):
            return eng.wait_loss()        # this step's loss (models.py:835) from the host mailbox: the backward half of the step is still running
        return st.loss_buf[0].item()

    def _custom_step(self, x, target, want_loss=True):
        """One training step with ``custom_loss`` set: the reference's ``train_batch`` (models.py:817-835) with a subclass's own
        ``loss_function(recon [1, T, n_items], gt [1, T * n_items], mu, logvar, beta)`` -- the engine's forward with a ``grad_fn``
        (``rtx_svae_forward_train``), the loss in torch, ``loss.backward()`` through ``rtx_svae_backward``, then the fused step's
        Adam (``rtx_svae_apply_adam``) with the optimizer's hyper-parameters and moments.  One ``[1, T]`` sequence per step: a pack
        has no reference ``loss_function`` signature (packs stay available on :class:`rectorch_amd.engine.SvaeEngine`)."""
        self._require_own_loss()
        if isinstance(x, SvaePack):
            raise NotImplementedError("custom_loss = True trains one [1, T] sequence per step: a pack of users has no reference "
                                      "loss_function signature; SvaeEngine.forward_train / backward take packs")
        if target is None:
            raise ValueError("SVAE.train_batch needs the target sequence (SVAE_Sampler yields it)")
        self._check_clip()
        _lib.require_gpu()
        st = self._rtx
        net = self.network
        params = net._param_list()
        spec, m, v = self._ensure_optim_state(params)
        dev = params[0].device
        if st.loss_buf is None:
            st.loss_buf = torch.zeros(2, dtype=torch.float32, device=dev)
        T = int(x.numel())
        if isinstance(target, SvaeTarget):
            assert target.n_steps == T, "the target has %d steps, the sequence %d" % (target.n_steps, T)
            gt = torch.zeros((T, net.n_items), dtype=torch.float32, device=dev)
            rows = torch.repeat_interleave(torch.arange(T, device=dev), target.indptr[1:] - target.indptr[:-1])
            gt[rows, target.indices.long()] = 1.0
            gt = gt.view(1, -1)
        else:
            gt = target.reshape(target.shape[0], -1).to(dev, torch.float32)      # models.py:822: flattened to [1, T * n_items]
        if self.annealing:
            anneal_beta = min(self.beta, 1. * self.gradient_updates / self.anneal_steps)
        else:
            anneal_beta = self.beta
        noise = st.inject[1] if st.inject else None
        with torch.enable_grad():
            logits, mu, logvar = net._differentiable_forward(x, noise=noise, moments=(m, v))
            loss = self.loss_function(logits.view(x.shape[0], x.shape[1], -1), gt, mu, logvar, anneal_beta)
        for p in params:                      # optimizer.zero_grad(set_to_none=False): buffers that exist are kept -- after a fused
            if p.grad is not None:            # step they are views of its one flat buffer, which detach_() refuses
                if p.grad.grad_fn is not None:
                    p.grad.detach_()
                else:
                    p.grad.requires_grad_(False)
                p.grad.zero_()
        loss.backward()
        # optimizer.step(): the engine's Adam reads its bound gradient buffers -- p.grad (the engine's gradients plus whatever the
        # loss reaches the parameters with through torch) goes there first
        grads = net._diff_buffers()[0]
        eng = net.svae_engine(T, train_buffers=(grads, m, v))
        for gbuf, p in zip(grads, params):
            if p.grad is None:
                gbuf.zero_()
            else:
                gbuf.copy_(p.grad)
        o = self._optim_step(eng, spec)
        step = _lib.Step()
        step.lr, step.beta1, step.beta2 = o['lr'], o['beta1'], o['beta2']
        step.eps, step.weight_decay, step.step = o['eps'], o['weight_decay'], o['step']
        eng.apply_adam(step)
        self._optim_stepped(spec, write_step=True)
        self.gradient_updates += 1.
        loss = loss.detach().to(torch.float32)
        st.loss_buf[0] = loss
        st.loss_buf[1] += loss
        return loss.item() if want_loss else None

    def predict(self, x, remove_train=True):
        r"""Scores of the step after the sequence ``x`` (reference models.py:1628-1635): ``(recon_x[:, -1, :], mu,
        logvar)``; with ``remove_train`` the items of ``x`` are scored :math:`-\infty`.  The latent code is sampled
        (the reference's ``VAE_net._reparameterize`` has no eval branch): seed torch's generator for repeatable scores.

        ``x`` may also be a :class:`rectorch_amd.engine.SvaeEvalPack` (``SVAE_Sampler(is_training=False, pack=N)``; not in the
        reference): N users are scored in one call and the three results have N rows, one per user in the pack's order."""
        _lib.require_gpu()
        self.network.eval()
        from .nets import draw_seed
        noise = self._rtx.inject[1] if self._rtx.inject else None
        if isinstance(x, SvaeEvalPack):
            # SVAE_Sampler(is_training=False, pack=N): every user's last step in ONE call -- (scores [N, n_items], mu [N, latent],
            # logvar [N, latent]); the injected noise is [n_steps, latent], of which user u takes the row of its last step
            eng = self.network.svae_engine(x.n_steps)
            return eng.predict_pack(x, noise=noise, seed=draw_seed(), remove_train=remove_train)
        eng = self.network.svae_engine(int(x.numel()))
        _, last, mu, logvar = eng.forward(x, noise=noise, seed=draw_seed(), remove_train=remove_train, want_all=False)
        return last.view(1, -1), mu, logvar
