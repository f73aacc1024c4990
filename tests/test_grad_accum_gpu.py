"""GPU (-m gpu): gradient accumulation on the device -- ``model.accumulate_grad_batches = k``, the accumulating epilogues of the
weight-gradient kernels, ``apply_accumulated`` and the bookkeeping around a window.

References.  A window is judged against the device's OWN per-micro-step gradients, taken on the plain-store path: a second model
with the same parameters and the same injected dropout masks / eps, attribute left at 1, trained with ``SGD(lr=0)`` (its
parameters do not move; the unfused schedule stores ``p.grad``).  Inputs, masks and eps are those of the clipping fixtures
(tests/golden/g18_clip_*.npz), micro-batch t cut to ``B - t`` rows so that the micro-batches of a window differ in size.

Bounds.  The accumulators see ``s g_1`` and then one ``fma(s, g_i, acc)`` per further micro-step with ``s = float32(1 / k)``: one
rounding each, of a partial sum no larger than ``sum_i |s g_i|`` -- element-wise ``|acc - sum_i s g_i| <= k 2^-24 sum_i |s g_i|``
against the float64 sum with the same float32 ``s``.  The update: the float64 clip + rule on the accumulated ``p.grad`` the
device holds, with the one-update bound of test_grad_clip_gpu.assert_clipped_update.  Micro-steps that apply nothing leave
parameters, optimizer states and step counts bit-equal.  A model that ignores the attribute moves its parameters at the first
call of a window and fails the same checks (test_ignoring_the_attribute_fails_the_window_checks).
"""
import numpy as np
import pytest
import torch
import torch.optim as optim

from conftest import load_golden
import optim_rules64 as R
from test_grad_clip_host import CONFIGS, FIXTURES, E24
from test_grad_clip_gpu import build, set_clip, assert_clipped_update, assert_norm
from test_optimizers_gpu import dev, host, loss_grads, snapshot, assert_one_update, rel

pytestmark = pytest.mark.gpu

WINDOW_CONFIGS = ["adam_norm", "sgdmom_norm", "rmsprop_value", "adagrad_norm", "adam_norm_loose"]


@pytest.fixture(scope="module", autouse=True)
def _require_native_path():
    from rectorch_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()


def test_native_driver_accum():
    """the accumulating epilogues alone, bit for bit against the host's scale * g and fmaf: every dw tile configuration, a grouped
    launch of three, the float32 epilogue and the split-slab reduce, guard bands, no leak of the mode (tests/native/test_accum.cpp)"""
    import os
    import subprocess
    from conftest import ROOT
    path = os.path.join(ROOT, "build", "native", "test_accum")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-s", "-f", "accum.mk"])
    out = subprocess.run([path], capture_output=True, text=True, timeout=600)
    print(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "ACCUM TESTS PASSED" in out.stdout


def micro(g, t, rows=None):
    """micro-batch t of a fixture: (x, keep-mask, eps), cut to ``rows`` rows (default B - t)"""
    n = g["xs"].shape[1] - t if rows is None else rows
    eps = dev(g["eps_%d" % t][:n]) if "eps_%d" % t in g else None
    return torch.from_numpy(g["xs"][t][:n]), dev(g["mask_%d" % t][:n], torch.uint8), eps


def reference_model(g, cfg, numerics, builder=None):
    """the plain-store side: same parameters, attribute at 1, an optimizer that moves nothing and stores every gradient"""
    net, ref = (builder or build)(g, cfg, numerics)
    ref.accumulate_grad_batches = 1
    ref.optimizer = optim.SGD(net.parameters(), lr=0.0)
    set_clip(ref, None)
    return ref


def micro_gradient(ref, model, x, mask, eps):
    """(loss, gradients) of one micro-batch at the window's parameters and the window's annealed beta"""
    if hasattr(model, "gradient_updates"):
        ref.gradient_updates = model.gradient_updates
    ref._rtx.inject = (mask, eps)
    loss = ref.train_batch(x)
    return loss, [host(p.grad) for p in ref.network._param_list()]


def run_window(tag, g, cfg, model, ref, ts, k, t_update, partial=False, unclipped=False, configs=None, batch=None):
    """one window of the micro-batches ``ts`` (k = model.accumulate_grad_batches; ``partial``: fewer than k, closed by
    apply_accumulated) with every check of this file's docstring; ``t_update``: the optimizer's step count the window ends with;
    ``unclipped``: the model's clip attributes were unset; ``configs`` / ``batch``: another table of configurations and another
    source of micro-batches than the clipping fixtures' (the g19 fixtures)"""
    cls, kw, clip = (configs or CONFIGS)[cfg]
    clip = None if unclipped else clip
    lam = float(g["model__lam"]) if "model__lam" in g else 0.0
    net = model.network
    before, states = snapshot(model, cls, kw)      # (before the first update the optimizer has no state: the rule's own first step)
    updates0 = getattr(model, "gradient_updates", None)
    norm0 = model.last_grad_norm if t_update > 1 else None
    s = float(np.float32(1.0 / k))
    want = [np.zeros_like(b) for b in before]
    scale = [np.zeros_like(b) for b in before]
    for j, t in enumerate(ts):
        x, mask, eps = (batch or micro)(g, t)
        ref_loss, gi = micro_gradient(ref, model, x, mask, eps)
        for a, b, c in zip(want, scale, gi):
            a += s * c
            b += np.abs(s * c)
        model._rtx.inject = (mask, eps)
        loss = model.train_batch(x)
        assert isinstance(loss, float) and loss == ref_loss, (tag, t, loss, ref_loss)      # THIS micro-batch's loss, unscaled
        applies = (j + 1 == k)
        if not applies:
            now, states_now = snapshot(model, cls, kw)
            assert all(np.array_equal(a, b) for a, b in zip(now, before)), (tag, t, "a micro-step moved the parameters")
            for sa, sb in zip(states_now, states):
                assert all(np.array_equal(sa[key], sb[key]) for key in sb), (tag, t, "a micro-step touched the optimizer state")
            assert model._rtx.adam_step == t_update - 1 and model.pending_micro_batches == j + 1, (tag, t)
            assert getattr(model, "gradient_updates", None) == updates0, (tag, t)
            if t_update > 1:
                assert model.last_grad_norm == norm0, (tag, t)
    if partial:
        assert model.pending_micro_batches == len(ts)
        assert model.apply_accumulated() is True
    assert model.pending_micro_batches == 0 and model._rtx.adam_step == t_update
    if updates0 is not None:
        assert model.gradient_updates == updates0 + 1
    # the accumulated gradient: p.grad keeps it, unclipped
    # (Mult-DAE's regulariser is part of every micro-step's loss: a partial window holds len(ts) of k terms of its gradient)
    grads, regs = loss_grads(model, before, lam * len(ts) / k if partial else lam)
    for i, (got, w, sc) in enumerate(zip(grads, want, scale)):
        bound = k * E24 * sc
        assert np.all(np.abs(got - w) <= bound), (tag, i, float(np.max(np.abs(got - w) / np.maximum(bound, 1e-300))))
    assert_norm(tag, model, grads, regs, clip)
    worst = assert_clipped_update(tag, model, cls, kw, clip, t_update, before, states, grads, regs)
    moved = [float(np.max(np.abs(host(p) - b))) for p, b in zip(net._param_list(), before)]
    assert all(m > 0 for m in moved), (tag, moved)
    # the reference side follows: same parameters for the next window
    with torch.no_grad():
        for pr, p in zip(ref.network._param_list(), net._param_list()):
            pr.copy_(p)
    return worst


@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("cfg", WINDOW_CONFIGS)
def test_windows(name, cfg, numerics):
    """two full windows of k = 3 micro-batches of unequal sizes, then a partial window of 2 closed by apply_accumulated"""
    g = load_golden(name)
    net, model = build(g, cfg, numerics, predict_numerics=numerics)
    ref = reference_model(g, cfg, numerics)
    model.accumulate_grad_batches = 3
    tag = "%s %s %s" % (name, cfg, numerics)
    worst = max(run_window(tag + " window 1", g, cfg, model, ref, [0, 1, 2], 3, 1),
                run_window(tag + " window 2", g, cfg, model, ref, [2, 0, 1], 3, 2),
                run_window(tag + " partial", g, cfg, model, ref, [1, 2], 3, 3, partial=True))
    assert model.apply_accumulated() is False
    print("%s: worst update error / bound = %.4f" % (tag, worst))
    # the compute copies were refreshed by the window's optimizer launch: predict at the training numerics equals, bit for bit, the
    # predict of a fresh engine built from the float32 masters
    model._rtx.inject = None
    x = torch.from_numpy(g["xs"][0])
    pred = model.predict(x, remove_train=False)[0]
    fresh_net, fresh = build(g, cfg, numerics, predict_numerics=numerics)
    fresh_net.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
    assert torch.equal(pred, fresh.predict(x, remove_train=False)[0])
    assert not torch.equal(pred, build(g, cfg, numerics, predict_numerics=numerics)[1].predict(x, remove_train=False)[0])


def test_ignoring_the_attribute_fails_the_window_checks():
    """what fails without the feature: the same calls on a model whose attribute is left at 1 update at every call"""
    g = load_golden(FIXTURES[0])
    net, model = build(g, "sgdmom_norm", "fp32")
    ref = reference_model(g, "sgdmom_norm", "fp32")
    assert model.accumulate_grad_batches == 1
    with pytest.raises(AssertionError, match="a micro-step moved the parameters"):
        run_window("attribute ignored", g, "sgdmom_norm", model, ref, [0, 1, 2], 3, 1)


@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
def test_same_batch_twice_is_exact(numerics):
    """k = 2 with the same micro-batch and mask twice: 0.5 g + 0.5 g is exact, so p.grad is bit-equal to the single stored gradient;
    in float32 parameters and states are bit-equal to one k = 1 step on that batch"""
    g = load_golden(FIXTURES[0])
    cfg = "adam_norm"
    cls, kw, clip = CONFIGS[cfg]
    net, model = build(g, cfg, numerics)
    net1, one = build(g, cfg, numerics)
    x, mask, eps = micro(g, 0)
    model.accumulate_grad_batches = 2
    for _ in range(2):
        model._rtx.inject = (mask, eps)
        model.train_batch(x)
    one._rtx.inject = (mask, eps)
    one.train_batch(x)
    for p, q in zip(net._param_list(), net1._param_list()):
        assert torch.equal(p.grad, q.grad)
        if numerics == "fp32":
            assert torch.equal(p.data, q.data)
            for key in R.state_keys(cls, kw):
                assert torch.equal(model.optimizer.state[p][key], one.optimizer.state[q][key]), key


def test_equal_split_fp32():
    """float32, dropout off: one step on 8 rows and a window of k = 4 micro-batches of 2 rows agree (every loss is a mean over the
    batch) to the float32 parity bounds -- gradients 2e-4, parameters within 5e-3 of the step's largest move; two runs of the window
    are bit-equal"""
    g = load_golden(FIXTURES[0])
    x = torch.from_numpy(np.concatenate([g["xs"][0], g["xs"][1]])[:8])
    ones = torch.ones(x.shape, dtype=torch.uint8, device="cuda")
    eps = dev(np.concatenate([g["eps_0"], g["eps_1"]])[:8])

    def run(k):
        net, model = build(g, "adam_norm", "fp32")
        before = [host(p) for p in net._param_list()]
        model.accumulate_grad_batches = k
        n = 8 // k
        for j in range(k):
            model._rtx.inject = (ones[j * n:(j + 1) * n], None if eps is None else eps[j * n:(j + 1) * n])
            model.train_batch(x[j * n:(j + 1) * n])
        return before, [host(p) for p in net._param_list()], [host(p.grad) for p in net._param_list()]

    before, p1, g1 = run(1)
    _, p4, g4 = run(4)
    _, p4b, g4b = run(4)
    for i in range(len(p1)):
        assert np.array_equal(p4[i], p4b[i]) and np.array_equal(g4[i], g4b[i]), i
        assert np.max(np.abs(g4[i] - g1[i])) <= 2e-4 * np.max(np.abs(g1[i])), i
        move = float(np.max(np.abs(p1[i] - before[i])))
        assert move > 0 and np.max(np.abs(p4[i] - p1[i])) <= 5e-3 * move, (i, move)


def _timing_names(eng):
    """the kernel sites the engine launched since the last call"""
    return sorted(name for name, (ms, n) in eng.get_timings().items() if n > 0)


def test_k1_is_untouched_bf16():
    """accumulate_grad_batches = 1: three fused bf16 steps are bit-equal to a model whose attribute was never assigned, and the
    engine launched the same kernel sites (the fused Adam epilogues, no accumulating site, no separate optimizer launch)"""
    g = load_golden(FIXTURES[0])
    outs, sites = [], []
    for assign in (False, True):
        net, model = build(g, "adam_norm", "bf16")
        set_clip(model, None)
        model.optimizer = optim.Adam(net.parameters(), lr=1e-2)
        if assign:
            model.accumulate_grad_batches = 1
        losses = []
        for t in range(3):
            x, mask, eps = micro(g, t, rows=g["xs"].shape[1])
            model._rtx.inject = (mask, eps)
            if t == 0:
                losses.append(model.train_batch(x))
                eng = next(iter(net._rtx_engines.values()))
                eng.set_timing(None, True)
            else:
                losses.append(model.train_batch(x))
        names = _timing_names(eng)
        outs.append((losses, [p.detach().clone() for p in net._param_list()]))
        sites.append(names)
    assert outs[0][0] == outs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    assert sites[0] == sites[1], (sites[0], sites[1])
    assert any(s.startswith("dW_adam") for s in sites[1]) and not any(s.endswith("_acc") or s == "adam" for s in sites[1]), sites[1]


def test_accumulating_sites_and_toggling_bf16():
    """k = 1 fused -> a window of 3 -> k = 1 fused again on one bf16 model: the window runs the accumulating weight kernels and one
    optimizer launch, the steps around it the fused epilogues; every update, fused or window, is judged by the update-alone bound"""
    g = load_golden(FIXTURES[0])
    cfg = "adam_norm_loose"
    cls, kw, clip = CONFIGS[cfg]
    net, model = build(g, cfg, "bf16")
    set_clip(model, None)
    model.keep_grads = True
    ref = reference_model(g, cfg, "bf16")
    B = g["xs"].shape[1]

    def fused_step(t, t_update):
        model._ensure_train_state()
        before, states = snapshot(model, cls, kw)
        x, mask, eps = micro(g, t, rows=B)
        model._rtx.inject = (mask, eps)
        model.train_batch(x)
        assert model._rtx.adam_step == t_update and model.pending_micro_batches == 0
        # the update alone: the float64 rule on the gradient the fused step kept (keep_grads), the one-update bound
        grads = [host(p.grad) for p in net._param_list()]
        assert_one_update("fused step %d" % t_update, model, cls, kw, t_update, before, states, grads)
        with torch.no_grad():
            for pr, p in zip(ref.network._param_list(), net._param_list()):
                pr.copy_(p)

    fused_step(0, 1)
    eng = next(iter(net._rtx_engines.values()))
    eng.set_timing(None, True)
    eng.get_timings()
    model.accumulate_grad_batches = 3
    run_window("toggled window", g, cfg, model, ref, [0, 1, 2], 3, 2, unclipped=True)
    names = _timing_names(eng)
    assert any(s.endswith("_acc") for s in names) and "adam" in names and not any(s.startswith("dW_adam") for s in names), names
    model.accumulate_grad_batches = 1
    fused_step(1, 3)
    names = _timing_names(eng)
    assert any(s.startswith("dW_adam") for s in names) and not any(s.endswith("_acc") for s in names), names


@pytest.mark.parametrize("mailbox", [True, False])
def test_each_micro_step_returns_its_own_loss(mailbox):
    """the micro-steps of a window share the optimizer's step number; train_batch still returns each one's own loss"""
    g = load_golden(FIXTURES[0])
    net, model = build(g, "adam_norm", "fp32")
    ref = reference_model(g, "adam_norm", "fp32")
    model.loss_mailbox = mailbox
    model.accumulate_grad_batches = 3
    got, want = [], []
    for t in range(3):
        x, mask, eps = micro(g, t)
        want.append(micro_gradient(ref, model, x, mask, eps)[0])
        model._rtx.inject = (mask, eps)
        got.append(model.train_batch(x))
    assert got == want and len(set(got)) == 3, (got, want)


def test_train_epoch_applies_partial_window_and_save_model_refuses_open_window(tmp_path):
    """7 batches with k = 3: three updates (3 + 3 + 1), no open window afterwards; save_model raises inside a window"""
    from scipy.sparse import csr_matrix
    from rectorch_amd import _lib
    from rectorch_amd.samplers import DataSampler
    g = load_golden(FIXTURES[0])
    net, model = build(g, "adam_norm", "bf16")
    rows = np.concatenate([g["xs"][t] for t in range(g["xs"].shape[0])])[:14]
    smp = DataSampler(csr_matrix(rows), batch_size=2, shuffle=False)
    assert len(smp) == 7
    model.accumulate_grad_batches = 3
    model.train_epoch(1, smp, verbose=0)
    torch.cuda.synchronize()
    assert model._rtx.adam_step == 3 and model.pending_micro_batches == 0
    assert model.gradient_updates == 3.0
    model.train_batch(torch.from_numpy(rows[:4]))
    assert model.pending_micro_batches == 1
    with pytest.raises(_lib.RtxError, match="apply_accumulated"):
        model.save_model(str(tmp_path / "open.pth"), 1)
    model.accumulate_grad_batches = 2
    with pytest.raises(_lib.RtxError, match="changed"):
        model.train_batch(torch.from_numpy(rows[:4]))
    model.accumulate_grad_batches = 3
    assert model.apply_accumulated() is True
    model.save_model(str(tmp_path / "closed.pth"), 1)


def _other_trainer(kind):
    from rectorch_amd.nets import VAE_net, MultiDAE_net
    from rectorch_amd.models import VAE, AETrainer
    torch.manual_seed(5)
    if kind == "vae":
        net = VAE_net([8, 24, 70], [70, 24, 8])
        return net, VAE(net, numerics="fp32")
    net = MultiDAE_net([12, 24, 70], [70, 24, 12], dropout=0.0)
    return net, AETrainer(net, numerics="fp32")


@pytest.mark.parametrize("kind", ["vae", "ae"])
def test_other_trainers_fp32(kind):
    """one window of k = 2 for VAE(VAE_net) and AETrainer(MultiDAE_net) in float32: micro-steps move nothing, the update is Adam's
    float64 rule on the accumulated p.grad, and that gradient is the sum of the two halves' own"""
    cls, kw = "Adam", dict(lr=1e-3)
    net, model = _other_trainer(kind)
    net_r, ref = _other_trainer(kind)
    net_r.load_state_dict(net.state_dict())
    ref.optimizer = optim.SGD(net_r.parameters(), lr=0.0)
    rng = np.random.default_rng(3)
    xs = [torch.from_numpy((rng.random((n, 70)) < 0.2).astype(np.float32)) for n in (6, 5)]
    eps = [dev(rng.standard_normal((x.shape[0], 8)).astype(np.float32)) for x in xs]
    model.accumulate_grad_batches = 2
    model._ensure_train_state()
    before, states = snapshot(model, cls, kw)
    want = [np.zeros_like(b) for b in before]
    scale = [np.zeros_like(b) for b in before]
    for j, x in enumerate(xs):
        inj = (torch.ones(x.shape, dtype=torch.uint8, device="cuda"), eps[j] if kind == "vae" else None)
        ref._rtx.inject = inj
        ref_loss = ref.train_batch(x)
        for a, b, p in zip(want, scale, net_r._param_list()):
            a += 0.5 * host(p.grad)
            b += np.abs(0.5 * host(p.grad))
        model._rtx.inject = inj
        assert model.train_batch(x) == ref_loss
        if j == 0:
            assert all(np.array_equal(host(p), b) for p, b in zip(net._param_list(), before))
    grads = [host(p.grad) for p in net._param_list()]
    for got, w, sc in zip(grads, want, scale):
        assert np.all(np.abs(got - w) <= 2 * E24 * sc)
    assert_clipped_update(kind, model, cls, kw, None, 1, before, states, grads)


def test_cmvae_resident_conditioned_sampler_window():
    """CMultiVAE on a resident conditioned sampler, float32: one window of k = 2 over the sampler's first two device-built batches,
    judged by the update-alone bound against the sum of the two batches' own plain-store gradients; then an epoch with k = 2 applies
    ceil(batches / 2) updates and leaves no open window"""
    from scipy.sparse import csr_matrix
    from rectorch_amd.nets import CMultiVAE_net
    from rectorch_amd.models import CMultiVAE
    from rectorch_amd.samplers import ConditionedDataSampler
    rng = np.random.default_rng(11)
    n_items, n_cond, users = 60, 3, 24
    tr = csr_matrix((rng.random((users, n_items)) < 0.2).astype(np.float32))
    iid2cids = {i: [int(i % n_cond)] for i in range(n_items)}
    cls, kw = "Adam", dict(lr=1e-3)

    def make():
        torch.manual_seed(1)
        net = CMultiVAE_net(n_cond, [8, 16, n_items], dropout=0.0)
        return net, CMultiVAE(net, beta=0.2, anneal_steps=0, numerics="fp32")
    net, model = make()
    net_r, ref = make()
    ref.optimizer = optim.SGD(net_r.parameters(), lr=0.0)
    smp = ConditionedDataSampler(iid2cids, n_cond, tr, None, batch_size=16, shuffle=False, resident=True)
    model.accumulate_grad_batches = 2
    before, states = snapshot(model, cls, kw)
    want = [np.zeros_like(b) for b in before]
    scale = [np.zeros_like(b) for b in before]
    it = smp.iter_rows()
    for j in range(2):
        item = next(it)
        eps = dev(rng.standard_normal((len(item), 8)).astype(np.float32))
        ref._rtx.inject = (None, eps)
        ref_loss = ref._fused_step(item, None, want_loss=True)
        for a, b, p in zip(want, scale, net_r._param_list()):
            a += 0.5 * host(p.grad)
            b += np.abs(0.5 * host(p.grad))
        model._rtx.inject = (None, eps)
        assert model._fused_step(item, None, want_loss=True) == ref_loss
        if j == 0:
            assert all(np.array_equal(host(p), b) for p, b in zip(net._param_list(), before)) and model.pending_micro_batches == 1
    del it
    grads = [host(p.grad) for p in net._param_list()]
    for got, w, sc in zip(grads, want, scale):
        assert np.all(np.abs(got - w) <= 2 * E24 * sc)
    assert any(np.max(np.abs(x)) > 0 for x in grads)
    assert_clipped_update("cmvae window", model, cls, kw, None, 1, before, states, grads)
    model._rtx.inject = ref._rtx.inject = None
    model.train_epoch(1, smp, verbose=0)
    torch.cuda.synchronize()
    assert model._rtx.adam_step == 1 + (len(smp) + 1) // 2 and model.pending_micro_batches == 0


def test_refusals_raise_before_any_launch():
    from rectorch_amd import _lib
    g = load_golden(FIXTURES[0])
    x, mask, eps = micro(g, 0)
    for bad in (0, 2.5, True, "3"):
        net, model = build(g, "adam_norm", "fp32")
        before = [p.detach().clone() for p in net._param_list()]
        model.accumulate_grad_batches = bad
        with pytest.raises(ValueError, match="int >= 1"):
            model.train_batch(x)
        assert all(torch.equal(p, b) for p, b in zip(net._param_list(), before)) and not net._rtx_engines
    net, model = build(g, "adam_norm", "fp32")
    model.accumulate_grad_batches = 2
    model._rtx.reducer = object()
    with pytest.raises(_lib.RtxError, match="data-parallel"):
        model.train_batch(x)
    assert not net._rtx_engines
    model._rtx.reducer = None
    from rectorch_amd import parallel
    set_clip(model, None)
    with pytest.raises(_lib.RtxError, match="gradient accumulation"):
        parallel.attach(model, emulate_world=2)
    set_clip(model, CONFIGS["adam_norm"][2])
    # the engine's own entry points
    model.train_batch(x)
    eng = next(iter(net._rtx_engines.values()))
    assert model.apply_accumulated() is True
    with pytest.raises(_lib.RtxError, match="RTX_ACCUM_FIRST"):
        eng.set_grad_accum(_lib.RTX_ACCUM_ADD, 0.5)        # nothing accumulated since the update
    with pytest.raises(_lib.RtxError):
        eng.set_grad_accum(7, 0.5)
    with pytest.raises(_lib.RtxError, match="finite"):
        eng.set_grad_accum(_lib.RTX_ACCUM_FIRST, float("inf"))


def test_svae_refuses():
    from rectorch_amd import _lib
    from rectorch_amd.nets import SVAE_net
    from rectorch_amd.models import SVAE
    net = SVAE_net(n_items=40, embed_size=8, rnn_size=8, dec_dims=[4, 8, 40], enc_dims=[8, 8, 4])
    model = SVAE(net)
    model.accumulate_grad_batches = 2
    with pytest.raises(_lib.RtxError, match="packs"):
        model.train_batch(torch.zeros(1, 3, dtype=torch.long), torch.zeros(1, 3, 40))


# ------------------------------------------------------------------------------- the recorded torch windows (g19_accum_*.npz)
from test_grad_accum_host import G19, G19_FIXTURES, G19_CONFIGS      # noqa: E402
from conftest import sd_from, params_in_order                         # noqa: E402


def build19(g, cfg, numerics, model_cls=None, **kw):
    """the fixture's network and trainer with the configuration's optimizer and clip attributes, k = 3"""
    from rectorch_amd.nets import MultiVAE_net, MultiDAE_net
    from rectorch_amd.models import MultiVAE, MultiDAE
    enc, dec = [int(v) for v in g["enc_dims"]], [int(v) for v in g["dec_dims"]]
    sd = {k: torch.from_numpy(np.array(v)) for k, v in sd_from(g, "sd0__").items()}
    if "model__lam" in g:
        net = MultiDAE_net(dec, enc, dropout=float(g["dropout"]))
        net.load_state_dict(sd)
        model = (model_cls or MultiDAE)(net, lam=float(g["model__lam"]), numerics=numerics, **kw)
    else:
        net = MultiVAE_net(dec, enc, dropout=float(g["dropout"]))
        net.load_state_dict(sd)
        model = (model_cls or MultiVAE)(net, beta=float(g["model__beta"]), anneal_steps=int(g["model__anneal_steps"]), numerics=numerics, **kw)
    cls, okw, clip = G19_CONFIGS[cfg]
    model.optimizer = getattr(optim, cls)(net.parameters(), **okw)
    set_clip(model, clip)
    model.accumulate_grad_batches = int(g["k"])
    return net, model


def parity19(g, cfg, model, net, tag):
    """the recorded torch loop against the device: every micro-batch's loss 1e-5 relative; per window the accumulated gradient 2e-4,
    parameters and states within 5e-3 x the reference's largest move (the bounds of test_fixture_parity_fp32); micro-steps that
    apply nothing leave parameters, states and step counts bit-equal; the partial window goes through apply_accumulated()"""
    cls, kw, clip = G19_CONFIGS[cfg]
    k = int(g["k"])
    keys = params_in_order(sd_from(g, "sd0__"))[1]
    lam = float(g["model__lam"]) if "model__lam" in g and not model.custom_loss else 0.0
    prev = [g["sd0__" + key.replace(".", "__")].astype(np.float64) for key in keys]
    prev_state = [R.init_state(cls, kw, p) for p in prev]
    worst = 0.0
    for w, window in enumerate(G19.WINDOWS):
        before, states = snapshot(model, cls, kw)
        for n, j in enumerate(window):
            model._rtx.inject = (dev(g["mask_%d" % j], torch.uint8), dev(g["eps_%d" % j]) if "eps_%d" % j in g else None)
            loss = model.train_batch(torch.from_numpy(g["x_%d" % j]))
            want = float(g["%s__loss_%d" % (cfg, j)])
            assert isinstance(loss, float) and abs(loss - want) < 1e-5 * abs(want), (tag, j, loss, want)
            if n + 1 < k:
                now, states_now = snapshot(model, cls, kw)
                assert all(np.array_equal(a, b) for a, b in zip(now, before)), (tag, j, "a micro-step moved the parameters")
                for sa, sb in zip(states_now, states):
                    assert all(np.array_equal(sa[key], sb[key]) for key in sb), (tag, j, "a micro-step touched the optimizer state")
                assert model._rtx.adam_step == w and model.pending_micro_batches == n + 1, (tag, j)
                if model.custom_loss:          # (this route writes optimizer.state's step at every update: untouched inside a window)
                    assert all(float(model.optimizer.state[p]["step"]) == w for p in net._param_list() if "step" in model.optimizer.state.get(p, {}))
        if len(window) < k:
            assert model.apply_accumulated() is True
        assert model.pending_micro_batches == 0 and model._rtx.adam_step == w + 1
        stored, regs = loss_grads(model, before, lam * len(window) / k)
        grads = [a + b for a, b in zip(stored, regs)]
        if clip and "value" not in clip:
            ref_total = float(g["%s__total_norm_%d" % (cfg, w)])
            assert abs(model.last_grad_norm - ref_total) < 2e-4 * ref_total, (tag, w, model.last_grad_norm, ref_total)
        for i, (key, prm) in enumerate(zip(keys, net._param_list())):
            kk = key.replace(".", "__")
            assert rel(grads[i], g["%s__grad_%d__%s" % (cfg, w, kk)]) < 2e-4, (tag, w, key)
            ref = g["%s__sd_%d__%s" % (cfg, w, kk)].astype(np.float64)
            move = float(np.max(np.abs(ref - prev[i])))
            err = float(np.max(np.abs(host(prm) - ref)))
            worst = max(worst, err / (5e-3 * move))
            assert err <= 5e-3 * move, (tag, w, key, err, move)
            for s in R.state_keys(cls, kw):
                ref_s = g["%s__%s_%d__%s" % (cfg, s, w, kk)].astype(np.float64)
                s_move = float(np.max(np.abs(ref_s - prev_state[i].get(s, 0.0))))
                s_err = float(np.max(np.abs(host(model.optimizer.state[prm][s]) - ref_s)))
                assert s_err <= 5e-3 * s_move, (tag, w, key, s, s_err, s_move)
                prev_state[i][s] = ref_s
            prev[i] = ref
    model._rtx.inject = None
    return worst


@pytest.mark.parametrize("name", G19_FIXTURES)
@pytest.mark.parametrize("cfg", sorted(G19_CONFIGS))
def test_fixture_parity_fp32(name, cfg):
    """the reference's networks and loss_functions inside torch's accumulation loop, two windows of k = 3 and a partial one of 2"""
    g = load_golden(name)
    net, model = build19(g, cfg, "fp32")
    worst = parity19(g, cfg, model, net, "%s %s" % (name, cfg))
    print("%s %s: worst parameter error / (5e-3 x the reference's largest move) = %.4f" % (name, cfg, worst))


def test_fixtures_bite():
    """a model with the attribute left at 1 fails that parity: it updates at the first call of the window"""
    g = load_golden(G19_FIXTURES[0])
    net, model = build19(g, "sgdmom", "fp32")
    model.accumulate_grad_batches = 1
    with pytest.raises(AssertionError, match="a micro-step moved the parameters"):
        parity19(g, "sgdmom", model, net, "attribute ignored")
    model._rtx.inject = None


@pytest.mark.parametrize("cfg", ["sgdmom", "adam_norm"])
def test_custom_loss_route(cfg):
    """custom_loss = True with super().loss_function(...) + a term of the user's own (of weight zero, so that the recorded loop stays
    the reference): loss.backward() on the unscaled loss, the engine's backward adds g / k into the accumulators; the same bounds"""
    from rectorch_amd.models import MultiVAE
    g = load_golden("g19_accum_mvae_small")

    class Own(MultiVAE):
        def loss_function(self, recon_x, x, mu, logvar, beta=1.0):
            return super().loss_function(recon_x, x, mu, logvar, beta) + 0.0 * (mu * mu).sum()

    net, model = build19(g, cfg, "fp32", model_cls=Own)
    model.custom_loss = True
    worst = parity19(g, cfg, model, net, "g19_accum_mvae_small %s custom" % cfg)
    print("custom-loss route, %s: worst ratio %.4f" % (cfg, worst))


def test_custom_loss_route_mdae_regulariser_through_torch():
    """Mult-DAE on the custom route: the regulariser reaches the parameters through torch alone and is accumulated with the same weight"""
    from rectorch_amd.models import MultiDAE
    g = load_golden("g19_accum_mdae_small")

    class Own(MultiDAE):
        def loss_function(self, *args, **kwargs):
            return super().loss_function(*args, **kwargs)

    net, model = build19(g, "sgdmom", "fp32", model_cls=Own)
    model.custom_loss = True
    parity19(g, "sgdmom", model, net, "g19_accum_mdae_small sgdmom custom")


def test_larger_micro_batch_inside_a_window_is_refused_and_nothing_goes_stale():
    """a micro-batch above the engine's max_batch in the middle of a window raises before the network rebuilds its engine; the window
    can still be applied, and the next step runs on current compute copies (bit-equal to a model that never saw the refusal)"""
    from rectorch_amd import _lib
    g = load_golden(FIXTURES[0])
    outs = []
    for provoke in (False, True):
        net, model = build(g, "adam_norm", "fp32")
        model.accumulate_grad_batches = 3
        x, mask, eps = micro(g, 0)
        model._rtx.inject = (mask, eps)
        model.train_batch(x)
        eng = model._rtx.accum_engine
        if provoke:
            big = torch.zeros(eng.max_batch + 1, x.shape[1])
            with pytest.raises(_lib.RtxError, match="largest micro-batch first"):
                model.train_batch(big)
            assert model.pending_micro_batches == 1 and next(iter(net._rtx_engines.values())) is eng
        assert model.apply_accumulated() is True
        model.accumulate_grad_batches = 1
        x1, mask1, eps1 = micro(g, 1)
        model._rtx.inject = (mask1, eps1)
        loss = model.train_batch(x1)
        outs.append((loss, [p.detach().clone() for p in net._param_list()]))
    assert outs[0][0] == outs[1][0] and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))


def micro19(g, j):
    return (torch.from_numpy(g["x_%d" % j]), dev(g["mask_%d" % j], torch.uint8), dev(g["eps_%d" % j]) if "eps_%d" % j in g else None)


@pytest.mark.parametrize("name", G19_FIXTURES)
@pytest.mark.parametrize("cfg", sorted(G19_CONFIGS))
def test_fixture_windows_bf16(name, cfg):
    """bf16, the update alone, on the g19 inputs and configurations (unclipped Adam, SGD with momentum and RMSprop, norm-clipped Adam,
    value-clipped Adagrad): the accumulated p.grad against the float64 sum of the device's own per-micro-step gradients within
    k 2^-24 sum |g_i / k|, the update against the float64 clip + rule on it, micro-steps bit-neutral, the partial window through
    apply_accumulated(), and the compute copies refreshed"""
    g = load_golden(name)
    net, model = build19(g, cfg, "bf16", predict_numerics="bf16")
    ref = reference_model(g, cfg, "bf16", builder=build19)
    tag = "%s %s bf16" % (name, cfg)
    worst = 0.0
    for w, window in enumerate(G19.WINDOWS):
        worst = max(worst, run_window("%s window %d" % (tag, w), g, cfg, model, ref, window, 3, w + 1, partial=len(window) < 3,
                                      configs=G19_CONFIGS, batch=micro19))
    print("%s: worst update error / bound = %.4f" % (tag, worst))
    model._rtx.inject = None
    x = torch.from_numpy(g["x_0"])
    pred = model.predict(x, remove_train=False)[0]
    fresh_net, fresh = build19(g, cfg, "bf16", predict_numerics="bf16")
    fresh_net.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
    assert torch.equal(pred, fresh.predict(x, remove_train=False)[0])
