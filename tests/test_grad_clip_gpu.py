"""GPU (-m gpu): gradient clipping on the device -- global 2-norm, global max-norm and value, on every single-GPU training route.

References: the reference's own recorded clipped steps (tests/golden/g18_clip_*.npz, made by tests/golden/make_golden_clip.py by
wrapping ``model.optimizer.step`` with ``clip_grad_norm_`` / ``clip_grad_value_``) for the float32 parity runs, and the float64
restatement of clip and rule (tests/clip_rules64.py with tests/optim_rules64.py, pinned to those fixtures by
tests/test_grad_clip_host.py) applied to the gradients the device itself stored wherever the update alone is judged.  The fixtures
were made so that an UNCLIPPED run misses every parity bound by a factor of 100 or more: without the feature every test below fails.

Bounds.  Float32 parity: those of test_optimizers_gpu.test_fixture_parity_fp32 -- loss 1e-5 relative, gradients 2e-4, parameters and
states within 5e-3 x the largest move the reference itself made in that tensor on that step.  ``last_grad_norm``: within
32 x 2^-24 x (||g|| + ||reg||) of the float64 norm of the device's own stored gradients plus the regulariser term formed from the
parameters before the step (the float32 sum of squares behind that term accounts for the slack).  The update alone: the one-update
bound of test_optimizers_gpu (16 x 2^-24 x the scales of the computation), with the roundings the clip puts in front of the rule
added on the gradient's terms as tests/test_grad_clip_host.py counts them: the device's norm is within those 32 roundings of the
float64 one, the coefficient and the product add 8 -- 16 + 40 on a G term, 16 + 80 on a G^2 term, for the norm modes; the clamp of
value clipping is exact and keeps 16.
"""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.optim as optim

from conftest import ROOT, load_golden, sd_from, params_in_order
import clip_rules64 as K
import optim_rules64 as R
from test_grad_clip_host import CONFIGS, FIXTURES, E24, g_roundings
from test_optimizers_gpu import dev, host, rel, inject, loss_grads, snapshot, device_kw, wd_of

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _require_native_path():
    from rectorch_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()


def set_clip(model, clip):
    model.clip_grad_norm = clip.get("max_norm") if clip else None
    model.clip_grad_norm_type = clip.get("norm_type", 2.0) if clip else 2.0
    model.clip_grad_value = clip.get("value") if clip else None


def build(g, cfg, numerics, model_cls=None, **kw):
    """the fixture's network and trainer with the configuration's optimizer and clip attributes"""
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
    cls, okw, clip = CONFIGS[cfg]
    model.optimizer = getattr(optim, cls)(net.parameters(), **okw)
    set_clip(model, clip)
    return net, model


def norm64(grads, regs, norm_type=2.0):
    return K.total_norm([a + b for a, b in zip(grads, regs)], norm_type)


def assert_norm(tag, model, grads, regs, clip):
    """model.last_grad_norm against the float64 norm of the stored gradients + the regulariser term"""
    got = model.last_grad_norm
    if not clip or "value" in clip:
        assert got is None, (tag, got)
        return None
    want = norm64(grads, regs, clip.get("norm_type", 2.0))
    slack = 32 * E24 * (K.total_norm(grads, clip.get("norm_type", 2.0)) + K.total_norm(regs, clip.get("norm_type", 2.0)))
    assert isinstance(got, float) and abs(got - want) <= slack, (tag, got, want, slack)
    return want


def assert_clipped_update(tag, model, cls, kw, clip, t, before, states_before, grads, regs=None):
    """the device's parameters and states against the float64 clip + rule applied to ``grads`` (+ ``regs``) from ``before``"""
    regs = regs or [np.zeros_like(x) for x in grads]
    cg, total, coef = K.clipped([a + b for a, b in zip(grads, regs)], clip)
    c = 1.0 if coef is None else coef
    rg, rg2 = g_roundings(clip)
    dkw = device_kw(cls, kw)
    worst = 0.0
    for i, p in enumerate(model.network._param_list()):
        st = dict(states_before[i])
        if not st and cls != "SGD":
            st = R.init_state(cls, kw, before[i])
        old = {k: v.copy() for k, v in st.items()}
        want = R.update(cls, dkw, t, before[i], cg[i], st)
        # the prepared gradient's terms, which may cancel, as in test_optimizers_gpu (the regulariser term is formed from a float32
        # sum of squares: its scale counts 1.5 times), times the coefficient; a clamped element's scale is at most the unclamped one
        G = c * (np.abs(grads[i]) + 1.5 * np.abs(regs[i])) + wd_of(cls, kw) * np.abs(before[i])
        bound = E24 * (16 * (np.abs(want) + np.abs(want - before[i])) + rg * kw["lr"] * G)
        err = np.abs(host(p) - want)
        assert np.all(err <= bound), (tag, i, float(np.max(err / np.maximum(bound, 1e-300))))
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        for k in R.state_keys(cls, kw):
            got = host(model.optimizer.state[p][k])
            second = k in ("exp_avg_sq", "sum", "square_avg")
            sb = E24 * (16 * (np.abs(st[k]) + np.abs(old.get(k, 0.0))) + (rg2 * G * G if second else rg * G))
            assert np.all(np.abs(got - st[k]) <= sb), (tag, i, k, float(np.max(np.abs(got - st[k]) / np.maximum(sb, 1e-300))))
    return worst


# ---------------------------------------------------------------------------------------------- native driver
def test_native_driver_clip():
    """the norm kernels and every rule x {coefficient, value} x every walk against float64, element by element
    (tests/native/test_clip.cpp)"""
    path = os.path.join(ROOT, "build", "native", "test_clip")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-s", "-f", "clip.mk"])
    out = subprocess.run([path], capture_output=True, text=True, timeout=600)
    print(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "CLIP TESTS PASSED" in out.stdout


# ---------------------------------------------------------------------------------------------- fixtures, float32
def _parity(g, cfg, model, net, tag):
    cls, kw, clip = CONFIGS[cfg]
    keys = params_in_order(sd_from(g, "sd0__"))[1]
    lam = float(g["model__lam"]) if "model__lam" in g and not model.custom_loss else 0.0
    prev = [g["sd0__" + k.replace(".", "__")].astype(np.float64) for k in keys]
    prev_state = [R.init_state(cls, kw, p) for p in prev]
    worst = 0.0
    for t in range(g["xs"].shape[0]):
        inject(model, g, t)
        before = [host(p) for p in net._param_list()]
        loss = model.train_batch(torch.from_numpy(g["xs"][t]))
        want = float(g["%s__loss_%d" % (cfg, t)])
        assert isinstance(loss, float) and abs(loss - want) < 1e-5 * abs(want), (tag, t, loss, want)
        stored, regs = loss_grads(model, before, lam)
        total = assert_norm("%s step %d" % (tag, t), model, stored, regs, clip)
        if total is not None:
            ref_total = float(g["%s__total_norm_%d" % (cfg, t)])
            assert abs(total - ref_total) < 2e-4 * ref_total, (tag, t, total, ref_total)      # (the gradients' own bound)
        grads = [a + b for a, b in zip(stored, regs)]           # p.grad keeps the UNCLIPPED gradient: the fixture's, not the clipped one
        for i, (k, prm) in enumerate(zip(keys, net._param_list())):
            kk = k.replace(".", "__")
            assert rel(grads[i], g["%s__grad_%d__%s" % (cfg, t, kk)]) < 2e-4, (tag, t, k)
            ref = g["%s__sd_%d__%s" % (cfg, t, kk)].astype(np.float64)
            move = float(np.max(np.abs(ref - prev[i])))
            err = float(np.max(np.abs(host(prm) - ref)))
            worst = max(worst, err / (5e-3 * move))
            assert err <= 5e-3 * move, (tag, t, k, err, move)
            for s in R.state_keys(cls, kw):
                ref_s = g["%s__%s_%d__%s" % (cfg, s, t, kk)].astype(np.float64)
                s_move = float(np.max(np.abs(ref_s - prev_state[i].get(s, 0.0))))
                s_err = float(np.max(np.abs(host(model.optimizer.state[prm][s]) - ref_s)))
                assert s_err <= 5e-3 * s_move, (tag, t, k, s, s_err, s_move)
                prev_state[i][s] = ref_s
            prev[i] = ref
    model._rtx.inject = None
    return worst


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_fixture_parity_fp32(name, cfg):
    """three clipped steps of the reference with each configuration, its dropout masks and eps injected: loss, (unclipped) gradients,
    the total norm, parameters, states.  ``adam_norm_loose`` (coefficient 1) is the unclipped Adam run on the unfused schedule with
    the clipping instantiation of the kernel: the same bounds."""
    g = load_golden(name)
    net, model = build(g, cfg, "fp32")
    worst = _parity(g, cfg, model, net, "%s %s" % (name, cfg))
    print("%s %s: worst parameter error / (5e-3 x the reference's largest move) = %.4f" % (name, cfg, worst))


def test_unclipped_run_misses_the_fixture():
    """the fixtures bite: the same model with the clip attributes left alone fails the parity bounds"""
    g = load_golden(FIXTURES[0])
    net, model = build(g, "sgd_norm", "fp32")
    set_clip(model, None)
    with pytest.raises(AssertionError):
        _parity(g, "sgd_norm", model, net, "unclipped")
    model._rtx.inject = None


# ---------------------------------------------------------------------------------------------- fixtures, bf16
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_fixture_update_bf16(name, cfg):
    """bf16 numerics: with a clip attribute set the step takes the unfused schedule and stores its gradients (Adam too); the update
    alone is judged (the float64 clip + rule on the stored p.grad), and the compute copies are refreshed: predict in bf16 equals, bit
    for bit, the predict of a fresh engine built from the float32 masters"""
    g = load_golden(name)
    cls, kw, clip = CONFIGS[cfg]
    net, model = build(g, cfg, "bf16", predict_numerics="bf16")
    lam = float(g["model__lam"]) if "model__lam" in g else 0.0
    for t in range(g["xs"].shape[0]):
        inject(model, g, t)
        before, states = snapshot(model, cls, kw)
        for p in net._param_list():
            if p.grad is not None:
                p.grad.fill_(float("nan"))          # a step that does not store its gradients shows
        loss = model.train_batch(torch.from_numpy(g["xs"][t]))
        assert np.isfinite(loss)
        grads, regs = loss_grads(model, before, lam)
        assert all(np.all(np.isfinite(x)) for x in grads)
        assert_norm("%s %s step %d" % (name, cfg, t), model, grads, regs, clip)
        ratio = assert_clipped_update("%s %s step %d" % (name, cfg, t), model, cls, kw, clip, t + 1, before, states, grads, regs)
        if cfg != "adam_norm_loose":
            with pytest.raises(AssertionError):         # ... and is not the unclipped rule's
                assert_clipped_update("unclipped", model, cls, kw, None, t + 1, before, states, grads, regs)
        moved = [float(np.max(np.abs(host(p) - b))) for p, b in zip(net._param_list(), before)]
        assert all(m > 0 for m in moved), (cfg, t, moved)
    print("%s %s bf16: worst error / one-update bound %.3f" % (name, cfg, ratio))
    model._rtx.inject = None
    x = torch.from_numpy(g["xs"][0])
    pred = model.predict(x, remove_train=False)[0]
    fresh_net, fresh = build(g, cfg, "bf16", predict_numerics="bf16")
    fresh_net.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
    assert torch.equal(pred, fresh.predict(x, remove_train=False)[0])
    assert not torch.equal(pred, build(g, cfg, "bf16", predict_numerics="bf16")[1].predict(x, remove_train=False)[0])     # (training moved it)


def test_toggling_between_the_fused_and_the_clipped_step_bf16():
    """bf16, Adam, five steps: clip, none, clip, none, none -- the fused step (Adam inside the weight-gradient kernels, compute copies
    swapped) and the unfused clipped step alternate.  Every step's update is the float64 rule's for its schedule on the gradients it
    stored (keep_grads stores them on the fused steps too), last_grad_norm is None after the unclipped steps, and the final predict
    equals a fresh engine's."""
    g = load_golden("g18_clip_mvae_deep")
    cls, kw, clip = CONFIGS["adam_norm"]
    net, model = build(g, "adam_norm", "bf16", predict_numerics="bf16")
    model.keep_grads = True
    for t, on in enumerate((True, False, True, False, False)):
        set_clip(model, clip if on else None)
        inject(model, g, t % 3)
        before, states = snapshot(model, cls, kw)
        for p in net._param_list():
            if p.grad is not None:
                p.grad.fill_(float("nan"))
        loss = model.train_batch(torch.from_numpy(g["xs"][t % 3]))
        assert np.isfinite(loss)
        grads = [host(p.grad) for p in net._param_list()]
        assert all(np.all(np.isfinite(x)) for x in grads)
        assert (model.last_grad_norm is not None) == on
        if on:
            assert model.last_grad_norm >= 2 * clip["max_norm"]
        assert_clipped_update("toggle step %d clip=%s" % (t, on), model, cls, kw, clip if on else None, t + 1, before, states, grads)
        with pytest.raises(AssertionError):
            assert_clipped_update("the other schedule", model, cls, kw, None if on else clip, t + 1, before, states, grads)
    model._rtx.inject = None
    x = torch.from_numpy(g["xs"][0])
    pred = model.predict(x, remove_train=False)[0]
    fresh_net, fresh = build(g, "adam_norm", "bf16", predict_numerics="bf16")
    fresh_net.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
    assert torch.equal(pred, fresh.predict(x, remove_train=False)[0])


def test_clipped_step_is_bit_reproducible_bf16():
    """two runs of three clipped bf16 steps from the same state: the same parameter bits and the same reported norms (the norm is a
    fixed-order sum: no atomics)"""
    g = load_golden("g18_clip_mvae_deep")
    runs = []
    for _ in range(2):
        net, model = build(g, "sgdmom_norm", "bf16")
        norms = []
        for t in range(3):
            inject(model, g, t)
            model.train_batch(torch.from_numpy(g["xs"][t]))
            norms.append(model.last_grad_norm)
        runs.append(([p.detach().clone() for p in net._param_list()], norms))
    assert runs[0][1] == runs[1][1]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))


# ---------------------------------------------------------------------------------------------- custom-loss route
@pytest.mark.parametrize("name", ["g18_clip_mvae_small", "g18_clip_mdae_small"])
@pytest.mark.parametrize("cfg", ["sgdmom_norm", "rmsprop_value"])
def test_custom_loss_route(name, cfg):
    """a subclass whose loss_function is super().loss_function(...), custom_loss = True: the same fixture under the same bounds (the
    loss, Mult-DAE's regulariser included, reaches p.grad through autograd; rtx_engine_apply_adam clips it)"""
    from rectorch_amd.models import MultiVAE, MultiDAE
    g = load_golden(name)
    base = MultiDAE if "model__lam" in g else MultiVAE

    class Own(base):
        def loss_function(self, *args, **kwargs):
            return super().loss_function(*args, **kwargs)

    net, model = build(g, cfg, "fp32", model_cls=Own)
    model.custom_loss = True
    worst = _parity(g, cfg, model, net, "%s %s custom" % (name, cfg))
    print("%s custom-loss route, %s: worst ratio %.4f" % (name, cfg, worst))


# ---------------------------------------------------------------------------------------------- SVAE
SVAE_CLIP = dict(max_norm=0.01, norm_type=2.0)


@pytest.mark.parametrize("cfg", ["sgdmom_norm", "adam_norm"])
def test_svae_fused_and_custom_routes(cfg, monkeypatch):
    """one [1, T] user, T = 33, three steps: the fused and the custom-loss route each match the float64 clip + rule on their own stored
    gradients, and each other within the bounds of test_optimizers_gpu.test_svae_fused_and_custom_routes (parameters: max < 1e-3,
    fraction above 2e-5 < 1e-4); then one pack of 4 users through train_batch(SvaePack) on the fused route"""
    from rectorch_amd.engine import SvaePack
    from rectorch_amd.models import SVAE
    from test_svae_custom_loss_gpu import build as build_svae, counting, ref_loss, seq
    from test_svae_custom_loss_host import make_sequence
    from test_svae_routes import _knobs
    _knobs(monkeypatch)
    cls, kw, _ = CONFIGS[cfg]
    kw = dict(kw, lr=kw["lr"] * 0.1)
    models = []
    for custom in (False, True):
        net, sd, model = build_svae(64, seed=41, model_cls=counting(ref_loss) if custom else SVAE)
        model.custom_loss = custom
        model.optimizer = getattr(optim, cls)(net.parameters(), **kw)
        set_clip(model, SVAE_CLIP)
        models.append((net, model))
    rng = np.random.RandomState(41)
    for t in range(3):
        items, y, eps = make_sequence(rng, 33)
        for net, model in models:
            model._rtx.inject = (None, dev(eps))
            before, states = snapshot(model, cls, kw)
            loss = model.train_batch(seq(items), torch.from_numpy(y[None].astype(np.float32)))
            assert np.isfinite(loss)
            grads = [host(p.grad) for p in net._param_list()]
            tag = "svae %s step %d custom=%s" % (cfg, t, model.custom_loss)
            total = assert_norm(tag, model, grads, [np.zeros_like(x) for x in grads], SVAE_CLIP)
            assert total >= 2 * SVAE_CLIP["max_norm"], (tag, total)
            assert_clipped_update(tag, model, cls, kw, SVAE_CLIP, t + 1, before, states, grads)
            with pytest.raises(AssertionError):
                assert_clipped_update("unclipped", model, cls, kw, None, t + 1, before, states, grads)
        for p, q in zip(models[0][0]._param_list(), models[1][0]._param_list()):
            d = np.abs(host(p) - host(q))
            assert d.max() < 1e-3 and np.mean(d > 2e-5) < 1e-4, (cfg, t, d.max())
    assert models[1][1].calls == 3
    # a pack of 4 users, ONE optimizer step, on the fused route
    net, model = models[0]
    n_items, latent = net.n_items, eps.shape[1]
    seqs, rows = [], []
    for n in (5, 1, 12, 3):
        seqs.append(rng.randint(0, n_items, size=n).tolist())
        rows.append([sorted(rng.choice(n_items, size=2, replace=False).tolist()) for _ in range(n)])
    pack = SvaePack(seqs, rows)
    model._rtx.inject = (None, dev(rng.randn(pack.n_steps, latent).astype(np.float32)))
    before, states = snapshot(model, cls, kw)
    loss = model.train_batch(pack, pack)
    model._rtx.inject = None
    assert np.isfinite(loss)
    grads = [host(p.grad) for p in net._param_list()]
    assert_norm("svae pack", model, grads, [np.zeros_like(x) for x in grads], SVAE_CLIP)
    assert_clipped_update("svae %s pack" % cfg, model, cls, kw, SVAE_CLIP, 4, before, states, grads)


# ---------------------------------------------------------------------------------------------- max_norm = inf
def test_infinite_max_norm_reports_the_norm_and_clips_nothing():
    """torch's idiom for reading the norm: the parameters move as an unclipped step's do (the float64 rule without any clip, the plain
    one-update bound), last_grad_norm is the norm"""
    g = load_golden("g18_clip_mdae_small")
    cls, kw, _ = CONFIGS["adam_norm"]
    net, model = build(g, "adam_norm", "fp32")
    model.clip_grad_norm = INF
    lam = float(g["model__lam"])
    inject(model, g, 0)
    before, states = snapshot(model, cls, kw)
    model.train_batch(torch.from_numpy(g["xs"][0]))
    model._rtx.inject = None
    grads, regs = loss_grads(model, before, lam)
    total = assert_norm("inf", model, grads, regs, dict(max_norm=INF, norm_type=2.0))
    assert np.isfinite(total) and total > 1.0
    assert_clipped_update("max_norm = inf", model, cls, kw, None, 1, before, states, grads, regs)


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("attrs", [dict(clip_grad_norm=1.0, clip_grad_norm_type=1.0), dict(clip_grad_norm=1.0, clip_grad_norm_type=3.0),
                                   dict(clip_grad_norm=1.0, clip_grad_value=1.0), dict(clip_grad_norm=-1.0), dict(clip_grad_value=-1.0)],
                         ids=lambda a: ",".join("%s=%s" % kv for kv in sorted(a.items())))
@pytest.mark.parametrize("custom", [False, True])
def test_refused_settings_raise_before_any_launch(attrs, custom):
    from rectorch_amd.models import MultiVAE
    g = load_golden("g18_clip_mvae_small")

    class Own(MultiVAE):
        def loss_function(self, *args, **kwargs):
            return super().loss_function(*args, **kwargs)

    net, model = build(g, "sgd_norm", "fp32", model_cls=Own if custom else None)
    model.custom_loss = custom
    set_clip(model, None)
    for k, v in attrs.items():
        setattr(model, k, v)
    with pytest.raises(ValueError, match="supported"):
        model.train_batch(torch.from_numpy(g["xs"][0]))
    assert not getattr(net, "_rtx_engines", {})          # no engine was even built
    for k, v in sd_from(g, "sd0__").items():
        assert np.array_equal(net.state_dict()[k].cpu().numpy(), v)


def test_data_parallel_refuses_clipping():
    from rectorch_amd import _lib, parallel
    g = load_golden("g18_clip_mvae_small")
    net, model = build(g, "adam_norm_loose", "bf16")
    model.optimizer = optim.Adam(net.parameters(), lr=1e-3)
    with pytest.raises(_lib.RtxError, match="clip"):
        parallel.attach(model, emulate_world=2)
    # ... and the engine's own data-parallel entry points refuse a mode set behind the trainer's back (RTX_EINVAL)
    set_clip(model, None)
    inject(model, g, 0)
    model.train_batch(torch.from_numpy(g["xs"][0]))
    model._rtx.inject = None
    eng = next(iter(net._rtx_engines.values()))
    eng.set_grad_clip(_lib.RTX_CLIP_NORM2, 1.0)
    step = eng._step(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=2)
    with pytest.raises(_lib.RtxError, match="error -1: .*clipping"):
        eng.apply_adam_layers(step, 0, 1)
    with pytest.raises(_lib.RtxError, match="error -1: .*clipping"):
        eng.apply_adam_rows(step, 0, 0, 1, True, None, None)
    with pytest.raises(_lib.RtxError, match="unknown mode"):
        eng.set_grad_clip(7, 1.0)
    with pytest.raises(_lib.RtxError, match="bound"):
        eng.set_grad_clip(_lib.RTX_CLIP_VALUE, -1.0)
    # rtx_engine_dp_attach: a plan attached to an engine that clips is refused, with nothing enqueued
    parallel.attach(model, emulate_world=2)
    inject(model, g, 1)
    with pytest.raises(_lib.RtxError, match="error -1: dp_attach: gradient clipping"):
        model.train_batch(torch.from_numpy(g["xs"][1]))
    model._rtx.inject = None
    eng.set_grad_clip(_lib.RTX_CLIP_NONE)
    # ... and under an attached plan the trainer refuses a clip attribute before anything else
    model.clip_grad_value = 0.5
    with pytest.raises(_lib.RtxError, match="data-parallel"):
        model.train_batch(torch.from_numpy(g["xs"][1]))


# ---------------------------------------------------------------------------------------------- the stand-alone operator
@pytest.mark.parametrize("norm_type", [2.0, INF])
def test_grad_norm_operator(norm_type):
    """engine.grad_norm and torch.ops.rectorch_hip.grad_norm agree to the bit, twice, and with float64 within the native driver's
    bound (2-norm: 4 x 2^-24 relative; max-norm: exact)"""
    from rectorch_amd import engine, ops  # noqa: F401  (registers the ops)
    rng = np.random.RandomState(7)
    shapes = [(1,), (3,), (4095,), (4096,), (4097,), (77, 21), (3 * 4096 + 5,), (300007,)]
    ts = [dev(rng.randn(*s).astype(np.float32)) for s in shapes]
    ts.append(dev(rng.randn(4098).astype(np.float32))[1:])          # a buffer offset by 4 bytes
    a = engine.grad_norm(ts, norm_type)
    b = torch.ops.rectorch_hip.grad_norm(ts, norm_type)
    c = engine.grad_norm(ts, norm_type)
    assert a.shape == () and a.dtype == torch.float32 and a.is_cuda
    assert torch.equal(a, b) and torch.equal(a, c)
    want = K.total_norm([host(t) for t in ts], norm_type)
    if norm_type == INF:
        assert float(a) == np.float32(want)
    else:
        assert abs(float(a) - want) <= 4 * E24 * want
    assert float(engine.grad_norm([torch.zeros(5, device="cuda")], norm_type)) == 0.0
    assert np.isnan(float(engine.grad_norm([dev(np.array([1.0, np.nan], np.float32)), ts[1]], norm_type)))
    with pytest.raises(ValueError, match="supported"):
        engine.grad_norm(ts, 3.0)
