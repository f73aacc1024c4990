"""GPU (-m gpu): training with the model's own optimizer -- SGD, AdamW, Adagrad, RMSprop on every single-GPU training route.

References: the reference's own recorded steps (tests/golden/g17_optim_*.npz, made by tests/golden/make_golden_optim.py) for the
float32 parity runs, and the float64 restatement of the rules (tests/optim_rules64.py, pinned to those fixtures by
tests/test_optimizers_host.py) applied to the gradients the device itself stored wherever the update alone is judged.

Bounds.  Float32 parity: loss 1e-5 relative and gradients 2e-4, the bounds of test_g2_train_steps_fp32; parameters and state tensors
after each step within 5e-3 x the largest move the reference itself made in that tensor on that step (the ratio of the Adam test:
5e-6 at a largest move of lr = 1e-3).  The update alone (``one_update_bound``): the float32 update is at most 12 roundings, each
relative to a term of the computation -- the quantity judged, old and new, the step it takes, or the prepared gradient's terms
G = |g| + wd |p| (lr G for a parameter, G for a first-moment state, G^2 for a second-moment one) -- so 16 x 2^-24 x the sum of those
scales, the bound tests/test_optimizers_host.py holds torch's own float32 steps to.  Two things the device does by design enter the
restatement it is judged by, not the bound: ``rtx_step`` carries Adam's betas as float32 and the kernel forms 1 - beta from those
(as its Adam always has), so the rule is evaluated at the float32 betas; and Mult-DAE's regulariser term lam p / ||p|| is formed on
the device from a float32 sum of squares (k_sumsq: at most 11 more roundings on the sum at these sizes, 5.5 on its root, and 2 for
the quotient and the product), so that term's scale counts 1.5 times (24 roundings instead of 16).
"""
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch
import torch.optim as optim

from conftest import ROOT, load_golden, sd_from, params_in_order
import optim_rules64 as R
from test_optimizers_host import CONFIGS, FIXTURES, E24

pytestmark = pytest.mark.gpu

WORST = {}      # configuration -> worst parameter error / (5e-3 x the reference's largest move) over the fixtures run so far


@pytest.fixture(scope="module", autouse=True)
def _require_native_path():
    from rectorch_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-30, np.max(np.abs(b))))


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def build(g, cfg, numerics, model_cls=None, **kw):
    """the fixture's network and trainer with the configuration's optimizer in place of Adam"""
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
    cls, okw = CONFIGS[cfg]
    model.optimizer = getattr(optim, cls)(net.parameters(), **okw)
    return net, model


def inject(model, g, t):
    model._rtx.inject = (dev(g["mask_%d" % t], torch.uint8), dev(g["eps_%d" % t]) if "eps_%d" % t in g else None)


def wd_of(cls, kw):
    return kw.get("weight_decay", 0.01 if cls == "AdamW" else 0.0)


def one_update_bound(cls, kw, p_old, p_new, grad, reg):
    G = np.abs(grad) + 1.5 * np.abs(reg) + wd_of(cls, kw) * np.abs(p_old)
    return 16 * E24 * (np.abs(p_new) + np.abs(p_new - p_old) + kw["lr"] * G), G


def device_kw(cls, kw):
    """the configuration as the device evaluates it: Adam's betas are float32 in rtx_step"""
    if cls in ("Adam", "AdamW"):
        b1, b2 = kw.get("betas", (0.9, 0.999))
        return dict(kw, betas=(float(np.float32(b1)), float(np.float32(b2))))
    return kw


def state_bound(key, s_old, s_new, G):
    return 16 * E24 * (np.abs(s_new) + np.abs(s_old) + (G * G if key in ("exp_avg_sq", "sum", "square_avg") else G))


def loss_grads(model, params_before, lam):
    """the gradient of the LOSS from what the step stored in p.grad, as (stored gradients, regulariser terms): Mult-DAE's regulariser
    lam sum ||W||_2 is added by the optimizer kernel (g += lam p / ||p||), not stored"""
    grads, regs = [], []
    for p, before in zip(model.network._param_list(), params_before):
        grads.append(host(p.grad))
        n = np.sqrt(np.sum(before * before))
        regs.append((lam / n) * before if lam and n > 0 else np.zeros_like(before))
    return grads, regs


def snapshot(model, cls, kw):
    net = model.network
    return ([host(p) for p in net._param_list()],
            [{k: host(model.optimizer.state[p][k]) for k in R.state_keys(cls, kw) if k in model.optimizer.state.get(p, {})} for p in net._param_list()])


def assert_one_update(tag, model, cls, kw, t, before, states_before, grads, regs=None):
    """the device's parameters and states against the float64 rule applied to ``grads`` (+ ``regs``) from ``before``"""
    worst = 0.0
    regs = regs or [np.zeros_like(x) for x in grads]
    dkw = device_kw(cls, kw)
    for i, p in enumerate(model.network._param_list()):
        st = dict(states_before[i])
        if cls == "Adagrad" and "sum" not in st:
            st = R.init_state(cls, kw, before[i])
        if cls in ("Adam", "AdamW", "RMSprop") and not st:
            st = R.init_state(cls, kw, before[i])
        old = {k: v.copy() for k, v in st.items()}
        want = R.update(cls, dkw, t, before[i], grads[i] + regs[i], st)
        bound, G = one_update_bound(cls, kw, before[i], want, grads[i], regs[i])
        err = np.abs(host(p) - want)
        assert np.all(err <= bound), (tag, i, float(np.max(err / np.maximum(bound, 1e-300))))
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        for k in R.state_keys(cls, kw):
            got = host(model.optimizer.state[p][k])
            sb = state_bound(k, old.get(k, 0.0), st[k], G)
            assert np.all(np.abs(got - st[k]) <= sb), (tag, i, k, float(np.max(np.abs(got - st[k]) / np.maximum(sb, 1e-300))))
    return worst


# ---------------------------------------------------------------------------------------------- native driver
def test_native_driver_optim():
    """every rule on every walk of k_optim against float64, element by element (tests/native/test_optim.cpp)"""
    path = os.path.join(ROOT, "build", "native", "test_optim")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-s", "-f", "optim.mk"])
    out = subprocess.run([path], capture_output=True, text=True, timeout=600)
    print(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "OPTIM TESTS PASSED" in out.stdout


# ---------------------------------------------------------------------------------------------- fixtures, float32
def _parity(g, cfg, model, net, tag):
    cls, kw = CONFIGS[cfg]
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
        grads = [a + b for a, b in zip(*loss_grads(model, before, lam))]
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
    """three steps of the reference with each optimizer, its dropout masks and eps injected: loss, gradients, parameters, states"""
    g = load_golden(name)
    net, model = build(g, cfg, "fp32")
    worst = _parity(g, cfg, model, net, "%s %s" % (name, cfg))
    WORST[cfg] = max(WORST.get(cfg, 0.0), worst)
    print("%s %s: worst parameter error / (5e-3 x the reference's largest move) = %.4f (this rule so far: %.4f)" % (name, cfg, worst, WORST[cfg]))
    if cfg == "sgd":
        assert len(model.optimizer.state) == 0          # plain SGD keeps no state at all, as in torch


# ---------------------------------------------------------------------------------------------- fixtures, bf16
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_fixture_update_bf16(name, cfg):
    """bf16 numerics: the step takes the unfused schedule and stores its gradients; the update alone is judged (the float64 rule on
    the stored p.grad, one-update bound), and the compute copies are refreshed: predict in bf16 equals, bit for bit, the predict of
    a fresh engine built from the float32 masters (the deep shape has hidden layers with transposed copies)"""
    g = load_golden(name)
    cls, kw = CONFIGS[cfg]
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
        ratio = assert_one_update("%s %s step %d" % (name, cfg, t), model, cls, kw, t + 1, before, states, grads, regs)
        moved = [float(np.max(np.abs(host(p) - b))) for p, b in zip(net._param_list(), before)]
        assert all(m > 0 for m in moved), (cfg, t, moved)
    print("%s %s bf16: worst error / one-update bound %.3f" % (name, cfg, ratio))
    model._rtx.inject = None
    x = torch.from_numpy(g["xs"][0])
    pred = model.predict(x, remove_train=False)[0]
    fresh_net, fresh = build(g, cfg, "bf16", predict_numerics="bf16")
    fresh_net.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
    pred_fresh = fresh.predict(x, remove_train=False)[0]
    assert torch.equal(pred, pred_fresh)
    assert not torch.equal(pred, build(g, cfg, "bf16", predict_numerics="bf16")[1].predict(x, remove_train=False)[0])     # (training moved it)


# ---------------------------------------------------------------------------------------------- custom-loss route
@pytest.mark.parametrize("name", ["g17_optim_mvae_small", "g17_optim_mdae_small"])
def test_custom_loss_route_with_sgd_momentum(name):
    """a subclass whose loss_function is super().loss_function(...), custom_loss = True, SGD with momentum: the same fixture under the
    same bounds (the loss reaches the optimizer through autograd and rtx_engine_apply_adam)"""
    from rectorch_amd.models import MultiVAE, MultiDAE
    g = load_golden(name)
    base = MultiDAE if "model__lam" in g else MultiVAE

    class Own(base):
        def loss_function(self, *args, **kwargs):
            return super().loss_function(*args, **kwargs)

    net, model = build(g, "sgd_mom", "fp32", model_cls=Own)
    model.custom_loss = True
    worst = _parity(g, "sgd_mom", model, net, name + " custom")
    print("%s custom-loss route, sgd_mom: worst ratio %.4f" % (name, worst))


# ---------------------------------------------------------------------------------------------- SVAE
@pytest.mark.parametrize("cfg", ["sgd_mom", "rmsprop"])
def test_svae_fused_and_custom_routes(cfg, monkeypatch):
    """one [1, T] user, three steps: the fused and the custom-loss route agree within the bounds the SVAE custom-loss tests hold Adam
    to (parameters: max < 1e-3, fraction above 2e-5 < 1e-4), and each matches the float64 rule on its own stored gradients"""
    from rectorch_amd.models import SVAE
    from test_svae_custom_loss_gpu import build as build_svae, counting, ref_loss, seq
    from test_svae_custom_loss_host import make_sequence
    from test_svae_routes import _knobs
    _knobs(monkeypatch)
    cls, kw = CONFIGS[cfg]
    kw = dict(kw, lr=kw["lr"] * 0.1)
    models = []
    for custom in (False, True):
        net, sd, model = build_svae(64, seed=41, model_cls=counting(ref_loss) if custom else SVAE)
        model.custom_loss = custom
        model.optimizer = getattr(optim, cls)(net.parameters(), **kw)
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
            assert_one_update("svae %s step %d custom=%s" % (cfg, t, model.custom_loss), model, cls, kw, t + 1, before, states, grads)
        for p, q in zip(models[0][0]._param_list(), models[1][0]._param_list()):
            d = np.abs(host(p) - host(q))
            assert d.max() < 1e-3 and np.mean(d > 2e-5) < 1e-4, (cfg, t, d.max())
    assert models[1][1].calls == 3


# ---------------------------------------------------------------------------------------------- checkpoints
@pytest.mark.parametrize("cfg", ["sgd_mom", "adagrad", "rmsprop_mom", "adamw"])
def test_checkpoint_round_trip(cfg, tmp_path):
    """save_model -> load_model -> one more step equals the uninterrupted run bit for bit (a loaded momentum buffer is not a first
    step); the checkpoint's optimizer entry loads into a plain torch optimizer of the same class with equal state"""
    g = load_golden("g17_optim_mvae_small")
    cls, kw = CONFIGS[cfg]
    net, model = build(g, cfg, "fp32")
    for t in range(2):
        inject(model, g, t)
        model.train_batch(torch.from_numpy(g["xs"][t]))
    path = str(tmp_path / "ckpt.pth")
    model.save_model(path, 1)
    inject(model, g, 2)
    model.train_batch(torch.from_numpy(g["xs"][2]))

    net2, model2 = build(g, cfg, "fp32")
    model2.load_model(path)
    assert model2.gradient_updates == 2.0
    inject(model2, g, 2)
    model2.train_batch(torch.from_numpy(g["xs"][2]))
    for p, q in zip(net._param_list(), net2._param_list()):
        assert torch.equal(p.detach(), q.detach())
        for k in R.state_keys(cls, kw):
            assert torch.equal(model.optimizer.state[p][k], model2.optimizer.state[q][k]), k

    ck = torch.load(path, map_location="cpu")
    plain_params = [torch.nn.Parameter(p.detach().cpu().clone()) for p in net.parameters()]
    plain = getattr(optim, cls)(plain_params, **kw)
    plain.load_state_dict(ck["optimizer"])
    assert set(ck) >= {"epoch", "state_dict", "optimizer"}
    net3, model3 = build(g, cfg, "fp32")
    model3.load_model(path)
    for pp, q in zip(plain_params, net3.parameters()):
        for k, v in plain.state[pp].items():
            assert torch.equal(torch.as_tensor(v).cpu(), torch.as_tensor(model3.optimizer.state[q][k]).cpu()), k
        if R.state_keys(cls, kw) != ("momentum_buffer",):
            assert float(plain.state[pp]["step"]) == 2.0


# ---------------------------------------------------------------------------------------------- learning-rate schedule
@pytest.mark.parametrize("cfg", ["sgd_mom", "rmsprop"])
def test_lr_scheduler_halves_the_step(cfg):
    """StepLR on model.optimizer halves lr after step 1: step 2's move is the float64 rule's at the halved lr; torch's "scheduler
    before optimizer.step()" warning stays quiet"""
    g = load_golden("g17_optim_mvae_small")
    cls, kw = CONFIGS[cfg]
    net, model = build(g, cfg, "fp32")
    sched = optim.lr_scheduler.StepLR(model.optimizer, step_size=1, gamma=0.5)
    inject(model, g, 0)
    model.train_batch(torch.from_numpy(g["xs"][0]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sched.step()
    assert model.optimizer.param_groups[0]["lr"] == kw["lr"] * 0.5
    before, states = snapshot(model, cls, kw)
    inject(model, g, 1)
    model.train_batch(torch.from_numpy(g["xs"][1]))
    grads = [host(p.grad) for p in net._param_list()]
    half = dict(kw, lr=kw["lr"] * 0.5)
    assert_one_update("halved lr", model, cls, half, 2, before, states, grads)
    with pytest.raises(AssertionError):       # ... and is not the rule's at the full lr
        assert_one_update("full lr", model, cls, kw, 2, before, states, grads)


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("make,exc", [
    (lambda ps: optim.Adam(ps, amsgrad=True), ValueError),
    (lambda ps: optim.SGD(ps, lr=0.1, maximize=True), ValueError),
    (lambda ps: optim.RMSprop(ps, centered=True), ValueError),
    (lambda ps: optim.Adam(ps, capturable=True), ValueError),
    (lambda ps: optim.Adamax(ps), TypeError),
    (lambda ps: optim.SGD([{"params": ps[:2]}, {"params": ps[2:]}], lr=0.1), ValueError),
    (lambda ps: optim.SGD(ps[:-1], lr=0.1), ValueError),
])
@pytest.mark.parametrize("custom", [False, True])
def test_refused_optimizers_raise_before_any_launch(make, exc, custom):
    from rectorch_amd.models import MultiVAE
    g = load_golden("g17_optim_mvae_small")

    class Own(MultiVAE):
        def loss_function(self, *args, **kwargs):
            return super().loss_function(*args, **kwargs)

    net, model = build(g, "sgd", "fp32", model_cls=Own if custom else None)
    model.custom_loss = custom
    model.optimizer = make(list(net.parameters()))
    with pytest.raises(exc, match="supported"):
        model.train_batch(torch.from_numpy(g["xs"][0]))
    assert not getattr(net, "_rtx_engines", {})          # no engine was even built
    for k, v in sd_from(g, "sd0__").items():
        assert np.array_equal(net.state_dict()[k].cpu().numpy(), v)


def test_data_parallel_refuses_other_optimizers():
    from rectorch_amd import _lib, parallel
    g = load_golden("g17_optim_mvae_small")
    net, model = build(g, "sgd_mom", "bf16")
    with pytest.raises(_lib.RtxError, match="Adam"):
        parallel.attach(model, emulate_world=2)
    # ... and the engine's own entry points refuse a rule set behind the trainer's back
    net, model = build(g, "adamw", "fp32")
    inject(model, g, 0)
    model.train_batch(torch.from_numpy(g["xs"][0]))
    eng = next(iter(net._rtx_engines.values()))
    step = eng._step(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=2)
    with pytest.raises(_lib.RtxError, match="Adam only"):
        eng.apply_adam_layers(step, 0, 1)
