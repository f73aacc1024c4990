"""Training with the model's own optimizer, the part that needs no device: the float64 restatement of the update rules
(tests/optim_rules64.py) against the reference's recorded steps, the translation of ``model.optimizer`` into the engine's rule with
everything it refuses, the optimizer state the device step creates against torch's own first ``step()``, the native driver's host
mode, and the two C entry points."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.optim as optim

from conftest import ROOT, load_golden, sd_from, params_in_order
import optim_rules64 as R

FIXTURES = ["g17_optim_mvae_small", "g17_optim_mdae_small", "g17_optim_mvae_deep"]
E24 = 2.0 ** -24


def _configs():
    spec = importlib.util.spec_from_file_location("make_golden_optim", os.path.join(ROOT, "tests", "golden", "make_golden_optim.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.CONFIGS


CONFIGS = _configs()


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_float64_rules_reproduce_the_reference(name, cfg):
    """Each rule in float64 on the fixture's own gradients, from the fixture's previous parameters and states, gives the fixture's
    next parameters and states at float32 rounding.  torch's float32 update is at most 12 roundings (the longest chain: RMSprop
    with momentum and decay -- decay 2, square_avg 4, sqrt + eps 2, division 1, buffer 2, parameter 2), each relative to a term
    of the computation: the quantity judged, old or new, the step it takes, or the prepared gradient's two terms G = |g| + wd |p|,
    which may cancel (lr G for a parameter, G for a first-moment state, G^2 for a second-moment one).  So 16 x 2^-24 x the sum of
    those scales bounds every element."""
    g = load_golden(name)
    assert cfg in list(g["configs"])
    cls, kw = CONFIGS[cfg]
    keys = params_in_order(sd_from(g, "sd0__"))[1]
    worst = 0.0
    for k in keys:
        kk = k.replace(".", "__")
        p = g["sd0__" + kk].astype(np.float64)
        state = R.init_state(cls, kw, p)
        for t in range(3):
            grad = g["%s__grad_%d__%s" % (cfg, t, kk)]
            old = {s: v.copy() for s, v in state.items() if v is not None}
            new_p = R.update(cls, kw, t + 1, p, grad, state)
            ref_p = g["%s__sd_%d__%s" % (cfg, t, kk)].astype(np.float64)
            G = np.abs(grad.astype(np.float64)) + kw.get("weight_decay", 0.01 if cls == "AdamW" else 0.0) * np.abs(p)
            bound = 16 * E24 * (np.abs(ref_p) + np.abs(ref_p - p) + kw["lr"] * G)
            err = np.abs(new_p - ref_p)
            assert np.all(err <= bound), (cfg, k, t, float(np.max(err / np.maximum(bound, 1e-300))))
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
            assert set(R.state_keys(cls, kw)) == {s for s in state}, (cfg, sorted(state))
            for s in R.state_keys(cls, kw):
                ref_s = g["%s__%s_%d__%s" % (cfg, s, t, kk)].astype(np.float64)
                sb = 16 * E24 * (np.abs(ref_s) + np.abs(old.get(s, 0.0)) + (G * G if s in ("exp_avg_sq", "sum", "square_avg") else G))
                assert np.all(np.abs(state[s] - ref_s) <= sb), (cfg, k, t, s)
                state[s] = ref_s          # the next step starts from what the reference held
            p = ref_p
    print("%s %s: worst error / bound %.3f" % (name, cfg, worst))
    assert worst > 0                      # (a float64 result equal to float32 bits everywhere would mean nothing was compared)


def test_fixture_holds_no_state_for_plain_sgd():
    g = load_golden(FIXTURES[0])
    assert not [k for k in g if k.startswith("sgd__") and "momentum_buffer" in k]
    assert [k for k in g if k.startswith("sgd_mom__momentum_buffer_0__")]


# ------------------------------------------------------------------------------------------------ optimizer -> rule
def _model(opt=None, **kw):
    from rectorch_amd.models import MultiVAE
    from rectorch_amd.nets import MultiVAE_net
    net = MultiVAE_net([3, 5, 12], dropout=0.5)
    model = MultiVAE(net)
    if opt is not None:
        model.optimizer = opt(net.parameters(), **kw)
    return net, model


SUPPORTED = [
    (optim.Adam, {}, dict(kind=0, flags=0, m_key="exp_avg", v_key="exp_avg_sq", keeps_step=True)),
    (optim.Adam, dict(weight_decay=0.1), dict(kind=0, flags=0)),
    (optim.Adam, dict(weight_decay=0.1, decoupled_weight_decay=True), dict(kind=0, flags=1)),
    (optim.AdamW, {}, dict(kind=0, flags=1, m_key="exp_avg", v_key="exp_avg_sq", keeps_step=True)),
    (optim.SGD, dict(lr=0.1), dict(kind=1, flags=0, momentum=0.0, m_key=None, v_key=None, keeps_step=False)),
    (optim.SGD, dict(lr=0.1, momentum=0.9, dampening=0.1), dict(kind=1, flags=0, momentum=0.9, dampening=0.1, m_key="momentum_buffer", v_key=None)),
    (optim.SGD, dict(lr=0.1, momentum=0.9, nesterov=True, weight_decay=0.01), dict(kind=1, flags=2, momentum=0.9, dampening=0.0)),
    (optim.Adagrad, dict(lr_decay=0.1, initial_accumulator_value=0.5), dict(kind=2, flags=0, lr_decay=0.1, m_key=None, v_key="sum", keeps_step=True)),
    (optim.RMSprop, dict(alpha=0.9), dict(kind=3, flags=0, alpha=0.9, momentum=0.0, m_key=None, v_key="square_avg", keeps_step=True)),
    (optim.RMSprop, dict(momentum=0.5), dict(kind=3, alpha=0.99, momentum=0.5, m_key="momentum_buffer", v_key="square_avg")),
]


@pytest.mark.parametrize("cls,kw,want", SUPPORTED, ids=lambda v: getattr(v, "__name__", None) or ",".join(sorted(v)) or "defaults")
def test_supported_optimizers_translate(cls, kw, want):
    from rectorch_amd import _lib
    from rectorch_amd.models import optimizer_spec
    net, model = _model(cls, **kw)
    spec = optimizer_spec(model.optimizer, net._param_list())
    for k, v in want.items():
        assert getattr(spec, k) == v, (k, spec)
    assert (_lib.RTX_OPTIM_ADAM, _lib.RTX_OPTIM_SGD, _lib.RTX_OPTIM_ADAGRAD, _lib.RTX_OPTIM_RMSPROP) == (0, 1, 2, 3)
    assert (_lib.RTX_OPTIM_DECOUPLED, _lib.RTX_OPTIM_NESTEROV, _lib.RTX_OPTIM_FIRST) == (1, 2, 4)


class _MyAdam(optim.Adam):
    pass


class _MySGD(optim.SGD):
    def step(self, closure=None):
        return None


REFUSED = [
    (optim.Adam, dict(amsgrad=True), ValueError, "amsgrad"),
    (optim.AdamW, dict(amsgrad=True), ValueError, "amsgrad"),
    (optim.Adam, dict(maximize=True), ValueError, "maximize"),
    (optim.SGD, dict(lr=0.1, maximize=True), ValueError, "maximize"),
    (optim.Adagrad, dict(maximize=True), ValueError, "maximize"),
    (optim.RMSprop, dict(maximize=True), ValueError, "maximize"),
    (optim.RMSprop, dict(centered=True), ValueError, "centered"),
    (optim.Adam, dict(capturable=True), ValueError, "capturable"),
    (optim.RMSprop, dict(capturable=True), ValueError, "capturable"),
    (optim.Adam, dict(differentiable=True), ValueError, "differentiable"),
    (optim.SGD, dict(lr=0.1, differentiable=True), ValueError, "differentiable"),
    (_MyAdam, {}, TypeError, "_MyAdam"),
    (_MySGD, dict(lr=0.1), TypeError, "_MySGD"),
    (optim.Adamax, {}, TypeError, "Adamax"),
    (optim.Adadelta, {}, TypeError, "Adadelta"),
    (optim.NAdam, {}, TypeError, "NAdam"),
]


@pytest.mark.parametrize("cls,kw,exc,word", REFUSED, ids=lambda v: getattr(v, "__name__", None) or (v if isinstance(v, str) else None))
def test_refused_optimizers_raise_and_name_what_is_supported(cls, kw, exc, word):
    from rectorch_amd.models import optimizer_spec
    net, model = _model(cls, **kw)
    with pytest.raises(exc, match=word) as e:
        optimizer_spec(model.optimizer, net._param_list())
    for name in ("Adam", "AdamW", "SGD", "Adagrad", "RMSprop"):
        assert name in str(e.value)
    # ... and the trainer raises the same before anything else happens (no device is needed to get there)
    with pytest.raises(exc, match=word):
        model._ensure_optim_state(net._param_list())


def test_param_groups_must_be_the_networks_parameters():
    from rectorch_amd.models import optimizer_spec
    net, model = _model()
    ps = list(net.parameters())
    with pytest.raises(ValueError, match="2 param groups"):
        optimizer_spec(optim.SGD([{"params": ps[:2]}, {"params": ps[2:]}], lr=0.1), net._param_list())
    with pytest.raises(ValueError, match="not exactly the network's"):
        optimizer_spec(optim.SGD(ps[:-1], lr=0.1), net._param_list())
    with pytest.raises(ValueError, match="not exactly the network's"):
        optimizer_spec(optim.SGD(ps[:-1] + [torch.nn.Parameter(torch.zeros_like(ps[-1]))], lr=0.1), net._param_list())


def test_data_parallel_refuses_other_optimizers():
    from rectorch_amd import _lib, parallel
    net, model = _model(optim.SGD, lr=0.1, momentum=0.9)
    with pytest.raises(_lib.RtxError, match="Adam"):
        parallel.attach(model, engine="python")


# ------------------------------------------------------------------------------------------------ state creation
@pytest.mark.parametrize("cfg", sorted(CONFIGS) + ["adam"])
def test_state_creation_equals_torchs_first_step(cfg):
    """keys, dtypes, shapes and ``step`` of ``optimizer.state`` after the device step's state creation and step bookkeeping equal
    those after one ``step()`` of the same torch optimizer"""
    cls, kw = CONFIGS.get(cfg, ("Adam", dict(lr=1e-3)))
    net, model = _model(getattr(optim, cls), **kw)
    params = net._param_list()
    spec, m, v = model._ensure_optim_state(params)
    assert len(m) == len(v) == len(params)
    for p, mm, vv in zip(params, m, v):
        assert mm.shape == p.shape and vv.shape == p.shape and mm.dtype == vv.dtype == torch.float32
        assert (mm.data_ptr() == p.data_ptr()) == (spec.m_key is None) and (vv.data_ptr() == p.data_ptr()) == (spec.v_key is None)
    if cls == "Adagrad":
        assert all(float(t.min()) == float(t.max()) == np.float32(kw["initial_accumulator_value"]) for t in v)
    else:
        assert all(float(t.abs().max()) == 0.0 for k, ts in ((spec.m_key, m), (spec.v_key, v)) if k for t in ts)
    assert model._rtx.sgd_first == (cls == "SGD" and kw.get("momentum", 0) != 0)
    model._rtx.adam_step = 1                      # what one device step leaves
    model._optim_stepped(spec, write_step=True)
    assert model._rtx.sgd_first is False and model.optimizer._opt_called is True

    twin_net, twin = _model(getattr(optim, cls), **kw)
    for p in twin_net.parameters():
        p.grad = torch.ones_like(p)
    twin.optimizer.step()
    for p, q in zip(params, twin_net._param_list()):
        ours, theirs = model.optimizer.state.get(p, {}), twin.optimizer.state.get(q, {})
        assert sorted(ours) == sorted(theirs), (cfg, sorted(ours), sorted(theirs))
        for k in theirs:
            assert ours[k].dtype == theirs[k].dtype and ours[k].shape == theirs[k].shape and ours[k].device == theirs[k].device, (cfg, k)
        if "step" in theirs:
            assert float(ours["step"]) == float(theirs["step"]) == 1.0
    assert len(model.optimizer.state) == len(twin.optimizer.state)     # (plain SGD: torch never touches it, nor does the step)
    # state_dict round trip into a plain torch optimizer of the same class
    fresh_net, fresh = _model(getattr(optim, cls), **kw)
    fresh.optimizer.load_state_dict(model.optimizer.state_dict())


def test_a_new_optimizer_counts_its_own_steps_and_a_loaded_buffer_is_not_a_first_step():
    net, model = _model()
    params = net._param_list()
    model._ensure_optim_state(params)
    model._rtx.adam_step = 7
    model.optimizer = optim.Adagrad(net.parameters(), lr=0.1)
    model._ensure_optim_state(params)
    assert model._rtx.adam_step == 0
    donor_net, donor = _model(optim.SGD, lr=0.1, momentum=0.9)
    for p in donor_net.parameters():
        p.grad = torch.ones_like(p)
    donor.optimizer.step()
    model.optimizer = optim.SGD(net.parameters(), lr=0.1, momentum=0.9)
    model.optimizer.load_state_dict(donor.optimizer.state_dict())
    model._ensure_optim_state(params)
    assert model._rtx.sgd_first is False


# ------------------------------------------------------------------------------------------------ native driver, ABI
def test_native_driver_host_mode():
    path = os.path.join(ROOT, "build", "native", "test_optim")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-s", "-f", "optim.mk"])
    out = subprocess.run([path, "--host"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "OPTIM TESTS PASSED" in out.stdout and "host reference only" in out.stdout


@pytest.mark.parametrize("name", ["rtx_engine_set_optimizer", "rtx_svae_set_optimizer"])
def test_set_optimizer_is_exported_declared_and_bound(name):
    from rectorch_amd import _lib
    raw = C.CDLL(_lib.build())
    assert hasattr(raw, name)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rectorch_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in the header" % name
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 2 and args[1] == "const rtx_optim* optim"
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int and argtypes == [C.c_void_p, C.POINTER(_lib.Optim)]
    # int32 x 2, double x 4, in the header's order
    assert C.sizeof(_lib.Optim) == 40 and _lib.Optim.momentum.offset == 8 and [f[0] for f in _lib.Optim._fields_] == ["kind", "flags", "momentum", "dampening", "alpha", "lr_decay"]
    body = re.search(r"typedef struct \{([^}]*)\} rtx_optim;", text).group(1)
    assert re.findall(r"\b(kind|flags|momentum|dampening|alpha|lr_decay)\b", body) == ["kind", "flags", "momentum", "dampening", "alpha", "lr_decay"]
    assert _lib.lib().rtx_abi_version() == 8
    # NULL arguments are refused before anything else
    assert _lib.lib()[name](None, None) != 0
