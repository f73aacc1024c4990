"""Gradient clipping on the device, the part that needs no device: the float64 restatement of the three modes
(tests/clip_rules64.py) composed with the optimizer rules (tests/optim_rules64.py) against the reference's recorded clipped steps
(tests/golden/g18_clip_*.npz), the translation of the model's clip attributes with everything it refuses, the native driver's host
mode, and the C entry points.

Bounds.  The recorded steps are torch's float32 ones.  ``clip_grad_norm_`` returns a float32 norm: the sum of at most 2^13 squares
by torch's cascade summation (at most 13 levels and 8 vector lanes of partial sums: under 32 roundings on the sum, half of that on
its root) and the root's own rounding -- the recorded norm is within 32 x 2^-24 relative of the float64 one.  The coefficient adds
three roundings (+ 1e-6, max_norm as float32, the division): 40 x 2^-24.  A clipped gradient is the product with it, one more
rounding, so against the float64 clipped gradient G the recorded step saw G (1 + d), |d| <= 40 x 2^-24.  The one-update bound of
tests/test_optimizers_host.py -- 16 x 2^-24 x (the quantity judged, old and new, the step it takes, lr G for a parameter, G for a
first-moment state, G^2 for a second-moment one) -- therefore holds with 16 + 40 on the G terms of a norm configuration and
16 + 2 x 40 on the G^2 terms; value clipping is exact in float32 and keeps 16 everywhere.
"""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, sd_from, params_in_order
import clip_rules64 as K
import optim_rules64 as R

FIXTURES = ["g18_clip_mvae_small", "g18_clip_mdae_small", "g18_clip_mvae_deep"]
E24 = 2.0 ** -24
NORM_REL = 32 * E24         # the recorded float32 total norm against the float64 one
COEF_REL = 40 * E24         # ... and the coefficient


def _configs():
    spec = importlib.util.spec_from_file_location("make_golden_clip", os.path.join(ROOT, "tests", "golden", "make_golden_clip.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.CONFIGS


CONFIGS = _configs()
INF = float("inf")


def g_roundings(clip):
    """(roundings on a G term, on a G^2 term) of one recorded update under ``clip``"""
    return (16, 16) if not clip or "value" in clip else (16 + 40, 16 + 80)


# ------------------------------------------------------------------------------------------------ the restatement
def test_three_modes_on_small_vectors():
    g = [np.array([3.0, -4.0]), np.array([[12.0]])]
    out, total, c = K.clip_norm(g, 6.5)
    assert total == 13.0 and abs(c - 6.5 / (13.0 + 1e-6)) < 1e-15 and np.allclose(out[0], np.array([3.0, -4.0]) * c)
    out, total, c = K.clip_norm(g, 6.0, INF)
    assert total == 12.0 and abs(c - 6.0 / (12.0 + 1e-6)) < 1e-15
    out, total, c = K.clip_norm(g, INF)                 # torch's idiom for reading the norm
    assert total == 13.0 and c == 1.0 and np.array_equal(out[0], g[0])
    out, total, c = K.clip_norm([np.zeros(3)], 1.0)
    assert total == 0.0 and c == 1.0
    out, total, c = K.clip_norm([np.array([1.0, INF])], 1.0)
    assert total == INF and c == 0.0 and out[0][0] == 0.0 and np.isnan(out[0][1])
    out, total, c = K.clip_norm([np.array([1.0, np.nan])], 1.0)
    assert np.isnan(total) and np.isnan(c) and np.all(np.isnan(out[0]))
    assert np.isnan(K.total_norm([np.array([1.0, np.nan]), np.array([5.0])], INF))
    v = K.clip_value([np.array([-2.0, 0.25, 7.0, np.nan])], 0.5)[0]
    assert np.array_equal(v[:3], [-0.5, 0.25, 0.5]) and np.isnan(v[3])
    # ... and torch agrees (float64 tensors: no rounding in the way)
    ts = [torch.tensor([3.0, -4.0], dtype=torch.float64), torch.tensor([[12.0]], dtype=torch.float64)]
    for t in ts:
        t.grad = t.clone()
    tot = torch.nn.utils.clip_grad_norm_(ts, 6.5)
    out, total, c = K.clip_norm(g, 6.5)
    assert float(tot) == total and all(np.allclose(t.grad.numpy(), o, rtol=1e-15) for t, o in zip(ts, out))


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_float64_clip_and_rules_reproduce_the_reference(name, cfg):
    """The clip in float64 on the fixture's own unclipped gradients, then the rule in float64 from the fixture's previous parameters
    and states, gives the fixture's recorded total norm, coefficient, next parameters and states at float32 rounding."""
    g = load_golden(name)
    assert cfg in list(g["configs"])
    cls, kw, clip = CONFIGS[cfg]
    keys = params_in_order(sd_from(g, "sd0__"))[1]
    kks = [k.replace(".", "__") for k in keys]
    ps = [g["sd0__" + kk].astype(np.float64) for kk in kks]
    states = [R.init_state(cls, kw, p) for p in ps]
    rg, rg2 = g_roundings(clip)
    wd = kw.get("weight_decay", 0.01 if cls == "AdamW" else 0.0)
    worst = 0.0
    for t in range(3):
        grads = [g["%s__grad_%d__%s" % (cfg, t, kk)] for kk in kks]
        cg, total, coef = K.clipped(grads, clip)
        if "value" not in clip:
            ref_total, ref_coef = float(g["%s__total_norm_%d" % (cfg, t)]), float(g["%s__coef_%d" % (cfg, t)])
            assert abs(total - ref_total) <= NORM_REL * total, (cfg, t, total, ref_total)
            assert abs(coef - ref_coef) <= COEF_REL * coef, (cfg, t, coef, ref_coef)
            assert (coef == 1.0) == (cfg == "adam_norm_loose")
        else:
            assert "%s__total_norm_%d" % (cfg, t) not in g
        for i, kk in enumerate(kks):
            p, state = ps[i], states[i]
            old = {s: v.copy() for s, v in state.items() if v is not None}
            new_p = R.update(cls, kw, t + 1, p, cg[i], state)
            ref_p = g["%s__sd_%d__%s" % (cfg, t, kk)].astype(np.float64)
            G = np.abs(cg[i]) + wd * np.abs(p)
            bound = E24 * (16 * (np.abs(ref_p) + np.abs(ref_p - p)) + rg * kw["lr"] * G)
            err = np.abs(new_p - ref_p)
            assert np.all(err <= bound), (cfg, kk, t, float(np.max(err / np.maximum(bound, 1e-300))))
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
            assert set(R.state_keys(cls, kw)) == {s for s in state}, (cfg, sorted(state))
            for s in R.state_keys(cls, kw):
                ref_s = g["%s__%s_%d__%s" % (cfg, s, t, kk)].astype(np.float64)
                second = s in ("exp_avg_sq", "sum", "square_avg")
                sb = E24 * (16 * (np.abs(ref_s) + np.abs(old.get(s, 0.0))) + (rg2 * G * G if second else rg * G))
                assert np.all(np.abs(state[s] - ref_s) <= sb), (cfg, kk, t, s)
                state[s] = ref_s          # the next step starts from what the reference held
            ps[i] = ref_p
    print("%s %s: worst error / bound %.3f" % (name, cfg, worst))
    assert worst > 0


@pytest.mark.parametrize("name", FIXTURES)
def test_unclipped_rules_miss_the_clipped_fixture(name):
    """what the fixtures were made for: the same float64 rule WITHOUT the clip is far outside the bound at the first step"""
    g = load_golden(name)
    keys = [k.replace(".", "__") for k in params_in_order(sd_from(g, "sd0__"))[1]]
    for cfg in ("sgd_norm", "adagrad_norm"):
        cls, kw, clip = CONFIGS[cfg]
        for kk in keys:
            p = g["sd0__" + kk].astype(np.float64)
            new_p = R.update(cls, kw, 1, p, g["%s__grad_0__%s" % (cfg, kk)], R.init_state(cls, kw, p))
            ref_p = g["%s__sd_0__%s" % (cfg, kk)].astype(np.float64)
            assert np.max(np.abs(new_p - ref_p)) > 0.5 * np.max(np.abs(ref_p - p)), (cfg, kk)


# ------------------------------------------------------------------------------------------------ attributes -> mode
def _model(**attrs):
    from rectorch_amd.models import MultiVAE
    from rectorch_amd.nets import MultiVAE_net
    net = MultiVAE_net([3, 5, 12], dropout=0.5)
    model = MultiVAE(net)
    for k, v in attrs.items():
        setattr(model, k, v)
    return net, model


def test_defaults_and_supported_settings_translate():
    from rectorch_amd import _lib
    from rectorch_amd.models import grad_clip_spec
    net, model = _model()
    assert model.clip_grad_norm is None and model.clip_grad_norm_type == 2.0 and model.clip_grad_value is None
    assert model.last_grad_norm is None
    assert grad_clip_spec(model) == (_lib.RTX_CLIP_NONE, 0.0)
    assert grad_clip_spec(_model(clip_grad_norm=2.5)[1]) == (_lib.RTX_CLIP_NORM2, 2.5)
    assert grad_clip_spec(_model(clip_grad_norm=1, clip_grad_norm_type=INF)[1]) == (_lib.RTX_CLIP_NORMINF, 1.0)
    assert grad_clip_spec(_model(clip_grad_norm=INF)[1]) == (_lib.RTX_CLIP_NORM2, INF)
    assert grad_clip_spec(_model(clip_grad_value=0.5)[1]) == (_lib.RTX_CLIP_VALUE, 0.5)
    assert grad_clip_spec(_model(clip_grad_value=0.5, clip_grad_norm_type=3.0)[1]) == (_lib.RTX_CLIP_VALUE, 0.5)    # (unused: not looked at)
    assert (_lib.RTX_CLIP_NONE, _lib.RTX_CLIP_NORM2, _lib.RTX_CLIP_NORMINF, _lib.RTX_CLIP_VALUE) == (0, 1, 2, 3)


REFUSED = [
    (dict(clip_grad_norm=1.0, clip_grad_norm_type=1.0), "clip_grad_norm_type"),
    (dict(clip_grad_norm=1.0, clip_grad_norm_type=3.0), "clip_grad_norm_type"),
    (dict(clip_grad_norm=1.0, clip_grad_norm_type=0.0), "clip_grad_norm_type"),
    (dict(clip_grad_norm=1.0, clip_grad_value=1.0), "both"),
    (dict(clip_grad_norm=-1.0), "clip_grad_norm"),
    (dict(clip_grad_value=-0.5), "clip_grad_value"),
    (dict(clip_grad_norm=float("nan")), "clip_grad_norm"),
    (dict(clip_grad_norm=1.0, clip_grad_error_if_nonfinite=True), "error_if_nonfinite"),
]


@pytest.mark.parametrize("attrs,word", REFUSED, ids=lambda v: v if isinstance(v, str) else ",".join("%s=%s" % kv for kv in sorted(v.items())))
def test_refused_settings_raise_and_name_what_is_supported(attrs, word):
    from rectorch_amd.models import grad_clip_spec
    net, model = _model(**attrs)
    with pytest.raises(ValueError, match=word) as e:
        grad_clip_spec(model)
    for name in ("clip_grad_norm", "clip_grad_norm_type", "clip_grad_value", "inf"):
        assert name in str(e.value)
    # ... and the trainer raises the same before anything else happens (no device is needed to get there)
    with pytest.raises(ValueError, match=word):
        model.train_batch(torch.zeros(2, 12))
    assert not getattr(net, "_rtx_engines", {})


def test_svae_refuses_the_same_way():
    from rectorch_amd.models import SVAE
    from rectorch_amd.nets import SVAE_net
    net = SVAE_net(n_items=12, embed_size=4, rnn_size=5, dec_dims=[3, 6, 12], enc_dims=[5, 6, 3])
    model = SVAE(net)
    assert model.clip_grad_norm is None and model.last_grad_norm is None
    model.clip_grad_norm, model.clip_grad_norm_type = 1.0, 1.0
    with pytest.raises(ValueError, match="clip_grad_norm_type"):
        model.train_batch(torch.zeros(1, 4, dtype=torch.long), torch.zeros(1, 4, 12))


def test_data_parallel_refuses_clipping():
    from rectorch_amd import _lib, parallel
    for attrs in (dict(clip_grad_norm=1.0), dict(clip_grad_value=1.0)):
        net, model = _model(**attrs)
        with pytest.raises(_lib.RtxError, match="clip"):
            parallel.attach(model, engine="python")


def test_settings_are_not_optimizer_state():
    """checkpoints are untouched: the settings are attributes of the trainer, nothing of them enters optimizer.state_dict()"""
    net, model = _model(clip_grad_norm=1.0)
    plain = _model()[1]
    assert sorted(model.optimizer.state_dict()) == sorted(plain.optimizer.state_dict())
    assert model.optimizer.state_dict()["param_groups"] == plain.optimizer.state_dict()["param_groups"]


# ------------------------------------------------------------------------------------------------ native driver, ABI
def test_native_driver_host_mode():
    path = os.path.join(ROOT, "build", "native", "test_clip")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-s", "-f", "clip.mk"])
    out = subprocess.run([path, "--host"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "CLIP TESTS PASSED" in out.stdout and "host reference only" in out.stdout


@pytest.mark.parametrize("name,n_args", [("rtx_engine_set_grad_clip", 3), ("rtx_svae_set_grad_clip", 3), ("rtx_engine_wait_grad_norm", 4),
                                         ("rtx_svae_wait_grad_norm", 3), ("rtx_grad_norm", 6)])
def test_entry_points_are_exported_declared_and_bound(name, n_args):
    from rectorch_amd import _lib
    raw = C.CDLL(_lib.build())
    assert hasattr(raw, name)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rectorch_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in the header" % name
    assert len(m.group(1).split(",")) == n_args
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int and len(argtypes) == n_args
    assert re.search(r"#define RTX_CLIP_NONE 0\n#define RTX_CLIP_NORM2 1\n#define RTX_CLIP_NORMINF 2\n#define RTX_CLIP_VALUE 3\n", text)
    assert _lib.lib().rtx_abi_version() == 8
    # NULL handles / arguments are refused before anything else
    if name.endswith("set_grad_clip"):
        assert getattr(_lib.lib(), name)(None, 1, 1.0) != 0
    elif name == "rtx_engine_wait_grad_norm":
        assert getattr(_lib.lib(), name)(None, 1, None, 0.0) != 0
    elif name == "rtx_svae_wait_grad_norm":
        assert getattr(_lib.lib(), name)(None, None, 0.0) != 0
    else:
        assert getattr(_lib.lib(), name)(None, None, 0, 2.0, None, None) != 0
