"""Gradient accumulation on the device, the part that needs no device: the attribute's validation and every refusal that is raised
before a launch, the window bookkeeping of the trainer, the C entry point's argument checks, and the arithmetic of the
accumulating epilogues restated on the host.

Bound.  The kernels store ``s g_1`` (RTX_ACCUM_FIRST) and then ``fma(s, g_i, acc)`` (RTX_ACCUM_ADD): one rounding per micro-step,
each of a partial sum no larger than ``sum_i |s g_i|``, so ``|acc - sum_i s g_i| <= k 2^-24 sum_i |s g_i|`` element-wise, with
``s`` the float32 the device is given.  tests/test_grad_accum_gpu.py judges the device by this bound;
test_float32_chain_meets_the_bound shows the bound is what a correctly rounded float32 chain meets, and that a chain which DROPS
or DOUBLES a term misses it by orders of magnitude.
"""
import ctypes as C

import numpy as np
import pytest
import torch

E24 = 2.0 ** -24


def _model(**attrs):
    from rectorch_amd.nets import MultiVAE_net
    from rectorch_amd.models import MultiVAE
    torch.manual_seed(0)
    net = MultiVAE_net([4, 8, 20], dropout=0.5)
    model = MultiVAE(net, numerics="fp32")
    for k, v in attrs.items():
        setattr(model, k, v)
    return net, model


def test_attribute_default_and_spec():
    from rectorch_amd.models import accum_spec, AETrainer, MultiDAE, CMultiVAE
    from rectorch_amd.nets import MultiDAE_net, CMultiVAE_net
    net, model = _model()
    assert model.accumulate_grad_batches == 1 and model.pending_micro_batches == 0
    assert AETrainer(MultiDAE_net([4, 8, 20])).accumulate_grad_batches == 1
    assert MultiDAE(MultiDAE_net([4, 8, 20])).accumulate_grad_batches == 1
    assert CMultiVAE(CMultiVAE_net(2, [4, 8, 20])).accumulate_grad_batches == 1
    assert accum_spec(1) == 1 and accum_spec(8) == 8 and accum_spec(np.int64(3)) == 3
    for bad in (0, -1, 2.5, 2.0, True, "3", None):
        with pytest.raises(ValueError, match="int >= 1"):
            accum_spec(bad)


@pytest.mark.parametrize("bad", [0, 2.5, True])
def test_bad_values_raise_before_the_device_is_touched(bad):
    net, model = _model(accumulate_grad_batches=bad)
    with pytest.raises(ValueError, match="int >= 1"):
        model.train_batch(torch.zeros(2, 20))
    assert not getattr(net, "_rtx_engines", {})


def test_refusals_that_need_no_device():
    from rectorch_amd import _lib, parallel
    net, model = _model(accumulate_grad_batches=2)
    model._rtx.reducer = object()
    with pytest.raises(_lib.RtxError, match="data-parallel"):
        model.train_batch(torch.zeros(2, 20))
    model._rtx.reducer = None
    model.custom_loss = True                             # the package's own loss_function is not a custom loss: as with k = 1
    with pytest.raises(ValueError, match="loss_function of your own"):
        model.train_batch(torch.zeros(2, 20))
    model.custom_loss = False
    with pytest.raises(_lib.RtxError, match="gradient accumulation"):
        parallel.attach(model, emulate_world=2)
    assert not getattr(net, "_rtx_engines", {})


def test_window_bookkeeping_without_a_device():
    from rectorch_amd import _lib
    net, model = _model(accumulate_grad_batches=3)
    assert model.apply_accumulated() is False            # an empty window: nothing to apply, nothing launched
    model._rtx.accum_pending, model._rtx.accum_k = 2, 3  # (what two micro-steps leave behind)
    assert model.pending_micro_batches == 2
    model.accumulate_grad_batches = 4
    with pytest.raises(_lib.RtxError, match="changed from 3 to 4"):
        model.train_batch(torch.zeros(2, 20))
    model.accumulate_grad_batches = 1                    # back to 1 inside a window is a change too
    with pytest.raises(_lib.RtxError, match="changed from 3 to 1"):
        model.train_batch(torch.zeros(2, 20))
    with pytest.raises(_lib.RtxError, match="apply_accumulated"):
        model.save_model("/nonexistent/never_written.pth", 1)


def test_svae_refuses():
    from rectorch_amd import _lib
    from rectorch_amd.nets import SVAE_net
    from rectorch_amd.models import SVAE
    net = SVAE_net(n_items=40, embed_size=8, rnn_size=8, dec_dims=[4, 8, 40], enc_dims=[8, 8, 4])
    model = SVAE(net)
    model.accumulate_grad_batches = 2
    with pytest.raises(_lib.RtxError, match="packs"):
        model.train_batch(torch.zeros(1, 3, dtype=torch.long), torch.zeros(1, 3, 40))


def test_c_entry_point_checks_its_arguments():
    from rectorch_amd import _lib
    lib = _lib.lib()
    assert (_lib.RTX_ACCUM_OFF, _lib.RTX_ACCUM_FIRST, _lib.RTX_ACCUM_ADD) == (0, 1, 2)
    assert lib.rtx_engine_set_grad_accum(None, _lib.RTX_ACCUM_FIRST, C.c_float(0.5)) != 0
    assert b"engine is NULL" in lib.rtx_last_error()
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "rectorch_hip.h")).read()
    for name, value in (("RTX_ACCUM_OFF", 0), ("RTX_ACCUM_FIRST", 1), ("RTX_ACCUM_ADD", 2)):
        assert "#define %s %d" % (name, value) in header


def _chain(gs, s, drop=None, double=None):
    """the epilogues' arithmetic in float32: s * g_1, then fma(s, g_i, acc) -- the product is exact in float64, the sum rounded once"""
    acc = None
    for i, g in enumerate(gs):
        if i == drop:
            continue
        for _ in range(2 if i == double else 1):
            prod = np.float64(s) * g.astype(np.float64)
            acc = prod.astype(np.float32) if acc is None else (prod + acc.astype(np.float64)).astype(np.float32)
    return acc.astype(np.float64)


@pytest.mark.parametrize("k", [2, 3, 4, 8])
def test_float32_chain_meets_the_bound(k):
    rng = np.random.default_rng(k)
    gs = [(rng.standard_normal(4096) * 10.0 ** rng.integers(-3, 2)).astype(np.float32) for _ in range(k)]
    s = np.float32(1.0 / k)
    want = sum(np.float64(s) * g.astype(np.float64) for g in gs)
    scale = sum(np.abs(np.float64(s) * g.astype(np.float64)) for g in gs)
    bound = k * E24 * scale
    assert np.all(np.abs(_chain(gs, s) - want) <= bound)
    # the bound bites: a dropped or a doubled micro-step misses it by far more than 100 x on most elements
    for wrong in (_chain(gs, s, drop=k - 1), _chain(gs, s, double=0)):
        assert np.median(np.abs(wrong - want) / np.maximum(bound, 1e-300)) > 100


def test_native_driver_host_mode():
    """tests/native/test_accum.cpp --host: the driver's own references (scale * g, fmaf chains), no HIP call"""
    import os
    import subprocess
    from conftest import ROOT
    path = os.path.join(ROOT, "build", "native", "test_accum")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-s", "-f", "accum.mk"])
    out = subprocess.run([path, "--host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "ACCUM TESTS PASSED" in out.stdout and "host reference only" in out.stdout


# ------------------------------------------------------------------------- the recorded torch windows (tests/golden/g19_accum_*.npz)
def _g19():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("make_golden_accum", os.path.join(ROOT, "tests", "golden", "make_golden_accum.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G19 = _g19()
G19_FIXTURES = ["g19_accum_mvae_small", "g19_accum_mdae_small", "g19_accum_mvae_deep"]
G19_CONFIGS = G19.CONFIGS


@pytest.mark.parametrize("name", G19_FIXTURES)
@pytest.mark.parametrize("cfg", sorted(G19_CONFIGS))
def test_float64_accumulate_clip_rule_reproduces_the_reference(name, cfg):
    """"accumulate -> clip -> rule" in float64 (tests/clip_rules64.py, tests/optim_rules64.py) on the recorded accumulated gradients,
    from the recorded previous parameters and states, gives the recorded parameters and states of every window at float32 rounding
    (the bounds of tests/test_grad_clip_host.py), the partial window included; the recorded norm is the float64 norm."""
    from conftest import load_golden, sd_from, params_in_order
    import clip_rules64 as K
    import optim_rules64 as R
    from test_grad_clip_host import g_roundings, NORM_REL
    g = load_golden(name)
    assert sorted(g["configs"]) == sorted(G19_CONFIGS) and int(g["k"]) == G19.K == 3 and int(g["n_micro"]) == 8
    assert [len(w) for w in G19.WINDOWS] == [3, 3, 2]
    sizes = [g["x_%d" % j].shape[0] for j in range(8)]
    assert len(set(sizes[:3])) == 3                                    # micro-batches of unequal sizes
    cls, kw, clip = G19_CONFIGS[cfg]
    kks = [k.replace(".", "__") for k in params_in_order(sd_from(g, "sd0__"))[1]]
    ps = [g["sd0__" + kk].astype(np.float64) for kk in kks]
    states = [R.init_state(cls, kw, p) for p in ps]
    rg, rg2 = g_roundings(clip)
    wd = kw.get("weight_decay", 0.0)
    for w in range(3):
        grads = [g["%s__grad_%d__%s" % (cfg, w, kk)] for kk in kks]
        cg, total, coef = K.clipped(grads, clip)
        total64 = K.total_norm(grads, 2.0)
        assert abs(total64 - float(g["%s__total_norm_%d" % (cfg, w)])) <= NORM_REL * total64
        if cfg == "adam_norm":
            assert coef < 1.0
        for i, kk in enumerate(kks):
            p, state = ps[i], states[i]
            old = {s: v.copy() for s, v in state.items() if v is not None}
            new_p = R.update(cls, kw, w + 1, p, cg[i], state)
            ref_p = g["%s__sd_%d__%s" % (cfg, w, kk)].astype(np.float64)
            G = np.abs(cg[i]) + wd * np.abs(p)
            bound = E24 * (16 * (np.abs(ref_p) + np.abs(ref_p - p)) + rg * kw["lr"] * G)
            assert np.all(np.abs(new_p - ref_p) <= bound), (cfg, kk, w)
            for s in R.state_keys(cls, kw):
                ref_s = g["%s__%s_%d__%s" % (cfg, s, w, kk)].astype(np.float64)
                second = s in ("exp_avg_sq", "sum", "square_avg")
                sb = E24 * (16 * (np.abs(ref_s) + np.abs(old.get(s, 0.0))) + (rg2 * G * G if second else rg * G))
                assert np.all(np.abs(state[s] - ref_s) <= sb), (cfg, kk, w, s)
                state[s] = ref_s
            ps[i] = ref_p


@pytest.mark.parametrize("name", G19_FIXTURES)
def test_fixtures_bite(name):
    """a run that ignores accumulate_grad_batches and updates at every call misses the parity bound of EVERY parameter tensor by a
    factor of 100 or more after every window, for every configuration (recorded, and asserted, by the generator from such a run of
    the reference itself)"""
    from conftest import load_golden
    g = load_golden(name)
    for cfg in sorted(G19_CONFIGS):
        for w in range(3):
            assert float(g["%s__ignored_%d" % (cfg, w)]) >= 100, (name, cfg, w)
