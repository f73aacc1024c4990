"""GPU (-m gpu): the tile-major optimizer state of the deferred fused step (engine option ``state_tiles``; include/rectorch_hip.h at
``RTX_STEP_DEFER_JOIN``).  Between two deferred fused steps the big layers' ``exp_avg`` / ``exp_avg_sq`` live in engine-owned images in the
order the weight-gradient + Adam kernel walks them; every other entry point gets them written back first.  Nothing may change but where
the bytes lie:

1. the two relayout kernels, bit for bit (tests/native/test_state_tiles.cpp);
2. 8 deferred steps with ``state_tiles`` 1 against 0, same seeds: parameters, both moments and the loss sum identical to the bit -- rows
   of a multiple of four floats and of an odd number (the encoder matrix on the kernel's unaligned epilogue), 4 and 2 K slices (late
   state loads on and off), the big layers alone and every fusable layer (``state_tiles_min_elems = 0``: the grouped launch's hidden layers);
3. 12 steps through every transition -- a joined step, a prediction, a loss read-back, a checkpoint save + restore, moments zeroed by torch
   behind a ``_join()``, a clipped (unfused) step, an engine rebuilt for a larger batch -- identical to the bit as well, with the imports and
   write-backs counted at exactly those points and none between two consecutive deferred steps.
"""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

H, L = 600, 200


@pytest.fixture(scope="module", autouse=True)
def _require_native_path():
    from rectorch_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()


def test_native_driver_state_tiles():
    path = os.path.join(ROOT, "build", "native", "test_state_tiles")
    if not os.path.exists(path):       # (the build step made it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), "-f", "state_tiles.mk"])
    out = subprocess.run([path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "STATE TILES TESTS PASSED (8 cases)" in out.stdout, out.stdout[-3000:]


# ==================================================================================================================== the engine
def make_model(I):
    from rectorch_amd.nets import MultiVAE_net
    from rectorch_amd.models import MultiVAE
    from rectorch_amd.utils import hash_state_dict
    sd = hash_state_dict([I, H, L], [L, H, I], "vae", 9)
    net = MultiVAE_net([L, H, I], [I, H, L], dropout=0.5)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    model = MultiVAE(net, beta=0.2, anneal_steps=0, learning_rate=1e-3, numerics="bf16", predict_numerics="bf16")
    net.to("cuda")
    return net, model


@functools.lru_cache(maxsize=None)
def interactions(I, rows):
    from rectorch_amd.utils import synth_interactions
    return synth_interactions(rows, I, mu=3.5, sigma=0.9, dmax=I // 2, seed=21)


def batches_of(I, B, rows):
    from rectorch_amd.samplers import DataSampler
    return list(DataSampler(interactions(I, rows), batch_size=B, shuffle=False).iter_rows())


def training_engine(net, model, B, tiles, min_elems=None):
    """the training engine for batches of B rows, with the knobs of this run (a rebuilt engine starts from the defaults again)"""
    st, _, m, v = model._ensure_train_state()
    eng = net.rtx_engine("bf16", B, train_buffers=(st.grads, m, v))
    eng.set_option("state_tiles", tiles)
    if min_elems is not None:
        eng.set_option("state_tiles_min_elems", min_elems)
    return eng


def counters(eng):
    return eng.get_option("state_imports"), eng.get_option("state_writebacks")


def state_of(net, model):
    """parameters, exp_avg, exp_avg_sq of every tensor as host arrays (the caller has joined)"""
    torch.cuda.synchronize()
    out = []
    for p in net._param_list():
        s = model.optimizer.state[p]
        out += [p.detach().cpu().numpy().copy(), s['exp_avg'].cpu().numpy().copy(), s['exp_avg_sq'].cpu().numpy().copy()]
    return out


def assert_same_bits(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, k
        assert x.tobytes() == y.tobytes(), "entry %d differs in %d elements" % (k, int(np.sum(x != y)))


@functools.lru_cache(maxsize=None)
def deferred_run(I, B, tiles, min_elems):
    """8 deferred steps with announced batches; returns (state, loss sum, counters before the join, counters behind it, join folds)"""
    net, model = make_model(I)
    batches = batches_of(I, B, 6 * B)
    eng = training_engine(net, model, B, tiles, min_elems)
    torch.manual_seed(31)
    for t in range(8):
        model._fused_step(batches[t % 6], None, want_loss=False, next_x=batches[(t + 1) % 6], defer_join=True)
    open_counts = counters(eng)
    model._join()
    loss = np.float64(model._read_loss_sum())
    return state_of(net, model), loss, open_counts, counters(eng), eng.get_option("join_folds")


# (n_items, batch rows): 3001 puts the encoder matrix's rows at an odd number of floats; 192 rows are 4 K slices (the late half of the state
# loads is on), 64 rows are 2 (off).  min_elems None: the two big matrices; 0: the hidden layers of the grouped launch as well.
@pytest.mark.parametrize("I,B,min_elems,layers", [(3000, 192, None, 2), (3000, 64, None, 2), (3001, 192, None, 2), (3001, 64, None, 2),
                                                  (3000, 192, 0, 4), (3001, 64, 0, 4)])
def test_deferred_steps_tiled_equal_row_major(I, B, min_elems, layers):
    ref_state, ref_loss, ref_open, ref_closed, _ = deferred_run(I, B, 0, None)
    state, loss, open_counts, closed_counts, folds = deferred_run(I, B, 1, min_elems)
    print("n_items %d, batch %d, min_elems %s: imports / write-backs %s -> %s, join folds %d, loss sum %.9g (row-major %.9g)"
          % (I, B, min_elems, open_counts, closed_counts, folds, loss, ref_loss))
    assert ref_open == (0, 0) and ref_closed == (0, 0)
    # one import per tiled layer at the first step, nothing until the join, one write-back per tiled layer there
    assert open_counts == (layers, 0) and closed_counts == (layers, layers)
    assert loss.tobytes() == ref_loss.tobytes()
    assert_same_bits(state, ref_state)


@functools.lru_cache(maxsize=None)
def transition_run(tiles):
    I, B, BIG = 3001, 192, 520          # (BIG: more rows than the engine was built for)
    net, model = make_model(I)
    batches = batches_of(I, B, 6 * B)
    big = batches_of(I, BIG, 6 * B)[0]
    eng = training_engine(net, model, B, tiles)
    torch.manual_seed(31)
    res, trace = [], []

    def step(x, defer=True):
        model._fused_step(x, None, want_loss=False, defer_join=defer)

    for t in range(10):
        if t == 8:
            model.clip_grad_norm = 5.0          # the unfused schedule for one step ...
        step(batches[t % 6], defer=(t != 2))    # (t == 2: a joined step between deferred ones)
        trace.append(counters(eng))
        if t == 8:
            model.clip_grad_norm = None         # ... and back
        if t == 3:                              # an engine call of another kind right behind a deferred step
            res.append(model.predict(batches[0].tr.gather_dense(batches[0].rows[:9]))[0].cpu().numpy())
            net.train()
            trace.append(counters(eng))
        if t == 4:                              # the loss read-back joins first
            res.append(np.float64(model._read_loss_sum()))
            trace.append(counters(eng))
        if t == 5:                              # a checkpoint: saved through torch, restored into new optimizer tensors
            with tempfile.TemporaryDirectory() as d:
                model.save_model(os.path.join(d, "ckpt.pth"), 1)
                trace.append(counters(eng))
                model.load_model(os.path.join(d, "ckpt.pth"))
        if t == 6:                              # torch changes the moments behind a join: the next step must see the zeros
            model._join()
            trace.append(counters(eng))
            model.optimizer.state[net._param_list()[0]]['exp_avg'].zero_()
    eng2 = training_engine(net, model, BIG, tiles)          # rebuilt for the larger batch: the old engine hands its state back first
    assert eng2 is not eng
    trace.append(counters(eng))
    step(big)
    step(batches[1])
    trace2 = [counters(eng2)]
    model._join()
    trace2.append(counters(eng2))
    res.append(np.float64(model._read_loss_sum()))
    return res + state_of(net, model), trace, trace2


def test_transitions_tiled_equal_row_major():
    ref, ref_trace, ref_trace2 = transition_run(0)
    got, trace, trace2 = transition_run(1)
    print("imports / write-backs of the first engine:", trace, "of the rebuilt one:", trace2)
    assert all(c == (0, 0) for c in ref_trace + ref_trace2)
    # in units of the two big layers: (imports, write-backs) behind step 0, 1, 2 (joined: written back at its head), 3, the prediction, 4,
    # the loss read-back, 5, the checkpoint's save, 6 (bound to the restored tensors), the join, 7, 8 (clipped: written back), 9, the rebuild
    want = [(1, 0), (1, 0), (1, 1), (2, 1), (2, 2), (3, 2), (3, 3), (4, 3), (4, 4), (5, 4), (5, 5), (6, 5), (6, 6), (7, 6), (7, 7)]
    assert trace == [(2 * a, 2 * b) for a, b in want]
    assert trace2 == [(2, 0), (2, 2)]       # the rebuilt engine: one import for its two deferred steps, written back at the join
    assert_same_bits(got, ref)
