"""The draw contract of the engine's counter RNG (include/rectorch_hip.h, at ``rtx_step``): which element gets which Philox draw.

The reference is oracle/philox_oracle.py (numpy integers and float64).  The CPU tests tie it to the published known answers
of Philox4x32-10 and to a host build of the very header the kernels compile (tests/native/philox_host.cpp).  The device tests
make the networks transparent -- identity first layer, zeroed VAE head, identity decoder -- so that the outputs of the public
entry points ARE the dropout decisions and the noise, and compare them with the reference element by element, on every path
that draws: dense and CSR batches, the scatter image, the sparse first layer, the prefetched batch, CMultiVAE's condition
columns, both VAE heads, VAE_net's eval-mode sampling and the sequence model.

The one measured tolerance (float32 normals against the float64 reference, ``|got - ref| <= tol * max(1, |ref|)``)
--------------------------------------------------------------------------------------------------------------------
Measured with the host build over the 131 072 indices ``0 .. 2^17 - 1`` of (SEED, offset 2^33 + 5):

    worst error, all draws                    5.76e-6   -> TOL       = 8 x that = 4.61e-5
    worst error, draws with (x >> 8) < 2^23   1.52e-7   -> TOL_EXACT = 8 x that = 1.22e-6
    worst on the MI355X over the 5 796 float32 draws these tests look at:  all draws 5.03e-7, (x >> 8) < 2^23: 1.70e-7

Why two lines: ``rtx_normal`` forms u1 = ((x >> 8) + 0.5) * 2^-24 in float32, and for (x >> 8) >= 2^23 the sum k + 0.5 has 25
significant bits: float32 rounds it to the even neighbour, so u1 is off by 2^-25 (and k = 2^24 - 1 gives u1 = 1, eps = 0).
Through sqrt(-2 ln u1) that is an absolute error of about 3e-8 / |eps| in the draws NEAR ZERO (u1 near 1) -- 2.4e-4 at the
very worst, one draw in 2^24; the sample's worst is 5.8e-6 -- while logf / sqrtf / cosf themselves contribute 1.5e-7.  It is a
property of the float32 formula, shared bit for bit by the host build and every device path, harmless to the
distribution, and left as it is: changing it would change every run's noise.  Both bounds are asserted: TOL on every draw
(the rule: 8 x the host build's worst), TOL_EXACT on the half of the draws whose u1 float32 holds exactly.  Two different
draws differ by O(1), four orders of magnitude above TOL: a wrong index cannot hide in it.  bf16 outputs add one bf16
rounding, relative 2^-8.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import philox_oracle as po

SEED = 0x9E3779B97F4A7C15          # bits above 32 set
OFFSETS = (0, 1, 2 ** 33 + 5)      # 0 / 1: what models.py passes as rank 0 / 1; the last one has bits above 32
HOST_WORST, HOST_WORST_EXACT = 5.76e-6, 1.52e-7      # measured with the host build (docstring above)
TOL, TOL_EXACT = 8 * HOST_WORST, 8 * HOST_WORST_EXACT
BF16 = 2.0 ** -8                   # one bf16 rounding, relative


def _normal_errors(got, seed, offset, index):
    """(worst error over all draws, worst over the draws whose u1 is exact in float32), each relative to max(1, |ref|)"""
    index = np.asarray(index, dtype=np.uint64)
    ref = po.normal(seed, offset, index)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    k = po.philox4x32_10(seed, int(offset) ^ po.NOISE_STREAM, index)[0] >> np.uint32(8)
    exact = k < 2 ** 23
    return float(err.max()), float(np.max(err[exact], initial=0.0))


# =============================================================================================================== CPU: the reference
KNOWN_ANSWERS = [   # Random123's kat_vectors for philox4x32-10: counter, key -> output
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_reference_reproduces_the_known_answers(counter, key, want):
    assert " ".join("%08x" % int(w) for w in po.philox4x32(counter, key)) == want
    # the same through the engine's (seed, offset, index) packing: index = counter words 0-1, offset = 2-3, seed = key
    index = np.array([counter[0] | (counter[1] << 32)], dtype=np.uint64)
    words = po.philox4x32_10(key[0] | (key[1] << 32), counter[2] | (counter[3] << 32), index)
    assert " ".join("%08x" % int(w[0]) for w in words) == want


def test_reference_layouts_index_by_batch_position_and_real_width():
    keep = po.dropout_mask(SEED, 7, 5, 77, 0.5)
    eps = po.noise(SEED, 7, 5, 21)
    assert keep.shape == (5, 77) and eps.shape == (5, 21) and keep.dtype == np.bool_ and eps.dtype == np.float64
    assert keep[3, 11] == po.dropout_keep(SEED, 7, np.uint64(3 * 77 + 11), 0.5)
    assert eps[4, 20] == po.normal(SEED, 7, np.uint64(4 * 21 + 20))
    # the noise is drawn on another stream than the dropout decisions: words x of the two streams differ
    idx = np.arange(64, dtype=np.uint64)
    assert not np.array_equal(po.philox4x32_10(SEED, 7, idx)[0], po.philox4x32_10(SEED, 7 ^ po.NOISE_STREAM, idx)[0])
    # 15 400 decisions / 10 000 normals: the keep rate is 1 - p to 5 sigma (0.02), the normals have unit variance to 5 sigma (0.035)
    assert abs(po.dropout_mask(SEED, 7, 200, 77, 0.3).mean() - 0.7) < 0.02 and abs(po.noise(SEED, 0, 200, 50).std() - 1.0) < 0.035


_HOST_BUILT = []


def _host_draws(seed, offset, index, p):
    """words [n][4], decisions [n], normals [n] (float32) of csrc/rtx_common.h compiled for the host (arrays of equal length)"""
    exe = os.path.join(ROOT, "build", "native", "philox_host")
    if not _HOST_BUILT:      # (build() makes it with the other native drivers; this is a no-op then)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), "../../build/native/philox_host"])
        _HOST_BUILT.append(exe)
    text = "".join("%d %d %d %.9g\n" % (int(s), int(o), int(i), float(q)) for s, o, i, q in zip(seed, offset, index, p))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    a = np.array([int(t, 16) for t in out], dtype=np.uint64).reshape(len(index), 6)
    return a[:, :4].astype(np.uint32), a[:, 4].astype(bool), a[:, 5].astype(np.uint32).view(np.float32)


def test_host_build_of_the_shipped_header_equals_the_reference():
    """a few thousand (seed, offset, index, p): seeds and offsets with bits above 32, indices above 2^32, p in {0.1, 0.5, 0.9};
    words and decisions exactly, normals within TOL / TOL_EXACT"""
    rng = np.random.default_rng(11)
    seeds = [0, 1, 42, SEED, 2 ** 64 - 1, 0x1234567800000000]
    offsets = [0, 1, 7, 2 ** 33 + 5, 2 ** 64 - 1, po.NOISE_STREAM]
    index = np.concatenate([np.arange(40, dtype=np.uint64), np.uint64(2 ** 32) + np.arange(-20, 20).astype(np.uint64),
                            rng.integers(0, 2 ** 63, 40, dtype=np.uint64) * np.uint64(2) + np.uint64(1)])
    cases = [(s, o, p) for s in seeds for o in offsets for p in (0.1, 0.5, 0.9)]
    k = len(index)
    words, keep, nrm = _host_draws([c[0] for c in cases for _ in range(k)], [c[1] for c in cases for _ in range(k)],   # (Python ints:
                                   np.tile(index, len(cases)), [c[2] for c in cases for _ in range(k)])               # 64 bits)
    worst = worst_exact = 0.0
    n = 0
    for ci, (s, o, p) in enumerate(cases):
        sl = slice(ci * k, (ci + 1) * k)
        want = po.philox4x32_10(s, o, index)
        for c in range(4):
            assert np.array_equal(words[sl, c], want[c]), (s, o, c)
        assert np.array_equal(keep[sl], po.dropout_keep(s, o, index, p)), (s, o, p)
        e_all, e_exact = _normal_errors(nrm[sl], s, o, index)
        worst, worst_exact, n = max(worst, e_all), max(worst_exact, e_exact), n + k
    print("host build, %d draws: worst normal error %.3g (u1 exact: %.3g)" % (n, worst, worst_exact))
    assert n >= 3000 and worst <= TOL and worst_exact <= TOL_EXACT


def _native(name, *args):
    """builds tests/native/<name> (build() has made it already; this is a no-op then) and runs it"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), "../../build/native/" + name])
    return subprocess.run([os.path.join(ROOT, "build", "native", name), *args], capture_output=True, text=True, timeout=300)


HOST_DRIVERS = [("test_loss", "LOSS TESTS PASSED"), ("test_layers", "LAYER TESTS PASSED"), ("test_adam", "ADAM TESTS PASSED"),
                ("test_solver", "SOLVER TESTS PASSED"), ("test_batch", "BATCH TESTS PASSED")]


@pytest.mark.parametrize("exe,closing", HOST_DRIVERS, ids=[d[0] for d in HOST_DRIVERS])
def test_driver_reference_holds_on_the_host(exe, closing):
    """tests/native/<exe>.cpp --host: no HIP call; the driver's case generators and float64 references against a second, independent
    formulation in long double, the conditions its bounds assume, and the refusals and returns of the launchers that come before
    the first HIP call (what each driver checks: the head comment of its source)"""
    out = _native(exe, "--host")
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert closing in out.stdout and "FAIL" not in out.stdout


def test_the_native_harness_can_fail():
    """tests/native/check_selftest.cpp: no HIP call; the judging, the guard scan, the poison and the closing line of tests/native/check.h,
    which every native float64 driver shares, each fed a case it must reject"""
    out = _native("check_selftest")
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "CHECK SELFTEST HOLDS" in out.stdout and "WRONG" not in out.stdout


def test_host_build_normals_the_measurement_behind_the_tolerance():
    """the 131 072 indices the tolerance was measured on: the recorded worst errors still hold (so TOL is 8 x a measured value)"""
    n = 1 << 17
    index = np.arange(n, dtype=np.uint64)
    words, _, nrm = _host_draws([SEED] * n, [OFFSETS[2]] * n, index, [0.5] * n)
    assert np.array_equal(words[:, 0], po.philox4x32_10(SEED, OFFSETS[2], index)[0])
    e_all, e_exact = _normal_errors(nrm, SEED, OFFSETS[2], index)
    print("host build, %d normals: worst error %.4g, with u1 exact in float32 %.4g" % (n, e_all, e_exact))
    assert e_all <= HOST_WORST and e_exact <= HOST_WORST_EXACT


# =============================================================================================================== device: helpers
N_ITEMS, BATCH, N_ROWS = 77, 37, 64
_WORST = {"all": 0.0, "exact": 0.0, "n": 0}      # worst device normal error over the session (printed by the last test)


def _matrix(n_items=N_ITEMS, cond=0, seed=2024):
    """64 x n_items ratings in 1..5 (so ||x|| matters): rows 0, 5, 10, ... store EVERY column, row 3 none, the rest ~15 %;
    `cond` extra columns carry a one-hot 2.0.  Returns (dense [64][n_items + cond], batch row ids: 37 shuffled rows)"""
    rng = np.random.default_rng(seed)
    dense = np.where(rng.random((N_ROWS, n_items)) < 0.15, rng.integers(1, 6, (N_ROWS, n_items)), 0).astype(np.float64)
    dense[::5] = rng.integers(1, 6, dense[::5].shape)
    dense[3] = 0
    if cond:
        c = np.zeros((N_ROWS, cond))
        c[np.arange(N_ROWS), np.arange(N_ROWS) % cond] = 2.0
        dense = np.concatenate([dense, c], axis=1)
    forced = [10, 3, 0, 55]
    rest = [int(r) for r in rng.permutation(N_ROWS) if r not in forced][:BATCH - len(forced)]
    for at, r in zip((1, 7, 20, 36), forced):
        rest.insert(at, r)
    rows = np.array(rest, dtype=np.int32)
    assert len(rows) == BATCH and len(set(rest)) == BATCH and not np.array_equal(rows, np.sort(rows))
    return dense, rows


def _row_batch(dense, rows):
    import torch
    from scipy.sparse import csr_matrix
    from rectorch_amd.engine import CsrMatrix, RowBatch
    return RowBatch(CsrMatrix(csr_matrix(dense.astype(np.float32))), None, torch.from_numpy(rows).cuda())


def _engine(enc, dec, variant, numerics, p, cond=0, fill=None):
    """an Engine bound to fresh parameter / gradient / Adam tensors; `fill(t, array)` sets parameter t (zeros otherwise)"""
    import torch
    from rectorch_amd import _lib
    from rectorch_amd.engine import Engine
    eng = Engine(enc, dec, variant, p, numerics, max_batch=N_ROWS, cond_dim=cond)
    params = []
    r, c = ctypes.c_int32(), ctypes.c_int32()
    for t in range(eng.n_tensors):
        _lib.check(_lib.lib().rtx_engine_tensor_shape(eng.handle, t, ctypes.byref(r), ctypes.byref(c)))
        a = np.zeros((r.value, c.value) if t % 2 == 0 else (r.value,), dtype=np.float32)
        if fill is not None:
            fill(t, a)
        params.append(torch.from_numpy(a).cuda())
    grads = [torch.zeros_like(q) for q in params]
    eng.bind(params, grads, [torch.zeros_like(q) for q in params], [torch.zeros_like(q) for q in params])
    eng.sync_shadows()
    return eng, params, grads


def _set(eng, key, value):
    """an engine knob; a path is skipped only when the engine refuses it, with the engine's message"""
    from rectorch_amd import _lib
    try:
        eng.set_option(key, value)
    except _lib.RtxError as e:
        pytest.skip("the engine refuses %s = %d: %s" % (key, value, e))


def _eye(t, a, which):
    """identity on the leading square of the weight tensors listed in `which`"""
    if t in which:
        n = min(a.shape)
        a[np.arange(n), np.arange(n)] = 1.0


def _random(seed, scales):
    """normal weights with the standard deviation `scales[t]` for weight tensor t, biases with 0.1"""
    rng = np.random.default_rng(seed)

    def fill(t, a):
        a[...] = rng.standard_normal(a.shape) * (scales[t] if a.ndim == 2 else 0.1)
    return fill


def _train_args(**kw):
    d = dict(beta=0.2, lam=0.0, inv_batch=1.0 / BATCH, lr=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, flags=0)
    d.update(kw)
    return d


def _dropped_out(x, keep, p):
    """float64 [B][n_items]: x / ||x||_2 / (1 - p) where kept, 0 elsewhere (F.normalize then dropout)"""
    inv = 1.0 / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-12)
    return np.where(keep, x * inv / (1.0 - p), 0.0)


def _check_noise(got, seed, offset, rows, latent, bf16=False, pick=None):
    """got [len(pick) or rows][latent] against the draws of rows `pick` of a [rows][latent] layout; no element is exempt"""
    idx = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(latent) + np.arange(latent, dtype=np.uint64)[None, :]
    if pick is not None:
        idx = idx[np.asarray(pick)]
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == idx.shape
    ref = po.normal(seed, offset, idx)
    assert np.array_equal(ref, po.noise(seed, offset, rows, latent)[np.arange(rows) if pick is None else np.asarray(pick)])
    k = po.philox4x32_10(seed, int(offset) ^ po.NOISE_STREAM, idx)[0] >> np.uint32(8)
    err = np.abs(got - ref)
    scale = np.maximum(1.0, np.abs(ref))
    extra = BF16 * np.abs(ref) if bf16 else 0.0
    if not bf16:
        _WORST["all"] = max(_WORST["all"], float((err / scale).max()))
        _WORST["exact"] = max(_WORST["exact"], float(np.max((err / scale)[k < 2 ** 23], initial=0.0)))
        _WORST["n"] += err.size
    print("noise offset %d: worst error %.3g (u1 exact: %.3g)%s" % (offset, (err / scale).max(), np.max((err / scale)[k < 2 ** 23], initial=0.0),
                                                                    ", one bf16 rounding included" if bf16 else ""))
    assert np.all(err <= TOL * scale + extra), float((err / scale).max())
    assert np.all((err <= TOL_EXACT * scale + extra)[k < 2 ** 23])


# =============================================================================================================== device: dropout
DROPOUT_PATHS = ["fp32-csr", "fp32-dense", "bf16-csr-gather_scatter0", "bf16-csr-gather_scatter1", "bf16-dense", "bf16-sparse_in",
                 "bf16-csr-prefetched", "fp32-csr-cond3", "bf16-csr-cond3"]


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.3, 0.5])
@pytest.mark.parametrize("path", DROPOUT_PATHS)
def test_dropout_decisions_and_values_follow_the_reference(path, p):
    """Every stored entry of the batch, on every path that builds the first layer's operand: ``output != 0`` is the device's
    decision and equals ``dropout_keep(seed, offset, b * n_items + i, p)`` exactly (b: position in the batch -- the row ids are
    shuffled rows of a 64-row matrix); kept values are ``x / ||x|| / (1 - p)`` to 1e-6 (fp32) / 2^-8 (bf16); every entry
    that is not stored reads exactly 0.  Offsets 0, 1 and 2^33 + 5 under a seed with high bits; offsets 0 and 1 differ.

    How each path is observed (engine.hip run_forward / gather_batch, engine_step.hip begin_and_forward):
      * csr / dense / gather_scatter: ``rtx_engine_encode(training = 1)`` runs the step's own gather_batch -> k_gather or
        k_gather_scatter (a dense batch is densified to a CSR view first) and the first-layer product; the net is a VAE with
        n_enc = 1, latent = n_in, W0 = [I; 0], so mu IS the operand.
      * sparse_in: needs a layer behind the first one and is not taken by a VAE whose head is the first layer
        (sparse_in_ok), so the net is a DAE [77, 77] + [77, 77] with two identities and ``rtx_engine_forward(training = 1)``
        runs k_in_chunks + k_spmm_in; logits = tanh(operand), non-zero exactly where the operand is.  No output of this path
        is one rounding away from the operand: the operand is rounded to bf16 (2^-8) and so is the tanh activation the
        decoder reads (2^-8; tanh's relative condition number is <= 1), so the values are held to 2 x 2^-8 (+ 2^-16, their
        product) here, the decisions exactly as everywhere.  ``last_sparse_in`` == 1.
      * prefetched: exists only inside rtx_engine_train_step (prefetch_next gathers on the side stream) and only when the first
        and last matrices have >= 2^20 elements (finish_in_on_main), so this case alone uses n_items = 2051 (odd) with a
        512-wide DAE.  Observed through the loss of the step that starts from the prefetched image -- ``prefetch_hits``
        counts it -- against the loss of a step with the reference mask injected, at the bf16 loss tolerance 2e-3; a
        reference mask of another offset is shown to move the loss by much more than that.
      * cond3: CMultiVAE engine, latent = n_items + 3: item columns as above at index b * n_items + i (not b * 80 + i), the
        three condition columns come through raw -- not normalised, not scaled, never dropped."""
    import torch
    bf16 = path.startswith("bf16")
    numerics = "bf16" if bf16 else "fp32"
    rel = BF16 if bf16 else 1e-6
    if path.endswith("sparse_in"):
        rel = 2 * BF16 + BF16 * BF16                                  # two bf16 roundings on the way (docstring)
    if path.endswith("prefetched"):
        return _prefetched_case(p)
    cond = 3 if path.endswith("cond3") else 0
    n_in = N_ITEMS + cond
    dense, rows = _matrix(cond=cond)
    xb = dense[rows]                                                  # the batch, by position
    if path.endswith("sparse_in"):
        eng, _, _ = _engine([N_ITEMS, N_ITEMS], [N_ITEMS, N_ITEMS], "dae", numerics, p, fill=lambda t, a: _eye(t, a, (0, 2)))
        _set(eng, "sparse_in", 1)
    else:
        eng, _, _ = _engine([N_ITEMS, n_in], [n_in, N_ITEMS], "vae", numerics, p, cond, fill=lambda t, a: _eye(t, a, (0,)))
        if "gather_scatter" in path:
            _set(eng, "gather_scatter", int(path[-1]))
    x = torch.from_numpy(xb.astype(np.float32)).cuda() if path.endswith("dense") else _row_batch(dense, rows)
    stored = xb[:, :N_ITEMS] != 0
    assert stored[1].all() and not stored[7].any() and 0.05 < stored[2].mean() < 0.4      # full, empty and sparse rows
    patterns = []
    for rep in range(2):                     # twice: the scatter image's second batch clears what the first one wrote
        for off in OFFSETS:
            keep = po.dropout_mask(SEED, off, BATCH, N_ITEMS, p)
            want = _dropped_out(xb[:, :N_ITEMS], keep & stored, p)
            if path.endswith("sparse_in"):
                got = eng.forward(x, training=True, seed=SEED, offset=off)[0]
                assert eng.get_option("last_sparse_in") == 1
                want = np.tanh(want)
            else:
                got = eng.encode(x, training=True, seed=SEED, offset=off)[0]
            got = got.cpu().numpy().astype(np.float64)
            assert got.shape == (BATCH, n_in if not path.endswith("sparse_in") else N_ITEMS)
            items = got[:, :N_ITEMS]
            assert np.array_equal(items != 0, keep & stored), (off, int(((items != 0) != (keep & stored)).sum()))
            err = np.abs(items - want)
            print("%s p=%.1f offset %d: kept %d of %d stored, worst relative value error %.3g" % (
                path, p, off, int((items != 0).sum()), int(stored.sum()), float((err[want != 0] / want[want != 0]).max())))
            assert np.all(err <= rel * np.abs(want))
            if cond:
                assert np.array_equal(got[:, N_ITEMS:], xb[:, N_ITEMS:])          # raw: 2.0 where stored, 0 elsewhere
            patterns.append(items != 0)
    assert not np.array_equal(patterns[0], patterns[1])      # offset = rank: two ranks drop different entries
    assert np.array_equal(patterns[0], patterns[3]) and np.array_equal(patterns[2], patterns[5])
    # eval mode drops nothing
    if not path.endswith("sparse_in"):
        got = eng.encode(x, training=False, seed=SEED)[0].cpu().numpy()
        assert np.array_equal(got[:, :N_ITEMS] != 0, stored)


def _prefetched_case(p):
    import torch
    I, H = 2051, 512
    dense, rows = _matrix(n_items=I)
    rb = _row_batch(dense, rows)
    eng, params, _ = _engine([I, H], [H, I], "dae", "bf16", p, fill=_random(3, {0: 1.0, 2: 1.0}))
    before = [q.clone() for q in params]
    loss = torch.zeros(1, device="cuda")
    step_no = 0

    def step(x, **kw):
        nonlocal step_no
        step_no += 1
        eng.train_step(x, None, eng._step(**kw, **_train_args(step=step_no)), loss)
        return float(loss.item())          # (drains the stream: an injected mask is read before its tensor goes)

    for off in OFFSETS:
        hits, issued = eng.get_option("prefetch_hits"), eng.get_option("prefetch_issued")
        assert eng.set_next_batch(rb, seed=SEED, offset=off)
        step(rb, seed=SEED ^ 0xABCDEF, offset=0)                      # gathers the announced batch under its last weight kernel
        assert eng.get_option("prefetch_issued") == issued + 1
        l_pre = step(rb, seed=SEED, offset=off)                       # starts from the prefetched image
        assert eng.get_option("prefetch_hits") == hits + 1
        mask = torch.from_numpy(po.dropout_mask(SEED, off, BATCH, I, p).astype(np.uint8)).cuda()
        l_inj = step(rb, seed=1, offset=0, mask=mask)
        other = torch.from_numpy(po.dropout_mask(SEED, off + 1, BATCH, I, p).astype(np.uint8)).cuda()
        l_other = step(rb, seed=1, offset=0, mask=other)
        print("prefetched p=%.1f offset %d: loss %.6f, injected reference mask %.6f, another offset's mask %.6f" % (p, off, l_pre, l_inj, l_other))
        assert abs(l_pre - l_inj) <= 2e-3 * abs(l_inj)
        assert abs(l_other - l_inj) > 5 * 2e-3 * abs(l_inj)             # the comparison can tell two masks apart
    for a, b in zip(params, before):
        assert torch.equal(a, b)                                        # lr = 0: the same network in every step


# =============================================================================================================== device: noise
Z, HID = 21, 40
NOISE_PATHS = {   # name: (variant, numerics, encoder dims, small_fwd option or None, training)
    "fp32-head": ("vae", "fp32", [N_ITEMS, HID, Z], None, True),
    "bf16-head-small_fwd0": ("vae", "bf16", [N_ITEMS, HID, Z], 0, True),
    "bf16-head-small_fwd1": ("vae", "bf16", [N_ITEMS, HID, Z], 1, True),
    "fp32-head-is-first-layer": ("vae", "fp32", [N_ITEMS, Z], None, True),
    "bf16-head-is-first-layer": ("vae", "bf16", [N_ITEMS, Z], None, True),
    "fp32-gvae-eval": ("gvae", "fp32", [N_ITEMS, HID, Z], None, False),
}


def _noise_engine(name):
    variant, numerics, enc, small, training = NOISE_PATHS[name]
    dec_w = 2 * (len(enc) - 1)             # the single decoder layer [n_items][Z] = [I_Z; 0]; everything else is zero
    eng, _, _ = _engine(enc, [Z, N_ITEMS], variant, numerics, 0.0 if variant == "gvae" else 0.5,     # (VAE_net has no dropout)
                        fill=lambda t, a: _eye(t, a, (dec_w,)))
    if small is not None:
        _set(eng, "small_fwd", small)
    return eng, numerics == "bf16", training


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(NOISE_PATHS))
def test_reparameterisation_noise_follows_the_reference(path):
    """Zeroed head (mu = logvar = 0, so z = eps) and a decoder [I_Z; 0]: ``logits[:, :Z]`` of rtx_engine_forward IS the noise,
    compared with ``normal(seed, offset, b * Z + j)`` at TOL / TOL_EXACT (bf16: + one rounding of z); the other logits are 0.
    fp32 head and bf16 with small_fwd = 0: k_vae_fwd (post_layers.hip); small_fwd = 1: k_fwd_head (small_layers.hip); head as
    the first layer: k_vae_fwd behind the K = n_items product.  RTX_GVAE samples in EVAL mode too and returns sigmoid
    probabilities: compared with sigmoid(reference) at 1e-6."""
    dense, rows = _matrix()
    rb = _row_batch(dense, rows)
    eng, bf16, training = _noise_engine(path)
    outs = []
    for off in OFFSETS:
        logits, mu, logvar = eng.forward(rb, training=training, seed=SEED, offset=off)
        got = logits.cpu().numpy().astype(np.float64)
        assert not mu.any().item() and not logvar.any().item()
        if path.endswith("gvae-eval"):
            ref = 1.0 / (1.0 + np.exp(-po.noise(SEED, off, BATCH, Z)))
            print("gvae eval offset %d: worst probability error %.3g" % (off, np.abs(got[:, :Z] - ref).max()))
            assert np.all(np.abs(got[:, :Z] - ref) <= 1e-6) and np.all(got[:, Z:] == 0.5)
        else:
            _check_noise(got[:, :Z], SEED, off, BATCH, Z, bf16)
            assert not got[:, Z:].any()
        outs.append(got[:, :Z])
    assert np.abs(outs[0] - outs[1]).max() > 1.0 or path.endswith("gvae-eval")        # two ranks draw different noise
    if training:      # eval mode of the Mult-VAE: z = mu, no draw
        assert not eng.forward(rb, training=False, seed=SEED)[0].any().item()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fp32-head", "bf16-head-small_fwd0", "bf16-head-small_fwd1", "fp32-gvae-eval"])
def test_injected_noise_wins_over_the_seed(path):
    import torch
    dense, rows = _matrix()
    rb = _row_batch(dense, rows)
    eng, bf16, training = _noise_engine(path)
    inj = np.random.default_rng(8).standard_normal((BATCH, Z)).astype(np.float32)
    got = eng.forward(rb, training=training, seed=SEED, offset=1, noise=torch.from_numpy(inj).cuda())[0].cpu().numpy()[:, :Z]
    if path.endswith("gvae-eval"):
        assert np.all(np.abs(got - 1.0 / (1.0 + np.exp(-inj.astype(np.float64)))) <= 1e-6)
    elif bf16:
        assert np.all(np.abs(got.astype(np.float64) - inj) <= BF16 * np.abs(inj))
    else:
        assert np.array_equal(got, inj)


# =============================================================================================================== device: SVAE
SV_ITEMS, SV_RNN = 50, 32


def _svae():
    import torch
    from rectorch_amd import _lib
    from rectorch_amd.engine import SvaeEngine
    eng = SvaeEngine(SV_ITEMS, 8, SV_RNN, [SV_RNN, Z], [Z, SV_ITEMS], max_len=16)
    params = []
    r, c = ctypes.c_int32(), ctypes.c_int32()
    for t in range(eng.n_tensors):
        _lib.check(_lib.lib().rtx_svae_tensor_shape(eng.handle, t, ctypes.byref(r), ctypes.byref(c)))
        a = np.zeros((r.value,) if c.value == 1 else (r.value, c.value), dtype=np.float32)
        if t == 2:                                      # the decoder [n_items][Z] = [I_Z; 0]; head, embedding and GRU are zero
            a[np.arange(Z), np.arange(Z)] = 1.0
        params.append(torch.from_numpy(a).cuda())
    eng.bind(params)
    return eng


def _sv_forward(eng, items, seed, offset):
    import torch
    from rectorch_amd import _lib
    it = torch.tensor(items, dtype=torch.int32, device="cuda")
    T = len(items)
    la = torch.empty((T, SV_ITEMS), device="cuda")
    ll = torch.empty((SV_ITEMS,), device="cuda")
    mu, lv = torch.empty((T, Z), device="cuda"), torch.empty((T, Z), device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().rtx_svae_forward(eng.handle, P(it), T, None, ctypes.c_uint64(seed), ctypes.c_uint64(offset), 0, P(la), P(ll),
                                           P(mu), P(lv), _lib.stream_ptr()))
    assert not mu.any().item() and not lv.any().item()
    return la.cpu().numpy(), ll.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5, 9])
def test_svae_forward_noise_is_indexed_by_time_step(T):
    """rtx_svae_forward, rnn_size 32: with the head zeroed and the decoder [I_Z; 0], logits_all[t, :Z] is draw t * Z + j"""
    eng = _svae()
    items = [(7 * t + 3) % SV_ITEMS for t in range(T)]
    for off in OFFSETS:
        la, ll = _sv_forward(eng, items, SEED, off)
        _check_noise(la[:, :Z], SEED, off, T, Z)
        assert not la[:, Z:].any() and np.array_equal(ll, la[-1])


@pytest.mark.gpu
def test_svae_predict_pack_takes_the_draws_of_each_users_last_row():
    """rtx_svae_predict_pack, users of 5, 1 and 9 steps: user u gets the draws of row seq_ptr[u + 1] - 1 of the concatenation
    ("per-user noise arrays concatenate").  That is rtx_svae_forward's last row for the concatenation as a whole and for user
    0 alone; users 1 and 2 scored alone start again at row 0 and draw something else."""
    import torch
    from rectorch_amd import _lib
    from rectorch_amd.engine import SvaeEvalPack
    eng = _svae()
    seqs = [[3, 10, 17, 24, 31], [40], [1, 2, 3, 4, 5, 6, 7, 8, 9]]
    pack = SvaeEvalPack(seqs)
    last = [4, 5, 14]
    total = 15
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    for off in OFFSETS:
        scores = torch.empty((3, SV_ITEMS), device="cuda")
        mu, lv = torch.empty((3, Z), device="cuda"), torch.empty((3, Z), device="cuda")
        _lib.check(_lib.lib().rtx_svae_predict_pack(eng.handle, P(pack.items), total, P(pack.seq_ptr), 3, None, ctypes.c_uint64(SEED),
                                                    ctypes.c_uint64(off), 0, P(scores), P(mu), P(lv), _lib.stream_ptr()))
        got = scores.cpu().numpy()
        _check_noise(got[:, :Z], SEED, off, total, Z, pick=last)
        assert not got[:, Z:].any() and not mu.any().item() and not lv.any().item()
        whole = _sv_forward(eng, [i for q in seqs for i in q], SEED, off)[0]
        assert np.array_equal(got, whole[last])
        alone = [_sv_forward(eng, q, SEED, off)[1] for q in seqs]
        assert np.array_equal(got[0], alone[0])
        assert np.abs(got[1] - alone[1]).max() > 1e-2 and np.abs(got[2] - alone[2]).max() > 1e-2


# =============================================================================================================== the whole step
STEP_NETS = {"dae": ([N_ITEMS, HID], [HID, N_ITEMS]), "vae": ([N_ITEMS, HID, Z], [Z, HID, N_ITEMS])}


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", ["fp32", "bf16"])
@pytest.mark.parametrize("variant", ["dae", "vae"])
def test_the_philox_step_is_the_injected_step(variant, numerics):
    """A step that draws from (seed, offset) equals the step with the REFERENCE's mask and noise injected -- which is what every
    parity test against the float64 oracle runs.  Random weights, p = 0.5, the shuffled 37-row CSR batch, all three offsets.
      * fp32, rtx_engine_loss_grads, DAE with lam = 0 (dropout only): loss and every gradient bit-identical (same kernels, same
        values, no float atomic on this path).
      * fp32 VAE: the injected noise is the float64 reference rounded to float32, up to TOL away from the device's draw: loss
        within relative 1e-5, every gradient tensor within 1e-5 of its largest element (the project's fp32 tolerance).
      * bf16, rtx_engine_train_step with RTX_STEP_KEEP_GRADS and lr = 0: loss within 2e-3 (the project's bf16 loss tolerance).
        DAE: the masks are equal, so loss and gradients are bit-identical here too.  VAE: the injected float32 noise is up to
        TOL away from the device's draw, which can carry an element of z across a bf16 rounding boundary: one bf16 ulp,
        2^-7 relative, in one operand element of the decoder and of its weight gradient.  The gradient tensors are therefore
        held to 2^-7 of their largest element (a first bound of 2e-3 overlooked this; offset 2^33 + 5 showed 7.0e-3 with
        offsets 0 and 1 bit-identical, MI355X)."""
    import torch
    from rectorch_amd import _lib
    enc, dec = STEP_NETS[variant]
    p = 0.5
    dense, rows = _matrix()
    rb = _row_batch(dense, rows)
    eng, params, grads = _engine(enc, dec, variant, numerics, p, fill=_random(5, {0: 0.4, 2: 0.4, 4: 0.4, 6: 0.4}))
    loss = torch.zeros(1, device="cuda")
    step_no = 0

    def run(**kw):
        nonlocal step_no
        step_no += 1
        for g in grads:
            g.fill_(float("nan"))
        if numerics == "fp32":
            eng.loss_grads(rb, None, eng._step(**kw, **_train_args(step=step_no)), loss)
        else:
            eng.train_step(rb, None, eng._step(**kw, **_train_args(step=step_no, flags=_lib.RTX_STEP_KEEP_GRADS)), loss)
        torch.cuda.synchronize()
        return loss.clone(), [g.clone() for g in grads]

    losses = []
    for off in OFFSETS:
        l_a, g_a = run(seed=SEED, offset=off)
        mask = torch.from_numpy(po.dropout_mask(SEED, off, BATCH, N_ITEMS, p).astype(np.uint8)).cuda()
        noise = torch.from_numpy(po.noise(SEED, off, BATCH, Z).astype(np.float32)).cuda() if variant == "vae" else None
        l_b, g_b = run(seed=12345, offset=99, mask=mask, noise=noise)
        assert all(bool(torch.isfinite(g).all()) for g in g_a + g_b) and bool(torch.isfinite(l_a).all())
        worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(g_a, g_b))
        print("%s %s offset %d: loss %.7f vs injected %.7f, worst gradient difference / largest element %.3g" % (
            variant, numerics, off, l_a.item(), l_b.item(), worst))
        if variant == "dae":
            assert torch.equal(l_a, l_b) and all(torch.equal(a, b) for a, b in zip(g_a, g_b))
        else:
            assert abs(l_a.item() - l_b.item()) <= (1e-5 if numerics == "fp32" else 2e-3) * abs(l_b.item())
            assert worst <= (1e-5 if numerics == "fp32" else 2.0 ** -7)
        losses.append(l_a.item())
    assert len({round(v, 4) for v in losses}) == 3                       # three offsets, three different steps


@pytest.mark.gpu
def test_zz_worst_device_normal_error_of_this_session():
    """prints the worst float32-output device error the noise tests above saw (the figure recorded in the module docstring)"""
    print("device normals, %d draws: worst error %.4g, with u1 exact in float32 %.4g (TOL %.3g / %.3g)" % (
        _WORST["n"], _WORST["all"], _WORST["exact"], TOL, TOL_EXACT))
    assert _WORST["all"] <= TOL and _WORST["exact"] <= TOL_EXACT
