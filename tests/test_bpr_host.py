"""CPU: the package's BPR triple sampler (samplers.BprTripleSampler over rtx_bpr_draw_host) bit for bit against the float64
restatement of BPRMF (bpr_ref64.py), and the restatement against itself -- the draws, its two formulations against each other,
batch = 1 against textbook sequential SGD, the training AUC's rise, the skipped samples and the fold-in."""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import bpr_ref64 as R

F, LR, REG, SEED = 8, 0.05, 0.01, 98765
_CACHE = {}


def block_data(U=96, I=80, seed=11):
    """4 user groups x 4 item groups: density 0.45 inside a user group's own item group, 0.04 elsewhere; row 5 empty, row 7 full"""
    rng = np.random.RandomState(seed)
    own = (np.arange(U)[:, None] * 4 // U) == (np.arange(I)[None, :] * 4 // I)
    d = (rng.rand(U, I) < np.where(own, 0.45, 0.04)).astype(np.float64)
    d[5] = 0
    d[7] = 1
    return csr_matrix(d)


def tables(U, I, f=F, seed=SEED):
    rng = np.random.RandomState(seed)
    Y0 = rng.normal(0, 0.01, (I, f))
    return rng.normal(0, 0.01, (U, f)), Y0


def _fits():
    """the restatement's fits of the block data, shared by the tests: nothing changes them"""
    if not _CACHE:
        X = block_data()
        U0, Y0 = tables(*X.shape)
        _CACHE["X"], _CACHE["U0"], _CACHE["Y0"] = X, U0, Y0
        _CACHE["loop"] = R.fit(X, U0, Y0, LR, REG, 10, 64, SEED, "loop", history=True)
        _CACHE["vector"] = R.fit(X, U0, Y0, LR, REG, 10, 64, SEED, "vector", history=True)
    return _CACHE


def test_draws_are_positives_and_true_negatives():
    X = _fits()["X"]
    dense = X.toarray() != 0
    for epoch in (0, 3):
        u, i, j = R.draws(X, SEED, epoch)
        assert len(u) == X.nnz and dense[u, i].all()
        ok = j >= 0
        assert not dense[u[ok], j[ok]].any() and (j[~ok] == -1).all()
    a, b = R.draws(X, SEED, 2, lo=100, count=50), R.draws(X, SEED, 2)
    assert all(np.array_equal(x, y[100:150]) for x, y in zip(a, b))        # a pure function of (seed, epoch, sample)
    assert not np.array_equal(R.draws(X, SEED, 0)[1], R.draws(X, SEED, 1)[1])
    assert not np.array_equal(R.draws(X, SEED, 0)[1], R.draws(X, SEED + 1, 0)[1])


def test_the_two_formulations_agree_within_their_own_spread():
    """They differ by roundings only: the sigmoid written two ways and two summation orders.  One sample's update of an entry is at
    most 8 float64 operations that are not shared with the other formulation bit for bit (the dot's sum, the sigmoid, the gradient's
    product, its sum and the update), each wrong by at most 2^-53 of a number no larger than the largest factor, and an entry is touched by at most every sample of
    every epoch; the updates do not amplify (|d theta' / d theta| = 1 - lr c reg - O(lr |theta|^2) < 1).  So the two differ by at most
    8 * 2^-53 * epochs * nnz of the largest factor -- about 1e-11 here; a disagreement of formulas would be O(1)."""
    c = _fits()
    (Ua, Ya, _), (Ub, Yb, _) = c["loop"], c["vector"]
    spread = max(np.abs(Ya - Yb).max() / np.abs(Ya).max(), np.abs(Ua - Ub).max() / np.abs(Ua).max())
    print("spread of the two formulations after 10 epochs: %.3g" % spread)
    bound = 8 * 2.0 ** -53 * 10 * c["X"].nnz
    print("bound %.3g" % bound)
    assert spread <= bound
    assert np.array_equal(Ua[5], c["U0"][5]) and np.array_equal(Ub[5], c["U0"][5])      # the empty row is never drawn
    assert np.array_equal(Ua[7], c["U0"][7]) and np.array_equal(Ub[7], c["U0"][7])      # the full row's samples are all skipped


def test_batch_one_is_sequential_sgd_bit_for_bit():
    c = _fits()
    X, U0, Y0 = c["X"], c["U0"], c["Y0"]
    Ua, Ya = R.fit(X, U0, Y0, LR, REG, 1, 1, SEED, "loop")
    Ub, Yb = R.fit_sequential(X, U0, Y0, LR, REG, 1, SEED)
    assert np.array_equal(Ua, Ub) and np.array_equal(Ya, Yb)


def test_training_auc_rises():
    c = _fits()
    X = c["X"]
    for how in ("loop", "vector"):
        hist = c[how][2]
        a0, a1, a10 = (R.auc(X, *hist[e]) for e in (0, 1, 10))
        print("%s: training AUC after 0, 1, 10 epochs: %.4f %.4f %.4f" % (how, a0, a1, a10))
        assert abs(a0 - 0.5) < 0.05 and a0 < a1 < a10


def test_the_objective_on_fixed_triples_falls():
    c = _fits()
    u, i, j = R.draws(c["X"], SEED + 5, 0)
    hist = c["loop"][2]
    obj = [R.objective(*hist[e], u, i, j, REG) for e in (0, 1, 10)]
    print("objective on a fixed triple set after 0, 1, 10 epochs:", obj)
    assert obj[0] > obj[1] > obj[2]


def test_skipped_samples_are_those_of_the_full_row_plus_the_restatements_own():
    """Row 7 stores every item, so each of its draws is skipped.  Any other row may be skipped only when all seven candidates fall
    into it: counted from the restatement's own candidates, not assumed."""
    X = _fits()["X"]
    m = R.canonical(X)
    for epoch in range(3):
        u, i, j = R.draws(X, SEED, epoch)
        full = u == 7
        assert full.sum() > 0 and (j[full] == -1).all()
        w = R._words(SEED, R.FIT_STREAM + epoch, np.arange(m.nnz))
        cand = R._mulhi(w[:, 1:8], m.shape[1])
        dense = m.toarray() != 0
        own = dense[u[:, None], cand].all(axis=1)
        assert np.array_equal(j == -1, own)
        assert (j == -1).sum() == full.sum() + (own & ~full).sum()
        assert (u != 5).all()


def test_fold_in_depends_on_the_row_alone_and_edge_rows_give_zero():
    c = _fits()
    X, Y = c["X"], c["loop"][1]
    rows = X[[3, 5, 7, 40]]
    a = R.fold_in(rows, Y, LR, REG, 3, SEED)
    b = R.fold_in(X[[40, 3]], Y, LR, REG, 3, SEED)
    assert np.array_equal(a[3], b[0]) and np.array_equal(a[0], b[1])
    assert (a[1] == 0).all() and (a[2] == 0).all() and np.abs(a[0]).max() > 0
    S = R.scores(rows, Y, LR, REG, 3, SEED, mask=rows)
    assert np.array_equal(np.isneginf(S), rows.toarray() != 0)


# ---- the package's sampler ------------------------------------------------------------------------------------------------------------
def _edge_data():
    """200 x 150 at density 0.1: row 2 stores every item, row 4 none, row 6 all but item 75"""
    d = (np.random.RandomState(7).rand(200, 150) < 0.1).astype(np.float64)
    d[2] = 1
    d[4] = 0
    d[6] = 1
    d[6, 75] = 0
    return csr_matrix(d)


@pytest.mark.parametrize("seed", [1, 98765, 2 ** 40 + 3, 2 ** 64 - 1])
def test_sampler_equals_the_restatement_bit_for_bit(seed):
    from rectorch_amd.samplers import BprTripleSampler
    for X in (_fits()["X"], _edge_data()):
        smp = BprTripleSampler(X, batch_size=64, seed=seed)
        for epoch in (0, 1, 5):
            got, want = smp.draw(epoch), R.draws(X, seed, epoch)
            for g, w in zip(got, want):
                assert g.dtype == np.int32 and np.array_equal(g, w)
        got, want = smp.draw(5, 37, X.nnz - 48), R.draws(X, seed, 5, 37, X.nnz - 48)        # a window inside an epoch
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_sampler_edge_rows():
    from rectorch_amd.samplers import BprTripleSampler
    X = _edge_data()
    dense = X.toarray() != 0
    u, i, j = BprTripleSampler(X, seed=3).draw(0)
    assert len(u) == X.nnz and dense[u, i].all() and (u != 4).all()                 # the empty row is never drawn
    assert (u == 2).sum() > 0 and (j[u == 2] == -1).all()                            # the full row: every sample skipped
    almost = u == 6
    assert almost.sum() > 0 and set(j[almost].tolist()) == {-1, 75}                  # one free item: that one or skipped
    ok = j >= 0
    assert not dense[u[ok], j[ok]].any() and (j >= -1).all() and (j < 150).all()


def test_sampler_batches_are_windows_of_the_epoch_and_epochs_advance():
    from rectorch_amd.samplers import BprTripleSampler, Sampler
    X = _fits()["X"]
    smp = BprTripleSampler(X, batch_size=100, seed=SEED)
    assert isinstance(smp, Sampler) and len(smp) == (X.nnz + 99) // 100 and X.nnz % 100 != 0
    for epoch in (0, 1):
        assert smp.epoch == epoch
        batches = list(smp)
        assert len(batches) == len(smp) and len(batches[-1][0]) == X.nnz % 100
        for k, whole in enumerate(smp.draw(epoch)):
            assert np.array_equal(np.concatenate([b[k] for b in batches]), whole)
    assert smp.epoch == 2
    other = BprTripleSampler(X, batch_size=7, seed=SEED)                              # any batching gives the same epoch
    assert np.array_equal(np.concatenate([b[2] for b in other]), smp.draw(0)[2])
    assert not np.array_equal(smp.draw(0)[1], smp.draw(1)[1])
    assert not np.array_equal(smp.draw(0)[1], BprTripleSampler(X, seed=SEED + 1).draw(0)[1])


def test_sampler_sorts_a_copy_and_reads_the_pattern_only():
    from rectorch_amd.samplers import BprTripleSampler
    X = _fits()["X"]
    shuffled = X.tocsr().copy()
    shuffled.indices[:] = np.concatenate([shuffled.indices[a:b][::-1] for a, b in zip(shuffled.indptr, shuffled.indptr[1:])])
    shuffled.data[:] = np.arange(1, X.nnz + 1)
    shuffled.has_sorted_indices = False
    before = shuffled.indices.copy()
    a, b = BprTripleSampler(shuffled, seed=5).draw(2), BprTripleSampler(X, seed=5).draw(2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(shuffled.indices, before)
    c = BprTripleSampler(X.tocoo(), seed=5).draw(2)
    assert all(np.array_equal(x, y) for x, y in zip(c, b))


def test_sampler_refusals_name_what_is_supported():
    from rectorch_amd import _lib
    from rectorch_amd.samplers import BprTripleSampler
    X = _fits()["X"]
    for kwargs, word in ((dict(batch_size=0), ">= 1"), (dict(batch_size=2.5), ">= 1"), (dict(batch_size=True), ">= 1"),
                         (dict(seed=-1), "[0, 2^64)"), (dict(seed=2 ** 64), "[0, 2^64)"), (dict(seed="x"), "[0, 2^64)")):
        with pytest.raises(ValueError) as e:
            BprTripleSampler(X, **kwargs)
        assert word in str(e.value) and list(kwargs)[0] in str(e.value)
    with pytest.raises(ValueError) as e:
        BprTripleSampler(csr_matrix((5, 6)))
    assert "no entries" in str(e.value)
    smp = BprTripleSampler(X)
    for args, word in (((0, X.nnz - 2, 3), "outside the epoch"), ((0, -1, 3), "outside the epoch"), ((0, 0, -1), "outside the epoch"),
                       ((-1, 0, 3), "epoch must be >= 0")):
        with pytest.raises(_lib.RtxError) as e:
            smp.draw(*args)
        assert word in str(e.value)
    assert all(len(t) == 0 for t in smp.draw(0, X.nnz, 0))


def test_native_entries_refuse_malformed_matrices_and_write_nothing():
    from rectorch_amd import _lib
    lib = _lib.lib()
    assert (_lib.BPR_NEG_TRIES, _lib.BPR_FIT_STREAM, _lib.BPR_FOLD_STREAM) == (R.NEG_TRIES, R.FIT_STREAM, R.FOLD_STREAM)
    assert lib.rtx_abi_version() == 8
    out = [np.full(4, -7, dtype=np.int32) for _ in range(3)]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731

    def arrays(indptr, indices):
        return np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32)

    def check_rows(indptr, indices, n_rows, n_items):
        ip, ix = arrays(indptr, indices)
        return lib.rtx_bpr_check_rows_host(ptr(ip), ptr(ix), n_rows, n_items)

    def draw(indptr, indices, n_rows, n_items, epoch=0, lo=0, count=2):
        ip, ix = arrays(indptr, indices)
        return lib.rtx_bpr_draw_host(ptr(ip), ptr(ix), n_rows, n_items, 1, epoch, lo, count, *[ptr(t) for t in out])
    good = ([0, 2, 2, 3], [0, 2, 1])
    # the one pass over the matrix: an interior row end beyond nnz is refused before the row's entries are read
    for args, word in (((good[0], [2, 0, 1], 3, 3), "sorted, unique"), ((good[0], [0, 0, 1], 3, 3), "sorted, unique"),
                       ((good[0], [0, 3, 1], 3, 3), "sorted, unique"), ((good[0], [-1, 2, 1], 3, 3), "sorted, unique"),
                       (([0, 2, 1, 3], good[1], 3, 3), "indptr decreases or passes nnz"), (([0, 9, 2, 3], good[1], 3, 3), "indptr decreases or passes nnz"),
                       (([0, 0, 0, 0], [0], 3, 3), "nnz = 0"), (([1, 2, 2, 3], good[1], 3, 3), "indptr must start at 0"), ((good[0], good[1], 3, 0), "[1, 2^31)")):
        assert check_rows(*args) == -1 and word in lib.rtx_last_error().decode(), word
    assert check_rows(*good, 3, 3) == 0 and lib.rtx_bpr_check_rows_host(None, None, 3, 3) != 0
    # the draws: their own arguments, with no overflow in lo + count, and a drawn row whose range cannot hold the position
    big = 2 ** 62
    for args, word in ((([0, 0, 0, 0], [0], 3, 3), "nnz = 0"), ((good[0], good[1], 3, 0), "[1, 2^31)"), ((good[0], good[1], 3, 3, 0, 2, 2), "outside the epoch"),
                       ((good[0], good[1], 3, 3, 0, big, big), "outside the epoch"), ((good[0], good[1], 3, 3, 0, 1, 2 ** 63 - 1), "outside the epoch"),
                       ((good[0], good[1], 3, 3, 0, -1, 1), "outside the epoch"), ((good[0], good[1], 3, 3, -1), "epoch must be >= 0")):
        assert draw(*args) == -1 and word in lib.rtx_last_error().decode(), word
    assert lib.rtx_bpr_draw_host(None, None, 3, 3, 1, 0, 0, 1, None, None, None) != 0
    assert all((t == -7).all() for t in out)                                            # a refused call wrote nothing
    for bad in ([0, 9, 2, 3], [0, 3, 1, 3], [0, -5, 2, 3]):                             # never read outside the arrays: refused or drawn
        rc = draw(bad, good[1], 3, 3, count=3)
        assert rc == 0 or (rc == -1 and "indptr is not ascending" in lib.rtx_last_error().decode())
    out = [np.full(4, -7, dtype=np.int32) for _ in range(3)]
    assert draw(*good, 3, 3) == 0 and (out[0][:2] != 1).all() and (out[0][2:] == -7).all()    # the empty row 1 is never drawn


def test_sampler_checks_its_matrix_once_and_draws_cost_their_samples_alone(monkeypatch):
    """one pass over the matrix at construction; a batch does not walk it again"""
    from rectorch_amd import _lib
    from rectorch_amd.samplers import BprTripleSampler
    calls = []
    real = _lib.lib()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name.startswith("rtx_bpr_"):
                return lambda *a: (calls.append(name), fn(*a))[1]
            return fn
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    smp = BprTripleSampler(_fits()["X"], batch_size=500)
    n = len(list(smp))
    assert calls.count("rtx_bpr_check_rows_host") == 1 and calls.count("rtx_bpr_draw_host") == n == len(smp)
