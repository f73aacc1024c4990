"""CPU: BPRMF's batch rule and fold-in as the library defines them on the host (rtx_bpr_update_host / rtx_bpr_fold_in_host through
rectorch_amd.bpr_rule) against the float64 restatement bpr_ref64.

Bit for bit where the definition fixes every operation: fed the restatement's own coefficients s_t, one batch equals
bpr_ref64.batch_loop (numpy's element-wise *, + and - are unfused, the sums run in ascending sample order in both).  Where the
definition leaves the dot product's summation tree and exp's rounding open -- the library's own s_t, whole fits, the fold-in -- the
distance to the "loop" formulation is held to max(16 x spread, 64 * 2^-52), the spread measured in the same test between the
restatement's "loop" and "vector" formulations: the rule bpr_ref64 states for an implementation.
"""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import bpr_ref64 as R
import test_bpr_host as H

LR, REG, SEED = 0.05, 0.01, H.SEED
FLOOR = 64 * 2.0 ** -52


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _loop_coefficients(U, Y, u, i, j):
    """what batch_loop computes for every sample, 0 for a skipped one"""
    s = np.zeros(len(u))
    for t, (ut, it, jt) in enumerate(zip(u, i, j)):
        if jt >= 0:
            s[t] = float(R.sigmoid_neg(float(np.dot(U[ut], Y[it] - Y[jt])), "loop"))
    return s


def _random_batch(n_users, n_items, f, count, seed, skipped=0.125):
    """tables of magnitude 0.5 and triples that collide heavily"""
    rng = np.random.RandomState(seed)
    U, Y = rng.uniform(-0.5, 0.5, (n_users, f)), rng.uniform(-0.5, 0.5, (n_items, f))
    u, i, j = rng.randint(0, n_users, count), rng.randint(0, n_items, count), rng.randint(0, n_items, count)
    j[rng.rand(count) < skipped] = -1
    return U, Y, u.astype(np.int64), i.astype(np.int64), j.astype(np.int64)


@pytest.mark.parametrize("f", [1, 8, 63, 64, 65, 128])
@pytest.mark.parametrize("count", [1, 63, 257])
def test_one_batch_equals_the_loop_formulation_bit_for_bit_given_its_coefficients(f, count):
    from rectorch_amd import bpr_rule
    U, Y, u, i, j = _random_batch(40, 30, f, count, 1000 + 131 * f + count)
    s = _loop_coefficients(U, Y, u, i, j)
    Ua, Ya = R.batch_loop(U, Y, u, i, j, LR, REG)
    before = (U.copy(), Y.copy())
    Ub, Yb, s_used = bpr_rule.update(U, Y, u, i, j, LR, REG, s=s, want_s=True)
    assert np.array_equal(_bits(Ub), _bits(Ua)) and np.array_equal(_bits(Yb), _bits(Ya))
    assert np.array_equal(_bits(s_used), _bits(s))
    assert np.array_equal(U, before[0]) and np.array_equal(Y, before[1])                # the caller's tables are not written
    live = j >= 0
    quiet_u = np.setdiff1d(np.arange(40), u[live])
    quiet_y = np.setdiff1d(np.arange(30), np.concatenate([i[live], j[live]]))
    assert np.array_equal(_bits(Ub[quiet_u]), _bits(U[quiet_u])) and np.array_equal(_bits(Yb[quiet_y]), _bits(Y[quiet_y]))
    # the library's own coefficients: within a few ulp of the restatement's (f products, one exp, one sum, one division)
    Uc, Yc, own = bpr_rule.update(U, Y, u, i, j, LR, REG, want_s=True)
    x_abs = np.array([np.abs(U[a] * (Y[b] - Y[c])).sum() if c >= 0 else 0.0 for a, b, c in zip(u, i, j)])
    err = np.abs(own - s)[live] / (s[live] * 2.0 ** -53) if live.any() else np.zeros(1)
    print("bpr_rule: f=%d count=%d: largest |s_lib - s_loop| = %.2f u s (bound: 2 f sum|u_k d_k| + 8, at most %.1f here)"
          % (f, count, err.max(), (2 * f * x_abs + 8).max()))
    assert (own[~live] == 0).all() and (np.abs(own - s) <= s * 2.0 ** -53 * (2 * f * x_abs + 8)).all()
    Ud, Yd = bpr_rule.update(U, Y, u, i, j, LR, REG)
    assert np.array_equal(_bits(Ud), _bits(Uc)) and np.array_equal(_bits(Yd), _bits(Yc))   # two calls agree


def test_hand_made_batches():
    from rectorch_amd import bpr_rule
    U, Y, u, i, j = _random_batch(40, 30, 8, 70, 11, skipped=0.0)
    cases = {"same user": (np.full(70, 7), i, j), "same positive": (u, np.full(70, 3), j),
             "an item positive then negative, and the reverse": (np.array([1, 2, 3, 4, 1]), np.array([5, 9, 6, 8, 5]), np.array([6, 5, 7, 6, 8])),
             "skipped between live ones": (u, i, np.where(np.arange(70) % 3 == 1, -1, j)),
             "one row in both roles of a sample": (np.array([2, 2]), np.array([4, 6]), np.array([4, 9]))}
    for name, (uu, ii, jj) in cases.items():
        uu, ii, jj = (np.asarray(t, dtype=np.int64) for t in (uu, ii, jj))
        s = _loop_coefficients(U, Y, uu, ii, jj)
        Ua, Ya = R.batch_loop(U, Y, uu, ii, jj, LR, REG)
        Ub, Yb = bpr_rule.update(U, Y, uu, ii, jj, LR, REG, s=s)
        assert np.array_equal(_bits(Ub), _bits(Ua)) and np.array_equal(_bits(Yb), _bits(Ya)), name
    for uu, ii, jj in ((u, i, np.full(70, -1)), (u[:0], i[:0], j[:0])):                   # only skipped samples; no samples
        Ub, Yb, s = bpr_rule.update(U, Y, uu, ii, jj, LR, REG, want_s=True)
        assert np.array_equal(_bits(Ub), _bits(U)) and np.array_equal(_bits(Yb), _bits(Y)) and (s == 0).all()


@pytest.mark.parametrize("lr", [0.05, 0.5])
@pytest.mark.parametrize("shape", [(96, 80, 8, 64), (96, 80, 128, 64), (130, 77, 40, 257)])
def test_a_fit_by_the_library_rule_lies_within_the_restatements_spread(shape, lr):
    """3 epochs of the package's sampler + rtx_bpr_update_host against bpr_ref64.fit: the larger rate moves the sigmoid away from 1/2"""
    from rectorch_amd import bpr_rule
    from rectorch_amd.samplers import BprTripleSampler
    n_users, n_items, f, batch = shape
    X = H.block_data() if (n_users, n_items) == (96, 80) else H.block_data(n_users, n_items, seed=12)
    U0, Y0 = H.tables(n_users, n_items, f, SEED)
    (Ua, Ya), (Ub, Yb) = (R.fit(X, U0, Y0, lr, REG, 3, batch, SEED, how) for how in ("loop", "vector"))
    U, Y = U0, Y0
    smp = BprTripleSampler(X, batch_size=batch, seed=SEED)
    for _ in range(3):
        for u, i, j in smp:
            U, Y = bpr_rule.update(U, Y, u, i, j, lr, REG)
    spread = max(_rel(Yb, Ya), _rel(Ub, Ua))
    dist = max(_rel(Y, Ya), _rel(U, Ua))
    print("bpr_rule: fit %s lr %g: distance to the loop formulation %.3e, spread of the two formulations %.3e" % (shape, lr, dist, spread))
    assert dist <= max(16 * spread, FLOOR)
    assert np.array_equal(_bits(U[5]), _bits(U0[5])) and np.array_equal(_bits(U[7]), _bits(U0[7]))     # never drawn; every sample skipped


@pytest.mark.parametrize("f", [8, 65, 128])
def test_fold_in_against_the_restatement(f):
    from rectorch_amd import bpr_rule
    X = H._edge_data()                                         # row 2 stores every item, row 4 none, row 6 all but item 75
    Y = np.random.RandomState(31 + f).uniform(-0.2, 0.2, (150, f))
    rows = X[[3, 4, 2, 40, 6, 41, 42, 60, 61, 62, 80, 90]]
    got = bpr_rule.fold_in(rows, Y, LR, REG, 3, SEED)
    a, b = (R.fold_in(rows, Y, LR, REG, 3, SEED, how) for how in ("loop", "vector"))
    spread, dist = _rel(b, a), _rel(got, a)
    print("bpr_rule: fold-in f=%d: distance to the loop formulation %.3e, spread %.3e" % (f, dist, spread))
    assert got.shape == (12, f) and dist <= max(16 * spread, FLOOR)
    assert (got[1] == 0).all() and (got[2] == 0).all() and np.abs(got[0]).max() > 0 and np.abs(got[4]).max() > 0
    alone = bpr_rule.fold_in(X[[40, 3]], Y, LR, REG, 3, SEED)                             # a function of the row's content alone
    assert np.array_equal(_bits(alone[0]), _bits(got[3])) and np.array_equal(_bits(alone[1]), _bits(got[0]))
    shuffled = rows.tocsr().copy()
    shuffled.indices[:] = np.concatenate([shuffled.indices[p:q][::-1] for p, q in zip(shuffled.indptr, shuffled.indptr[1:])])
    shuffled.has_sorted_indices = False
    assert np.array_equal(_bits(bpr_rule.fold_in(shuffled, Y, LR, REG, 3, SEED)), _bits(got))
    assert (bpr_rule.fold_in(rows, Y, LR, REG, 0, SEED) == 0).all()
    assert (bpr_rule.fold_in(csr_matrix((3, 150)), Y, LR, REG, 3, SEED) == 0).all()       # a matrix of empty rows


def test_refusals_name_what_is_supported_and_write_nothing():
    from rectorch_amd import _lib, bpr_rule
    lib = _lib.lib()
    assert lib.rtx_abi_version() == 8 and _lib.BPR_MAX_FACTORS == 128
    U, Y, u, i, j = _random_batch(40, 30, 8, 20, 91)
    for kwargs, word in ((dict(lr=0.0), "lr must be finite and > 0"), (dict(lr=float("nan")), "lr must be finite and > 0"),
                         (dict(lr=float("inf")), "lr must be finite and > 0"), (dict(reg=-0.1), "reg must be finite and >= 0"),
                         (dict(reg=float("nan")), "reg must be finite and >= 0")):
        args = dict(lr=LR, reg=REG)
        args.update(kwargs)
        with pytest.raises(_lib.RtxError) as e:
            bpr_rule.update(U, Y, u, i, j, **args)
        assert word in str(e.value)
        with pytest.raises(_lib.RtxError) as e:
            bpr_rule.fold_in(csr_matrix(np.eye(30)), Y, args["lr"], args["reg"], 1, SEED)
        assert word in str(e.value)
    with pytest.raises(_lib.RtxError) as e:
        bpr_rule.update(np.zeros((4, 129)), np.zeros((4, 129)), [0], [1], [2], LR, REG)
    assert "f must be in [1, 128]" in str(e.value)
    with pytest.raises(_lib.RtxError) as e:
        bpr_rule.fold_in(csr_matrix(np.eye(30)), Y, LR, REG, -1, SEED)
    assert "fold_in_epochs must be >= 0" in str(e.value)
    with pytest.raises(ValueError):
        bpr_rule.update(U, Y[:, :7], u, i, j, LR, REG)
    with pytest.raises(ValueError):
        bpr_rule.update(U, Y, u, i[:-1], j, LR, REG)
    with pytest.raises(ValueError):
        bpr_rule.fold_in(csr_matrix(np.eye(29)), Y, LR, REG, 1, SEED)
    # through the C ABI: a triple outside the tables is refused before anything is written; NULL arguments
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    u32, i32, j32 = (np.ascontiguousarray(t, dtype=np.int32) for t in (u, i, j))
    for which, (arr, pos, val) in enumerate(((u32, 7, 40), (i32, 19, -1), (j32, 0, 30), (j32, 3, -2))):
        bad = [t.copy() for t in (u32, i32, j32)]
        bad[[0, 1, 2, 2][which]][pos] = val
        Uc, Yc = U.copy(), Y.copy()
        s_out = np.full(20, -7.0)
        rc = lib.rtx_bpr_update_host(ptr(Uc), ptr(Yc), 40, 30, 8, ptr(bad[0]), ptr(bad[1]), ptr(bad[2]), 20, LR, REG, None, ptr(s_out))
        assert rc == -1 and "outside the tables" in lib.rtx_last_error().decode()
        assert np.array_equal(_bits(Uc), _bits(U)) and np.array_equal(_bits(Yc), _bits(Y)) and (s_out == -7.0).all()
    assert lib.rtx_bpr_update_host(None, ptr(Y), 40, 30, 8, ptr(u32), ptr(i32), ptr(j32), 20, LR, REG, None, None) == -1
    assert b"NULL" in lib.rtx_last_error()
    assert lib.rtx_bpr_update_host(ptr(U.copy()), ptr(Y.copy()), 40, 30, 8, ptr(u32), ptr(i32), ptr(j32), -1, LR, REG, None, None) == -1
    assert lib.rtx_bpr_fold_in_host(None, None, 3, 30, ptr(Y), 8, LR, REG, 1, 1, None) == -1 and b"NULL" in lib.rtx_last_error()
    ip, ix = np.array([0, 2, 2, 3], dtype=np.int64), np.array([3, 1, 0], dtype=np.int32)                # row 0 is not sorted
    out = np.full((3, 8), -7.0)
    assert lib.rtx_bpr_fold_in_host(ptr(ip), ptr(ix), 3, 30, ptr(Y), 8, LR, REG, 1, 1, ptr(out)) == -1
    assert "sorted, unique" in lib.rtx_last_error().decode() and (out == -7.0).all()
    ip0 = np.array([0, 1, 0, 0], dtype=np.int64)                                                      # nnz = 0, but indptr is not all zeros
    assert lib.rtx_bpr_fold_in_host(ptr(ip0), None, 3, 30, ptr(Y), 8, LR, REG, 1, 1, ptr(out)) == -1
    assert "indptr must be ascending" in lib.rtx_last_error().decode() and (out == -7.0).all()
