#!/usr/bin/env python
"""WMF (implicit-feedback ALS) on the ml-20m shape (utils.synth.synth_interactions(116677, 20108), binary), f = 64, alpha = 40, lam = 1,
on ONE MI355X.  One GPU step per invocation, each merged into profiles/wmf_bench.json:

    python tools/bench_wmf.py fit      per sweep: Gram matrices, user half-sweep, item half-sweep in ms (rtx_wmf_timings of a fit of
                                       `iters` iterations after a one-iteration warm-up fit, divided by `iters`), the host wall time,
                                       and beside them the arithmetic floor: 2 nnz fp^2 flops per half-sweep (fp = f rounded up to 16:
                                       what the MFMA tiles of the accumulation do, the triangle counted as the full square it stands
                                       for) at the f64 MFMA rate that profiles/admm_bench.json records for the ADMM GEMM
                                       (iter_tflops_f64), and the fraction of that rate reached; then 256 users and the 8 longest
                                       item rows of the fitted model solved again and compared with numpy.linalg.solve
    python tools/bench_wmf.py scores   WmfSolver.scores (fold-in + scores) and WMF.recommend(k=100) on 10 000 training users in chunks
                                       of 1 024, users/s
    python tools/bench_wmf.py ease     EaseSolver.scores on the same users and chunks: the dense yardstick of the family
    python tools/bench_wmf.py numpy    a numpy half-sweep (wmf_ref64's "solve" formulation, inlined) on a 2 000-user subsample,
                                       SCALED to the full user count and labelled so (no GPU work)
    python tools/bench_wmf.py          the four steps, each a fresh child process under `timeout` of its own, chained: a step that
                                       fails or runs out of time ends the run

Timed windows as in tools/bench_item_knn.py: device synchronise at both ends, enough passes to last >= 0.25 s, one warm-up pass, the
MEDIAN window reported with min / max.  No target is set in advance.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "wmf_bench.json")
U, I, F, ALPHA, LAM, ITERS = 116677, 20108, 64, 40.0, 1.0, 3
N_SCORE, CHUNK, REPS = 10000, 1024, 5
MIN_WINDOW_S = 0.25
STEPS = (("fit", 600), ("scores", 300), ("ease", 300), ("numpy", 600))


def data():
    from rectorch_amd.utils import synth_interactions
    X = synth_interactions(U, I)
    X.data[:] = 1.0
    return X


def y0():
    return np.random.RandomState(98765).normal(0, 0.01, (I, F))


def merge(key, value):
    out = {}
    if os.path.exists(OUT):
        with open(OUT) as fh:
            out = json.loads(fh.read() or "{}")
    out.update({"metric": "WMF (f=%d, alpha=%g, lam=%g) fit and scoring on the ml-20m shape" % (F, ALPHA, LAM), "n_users": U, "n_items": I,
                "factors": F, "alpha": ALPHA, "lam": LAM})
    out[key] = value
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(json.dumps(out) + "\n")
    print(json.dumps({key: value}), flush=True)


def windows(fn, reps):
    import torch
    fn()                                                    # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()                                                    # one pass to size the windows by
    torch.cuda.synchronize()
    once = max(time.perf_counter() - t0, 1e-6)
    inner = max(1, int(np.ceil(MIN_WINDOW_S / once)))
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / inner)
    return {"users_per_s": N_SCORE / float(np.median(ts)), "median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)),
            "windows": len(ts), "passes_per_window": inner}


def step_fit():
    import torch
    from rectorch_amd.engine import WmfSolver
    X = data()
    WmfSolver(X, y0(), ALPHA, LAM, 1)                       # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = WmfSolver(X, y0(), ALPHA, LAM, ITERS)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    t = s.timings()
    fp = (F + 15) // 16 * 16
    flops = 2.0 * X.nnz * fp * fp
    with open(os.path.join(ROOT, "profiles", "admm_bench.json")) as fh:
        rate = float(json.loads(fh.readline())["iter_tflops_f64"])
    res = {"iterations": ITERS, "nnz": int(X.nnz), "device": torch.cuda.get_device_name(0),
           "gram_ms_per_sweep": t["gram_ms"] / ITERS, "user_half_ms": t["user_ms"] / ITERS, "item_half_ms": t["item_ms"] / ITERS,
           "fit_ms": t["fit_ms"], "host_wall_ms": 1e3 * wall, "longest_user_row": int(np.diff(X.indptr).max()),
           "longest_item_row": int(np.diff(X.T.tocsr().indptr).max()),
           "floor": {"flops_per_half_sweep": flops, "f64_mfma_tflops_of_admm_gemm": rate, "floor_ms_per_half_sweep": flops / rate / 1e9,
                     "user_half_fraction_of_rate": flops / (t["user_ms"] / ITERS * 1e-3) / 1e12 / rate,
                     "item_half_fraction_of_rate": flops / (t["item_ms"] / ITERS * 1e-3) / 1e12 / rate}}
    # what was timed is also right at this shape: 256 users and the 8 longest item rows (the segmented ones) against numpy
    from rectorch_amd.engine import wmf_solve_rows
    Yf, Uf = s.factors("items"), s.factors("users")
    XT = X.T.tocsr()
    XT.sort_indices()
    longest = np.argsort(-np.diff(XT.indptr))[:8].astype(np.int32)
    res["check_vs_numpy"] = {"user_rows": 256, "item_rows": [int(v) for v in np.diff(XT.indptr)[longest]],
                             "user_max_rel": _check(X, Yf, np.arange(256, dtype=np.int32), wmf_solve_rows(s.train, Yf, ALPHA, LAM, np.arange(256))),
                             "item_max_rel": _check(XT, Uf, longest, wmf_solve_rows(s.train_t, Uf, ALPHA, LAM, longest))}
    merge("fit", res)


def _check(M, table, rows, got):
    """max over the rows of |x_device - x_numpy|_inf / |x_numpy|_inf, x_numpy by numpy.linalg.solve on the definition"""
    T = table.cpu().numpy()
    got = got.cpu().numpy()
    G = T.T @ T
    worst = 0.0
    for q, u in enumerate(rows):
        idx = M.indices[M.indptr[u]:M.indptr[u + 1]]
        w = ALPHA * M.data[M.indptr[u]:M.indptr[u + 1]].astype(np.float64)
        Tu = T[idx]
        x = np.linalg.solve(G + Tu.T @ (w[:, None] * Tu) + LAM * np.eye(F), Tu.T @ (1.0 + w)) if len(idx) else np.zeros(F)
        worst = max(worst, float(np.abs(got[q] - x).max() / max(np.abs(x).max(), 1e-300)))
    return worst


def step_scores():
    import torch
    from rectorch_amd.engine import WmfSolver
    from rectorch_amd.models import WMF
    X = data()
    s = WmfSolver(X, y0(), ALPHA, LAM, 1)
    ids = torch.arange(N_SCORE, dtype=torch.int32, device="cuda")
    scratch = torch.empty((CHUNK, I), dtype=torch.float64, device="cuda")

    def score_pass():
        for lo in range(0, N_SCORE, CHUNK):
            part = ids[lo:lo + CHUNK]
            s.scores(part, None, out=scratch[:part.numel()])

    merge("scores", windows(score_pass, REPS))
    model = WMF(factors=F, alpha=ALPHA, lam=LAM, num_iter=1)
    model._solver = s
    test_tr = X[:N_SCORE]
    ids_host = np.arange(N_SCORE, dtype=np.int32)
    merge("recommend", windows(lambda: model.recommend(ids_host, test_tr, k=100), REPS))


def step_ease():
    import torch
    from rectorch_amd.engine import CsrMatrix, EaseSolver
    X = data()
    ease = EaseSolver(CsrMatrix(X), 500.0)
    ids = torch.arange(N_SCORE, dtype=torch.int32, device="cuda")
    scratch = torch.empty((CHUNK, I), dtype=torch.float64, device="cuda")

    def score_pass():
        for lo in range(0, N_SCORE, CHUNK):
            part = ids[lo:lo + CHUNK]
            ease.scores(part, None, out=scratch[:part.numel()])

    merge("ease_scores", windows(score_pass, REPS))


def step_numpy(sample=2000):
    X = data().tocsr()
    Y = y0()
    G = Y.T @ Y
    t0 = time.perf_counter()
    for u in range(sample):
        idx = X.indices[X.indptr[u]:X.indptr[u + 1]]
        if not len(idx):
            continue
        w = ALPHA * X.data[X.indptr[u]:X.indptr[u + 1]]
        Yu = Y[idx]
        np.linalg.solve(G + Yu.T @ (w[:, None] * Yu) + LAM * np.eye(F), Yu.T @ (1.0 + w))
    dt = time.perf_counter() - t0
    merge("numpy_user_half", {"label": "SCALED: %d users timed, multiplied by n_users / %d" % (sample, sample), "sample_users": sample,
                              "sample_s": dt, "scaled_user_half_ms": 1e3 * dt * U / sample})


def main():
    if len(sys.argv) > 1:
        {"fit": step_fit, "scores": step_scores, "ease": step_ease, "numpy": step_numpy}[sys.argv[1]]()
        return
    for name, limit in STEPS:
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), name])
        if rc != 0:
            print("bench_wmf: step %s ended with status %d: the run stops here" % (name, rc), flush=True)
            sys.exit(rc)
    with open(OUT) as fh:
        print(fh.read().strip(), flush=True)


if __name__ == "__main__":
    main()
