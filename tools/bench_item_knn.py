#!/usr/bin/env python
"""ItemKNN on the ml-20m shape (utils.synth.synth_interactions(116677, 20108), binary), cosine, k = 100, on ONE MI355X:

  fit               rtx_knn_fit: HIP-event durations of the whole fit and of its phases (Gram matrix, similarity, selection; the rest is
                    the CSR build) from rtx_knn_timings, and the host wall time of KnnSolver(...) -- median of `fit_reps` fits after one
                    warm-up fit
  scores            KnnSolver.scores (k_knn_scores) on 10 000 training users in chunks of 1 024 into one scratch buffer, users/s
  recommend         ItemKNN.recommend(k=100, remove_train=True) on the same users (scores + the float64 selection kernel; the upload of
                    the exclusion matrix is inside the call), users/s
  ease_scores       EaseSolver.scores (k_ease_scores, the dense item-item product) on the same users and chunks in the same run: the
                    dense yardstick
  scipy_host        scipy `X[users] @ W` on the host CPU (W = the fitted model as a csr_matrix), users/s

Every timed window starts and ends with a device synchronise and holds enough passes over the users to last >= `min_window_s`; one
warm-up pass comes first; the MEDIAN window is reported with min / max.  Bytes per user: what the two kernels read from the model
(stored weights touched x 12 bytes against dense rows x 8 n_items bytes), computed from the data, not measured.
Writes profiles/item_knn_bench.json and prints the same JSON line.

    python tools/bench_item_knn.py [users=10000] [chunk=1024] [k=100] [reps=5] [fit_reps=3] [n_users=116677] [n_items=20108]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rectorch_amd.utils import synth_interactions                            # noqa: E402
from rectorch_amd.engine import CsrMatrix, EaseSolver, KnnSolver             # noqa: E402
from rectorch_amd.models import ItemKNN                                      # noqa: E402

MIN_WINDOW_S = 0.25


def windows(fn, reps, min_window_s=MIN_WINDOW_S):
    """median / min / max seconds of ONE call of fn over `reps` windows of `inner` calls each (inner sized by a warm-up call)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()                                                    # warm-up
    torch.cuda.synchronize()
    once = max(time.perf_counter() - t0, 1e-6)
    inner = max(1, int(np.ceil(min_window_s / once)))
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / inner)
    return ts, inner


def rate(n, ts, inner):
    return {"users_per_s": n / float(np.median(ts)), "median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)),
            "windows": len(ts), "passes_per_window": inner}


def main():
    arg = [int(v) for v in sys.argv[1:]]
    n_score, chunk, k, reps, fit_reps, U, I = (arg + [10000, 1024, 100, 5, 3, 116677, 20108][len(arg):])[:7]
    assert torch.cuda.is_available(), "bench_item_knn needs the MI355X"
    X = synth_interactions(U, I)
    X.data[:] = 1.0
    n_score = min(n_score, U)
    train = CsrMatrix(X)
    out = {"metric": "ItemKNN (cosine, k=%d) fit and scoring on the ml-20m shape" % k, "n_users": U, "n_items": I, "nnz": int(X.nnz), "k": k,
           "similarity": "cosine", "shrink": 0.0, "normalize": False, "score_users": n_score, "chunk": chunk, "unit": "users/s",
           "device": torch.cuda.get_device_name(0)}
    # ---- fit
    KnnSolver(train, k)                                     # warm-up: code objects, allocator
    fits, walls = [], []
    solver = None
    for _ in range(fit_reps):
        solver = None                                       # (free the last model first)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver = KnnSolver(train, k)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        fits.append(solver.timings())
    out["fit"] = {key: float(np.median([f[key] for f in fits])) for key in ("fit_ms", "gram_ms", "sim_ms", "select_ms")}
    out["fit"]["csr_build_ms"] = out["fit"]["fit_ms"] - out["fit"]["gram_ms"] - out["fit"]["sim_ms"] - out["fit"]["select_ms"]
    out["fit"]["host_wall_ms"] = 1e3 * float(np.median(walls))
    out["fit"]["fits"] = fit_reps
    out["model_nnz"] = solver.nnz
    # ---- scoring: the sparse kernel and the dense yardstick on the same users, same chunks
    ids = torch.arange(n_score, dtype=torch.int32, device="cuda")
    scratch = torch.empty((min(chunk, n_score), I), dtype=torch.float64, device="cuda")

    def score_pass(s):
        for lo in range(0, n_score, chunk):
            part = ids[lo:lo + chunk]
            s.scores(part, None, out=scratch[:part.numel()])

    ts, inner = windows(lambda: score_pass(solver), reps)
    out["scores"] = rate(n_score, ts, inner)
    model = ItemKNN(k=k)
    model._solver = solver
    test_tr = X[:n_score]
    ids_host = np.arange(n_score, dtype=np.int32)
    ts, inner = windows(lambda: model.recommend(ids_host, test_tr, k=100), reps)
    out["recommend"] = rate(n_score, ts, inner)
    ease = EaseSolver(train, 500.0)
    ts, inner = windows(lambda: score_pass(ease), reps)
    out["ease_scores"] = rate(n_score, ts, inner)
    out["sparse_over_dense"] = out["scores"]["users_per_s"] / out["ease_scores"]["users_per_s"]
    del ease
    # ---- bytes per user read from the model (computed from the data)
    W = model.W
    row_len = np.diff(W.indptr)
    per_user_weights = np.add.reduceat(row_len[test_tr.indices], test_tr.indptr[:-1])[np.diff(test_tr.indptr) > 0]
    out["bytes_per_user"] = {"sparse_model_bytes": 12.0 * float(per_user_weights.mean()),
                             "dense_model_bytes": 8.0 * I * float(np.diff(test_tr.indptr).mean()),
                             "stored_weights_touched": float(per_user_weights.mean()),
                             "entries_per_user": float(np.diff(test_tr.indptr).mean())}
    # ---- the host CPU
    Xs = test_tr.astype(np.float64)
    t0 = time.perf_counter()
    ref = Xs @ W
    out["scipy_host"] = {"users_per_s": n_score / (time.perf_counter() - t0), "windows": 1}
    # the two agree (first chunk; the orders of the sums differ)
    m = min(chunk, n_score)
    got = solver.scores(ids[:m]).cpu().numpy()
    out["max_abs_diff_vs_scipy"] = float(np.max(np.abs(got - ref[:m].toarray())))
    out["value"] = out["scores"]["users_per_s"]
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "item_knn_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
