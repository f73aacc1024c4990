#!/usr/bin/env python
"""How far the conditioned samplers hold CMultiVAE's epoch loop below MultiVAE's, and what building the batches on the device
(``resident=True``) gives back.  Synthetic data at the ml-20m item count, network [20108, 600, 200], 20 conditions with every
item in 1-3 of them, B = 500, bf16.

    python tools/bench_cmvae_sampler.py [--users 1500] [--eval-users 300] [--items 20108] [--batch 500]
                                        [--out profiles/cmvae_sampler_bench.json]

Four training cases, each ``train_epoch`` over the SAME examples (the same number of batches) after an untimed warm-up epoch over a
short sampler of the same batch shape: the dense host sampler, ``sparse=True`` (the host builds two small CSR matrices per batch),
``resident=True`` (the device builds them), and MultiVAE on a resident ``DataSampler`` with as many batches -- the rate the engine
itself runs at.  The fast cases repeat the epoch until the timed window is long enough to mean something.  Then
``evaluate(["ndcg@100", "recall@20"])`` of a conditioned validation loader through the host loop (``sparse=True`` loader) and
through the device route of a ``resident=True`` loader.  Prints one JSON line per case and writes examples/s and the ratios to
--out; the ratio resident / sparse within one run is the number that matters."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy.sparse import csr_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rectorch_amd import _lib                                                   # noqa: E402
from rectorch_amd.evaluation import evaluate                                    # noqa: E402
from rectorch_amd.models import CMultiVAE, MultiVAE                             # noqa: E402
from rectorch_amd.nets import CMultiVAE_net, MultiVAE_net                       # noqa: E402
from rectorch_amd.samplers import ConditionedDataSampler, DataSampler           # noqa: E402
from rectorch_amd.utils import synth_interactions                               # noqa: E402

N_COND = 20
SAMPLER_KW = {"dense": {}, "sparse": {"sparse": True}, "resident": {"resident": True}}


def conditions(n_items, seed=3):
    rng = np.random.RandomState(seed)
    return {i: sorted(rng.choice(N_COND, size=rng.randint(1, 4), replace=False).tolist()) for i in range(n_items)}


def timed_epochs(model, sampler, min_s, max_epochs):
    """(seconds, epochs): whole train_epoch calls (each ends by reading the loss sum: a device synchronise) until min_s is reached"""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while n < max_epochs and (n == 0 or time.perf_counter() - t0 < min_s):
        n += 1
        model.train_epoch(n, sampler, verbose=0)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, n


def run_cmvae(kind, X, X_warm, iid2cids, a):
    torch.manual_seed(0)
    np.random.seed(0)
    net = CMultiVAE_net(N_COND, [200, 600, a.items], dropout=0.5)
    model = CMultiVAE(net, beta=0.2, numerics="bf16")
    warm = ConditionedDataSampler(iid2cids, N_COND, X_warm, None, batch_size=a.batch, shuffle=True, **SAMPLER_KW[kind])
    smp = ConditionedDataSampler(iid2cids, N_COND, X, None, batch_size=a.batch, shuffle=True, **SAMPLER_KW[kind])
    model.train_epoch(0, warm, verbose=0)
    secs, epochs = timed_epochs(model, smp, a.min_seconds, 1 if kind == "dense" else a.max_epochs)
    n_ex = len(smp.examples)            # (targets are the input rows: no example is dropped)
    return {"case": "cmvae_" + kind, "examples": n_ex, "batches": len(smp), "epochs": epochs, "seconds": round(secs, 4),
            "examples_per_s": round(n_ex * epochs / secs, 1), "us_per_batch": round(1e6 * secs / (epochs * len(smp)), 1)}


def run_mvae(n_batches, a):
    torch.manual_seed(0)
    np.random.seed(0)
    X = synth_interactions(n_batches * a.batch, a.items, seed=11)
    net = MultiVAE_net([200, 600, a.items], dropout=0.5)
    model = MultiVAE(net, beta=0.2, numerics="bf16")
    model.train_epoch(0, DataSampler(X[:4 * a.batch], batch_size=a.batch, shuffle=True), verbose=0)
    smp = DataSampler(X, batch_size=a.batch, shuffle=True)
    secs, epochs = timed_epochs(model, smp, a.min_seconds, a.max_epochs)
    return {"case": "mvae_resident_datasampler", "examples": X.shape[0], "batches": len(smp), "epochs": epochs, "seconds": round(secs, 4),
            "examples_per_s": round(X.shape[0] * epochs / secs, 1), "us_per_batch": round(1e6 * secs / (epochs * len(smp)), 1)}


def run_eval(kind, Xtr, Xte, iid2cids, a):
    torch.manual_seed(0)
    net = CMultiVAE_net(N_COND, [200, 600, a.items], dropout=0.5)
    model = CMultiVAE(net, beta=0.2, numerics="bf16")
    smp = ConditionedDataSampler(iid2cids, N_COND, Xtr, Xte, batch_size=a.batch, shuffle=False, **SAMPLER_KW[kind])
    metrics = ["ndcg@100", "recall@20"]
    warm = ConditionedDataSampler(iid2cids, N_COND, Xtr[:40], Xte[:40], batch_size=a.batch, shuffle=False, **SAMPLER_KW[kind])
    evaluate(model, warm, metrics)
    torch.cuda.synchronize()
    t0, reps = time.perf_counter(), 0
    while reps < a.max_epochs and (reps == 0 or time.perf_counter() - t0 < a.min_seconds):
        res = evaluate(model, smp, metrics)
        reps += 1
    secs = time.perf_counter() - t0
    n = len(res[metrics[0]])
    return {"case": "evaluate_" + ("device_route_resident" if kind == "resident" else "host_loop_" + kind), "examples": n, "reps": reps,
            "seconds": round(secs, 4), "examples_per_s": round(n * reps / secs, 1),
            "ndcg@100": float(np.nanmean(res["ndcg@100"])), "recall@20": float(np.nanmean(res["recall@20"]))}


def split(X, seed=5):
    """every user's items cut 80 / 20 into (tr, te), at least one item on each side"""
    rng = np.random.RandomState(seed)
    X = X.tocsr()
    held = np.zeros(X.nnz, dtype=bool)
    for u in range(X.shape[0]):
        lo, hi = X.indptr[u], X.indptr[u + 1]
        k = min(max(1, (hi - lo) // 5), hi - lo - 1)
        held[lo + rng.choice(hi - lo, size=k, replace=False)] = True
    tr, te = X.copy(), X.copy()
    tr.data = np.where(held, 0.0, 1.0)
    te.data = np.where(held, 1.0, 0.0)
    tr.eliminate_zeros()
    te.eliminate_zeros()
    return csr_matrix(tr), csr_matrix(te)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1500)
    ap.add_argument("--warm-users", type=int, default=100)
    ap.add_argument("--eval-users", type=int, default=300)
    ap.add_argument("--items", type=int, default=20108)
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--max-epochs", type=int, default=40)
    ap.add_argument("--cases", nargs="+", default=["dense", "sparse", "resident"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmvae_sampler_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    X = synth_interactions(a.users + a.warm_users + a.eval_users, a.items, seed=7)
    X.data[:] = 1.0
    X_train, X_warm, X_eval = X[:a.users], X[a.users:a.users + a.warm_users], X[a.users + a.warm_users:]
    iid2cids = conditions(a.items)
    results = {}
    for kind in a.cases:
        r = results["cmvae_" + kind] = run_cmvae(kind, X_train, X_warm, iid2cids, a)
        print(json.dumps(r), flush=True)
    n_batches = max(r["batches"] for r in results.values())
    r = results["mvae_resident_datasampler"] = run_mvae(n_batches, a)
    print(json.dumps(r), flush=True)
    Xtr, Xte = split(X_eval)
    for kind in ("sparse", "resident"):
        if kind in a.cases:
            r = run_eval(kind, Xtr, Xte, iid2cids, a)
            results[r["case"]] = r
            print(json.dumps(r), flush=True)

    def ratio(num, den):
        if num in results and den in results:
            return round(results[num]["examples_per_s"] / results[den]["examples_per_s"], 3)
        return None
    ratios = {"train_resident_over_sparse": ratio("cmvae_resident", "cmvae_sparse"),
              "train_resident_over_dense": ratio("cmvae_resident", "cmvae_dense"),
              "train_sparse_over_dense": ratio("cmvae_sparse", "cmvae_dense"),
              "train_resident_over_mvae": ratio("cmvae_resident", "mvae_resident_datasampler"),
              "evaluate_device_route_over_host_loop": ratio("evaluate_device_route_resident", "evaluate_host_loop_sparse")}
    summary = {"layers": [a.items, 600, 200], "n_cond": N_COND, "batch": a.batch, "numerics": "bf16", "users": a.users,
               "min_seconds": a.min_seconds, "results": results, "ratios": ratios}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")
    print(json.dumps({"ratios": ratios}), flush=True)


if __name__ == "__main__":
    main()
