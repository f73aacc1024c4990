#!/usr/bin/env python
"""Training throughput of the reference's plain autoencoder, AETrainer(MultiDAE_net([200, 600, n_items])) (MSE loss), beside
MultiDAE(MultiDAE_net([200, 600, n_items])) (multinomial loss + norm regulariser) on the same data in the same process, at the
ml-20m item count.

    python tools/bench_ae.py [--users 20000] [--items 20108] [--batch 500] [--steps 200] [--warmup 20] [--numerics bf16]
                             [--out profiles/ae_mse_bench.json]

Prints one JSON line per (model, numerics): users/s and us/step of the epoch loop's fused step (resident DataSampler rows,
steps enqueued back to back, loss read once at the end), and the HIP time of the step's loss kernel.  Writes both results and
the ratio AETrainer / MultiDAE of users/s per numerics mode to --out: the ratio within one run is the number that matters."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rectorch_amd.models import AETrainer, MultiDAE        # noqa: E402
from rectorch_amd.nets import MultiDAE_net                 # noqa: E402
from rectorch_amd.samplers import DataSampler              # noqa: E402
from rectorch_amd.utils import synth_interactions          # noqa: E402
from rectorch_amd import _lib                              # noqa: E402


def run(kind, numerics, X, a):
    torch.manual_seed(0)
    net = MultiDAE_net([200, 600, a.items], dropout=0.5)
    model = AETrainer(net, numerics=numerics) if kind == "AETrainer" else MultiDAE(net, lam=0.2, numerics=numerics)
    smp = DataSampler(X, batch_size=a.batch, shuffle=False)
    rows = list(smp.iter_rows())
    need = a.warmup + a.steps
    seq = [rows[i % len(rows)] for i in range(need)]
    for i in range(a.warmup):
        model._fused_step(seq[i], None, want_loss=False, next_x=seq[i + 1], defer_join=True)
    model._join()
    torch.cuda.synchronize()
    eng = net._rtx_engines[net._rtx_engine_key(numerics, model._loss_kind)]
    site = "mse_dlogits_loss" if kind == "AETrainer" else "dlogits_loss"
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(a.warmup, need):
        nxt = seq[i + 1] if i + 1 < need else None
        model._fused_step(seq[i], None, want_loss=False, next_x=nxt, defer_join=True)
    model._join()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.steps
    loss_sum = model._read_loss_sum()
    # the loss kernel alone, sampled on a few more steps (events around one launch per step)
    eng.set_timing(site, 1)
    for i in range(10):
        model._fused_step(seq[i], None, want_loss=False)
    torch.cuda.synchronize()
    timings = eng.get_timings()
    eng.set_timing(site, 0)
    loss_us = None
    if site in timings:
        tot, n = timings[site]
        loss_us = 1000.0 * tot / max(1, n)
    return {"model": kind, "numerics": numerics, "users": int(X.shape[0]), "items": a.items, "batch": a.batch,
            "us_per_step": round(1000.0 * ms, 2), "users_per_s": round(a.batch / (ms / 1000.0), 1),
            "loss_kernel_us": None if loss_us is None else round(loss_us, 2), "loss_finite": bool(np.isfinite(loss_sum))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--items", type=int, default=20108)
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--numerics", nargs="+", default=["bf16"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ae_mse_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    X = synth_interactions(a.users, a.items, seed=7)
    results, ratios = [], {}
    for numerics in a.numerics:
        per = {}
        for kind in ("MultiDAE", "AETrainer"):
            per[kind] = run(kind, numerics, X, a)
            results.append(per[kind])
            print(json.dumps(per[kind]), flush=True)
        ratios[numerics] = round(per["AETrainer"]["users_per_s"] / per["MultiDAE"]["users_per_s"], 4)
    summary = {"layers": [a.items, 600, 200], "batch": a.batch, "steps": a.steps, "warmup": a.warmup, "results": results,
               "aetrainer_over_multidae_users_per_s": ratios}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")
    print(json.dumps({"aetrainer_over_multidae_users_per_s": ratios}), flush=True)


if __name__ == "__main__":
    main()
