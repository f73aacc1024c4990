#!/usr/bin/env python
"""Training throughput of CDAE, MultiDAE(CDAE_net(n_items, n_users, 200)), beside Mult-DAE with the same two layers,
MultiDAE(MultiDAE_net([200, n_items])), on the same data in the same process, at the ml-20m shape.

    python tools/bench_cdae.py [--users 116677] [--items 20108] [--latent 200] [--batch 500] [--steps 200] [--warmup 20]
                               [--numerics bf16] [--out profiles/cdae_bench.json]

One run: the Mult-DAE line, the CDAE line, the Mult-DAE line again -- the two Mult-DAE lines are the run's own spread, which the
ratio CDAE / Mult-DAE is read against.  Per line: users/s and us/step of the epoch loop's fused step (resident DataSampler rows with
user_ids="rows", steps enqueued back to back, the next batch announced, joins deferred), and the HIP time of the two launch sites the
user node lives in, post_fwd and post_bwd (events around one launch per step, on steps of their own)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rectorch_amd.models import MultiDAE                   # noqa: E402
from rectorch_amd.nets import CDAE_net, MultiDAE_net       # noqa: E402
from rectorch_amd.samplers import DataSampler              # noqa: E402
from rectorch_amd.utils import synth_interactions          # noqa: E402
from rectorch_amd import _lib                              # noqa: E402

SITES = ("post_fwd", "post_bwd")


def run(kind, numerics, X, a):
    torch.manual_seed(0)
    if kind == "CDAE":
        net = CDAE_net(a.items, X.shape[0], a.latent, dropout=0.5)
        torch.nn.init.normal_(net.user_factors.weight, std=0.01)        # (a table in use, not the zero start)
    else:
        net = MultiDAE_net([a.latent, a.items], dropout=0.5)
    model = MultiDAE(net, lam=0.2, numerics=numerics)
    smp = DataSampler(X, batch_size=a.batch, shuffle=True, user_ids="rows" if kind == "CDAE" else None)
    np.random.seed(3)
    rows = [rb for rb in smp.iter_rows() if len(rb) == a.batch]
    need = a.warmup + a.steps
    seq = [rows[i % len(rows)] for i in range(need)]
    for i in range(a.warmup):
        model._fused_step(seq[i], None, want_loss=False, next_x=seq[i + 1], defer_join=True)
    model._join()
    torch.cuda.synchronize()
    eng = net._rtx_engines[net._rtx_engine_key(numerics, model._loss_kind)]
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
    for s in SITES:
        eng.set_timing(s, 1)
    for i in range(20):
        model._fused_step(seq[i], None, want_loss=False)
    torch.cuda.synchronize()
    timings = eng.get_timings()
    for s in SITES:
        eng.set_timing(s, 0)
    site_us = {s: round(1000.0 * timings[s][0] / max(1, timings[s][1]), 2) for s in SITES if s in timings}
    return {"model": kind, "numerics": numerics, "users": int(X.shape[0]), "items": a.items, "latent": a.latent, "batch": a.batch,
            "us_per_step": round(1000.0 * ms, 2), "users_per_s": round(a.batch / (ms / 1000.0), 1), "site_us": site_us,
            "loss_finite": bool(np.isfinite(loss_sum))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=116677)
    ap.add_argument("--items", type=int, default=20108)
    ap.add_argument("--latent", type=int, default=200)
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--numerics", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdae_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    X = synth_interactions(a.users, a.items, seed=7)
    results = []
    for kind in ("MultiDAE", "CDAE", "MultiDAE"):
        results.append(run(kind, a.numerics, X, a))
        print(json.dumps(results[-1]), flush=True)
    dae = [r["users_per_s"] for r in results if r["model"] == "MultiDAE"]
    cdae = results[1]["users_per_s"]
    summary = {"layers": [a.items, a.latent], "n_users": a.users, "batch": a.batch, "steps": a.steps, "warmup": a.warmup, "results": results,
               "multidae_users_per_s": dae, "multidae_spread": round(abs(dae[0] - dae[1]) / max(dae), 4),
               "cdae_over_multidae_users_per_s": [round(cdae / d, 4) for d in dae]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")
    print(json.dumps({k: summary[k] for k in ("multidae_users_per_s", "multidae_spread", "cdae_over_multidae_users_per_s")}), flush=True)


if __name__ == "__main__":
    main()
