#!/usr/bin/env python
"""Evaluation throughput of an item-item model (EASE fitted at 4 096 items, synthetic users), users/s of

  evaluate_device   evaluate() on a device-resident DataSampler(test_tr, test_te): per chunk of 1024 users rtx_ease_scores into one
                    float64 scratch buffer, the float64 selection kernel, rtx_list_metrics; one device -> host copy at the end
  host_loop         the same call with model.device_metrics = False: score_rows -> numpy -> Metrics, batch after batch (what the
                    parent commit leaves a user to write by hand)

One warm-up call each, then `reps` timed calls (device synchronised around each); the MEDIAN is reported, min / max beside it.
Writes profiles/item_item_eval_bench.json and prints the same JSON line.

    python tools/bench_item_item_eval.py [users=4000] [batch=500] [n_items=4096] [reps=5] [host_reps=3]
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
from rectorch_amd.utils.synth import split_heldout                           # noqa: E402
from rectorch_amd.models import EASE                                         # noqa: E402
from rectorch_amd.samplers import DataSampler                                # noqa: E402
from rectorch_amd.evaluation import evaluate, _item_item_plan                # noqa: E402

METRICS = ["ndcg@100", "recall@100", "recall@20", "hit@10", "mrr@100"]


def windows(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts, r


def rate(U, ts):
    return {"users_per_s": U / float(np.median(ts)), "median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)),
            "windows": len(ts)}


def main():
    arg = [int(v) for v in sys.argv[1:]]
    U, B, I, reps, host_reps = (arg + [4000, 500, 4096, 5, 3][len(arg):])[:5]
    X = synth_interactions(U, I, seed=9)
    tr, te = split_heldout(X, 0.2, seed=1)
    ease = EASE(lam=100.)
    ease.train(tr)
    smp = DataSampler(tr, te, batch_size=B, shuffle=False)
    assert _item_item_plan(ease, smp, METRICS) is not None
    out = {"metric": "EASE evaluate() users/sec, fold-in of DataSampler(test_tr, test_te)", "users": U, "batch": B, "n_items": I,
           "metrics": METRICS, "unit": "users/s"}
    evaluate(ease, smp, METRICS)                            # warm-up
    ts, dev = windows(lambda: evaluate(ease, smp, METRICS), reps)
    out["evaluate_device"] = rate(U, ts)
    ease.device_metrics = False
    evaluate(ease, smp, METRICS)                            # warm-up
    ts, host = windows(lambda: evaluate(ease, smp, METRICS), host_reps)
    out["host_loop"] = rate(U, ts)
    del ease.device_metrics
    out["max_abs_diff"] = max(float(np.nanmax(np.abs(np.asarray(dev[m], dtype=np.float64) - np.asarray(host[m], dtype=np.float64))))
                              for m in METRICS)
    out["device_over_host"] = out["evaluate_device"]["users_per_s"] / out["host_loop"]["users_per_s"]
    out["value"] = out["evaluate_device"]["users_per_s"]
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "item_item_eval_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
