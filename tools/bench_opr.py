#!/usr/bin/env python
"""One-plus-random evaluation throughput (reference rectorch/evaluation.py:113-178) on ml-20m-shaped held-out users, and the
cost of hit@k / mrr@k in evaluate_device:

  opr_host            the reference's loop (one_plus_random_host): scores to the host, a sorted Python list of negatives and
                      random.sample per held-out positive, Metrics on [contests, r + 1]; a bounded sample of users, extrapolated
                      per contest to the whole loader
  opr_device          one_plus_random_device end to end (the same draws and values), median of 3
  draws_host          rtx_opr_draw alone over every user (the host half of the device route: the Python RNG reproduced)
  upload              the draws' host -> device copy alone (pinned memory)
  evaluate_device     users/s with nDCG@100 / Recall@50 and with nDCG / Recall / hit / mrr @100 and @50

    python tools/bench_opr.py [users=10000] [r=1000] [batch=500] [host_sample_users=200]

The contest kernel's own time (k_opr_rank) comes from a kernel trace of this script (rocprofv3 --kernel-trace --stats).
"""
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rectorch_amd.utils import synth_interactions, hash_state_dict          # noqa: E402
from rectorch_amd.utils.synth import split_heldout                           # noqa: E402
from rectorch_amd.nets import MultiVAE_net                                   # noqa: E402
from rectorch_amd.models import MultiVAE                                     # noqa: E402
from rectorch_amd.samplers import DataSampler                                # noqa: E402
from rectorch_amd.evaluation import evaluate_device, one_plus_random_device, one_plus_random_host   # noqa: E402
from rectorch_amd.engine import opr_draw                                     # noqa: E402


def timed(fn, reps):
    ts, r = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def main():
    U = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    r = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 500
    S = int(sys.argv[4]) if len(sys.argv) > 4 else 200
    I, H, L = 20108, 600, 200
    X = synth_interactions(U, I, seed=7)
    tr, te = split_heldout(X, 0.2, seed=1)
    sd = hash_state_dict([I, H, L], [L, H, I], "vae", 5, bias_std=0.05)
    net = MultiVAE_net([L, H, I])
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model = MultiVAE(net, predict_numerics="bf16")
    mets = ["ndcg@10", "recall@10", "hit@10", "mrr@10"]
    smp = DataSampler(tr, te, batch_size=B, shuffle=False)
    contests = int((te.tocsr().data != 0).sum())
    out = {"metric": "one_plus_random users/s on ml-20m-shaped held-out users", "users": U, "items": I, "r": r, "batch": B,
           "contests": contests, "metrics": mets}

    # device route, end to end
    random.seed(0)
    one_plus_random_device(model, smp, mets, r=r)                   # warm-up (engine creation)
    random.seed(0)
    t_dev, d = timed(lambda: one_plus_random_device(model, smp, mets, r=r), 3)
    out["opr_device"] = {"s": t_dev, "users_per_s": U / t_dev, "contests_per_s": contests / t_dev}

    # the host half alone: every user's draws
    te_c = te.tocsr().copy()
    te_c.sum_duplicates()
    held = (te_c.indptr.astype(np.int64), te_c.indices.astype(np.int32), te_c.data.astype(np.float32))
    t0 = time.perf_counter()
    parts = [opr_draw(held, np.arange(lo, min(lo + B, U)), I, r, pin=True) for lo in range(0, U, B)]
    t_draw = time.perf_counter() - t0
    out["draws_host"] = {"s": t_draw, "draws_per_s": contests * r / t_draw}

    # the upload alone
    def upload():
        return [p[2].to("cuda", non_blocking=True) for p in parts]
    upload()
    t_up, _ = timed(upload, 3)
    out["upload"] = {"s": t_up, "bytes": contests * r * 4, "GB_per_s": contests * r * 4 / t_up / 1e9}
    del parts

    # host route on the first S users, extrapolated per contest
    smp_s = DataSampler(tr[:S], te[:S], batch_size=min(B, S), shuffle=False)
    c_s = int((te[:S].tocsr().data != 0).sum())
    random.seed(0)
    t_host, h = timed(lambda: one_plus_random_host(model, smp_s, mets, r=r), 1)
    random.seed(0)
    d_s = one_plus_random_device(model, smp_s, mets, r=r)
    out["opr_host"] = {"sample_users": S, "sample_contests": c_s, "sample_s": t_host,
                       "extrapolated_s": t_host * contests / max(c_s, 1), "users_per_s": U / (t_host * contests / max(c_s, 1)),
                       "sample_equal_to_device": bool(all(np.array_equal(h[m], d_s[m]) for m in mets))}
    out["speedup_vs_host"] = out["opr_host"]["extrapolated_s"] / t_dev

    # evaluate_device: nDCG / Recall only (the kernel's first instantiation) and all four metrics (the second)
    ev = {}
    for name, ms in (("ndcg_recall", ["ndcg@100", "recall@50"]),
                     ("all_four", ["ndcg@100", "recall@50", "hit@100", "mrr@100", "hit@50", "mrr@50"])):
        evaluate_device(model, smp, ms)
        t, _ = timed(lambda: evaluate_device(model, smp, ms), 5)
        ev[name] = {"s": t, "users_per_s": U / t, "metrics": ms}
    out["evaluate_device_bf16"] = ev
    out["value"] = out["opr_device"]["users_per_s"]
    out["unit"] = "users/s"
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
