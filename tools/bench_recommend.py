#!/usr/bin/env python
"""Top-N list throughput on ml-20m-shaped users (synthetic): users/s at k = 100 and k = 1000 of

  one_call          recommend(): rtx_engine_recommend, forward + selection kernel for the whole loader in ONE C call
  per_batch         recommend() with the one-call route switched off: model.predict per batch + rtx_topk_items on its scores
  recommend_host    predict -> D2H of the [B, n_items] scores -> numpy lexsort (what a user of the reference writes)
  torch_topk        predict -> torch.topk on the device (a second yardstick; its tie order is unspecified)
  evaluate_device   the metrics twin of one_call on the same loader (nDCG@k, Recall@k): same forward, a selection with more
                    reduction work and no list written; five windows each, their spread is printed
  ease              EASE.recommend (float64 scores in chunks + the float64 selection kernel) against EASE.predict + a host sort

One JSON line.

    python tools/bench_recommend.py [users=10000] [batch=500] [ease_items=4096]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rectorch_amd.utils import synth_interactions, hash_state_dict          # noqa: E402
from rectorch_amd.utils.synth import split_heldout                           # noqa: E402
from rectorch_amd.nets import MultiVAE_net                                   # noqa: E402
from rectorch_amd.models import MultiVAE, EASE                               # noqa: E402
from rectorch_amd.samplers import DataSampler                                # noqa: E402
from rectorch_amd import evaluation                                          # noqa: E402
from rectorch_amd.evaluation import recommend, recommend_host, evaluate_device, _lexsort_topk   # noqa: E402


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


def per_batch(model, smp, k):
    """recommend()'s per-batch route on a loader that would take the one-call route"""
    route = evaluation._recommend_route
    evaluation._recommend_route = lambda m, l, kk: "batch"
    try:
        return recommend(model, smp, k=k)
    finally:
        evaluation._recommend_route = route


def torch_topk(model, smp, k):
    parts = []
    for rb in smp.iter_rows():
        v, i = torch.topk(model.predict(rb)[0], k, dim=1)
        parts.append((i, v))
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def main():
    U = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 500
    EI = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    I, H, L = 20108, 600, 200
    X = synth_interactions(U, I, seed=7)
    tr, te = split_heldout(X, 0.2, seed=1)
    sd = hash_state_dict([I, H, L], [L, H, I], "vae", 5, bias_std=0.05)
    smp = DataSampler(tr, te, batch_size=B, shuffle=False)
    UH = min(U, 2000)                                    # the host loop sorts ~300 users/s: a bounded sample of the same users
    smp_host = DataSampler(tr[:UH], te[:UH], batch_size=B, shuffle=False)
    net = MultiVAE_net([L, H, I])
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model = MultiVAE(net, predict_numerics="bf16")
    out = {"metric": "MultiVAE recommend() users/sec on ml-20m-shaped users (bf16 predict numerics)", "users": U, "batch": B, "unit": "users/s"}
    for k in (100, 1000):
        res = {}
        recommend(model, smp, k=k)                       # warm-up (engine creation, compute copies)
        ts, one = windows(lambda: recommend(model, smp, k=k), 5)
        res["one_call"] = rate(U, ts)
        ts, pb = windows(lambda: per_batch(model, smp, k), 5)
        res["per_batch"] = rate(U, ts)
        res["per_batch_equals_one_call"] = bool(torch.equal(one[0], pb[0]) and torch.equal(one[1], pb[1]))
        ts, tt = windows(lambda: torch_topk(model, smp, k), 5)
        res["torch_topk"] = rate(U, ts)
        res["torch_topk_same_scores"] = bool(torch.equal(one[1], tt[1]))
        ts, host = windows(lambda: recommend_host(model, smp_host, k=k), 1)
        res["recommend_host"] = dict(rate(UH, ts), users=UH)
        res["host_equals_one_call"] = bool(torch.equal(one[0][:UH], host[0]) and torch.equal(one[1][:UH], host[1]))
        mets = ["ndcg@%d" % k, "recall@%d" % k]
        evaluate_device(model, smp, mets)
        ts, _ = windows(lambda: evaluate_device(model, smp, mets), 5)
        res["evaluate_device"] = rate(U, ts)
        out["k%d" % k] = res
    out["value"] = out["k100"]["one_call"]["users_per_s"]
    del model, net
    # EASE: float64 scores; a narrower item set keeps the fit (an n_items^3 Cholesky) out of the way of what is measured
    Xe = synth_interactions(U, EI, seed=9)
    ease = EASE(lam=100.)
    ease.train(Xe)
    ids = np.arange(min(U, 4000))
    test_tr = Xe[ids]
    out["ease"] = {"users": int(len(ids)), "n_items": EI}
    for k in (100, 1000):
        ease.recommend(ids, test_tr, k=k)
        ts, dev = windows(lambda: ease.recommend(ids, test_tr, k=k), 5)

        def host_sort():
            return _lexsort_topk(ease.predict(ids, test_tr)[0], k)
        th, hs = windows(host_sort, 1)
        out["ease"]["k%d" % k] = {"recommend": rate(len(ids), ts), "predict_host_sort": rate(len(ids), th),
                                  "equal": bool(np.array_equal(dev[0].cpu().numpy(), hs[0]))}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
