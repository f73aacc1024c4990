#!/usr/bin/env python
"""SVAE training throughput of the custom-loss route beside the fused step, in one process: the shape and sequence lengths of
tools/bench_svae.py (synthetic ml-1m: embedding 256 -> GRU 200 -> [150] -> latent 64 -> [150] -> n_items, 'next_k' targets), one user
per Adam step, float32 and bf16 products.

    python tools/bench_svae_custom_loss.py [--users 6040] [--items 3416] [--mean-len 165] [--steps 600] [--warmup 60]
                                           [--out profiles/svae_custom_loss_bench.json]

Routes:  (a) "fused"        rtx_svae_train_step (custom_loss = False)
         (b) "torch_loss"   custom_loss = True, the reference's SVAE loss (models.py:1622-1626) written in torch ops
         (c) "device_loss"  custom_loss = True, loss_function = super().loss_function(...): the package's differentiable loss
Every route trains the same users in the same order from the same initial parameters and reads the loss once per step, as
``train_batch`` does.  Prints one JSON line per route and numerics (users/s), then the ratios b / a and c / a, and writes everything
to --out.  One run; there is no threshold."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402

from rectorch_amd.models import SVAE                       # noqa: E402
from rectorch_amd.nets import SVAE_net                     # noqa: E402
from rectorch_amd.samplers import SVAE_Sampler             # noqa: E402
from rectorch_amd import _lib                              # noqa: E402


class TorchLossSVAE(SVAE):
    """the reference's SVAE loss in torch ops"""
    def loss_function(self, recon_x, x, mu, logvar, beta=1.0):
        nll = -(torch.log_softmax(recon_x, -1) * x.view(recon_x.shape)).sum()
        d = float(x[0, :recon_x.shape[2]].sum())
        kl = -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=-1))
        return nll / d + beta * kl


class DeviceLossSVAE(SVAE):
    """the common override's core: the package's loss through super()"""
    def loss_function(self, recon_x, x, mu, logvar, beta=1.0):
        return super().loss_function(recon_x, x, mu, logvar, beta)


def sequences(a):
    """the users of tools/bench_svae.py"""
    rng = np.random.RandomState(1)
    lens = np.clip(rng.lognormal(np.log(a.mean_len) - 0.5, 1.0, size=a.users).astype(int), 5, a.max_len)
    pop = rng.zipf(1.3, size=int(lens.sum()) * 2)
    pop = pop[pop <= a.items][: int(lens.sum())] - 1
    seqs, o = {}, 0
    for u in range(a.users):
        seqs[u] = pop[o:o + lens[u]].tolist()
        o += lens[u]
    return seqs


def run(route, numerics, seqs, a):
    classes = {"fused": SVAE, "torch_loss": TorchLossSVAE, "device_loss": DeviceLossSVAE}
    torch.manual_seed(0)
    net = SVAE_net(n_items=a.items, embed_size=256, rnn_size=200, dec_dims=[64, 150, a.items], enc_dims=[200, 150, 64])
    model = classes[route](net.to("cuda"), beta=0.2, anneal_steps=20000, numerics=numerics)
    model.custom_loss = route != "fused"
    np.random.seed(0)
    smp = SVAE_Sampler(a.items, seqs, None, pred_type="next_k", k=a.k, shuffle=True, sparse=True)
    batches = []
    for i, (x, y) in enumerate(smp):
        batches.append((x.to("cuda"), y))
        if i + 1 >= a.steps + a.warmup:
            break
    w = min(a.warmup, len(batches) // 2)
    for x, y in batches[:w]:
        model.train_batch(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps_t, loss = 0, 0.0
    for x, y in batches[w:]:
        loss = model.train_batch(x, y)
        steps_t += x.numel()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = len(batches) - w
    return {"route": route, "numerics": numerics, "items": a.items, "users_timed": n, "mean_len": round(steps_t / n, 2),
            "users_per_s": round(n / dt, 1), "ms_per_user": round(dt / n * 1e3, 4), "last_loss_finite": bool(np.isfinite(loss))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3416)
    ap.add_argument("--mean-len", type=float, default=165.0)
    ap.add_argument("--max-len", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svae_custom_loss_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    seqs = sequences(a)
    summary = {"workload": "SVAE train, synthetic ml-1m shape: %d items, embed 256, GRU 200, enc [200,150,64], dec [64,150,I], next_k "
                           "k=%d, one user per Adam step" % (a.items, a.k), "steps": a.steps, "warmup": a.warmup, "runs": 1, "results": []}
    for numerics in ("fp32", "bf16"):
        ups = {}
        for route in ("fused", "torch_loss", "device_loss"):
            r = run(route, numerics, seqs, a)
            summary["results"].append(r)
            ups[route] = r["users_per_s"]
            print(json.dumps(r), flush=True)
        ratios = {"torch_loss_over_fused_users_per_s": round(ups["torch_loss"] / ups["fused"], 4),
                  "device_loss_over_fused_users_per_s": round(ups["device_loss"] / ups["fused"], 4)}
        summary[numerics] = ratios
        print(json.dumps({numerics: ratios}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
