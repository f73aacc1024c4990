#!/usr/bin/env python
"""Training throughput of a forward composed from the network's three pieces (a ``MultiVAE_net`` subclass whose ``forward`` is
``decode(_reparameterize(*encode(x)))``: ``rtx_engine_encode_train`` / ``rtx_reparam`` / ``rtx_engine_decode_train`` and their
backward calls) beside the two routes it extends, in one process: MultiVAE at the ml-20m shape on a resident sampler, one run.

    python tools/bench_split_forward.py [--users 20000] [--items 20108] [--batch 500] [--steps 100] [--warmup 10] [--numerics bf16]
                                        [--out profiles/split_forward_bench.json]

Prints one JSON line per route -- the fused step, ``custom_loss`` through ``net(x)``, ``custom_loss`` through the composed
``forward`` (both with the reference's loss written in torch ops) -- with users/s and us/step of back-to-back steps (loss read once at
the end), then the ratio composed / net(x).  Writes everything to --out.  There is no threshold: the composed route launches no
product twice; it adds two C calls, a pad-convert, and the reparam, import and export kernels."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rectorch_amd.models import MultiVAE                   # noqa: E402
from rectorch_amd.nets import MultiVAE_net                 # noqa: E402
from rectorch_amd.samplers import DataSampler              # noqa: E402
from rectorch_amd.utils import synth_interactions          # noqa: E402
from rectorch_amd import _lib                              # noqa: E402


class TorchLossMultiVAE(MultiVAE):
    """the reference's MultiVAE.loss_function (rectorch/models.py:813-815) in torch ops"""
    def loss_function(self, recon_x, x, mu, logvar, beta=1.0):
        nll = -torch.mean(torch.sum(torch.log_softmax(recon_x, 1) * x, -1))
        kld = -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))
        return nll + beta * kld


class ComposedMultiVAE_net(MultiVAE_net):
    """the reference's MultiVAE_net.forward (rectorch/nets.py:407-411) written from its three pieces"""
    def forward(self, x):
        mu, logvar = self.encode(x)
        z = self._reparameterize(mu, logvar)
        return self.decode(z), mu, logvar


ROUTES = ("fused", "custom_loss_net", "custom_loss_composed")


def run(route, X, a):
    torch.manual_seed(0)
    net = (ComposedMultiVAE_net if route == "custom_loss_composed" else MultiVAE_net)([200, 600, a.items], dropout=0.5)
    model = (MultiVAE if route == "fused" else TorchLossMultiVAE)(net, beta=0.2, anneal_steps=20000, numerics=a.numerics)
    model.custom_loss = route != "fused"
    rows = list(DataSampler(X, batch_size=a.batch, shuffle=False).iter_rows())
    need = a.warmup + a.steps
    seq = [rows[i % len(rows)] for i in range(need + 1)]

    def step(i):
        model._fused_step(seq[i], None, want_loss=False, next_x=seq[i + 1], defer_join=True)
    for i in range(a.warmup):
        step(i)
    model._join()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(a.warmup, need):
        step(i)
    model._join()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.steps
    loss_sum = model._read_loss_sum()
    return {"route": route, "numerics": a.numerics, "users": int(X.shape[0]), "items": a.items, "batch": a.batch,
            "us_per_step": round(1000.0 * ms, 2), "users_per_s": round(a.batch / (ms / 1000.0), 1),
            "loss_finite": bool(np.isfinite(loss_sum))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--items", type=int, default=20108)
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--numerics", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_forward_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    X = synth_interactions(a.users, a.items, seed=7)
    results = []
    for route in ROUTES:
        results.append(run(route, X, a))
        print(json.dumps(results[-1]), flush=True)
    ratio = round(results[2]["users_per_s"] / results[1]["users_per_s"], 4)
    summary = {"layers": [a.items, 600, 200], "batch": a.batch, "steps": a.steps, "warmup": a.warmup, "results": results,
               "composed_over_net_users_per_s": ratio}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")
    print(json.dumps({"composed_over_net_users_per_s": ratio}), flush=True)


if __name__ == "__main__":
    main()
