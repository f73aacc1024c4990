#!/usr/bin/env python
"""Training throughput of the custom-loss route with the package's own differentiable loss, beside the same route with the
reference's loss written in torch ops and beside the fused step, in one process: MultiVAE at the ml-20m shape on a resident sampler.

    python tools/bench_device_loss.py [--users 20000] [--items 20108] [--batch 500] [--steps 100] [--warmup 10] [--numerics bf16]
                                      [--out profiles/device_loss_bench.json]

Routes:  (a) "fused"        the fused step (custom_loss = False)
         (b) "torch_loss"   custom_loss = True, loss_function in torch ops (tools/bench_custom_loss.py's class)
         (c) "device_loss"  custom_loss = True, loss_function = super().loss_function(...): one rtx_multinomial_loss_grad call
                            forward, the saved gradients times the upstream one backward
Prints one JSON line per route (users/s and us/step of back-to-back steps, loss read once at the end), then the ratios c / b and
c / a, and writes everything to --out.  There is no threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402

from rectorch_amd.models import MultiVAE                   # noqa: E402
from rectorch_amd.nets import MultiVAE_net                 # noqa: E402
from rectorch_amd.samplers import DataSampler              # noqa: E402
from rectorch_amd.utils import synth_interactions          # noqa: E402
from rectorch_amd import _lib                              # noqa: E402
import bench_custom_loss as bcl                            # noqa: E402


class DeviceLossMultiVAE(MultiVAE):
    """the common override's core: the package's loss through super()"""
    def loss_function(self, recon_x, x, mu, logvar, beta=1.0):
        return super().loss_function(recon_x, x, mu, logvar, beta)


def run(route, X, a):
    """the timing loop of bench_custom_loss.run with the model class of ``route``"""
    classes = {"fused": MultiVAE, "torch_loss": bcl.TorchLossMultiVAE, "device_loss": DeviceLossMultiVAE}
    torch.manual_seed(0)
    net = MultiVAE_net([200, 600, a.items], dropout=0.5)
    model = classes[route](net, beta=0.2, anneal_steps=20000, numerics=a.numerics)
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
    return {"route": route, "numerics": a.numerics, "users": int(X.shape[0]), "items": a.items, "batch": a.batch,
            "us_per_step": round(1000.0 * ms, 2), "users_per_s": round(a.batch / (ms / 1000.0), 1),
            "loss_finite": bool(np.isfinite(model._read_loss_sum()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--items", type=int, default=20108)
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--numerics", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_loss_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    X = synth_interactions(a.users, a.items, seed=7)
    results = []
    for route in ("fused", "torch_loss", "device_loss"):
        results.append(run(route, X, a))
        print(json.dumps(results[-1]), flush=True)
    ups = {r["route"]: r["users_per_s"] for r in results}
    ratios = {"device_over_torch_loss_users_per_s": round(ups["device_loss"] / ups["torch_loss"], 4),
              "device_over_fused_users_per_s": round(ups["device_loss"] / ups["fused"], 4)}
    summary = {"layers": [a.items, 600, 200], "batch": a.batch, "steps": a.steps, "warmup": a.warmup, "results": results}
    summary.update(ratios)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")
    print(json.dumps(ratios), flush=True)


if __name__ == "__main__":
    main()
