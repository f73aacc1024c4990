#!/usr/bin/env python
"""Training throughput of the custom-loss route (``model.custom_loss = True``: the engine's training forward with a grad_fn, the
loss in torch, ``loss.backward()`` through ``rtx_engine_backward``, ``rtx_engine_apply_adam``) beside the fused step, in one
process: MultiVAE at the ml-20m shape on a resident sampler, the custom route trained with the reference's own loss written in
torch ops.

    python tools/bench_custom_loss.py [--users 20000] [--items 20108] [--batch 500] [--steps 100] [--warmup 10] [--numerics bf16]
                                      [--out profiles/custom_loss_bench.json]

Prints one JSON line per route: users/s and us/step of back-to-back steps (loss read once at the end), then the ratio custom /
fused and the HIP time of the import kernel (k_import_dout, the engine's timing site "import_dout") against the bytes it moves --
the float32 gradient in, the engine's D out -- at the 8 TB/s roofline the README uses.  Writes everything to --out.  There is no
threshold: the route is expected to be slower (float32 logits leave the engine, torch's loss ops run, the gradient comes back)."""
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

HBM_ROOF = 8.0e12      # bytes / s


class TorchLossMultiVAE(MultiVAE):
    """the reference's MultiVAE.loss_function (rectorch/models.py:813-815) in torch ops"""
    def loss_function(self, recon_x, x, mu, logvar, beta=1.0):
        nll = -torch.mean(torch.sum(torch.log_softmax(recon_x, 1) * x, -1))
        kld = -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))
        return nll + beta * kld


def run(custom, X, a):
    torch.manual_seed(0)
    net = MultiVAE_net([200, 600, a.items], dropout=0.5)
    model = (TorchLossMultiVAE if custom else MultiVAE)(net, beta=0.2, anneal_steps=20000, numerics=a.numerics)
    model.custom_loss = custom
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
    out = {"route": "custom_loss" if custom else "fused", "numerics": a.numerics, "users": int(X.shape[0]), "items": a.items,
           "batch": a.batch, "us_per_step": round(1000.0 * ms, 2), "users_per_s": round(a.batch / (ms / 1000.0), 1),
           "loss_finite": bool(np.isfinite(loss_sum))}
    if custom:
        eng = net._rtx_engines[net._rtx_engine_key(a.numerics)]
        eng.set_timing("import_dout", 1)
        for i in range(10):
            step(i)
        torch.cuda.synchronize()
        timings = eng.get_timings()
        eng.set_timing("import_dout", 0)
        if "import_dout" in timings:
            tot, n = timings["import_dout"]
            us = 1000.0 * tot / max(1, n)
            esz = 2 if a.numerics == "bf16" else 4
            pad = lambda v, m: (v + m - 1) // m * m      # noqa: E731  (the engine pads the batch to 64 rows, the items to 128 columns)
            moved = 4.0 * a.batch * a.items + esz * pad(a.batch, 64) * pad(a.items + 1, 128)
            out.update({"import_kernel_us": round(us, 2), "import_bytes": int(moved),
                        "import_roofline_us": round(moved / HBM_ROOF * 1e6, 2),
                        "import_fraction_of_roofline": round(moved / HBM_ROOF * 1e6 / us, 3) if us > 0 else None})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--items", type=int, default=20108)
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--numerics", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "custom_loss_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    X = synth_interactions(a.users, a.items, seed=7)
    fused = run(False, X, a)
    print(json.dumps(fused), flush=True)
    custom = run(True, X, a)
    print(json.dumps(custom), flush=True)
    ratio = round(custom["users_per_s"] / fused["users_per_s"], 4)
    summary = {"layers": [a.items, 600, 200], "batch": a.batch, "steps": a.steps, "warmup": a.warmup, "results": [fused, custom],
               "custom_over_fused_users_per_s": ratio}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")
    print(json.dumps({"custom_over_fused_users_per_s": ratio}), flush=True)


if __name__ == "__main__":
    main()
