#!/usr/bin/env python
"""What gradient accumulation costs or gains, in one process on the same data:

* MultiVAE(MultiVAE_net([200, 600, n_items])), B = 500 rows per micro-batch, resident sampler -- users/s of fused Adam (the shipped
  schedule), unfused Adam (``fuse_adam = 0``), and ``accumulate_grad_batches`` = 2, 4, 8 in bf16; k = 4 with norm clipping; k = 4 in
  float32 next to float32 without accumulation;
* the per-launch time of the accumulating weight-gradient kernels (timing sites ``gemm_dW_*_acc``) next to the plain-store ones
  (``gemm_dW_*``) and of the optimizer launch (``adam``), sampled in the same run.

By bytes per parameter a micro-step that only accumulates reads and writes the float32 accumulator (8 B) where the optimizer launch
moves 12-28 B, so a window should cost less per user than unfused Adam; the numbers say whether it does.

    python tools/bench_grad_accum.py [--users 20000] [--items 20108] [--batch 500] [--steps 240] [--warmup 24]
                                     [--out profiles/grad_accum_bench.json]

Prints one JSON line per case and writes all of them, with the ratios, to --out."""
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

# name -> (numerics, accumulate_grad_batches, engine knobs, clip attributes)
CASES = [
    ("adam_fused", "bf16", 1, {}, {}),
    ("adam_unfused", "bf16", 1, {"fuse_adam": 0}, {}),
    ("accum_k2", "bf16", 2, {}, {}),
    ("accum_k4", "bf16", 4, {}, {}),
    ("accum_k8", "bf16", 8, {}, {}),
    ("accum_k4_norm_clip", "bf16", 4, {}, {"clip_grad_norm": 1.0}),
    ("fp32_adam", "fp32", 1, {}, {}),
    ("fp32_accum_k4", "fp32", 4, {}, {}),
]
W_SITES = ("gemm_dW_out", "gemm_dW_in", "gemm_dW_hidden")


def site_us(timings, name):
    if name in timings and timings[name][1]:
        return round(1000.0 * timings[name][0] / timings[name][1], 2)
    return None


def run(name, numerics, k, knobs, clip, X, a):
    torch.manual_seed(0)
    net = MultiVAE_net([200, 600, a.items], dropout=0.5)
    model = MultiVAE(net, beta=0.2, anneal_steps=0, numerics=numerics)
    for key, v in clip.items():
        setattr(model, key, v)
    model.accumulate_grad_batches = k
    smp = DataSampler(X, batch_size=a.batch, shuffle=False)
    rows = list(smp.iter_rows())
    steps = a.steps // k * k                            # whole windows
    warm = (a.warmup + k - 1) // k * k
    need = warm + steps
    seq = [rows[i % len(rows)] for i in range(need)]
    st, _, m, v = model._ensure_train_state()          # the engine exists before its first step: knobs are set by then
    eng = net.rtx_engine(numerics, a.batch, train_buffers=(st.grads, m, v), loss=model._loss_kind)
    for key, val in knobs.items():
        eng.set_option(key, int(val))
    for i in range(warm):
        model._fused_step(seq[i], None, want_loss=False, next_x=seq[i + 1] if i + 1 < need else None, defer_join=True)
    model._join()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(warm, need):
        model._fused_step(seq[i], None, want_loss=False, next_x=seq[i + 1] if i + 1 < need else None, defer_join=True)
    model._join()
    t1.record()
    torch.cuda.synchronize()
    assert model.pending_micro_batches == 0
    ms = t0.elapsed_time(t1) / steps
    loss_sum = model._read_loss_sum()
    sites = [s for w in W_SITES for s in (w, w + "_acc")] + ["adam", "grad_norm"]
    for s in sites:                                     # the launches alone, on a few more windows
        eng.set_timing(s, 1)
    for i in range(4 * k if k > 1 else 12):
        model._fused_step(seq[i], None, want_loss=False)
    torch.cuda.synchronize()
    timings = eng.get_timings()
    for s in sites:
        eng.set_timing(s, 0)
    launches = {s: site_us(timings, s) for s in sites if site_us(timings, s) is not None}
    return {"case": name, "numerics": numerics, "accumulate_grad_batches": k, "users": int(X.shape[0]), "items": a.items,
            "micro_batch": a.batch, "us_per_micro_step": round(1000.0 * ms, 2), "users_per_s": round(a.batch / (ms / 1000.0), 1),
            "launch_us": launches, "parameters": int(sum(p.numel() for p in net.parameters())),
            "last_grad_norm": model.last_grad_norm, "loss_finite": bool(np.isfinite(loss_sum))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--items", type=int, default=20108)
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    X = synth_interactions(a.users, a.items, seed=7)
    results = []
    for name, numerics, k, knobs, clip in CASES:
        results.append(run(name, numerics, k, knobs, clip, X, a))
        print(json.dumps(results[-1]), flush=True)
    by = {r["case"]: r for r in results}
    ratios = {r["case"]: round(r["users_per_s"] / by["adam_unfused" if r["numerics"] == "bf16" else "fp32_adam"]["users_per_s"], 4)
              for r in results}
    summary = {"layers": [a.items, 600, 200], "micro_batch": a.batch, "steps": a.steps, "warmup": a.warmup, "results": results,
               "users_per_s_over_unfused_adam_of_the_same_numerics": ratios}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")
    print(json.dumps({"users_per_s_over_unfused_adam_of_the_same_numerics": ratios}), flush=True)


if __name__ == "__main__":
    main()
