#!/usr/bin/env python
"""Training throughput of MultiVAE(MultiVAE_net([200, 600, n_items])) in bf16 under each optimizer the device step has a rule for, in
one process on the same data: fused Adam (the shipped schedule), Adam with the engine knob ``fuse_adam = 0`` (the schedule every other
rule takes: gradients stored, one optimizer launch behind them), and SGD without and with momentum, AdamW, Adagrad, RMSprop without
and with momentum.

    python tools/bench_optimizers.py [--users 20000] [--items 20108] [--batch 500] [--steps 200] [--warmup 20]
                                     [--out profiles/optimizers_bench.json]

Prints one JSON line per optimizer: users/s and us/step of the epoch loop's step (resident DataSampler rows, steps enqueued back to
back, the loss read once at the end) and the HIP time of the optimizer launch ("adam": one multi-tensor launch of k_optim over all
tensors; absent for fused Adam, whose update runs inside the weight-gradient kernels).  Writes all results and each rule's users/s
relative to unfused Adam to --out: every rule moves at most Adam's bytes per parameter, so that ratio within one run is the number
that matters."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.optim as optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rectorch_amd.models import MultiVAE                   # noqa: E402
from rectorch_amd.nets import MultiVAE_net                 # noqa: E402
from rectorch_amd.samplers import DataSampler              # noqa: E402
from rectorch_amd.utils import synth_interactions          # noqa: E402
from rectorch_amd import _lib                              # noqa: E402

# name -> (optimizer factory or None for the model's own Adam, engine knobs, state bytes moved per parameter: p, g and the state)
CASES = [
    ("adam_fused", None, {}, 28),
    ("adam_unfused", None, {"fuse_adam": 0}, 28),
    ("adamw", lambda ps: optim.AdamW(ps, lr=1e-3, weight_decay=0.01), {}, 28),
    ("sgd", lambda ps: optim.SGD(ps, lr=0.01), {}, 12),
    ("sgd_momentum", lambda ps: optim.SGD(ps, lr=0.01, momentum=0.9), {}, 20),
    ("adagrad", lambda ps: optim.Adagrad(ps, lr=0.01), {}, 20),
    ("rmsprop", lambda ps: optim.RMSprop(ps, lr=1e-3), {}, 20),
    ("rmsprop_momentum", lambda ps: optim.RMSprop(ps, lr=1e-3, momentum=0.9), {}, 28),
]


def run(name, make, knobs, bytes_per_param, X, a):
    torch.manual_seed(0)
    net = MultiVAE_net([200, 600, a.items], dropout=0.5)
    model = MultiVAE(net, beta=0.2, anneal_steps=0, numerics="bf16")
    if make is not None:
        model.optimizer = make(net.parameters())
    smp = DataSampler(X, batch_size=a.batch, shuffle=False)
    rows = list(smp.iter_rows())
    need = a.warmup + a.steps
    seq = [rows[i % len(rows)] for i in range(need)]
    st, _, m, v = model._ensure_train_state()          # the engine exists before its first step: knobs are set by then
    eng = net.rtx_engine("bf16", a.batch, train_buffers=(st.grads, m, v), loss=model._loss_kind)
    for k, val in knobs.items():
        eng.set_option(k, int(val))
    for i in range(a.warmup):
        model._fused_step(seq[i], None, want_loss=False, next_x=seq[i + 1], defer_join=True)
    model._join()
    torch.cuda.synchronize()
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
    eng.set_timing("adam", 1)                          # the optimizer launch alone, sampled on a few more steps
    for i in range(10):
        model._fused_step(seq[i], None, want_loss=False)
    torch.cuda.synchronize()
    timings = eng.get_timings()
    eng.set_timing("adam", 0)
    opt_us = None
    if "adam" in timings and timings["adam"][1]:
        opt_us = 1000.0 * timings["adam"][0] / timings["adam"][1]
    n_params = sum(p.numel() for p in net.parameters())
    return {"optimizer": name, "class": type(model.optimizer).__name__, "numerics": "bf16", "users": int(X.shape[0]), "items": a.items,
            "batch": a.batch, "us_per_step": round(1000.0 * ms, 2), "users_per_s": round(a.batch / (ms / 1000.0), 1),
            "optimizer_launch_us": None if opt_us is None else round(opt_us, 2), "state_bytes_per_param": bytes_per_param,
            "parameters": int(n_params), "loss_finite": bool(np.isfinite(loss_sum))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--items", type=int, default=20108)
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizers_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    X = synth_interactions(a.users, a.items, seed=7)
    results = []
    for name, make, knobs, bpp in CASES:
        results.append(run(name, make, knobs, bpp, X, a))
        print(json.dumps(results[-1]), flush=True)
    base = next(r for r in results if r["optimizer"] == "adam_unfused")["users_per_s"]
    ratios = {r["optimizer"]: round(r["users_per_s"] / base, 4) for r in results}
    summary = {"layers": [a.items, 600, 200], "batch": a.batch, "steps": a.steps, "warmup": a.warmup, "results": results,
               "users_per_s_over_unfused_adam": ratios}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")
    print(json.dumps({"users_per_s_over_unfused_adam": ratios}), flush=True)


if __name__ == "__main__":
    main()
