#!/usr/bin/env python
"""What gradient clipping costs, in one process on the same data:

* MultiVAE(MultiVAE_net([200, 600, n_items])) in bf16, B = 500, resident sampler -- users/s of fused Adam (the shipped schedule),
  unfused Adam (``fuse_adam = 0``: the schedule a clipped step takes), unfused Adam + norm clip, + value clip, and SGD with momentum
  without and with norm clip;
* SVAE in float32, one user per optimizer step, without and with norm clip;
* the add-on of the norm pass (k_grad_norm_part + k_grad_norm_finish, timing site "grad_norm") in us per step next to the optimizer
  launch's own time (site "adam") from the same run, and both per byte they move: the norm pass re-reads 4 B per parameter, Adam's
  launch moves 28 B per parameter (+ the compute copy).

    python tools/bench_grad_clip.py [--users 20000] [--items 20108] [--batch 500] [--steps 200] [--warmup 20]
                                    [--out profiles/grad_clip_bench.json]

Prints one JSON line per case and writes all of them, with the ratios, to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.optim as optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rectorch_amd.models import MultiVAE, SVAE             # noqa: E402
from rectorch_amd.nets import MultiVAE_net, SVAE_net       # noqa: E402
from rectorch_amd.samplers import DataSampler              # noqa: E402
from rectorch_amd.utils import synth_interactions          # noqa: E402
from rectorch_amd import _lib                              # noqa: E402

# name -> (optimizer factory or None for the model's own Adam, engine knobs, clip attributes, bytes the optimizer launch moves per parameter)
CASES = [
    ("adam_fused", None, {}, {}, 28),
    ("adam_unfused", None, {"fuse_adam": 0}, {}, 28),
    ("adam_norm_clip", None, {}, {"clip_grad_norm": 1.0}, 28),
    ("adam_value_clip", None, {}, {"clip_grad_value": 1e-3}, 28),
    ("sgd_momentum", lambda ps: optim.SGD(ps, lr=0.01, momentum=0.9), {}, {}, 20),
    ("sgd_momentum_norm_clip", lambda ps: optim.SGD(ps, lr=0.01, momentum=0.9), {}, {"clip_grad_norm": 1.0}, 20),
]


def site_us(timings, name):
    if name in timings and timings[name][1]:
        return round(1000.0 * timings[name][0] / timings[name][1], 2)
    return None


def run(name, make, knobs, clip, bytes_per_param, X, a):
    torch.manual_seed(0)
    net = MultiVAE_net([200, 600, a.items], dropout=0.5)
    model = MultiVAE(net, beta=0.2, anneal_steps=0, numerics="bf16")
    if make is not None:
        model.optimizer = make(net.parameters())
    for k, v in clip.items():
        setattr(model, k, v)
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
    norm = model.last_grad_norm
    for site in ("adam", "grad_norm"):                 # the two launches alone, sampled on a few more steps
        eng.set_timing(site, 1)
    for i in range(20):
        model._fused_step(seq[i], None, want_loss=False)
    torch.cuda.synchronize()
    timings = eng.get_timings()
    for site in ("adam", "grad_norm"):
        eng.set_timing(site, 0)
    n_params = sum(p.numel() for p in net.parameters())
    return {"case": name, "class": type(model.optimizer).__name__, "numerics": "bf16", "users": int(X.shape[0]), "items": a.items,
            "batch": a.batch, "us_per_step": round(1000.0 * ms, 2), "users_per_s": round(a.batch / (ms / 1000.0), 1),
            "optimizer_launch_us": site_us(timings, "adam"), "norm_pass_us": site_us(timings, "grad_norm"),
            "optimizer_bytes_per_param": bytes_per_param, "parameters": int(n_params), "last_grad_norm": norm,
            "loss_finite": bool(np.isfinite(loss_sum))}


def run_svae(clip, a):
    """SVAE float32, one [1, T] user per optimizer step (T = 64, 5000 items), train_batch as the epoch loop calls it"""
    torch.manual_seed(0)
    n_items, T = 5000, 64
    net = SVAE_net(n_items=n_items, embed_size=256, rnn_size=200, dec_dims=[64, 150, n_items], enc_dims=[200, 150, 64]).to("cuda")
    model = SVAE(net, beta=0.2, anneal_steps=0)
    for k, v in clip.items():
        setattr(model, k, v)
    rng = np.random.RandomState(3)
    users = []
    for _ in range(16):
        items = torch.from_numpy(rng.randint(0, n_items, size=(1, T)))
        y = torch.zeros(1, T, n_items)
        for t in range(T):
            y[0, t, rng.choice(n_items, size=4, replace=False)] = 1.0
        users.append((items, y.to("cuda")))
    steps = max(a.steps, 50)
    for i in range(10):
        model.train_batch(*users[i % len(users)])
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        model.train_batch(*users[i % len(users)])
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    return {"case": "svae_norm_clip" if clip else "svae", "numerics": "fp32", "items": n_items, "steps_per_user": T,
            "us_per_user": round(1000.0 * ms, 2), "users_per_s": round(1000.0 / ms, 1), "last_grad_norm": model.last_grad_norm,
            "parameters": int(sum(p.numel() for p in net.parameters()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--items", type=int, default=20108)
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    X = synth_interactions(a.users, a.items, seed=7)
    results = []
    for name, make, knobs, clip, bpp in CASES:
        results.append(run(name, make, knobs, clip, bpp, X, a))
        print(json.dumps(results[-1]), flush=True)
    svae = [run_svae({}, a), run_svae({"clip_grad_norm": 1.0}, a)]
    for r in svae:
        print(json.dumps(r), flush=True)
    by = {r["case"]: r for r in results}
    base = by["adam_unfused"]["users_per_s"]
    ratios = {r["case"]: round(r["users_per_s"] / base, 4) for r in results}
    # the yardstick: what the same run's optimizer launch takes per byte it moves, against the norm pass's 4 B per parameter
    c = by["adam_norm_clip"]
    per_byte = None
    if c["optimizer_launch_us"] and c["norm_pass_us"]:
        opt_ps_per_byte = 1e6 * c["optimizer_launch_us"] / (c["optimizer_bytes_per_param"] * c["parameters"])
        norm_ps_per_byte = 1e6 * c["norm_pass_us"] / (4 * c["parameters"])
        per_byte = {"optimizer_ps_per_byte": round(opt_ps_per_byte, 3), "norm_pass_ps_per_byte": round(norm_ps_per_byte, 3),
                    "norm_pass_over_its_share": round(norm_ps_per_byte / opt_ps_per_byte, 3)}
    summary = {"layers": [a.items, 600, 200], "batch": a.batch, "steps": a.steps, "warmup": a.warmup, "results": results, "svae": svae,
               "users_per_s_over_unfused_adam": ratios, "norm_pass_per_byte": per_byte,
               "svae_users_per_s_clipped_over_unclipped": round(svae[1]["users_per_s"] / svae[0]["users_per_s"], 4)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")
    print(json.dumps({"users_per_s_over_unfused_adam": ratios, "norm_pass_per_byte": per_byte}), flush=True)


if __name__ == "__main__":
    main()
