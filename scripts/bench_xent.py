"""States/s of one cross-entropy training step against per-row target distributions, two ways on identical tensors in one process:
    kernel   PMLPPolicy.xent_step: forward, loss, statistics and gradients in one library call (bbx_pmlp_xent_grad, or
             bbx_pmlp2_xent_grad for --hidden H1,H2); hidden activations recomputed, never stored
    torch    what the same job took before the kernels: policy.forward(states), the cross-entropy -(t * log p) over the live rows
             with torch ops, backward() through autograd
Prints one JSON line.

    python scripts/bench_xent.py [--states 4096] [--rows 64] [--cols 12] [--hidden 128 | 128,128] [--repeats 5] [--reps 20]

--repeats repeats, each a block of --reps timed steps per path (device events), the paths alternating repeat by repeat so that
drift hits both; per path the median step of every repeat, the median and the spread (min - max) of those, states/s over the
median, and torch.cuda.max_memory_allocated of one step above what is allocated before it.  The gradients of the two paths on
these tensors are compared (per parameter, relative to its largest entry).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from deepgroebner_amd.rollout import PMLPPolicy

ap = argparse.ArgumentParser()
ap.add_argument("--states", type=int, default=4096)
ap.add_argument("--rows", type=int, default=64, help="rows per state block (R); the live rows of a state are uniform in [2, R]")
ap.add_argument("--cols", type=int, default=12)
ap.add_argument("--hidden", type=lambda t: [int(h) for h in t.split(",")], default=[128], help="hidden units: H, or H1,H2 for two hidden layers")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--reps", type=int, default=20, help="timed steps per path and repeat")
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
if len(a.hidden) not in (1, 2):
    ap.error("--hidden takes one or two layer sizes")
if not torch.cuda.is_available():
    sys.exit("bench_xent: no GPU (there is no CPU fall-back for a measurement)")

N, R, cols = a.states, a.rows, a.cols
rng = np.random.default_rng(a.seed)
torch.manual_seed(a.seed)
policy = PMLPPolicy(cols, a.hidden, deep_kernels=len(a.hidden) == 2).cuda()
rows_h = rng.integers(2, R + 1, size=N).astype(np.int32)
obs_h = rng.integers(0, 10, size=(N, R, cols)).astype(np.int32)
live_h = np.arange(R)[None, :] < rows_h[:, None]
obs_h[~live_h] = -1
t_h = np.where(live_h, rng.uniform(0.05, 1.0, size=(N, R)), 0.0)
t_h = (t_h / t_h.sum(axis=1, keepdims=True)).astype(np.float32)
states = torch.from_numpy(obs_h).cuda(); rows = torch.from_numpy(rows_h).cuda(); targets = torch.from_numpy(t_h).cuda()
live = torch.from_numpy(live_h).cuda()


def kernel():
    policy.zero_grad(set_to_none=True)
    policy.xent_step(states, rows, targets)


def torch_path():
    policy.zero_grad(set_to_none=True)
    lp = policy.forward(states)                                   # (log-softmax over the live rows: the padded ones at -1e9)
    loss = -(targets * torch.where(live, lp, torch.zeros_like(lp))).sum() / N
    loss.backward()


PATHS = {"kernel": kernel, "torch": torch_path}
grads, peak = {}, {}
for name, fn in PATHS.items():
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    grads[name] = [p.grad.detach().clone() for p in policy.parameters()]
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak[name] = torch.cuda.max_memory_allocated() - base
names = [n for n, _ in policy.named_parameters()]
rel = {n: float((x - y).abs().max() / y.abs().max().clamp(min=1e-30)) for n, x, y in zip(names, grads["kernel"], grads["torch"]) if n != "deciding.bias"}

per_repeat = {name: [] for name in PATHS}
for _ in range(a.repeats):
    for name, fn in PATHS.items():
        t = []
        for _ in range(a.reps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        per_repeat[name].append(statistics.median(t))

out = {"bench": "xent", "device": torch.cuda.get_device_name(0), "states": N, "rows": R, "cols": cols,
       "hidden": a.hidden[0] if len(a.hidden) == 1 else a.hidden, "repeats": a.repeats, "reps": a.reps, "live_rows_mean": float(rows_h.mean())}
for name in PATHS:
    t = per_repeat[name]; med = statistics.median(t)
    out[name] = {"states_per_s": N / (med * 1e-3), "median_ms": med, "min_ms": min(t), "max_ms": max(t), "repeat_ms": t, "peak_bytes": int(peak[name])}
out["kernel_over_torch"] = out["torch"]["median_ms"] / out["kernel"]["median_ms"]
out["rel_grad_difference"] = rel
print(json.dumps(out))
