"""States/s of one policy-gradient evaluation on recorded experience: PMLPPolicy.evaluate + loss.backward() through the HIP
kernels (bbx_pmlp_logprob / bbx_pmlp_grad, or bbx_pmlp2_logprob / bbx_pmlp2_grad for --hidden H1,H2 — PMLPPolicy(deep_kernels=True):
hidden activations recomputed, never stored) and through evaluate_torch (torch ops
and autograd over the whole [N, R, cols] block), on identical tensors in the same process.  Prints one JSON line.

    python scripts/bench_policy_grad.py [--states 4096] [--rows 64] [--cols 12] [--hidden 128 | 128,128] [--reps 30]

Each repetition is timed with device events; the rate is states over the MEDIAN repetition; the two paths alternate in blocks
of --block repetitions so that drift hits both.  Peak memory: torch.cuda.max_memory_allocated over one evaluate + backward of
each path, above what is allocated before it.
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
ap.add_argument("--reps", type=int, default=30, help="timed repetitions per path (at least 20)")
ap.add_argument("--block", type=int, default=5)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
if a.reps < 20:
    ap.error("--reps must be at least 20")
if len(a.hidden) not in (1, 2):
    ap.error("--hidden takes one or two layer sizes")
if not torch.cuda.is_available():
    sys.exit("bench_policy_grad: no GPU (there is no CPU fall-back for a measurement)")

N, R, cols = a.states, a.rows, a.cols
rng = np.random.default_rng(a.seed)
torch.manual_seed(a.seed)
policy = PMLPPolicy(cols, a.hidden, deep_kernels=len(a.hidden) == 2).cuda()
rows_h = rng.integers(2, R + 1, size=N).astype(np.int32)
obs_h = rng.integers(0, 10, size=(N, R, cols)).astype(np.int32)
obs_h[np.arange(R)[None, :] >= rows_h[:, None]] = -1
states = torch.from_numpy(obs_h).cuda(); rows = torch.from_numpy(rows_h).cuda()
actions = torch.from_numpy((rng.integers(0, 1 << 30, size=N) % rows_h).astype(np.int32)).cuda()
adv = torch.from_numpy(rng.normal(size=N).astype(np.float32)).cuda()
old = torch.from_numpy((-np.log(rows_h)).astype(np.float32)).cuda()


def step(evaluate):
    """One PPO-style evaluation: clipped surrogate minus an entropy bonus, gradients into the parameters' .grad."""
    policy.zero_grad(set_to_none=True)
    logp, ent = evaluate(states, actions)
    ratio = torch.exp(logp - old)
    loss = -torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean() - 0.01 * ent.mean()
    loss.backward()


PATHS = {"kernel": policy.evaluate, "torch": policy.evaluate_torch}
grads, peak = {}, {}
for name, fn in PATHS.items():
    for _ in range(a.warmup):
        step(fn)
    torch.cuda.synchronize()
    grads[name] = [p.grad.detach().clone() for p in policy.parameters()]
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step(fn)
    torch.cuda.synchronize()
    peak[name] = torch.cuda.max_memory_allocated() - base
# faster and different is not faster: the two paths' gradients on these tensors
# (per parameter, relative to its largest entry; the deciding bias is left out: a softmax does not see a common shift of the
# logits, so its gradient is zero up to rounding on both paths)
names = [n for n, _ in policy.named_parameters()]
rel = {n: float((x - y).abs().max() / y.abs().max().clamp(min=1e-30)) for n, x, y in zip(names, grads["kernel"], grads["torch"]) if n != "deciding.bias"}

times = {name: [] for name in PATHS}
done = 0
while done < a.reps:
    k = min(a.block, a.reps - done)
    for name, fn in PATHS.items():
        for _ in range(k):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); step(fn); e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e-3)
    done += k

med = {name: statistics.median(t) for name, t in times.items()}
out = {"bench": "policy_grad", "device": torch.cuda.get_device_name(0), "states": N, "rows": R, "cols": cols, "hidden": a.hidden[0] if len(a.hidden) == 1 else a.hidden, "reps": a.reps,
       "live_rows_mean": float(rows_h.mean())}
for name in PATHS:
    t = sorted(times[name])
    out[name] = {"states_per_s": N / med[name], "median_ms": med[name] * 1e3, "min_ms": t[0] * 1e3, "p90_ms": t[int(0.9 * (len(t) - 1))] * 1e3,
                 "peak_bytes": int(peak[name])}
out["kernel_over_torch"] = med["torch"] / med["kernel"]
out["rel_grad_difference"] = rel
print(json.dumps(out))
