"""States/s of one policy-gradient evaluation on recorded experience: PMLPPolicy.evaluate + loss.backward() through the HIP
kernels (bbx_pmlp_logprob / bbx_pmlp_grad, or bbx_pmlp2_logprob / bbx_pmlp2_grad for --hidden H1,H2 — PMLPPolicy(deep_kernels=True):
hidden activations recomputed, never stored) and through evaluate_torch (torch ops
and autograd over the whole [N, R, cols] block), on identical tensors in the same process.  Prints one JSON line.

    python scripts/bench_policy_grad.py [--states 4096] [--rows 64] [--cols 12] [--hidden 128 | 128,128] [--reps 30]

A third path, "ppo": PMLPPolicy.ppo_step — forward, the same loss and the gradients in one library call (bbx_pmlp_ppo_grad /
bbx_pmlp2_ppo_grad), no autograd.

Each repetition is timed with device events; the rate is states over the MEDIAN repetition; the paths alternate in blocks
of --block repetitions so that drift hits all of them.  Peak memory: torch.cuda.max_memory_allocated over one evaluate + backward of
each path, above what is allocated before it.

    python scripts/bench_policy_grad.py --from-buffer [--T 64] [--B 1024] [--rows 64] [--batch-size 4096] [--pairs 5] [--hidden ...]

One PPO pass over all minibatches of a DeviceTrajectoryBuffer of T x B recorded steps (about a quarter of them left out: episodes
still running at the end of the buffer, states with one row), two ways, alternating in one process:
    gather   buffer.get(batch_size, sort=True)        then evaluate    + loss + backward per minibatch
    index    buffer.get_index(batch_size, sort=True)  then evaluate_at + loss + backward per minibatch (nothing of the size of a
             state block is allocated: the kernels read the buffer in place)
    ppo      buffer.get_index(batch_size, sort=True)  then ppo_step_at per minibatch: forward, loss and gradients in one library call
             (bbx_pmlp_ppo_grad_at / bbx_pmlp2_ppo_grad_at), no autograd; "ppo_vs_index" pairs every ppo pass with the index pass
             before it
Each pass is timed from its get / get_index to the end of its last backward (wall clock between device synchronisations: get()
waits for the device per minibatch); states/s over the median pass with min-max, and torch.cuda.max_memory_allocated of a pass
beyond what the buffer and the policy hold.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

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
ap.add_argument("--from-buffer", action="store_true", help="one PPO pass over a trajectory buffer: get + evaluate against get_index + evaluate_at")
ap.add_argument("--T", type=int, default=64, help="--from-buffer: recorded steps per environment")
ap.add_argument("--B", type=int, default=1024, help="--from-buffer: environments")
ap.add_argument("--batch-size", type=int, default=4096, help="--from-buffer: steps per minibatch")
ap.add_argument("--pairs", type=int, default=5, help="--from-buffer: timed (gather, index) pairs of passes (at least 5)")
a = ap.parse_args()
if a.from_buffer and a.pairs < 5:
    ap.error("--pairs must be at least 5")
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


def from_buffer():
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer
    T, B = a.T, a.B
    gen = torch.Generator(device="cuda"); gen.manual_seed(a.seed)
    rnd = lambda *shape: torch.rand(shape, device="cuda", generator=gen)
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(R, cols))
    # row counts uniform in [2, R] as in the other modes, one state in eight with a single row; an episode ends at a step with
    # probability 8 / T (the steps behind an environment's last end, about T / 8 of them, are incomplete): about a quarter left out
    n = torch.randint(2, R + 1, (T, B), device="cuda", generator=gen, dtype=torch.int32)
    buf.rows.copy_(torch.where(rnd(T, B) < 0.125, torch.ones_like(n), n))
    buf.dones.copy_(rnd(T, B) < 8.0 / T)
    buf.states.copy_(torch.randint(0, 10, buf.states.shape, device="cuda", generator=gen, dtype=torch.int32))
    buf.states.masked_fill_(torch.arange(R, device="cuda")[None, None, :, None] >= buf.rows[:, :, None, None], -1)
    buf.actions.copy_((rnd(T, B) * buf.rows).to(torch.int32).clamp_(max=R - 1))
    buf.logprobs.copy_(-torch.log(buf.rows.float()))
    buf.rewards.copy_(-torch.randint(1, 30, (T, B), device="cuda", generator=gen).double())
    buf.values.copy_(rnd(T, B).double())
    buf.t = T
    buf.finish()

    def loss_of(logp, ent, old, adv):
        ratio = torch.exp(logp - old)
        return -torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean() - 0.01 * ent.mean()

    def gather():
        policy.zero_grad(set_to_none=True)
        count = 0
        for st, act, old, adv, _, rows in buf.get(a.batch_size, sort=True, with_rows=True):
            logp, ent = policy.evaluate(st, act, rows)
            loss_of(logp, ent, old, adv).backward()
            count += act.numel()
        return count

    def index():
        policy.zero_grad(set_to_none=True)
        count = 0
        for idx, act, old, adv, _ in buf.get_index(a.batch_size, sort=True):
            logp, ent = policy.evaluate_at(buf.states, buf.actions, buf.rows, idx)
            loss_of(logp, ent, old, adv).backward()
            count += idx.numel()
        return count

    def ppo():
        policy.zero_grad(set_to_none=True)
        count = 0
        for idx, act, old, adv, _ in buf.get_index(a.batch_size, sort=True):
            policy.ppo_step_at(buf.states, buf.actions, buf.rows, idx, old, adv, clip=0.2, ent_coef=0.01)
            count += idx.numel()
        return count

    paths = {"gather": gather, "index": index, "ppo": ppo}
    grads, times, peak, count = {}, {k: [] for k in paths}, {}, {}
    for name, fn in paths.items():                     # warm up; the gradients of the two paths must be the same numbers
        fn()
        torch.cuda.synchronize()
        grads[name] = [p.grad.detach().clone() for p in policy.parameters()]
    same = all(torch.equal(x, y) for x, y in zip(grads["gather"], grads["index"]))
    # (the fused loss rounds 1 / n and the ratio in its own order: the same gradients up to float32 rounding, not bit for bit; per
    # parameter, relative to its largest entry, the deciding bias left out as in the plain mode: its gradient is rounding on every path)
    ppo_rel = max(float((x - y).abs().max() / y.abs().max().clamp(min=1e-30))
                  for (n, _), x, y in zip(policy.named_parameters(), grads["ppo"], grads["index"]) if n != "deciding.bias")
    del grads
    for _ in range(a.pairs):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            count[name] = fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - base)
    out = {"bench": "policy_grad_from_buffer", "device": torch.cuda.get_device_name(0), "T": T, "B": B, "rows": R, "cols": cols,
           "hidden": a.hidden[0] if len(a.hidden) == 1 else a.hidden, "batch_size": a.batch_size, "pairs": a.pairs,
           "steps_selected": count["index"], "steps_recorded": T * B, "state_block_bytes": buf.states.numel() * 4, "gradients_identical": same}
    for name in paths:
        t = sorted(times[name]); med = statistics.median(t)
        out[name] = {"states_per_s": count[name] / med, "median_ms": med * 1e3, "min_ms": t[0] * 1e3, "max_ms": t[-1] * 1e3, "peak_bytes": int(peak[name])}
    out["index_over_gather"] = statistics.median(times["gather"]) / statistics.median(times["index"])
    pairs = sorted(i / p for i, p in zip(times["index"], times["ppo"]))
    out["ppo_vs_index"] = {"median": statistics.median(pairs), "min": pairs[0], "max": pairs[-1], "rel_grad_difference": ppo_rel}
    print(json.dumps(out))


if a.from_buffer:
    from_buffer()
    sys.exit(0)
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


def ppo_step(_):
    """The same evaluation through PMLPPolicy.ppo_step: one library call, no autograd."""
    policy.zero_grad(set_to_none=True)
    policy.ppo_step(states, actions, None, old, adv, clip=0.2, ent_coef=0.01)      # (rows from the padding, as the other paths)


PATHS = {"kernel": policy.evaluate, "torch": policy.evaluate_torch, "ppo": None}
run = lambda fn: ppo_step(fn) if fn is None else step(fn)
grads, peak = {}, {}
for name, fn in PATHS.items():
    for _ in range(a.warmup):
        run(fn)
    torch.cuda.synchronize()
    grads[name] = [p.grad.detach().clone() for p in policy.parameters()]
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    run(fn)
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
            e0.record(); run(fn); e1.record()
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
# the new path against the autograd path through the same kernels: repetition i of one against repetition i of the other (they
# alternate in blocks), and the gradients (relative to each parameter's largest entry)
pairs = sorted(k / p for k, p in zip(times["kernel"], times["ppo"]))
out["ppo_vs_kernel"] = {"median": statistics.median(pairs), "min": pairs[0], "max": pairs[-1],
                        "rel_grad_difference": max(float((x - y).abs().max() / y.abs().max().clamp(min=1e-30))
                                                   for n, x, y in zip(names, grads["ppo"], grads["kernel"]) if n != "deciding.bias")}
print(json.dumps(out))
