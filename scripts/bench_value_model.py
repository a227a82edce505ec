"""The learned value baseline (PMLPValue, bbx_pmlp_value / bbx_pmlp_value_fit; two hidden layers: bbx_pmlp2_value / bbx_pmlp2_value_fit
through deep_kernels=True) measured three ways; one JSON line per part.

    python scripts/bench_value_model.py [--part all|values|fit|rollout] [--hidden 128 | 128,128 | 64,64] [--pool mean]

values   values/s of DeviceTrajectoryBuffer.fill_values over a recorded block of --T 128 x --B 2048 states of --rows 128 rows (live
         rows uniform in [2, rows]): ONE bbx_pmlp_value call over the block in place, float64 straight into buffer.values.  Each
         repetition timed with device events; the rate is states over the MEDIAN repetition (--reps, at least 20).  Beside it,
         alternating in blocks of --block repetitions, values_torch of the SAME module over the first --torch-states 8192 states of
         the block (the torch path holds [states, rows, hidden] tensors: the whole block does not fit).
fit      one minibatch of the critic's update on --states 4096 positions of that block, two ways on identical tensors,
         alternating in blocks of --block repetitions:
             kernel   PMLPValue.fit_step_at: forward, squared error, statistics and gradients in one library call, the block
                      read in place
             torch    the gathered states through evaluate_torch, 1/2 mean squared error, backward()
         states/s over the median repetition, torch.cuda.max_memory_allocated of one step of each beyond what is allocated before
         it, and the two paths' gradients against each other (faster and different is not faster).
rollout  env-steps/s of run_rollout_fused into a state-keeping buffer with critic=... and without (the same call: the difference
         is fill_values), and of run_rollout(value_strategy="degree") — the baseline the library had before — on fresh batches of
         --batch 4096 environments of --dist for --steps 256 steps: a full warm-up rollout, then the timed one, on the host clock
         around work that ends in env.sync() and torch.cuda.synchronize(); the modes alternate for --pairs pairs (at least 5);
         median with min and max.
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
from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, PMLPValue, run_rollout, run_rollout_fused

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all", choices=["all", "values", "fit", "rollout"])
ap.add_argument("--T", type=int, default=128)
ap.add_argument("--B", type=int, default=2048)
ap.add_argument("--rows", type=int, default=128)
ap.add_argument("--cols", type=int, default=12)
ap.add_argument("--hidden", type=lambda t: [int(h) for h in t.split(",")], default=[128],
                help="units of the hidden layer, or of two: 128,128 (the critic then has deep_kernels=True)")
ap.add_argument("--torch-states", type=int, default=8192, help="values: states of the block the torch path is timed on")
ap.add_argument("--pool", default="mean", choices=sorted(PMLPValue.POOLS))
ap.add_argument("--states", type=int, default=4096, help="fit: positions per minibatch")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=30, help="values, fit: timed repetitions per path (at least 20)")
ap.add_argument("--block", type=int, default=5)
ap.add_argument("--dist", default="3-20-10-weighted")
ap.add_argument("--batch", type=int, default=4096, help="rollout: environments")
ap.add_argument("--steps", type=int, default=256, help="rollout: vector steps")
ap.add_argument("--obs-rows", type=int, default=256, help="rollout: rows per recorded block")
ap.add_argument("--pairs", type=int, default=5, help="rollout: timed runs per mode (at least 5)")
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
if a.reps < 20:
    ap.error("--reps must be at least 20")
if a.pairs < 5:
    ap.error("--pairs must be at least 5")
if len(a.hidden) not in (1, 2):
    ap.error("--hidden takes one or two layer sizes")
if not torch.cuda.is_available():
    sys.exit("bench_value_model: no GPU (there is no CPU fall-back for a measurement)")
dev = torch.device("cuda", torch.cuda.current_device())
name = torch.cuda.get_device_name(0)


def recorded_block():
    """A buffer of T x B recorded states as a rollout leaves them: -1 beyond the live rows."""
    T, B, R, cols = a.T, a.B, a.rows, a.cols
    gen = torch.Generator(device="cuda"); gen.manual_seed(a.seed)
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(R, cols))
    buf.rows.copy_(torch.randint(2, R + 1, (T, B), device="cuda", generator=gen, dtype=torch.int32))
    buf.states.copy_(torch.randint(0, 10, buf.states.shape, device="cuda", generator=gen, dtype=torch.int32))
    buf.states.masked_fill_(torch.arange(R, device="cuda")[None, None, :, None] >= buf.rows[:, :, None, None], -1)
    buf.t = T
    return buf, gen


def event_times(fn, reps):
    out = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    return out


def summary(times, count):
    t = sorted(times); med = statistics.median(t)
    return {"per_s": count / med, "median_ms": med * 1e3, "min_ms": t[0] * 1e3, "p90_ms": t[int(0.9 * (len(t) - 1))] * 1e3}


def part_values(buf, critic):
    n = a.T * a.B
    fill = lambda: buf.fill_values(critic)
    for _ in range(a.warmup):
        fill()
    torch.cuda.synchronize()
    assert critic.last_path == "kernels"
    m = min(a.torch_states, n)
    st, rw = buf.states.view(-1, a.rows, a.cols)[:m], buf.rows.view(-1)[:m]
    out32 = torch.empty(m, dtype=torch.float32, device="cuda")
    fill_torch = lambda: critic.values_torch(st, rw, out=out32)
    for _ in range(a.warmup):
        fill_torch()
    torch.cuda.synchronize()
    times, times_torch, done = [], [], 0
    while done < a.reps:
        k = min(a.block, a.reps - done)
        times += event_times(fill, k); times_torch += event_times(fill_torch, k)
        done += k
    live = float(buf.rows.float().mean())
    out = {"bench": "value_model_values", "device": name, "T": a.T, "B": a.B, "rows": a.rows, "cols": a.cols, "hidden": a.hidden, "pool": a.pool,
           "reps": a.reps, "live_rows_mean": live, "block_bytes": buf.states.numel() * 4, "values": summary(times, n),
           "values_torch": dict(summary(times_torch, m), states=m)}
    out["kernel_over_torch"] = out["values"]["per_s"] / out["values_torch"]["per_s"]
    out["block_GB_per_s"] = out["block_bytes"] / (out["values"]["median_ms"] * 1e-3) / 1e9      # (the whole padded block over the median: an upper
    print(json.dumps(out), flush=True)                                                          # bound on what the kernel reads — it skips dead rows)


def part_fit(buf, critic, gen):
    N, S = a.states, a.T * a.B
    index = torch.randint(0, S, (N,), device="cuda", generator=gen, dtype=torch.int32)
    targets = -30.0 * torch.rand(N, device="cuda", generator=gen)
    flat_states, flat_rows = buf.states.view(-1, a.rows, a.cols), buf.rows.view(-1)

    def kernel():
        critic.zero_grad(set_to_none=True)
        critic.fit_step_at(buf.states, buf.rows, index, targets)

    def torch_path():
        critic.zero_grad(set_to_none=True)
        j = index.to(torch.int64)
        v = critic.evaluate_torch(flat_states[j], flat_rows[j])
        (0.5 * ((v - targets) ** 2).mean()).backward()

    paths = {"kernel": kernel, "torch": torch_path}
    grads, peak = {}, {}
    for key, fn in paths.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        grads[key] = [p.grad.detach().clone() for p in critic.parameters()]
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[key] = torch.cuda.max_memory_allocated() - base
    rel = {n: float((x - y).abs().max() / y.abs().max().clamp(min=1e-30)) for (n, _), x, y in zip(critic.named_parameters(), grads["kernel"], grads["torch"])}
    times = {key: [] for key in paths}
    done = 0
    while done < a.reps:
        k = min(a.block, a.reps - done)
        for key, fn in paths.items():
            times[key] += event_times(fn, k)
        done += k
    out = {"bench": "value_model_fit", "device": name, "states": N, "rows": a.rows, "cols": a.cols, "hidden": a.hidden, "pool": a.pool, "reps": a.reps}
    for key in paths:
        out[key] = dict(summary(times[key], N), peak_bytes=int(peak[key]))
    out["kernel_over_torch"] = statistics.median(times["torch"]) / statistics.median(times["kernel"])
    out["rel_grad_difference"] = rel
    print(json.dumps(out), flush=True)


def part_rollout():
    from deepgroebner_amd import VecLeadMonomialsEnv
    B, T, R = a.batch, a.steps, a.obs_rows
    cols = 2 * int(a.dist.split("-")[0]) * 2                     # (cols = 2 nvars k)
    torch.manual_seed(1)
    policy = PMLPPolicy(cols, a.hidden).to(dev)
    critic = PMLPValue(cols, a.hidden, pool=a.pool, deep_kernels=len(a.hidden) == 2).to(dev)

    def one_run(mode):
        env = VecLeadMonomialsEnv(a.dist, batch=B, k=2)
        env.seed(np.arange(B) + 1000); env.seed_agent(np.arange(B)); env.reset()
        env.accounting(False)
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        buffer = None
        for timed in (False, True):                              # a full warm-up rollout, then the timed one
            del buffer
            buffer = DeviceTrajectoryBuffer(T, B, obs_shape=(R, cols) if mode != "degree" else None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "degree":
                run_rollout(env, policy, T, buffer, obs_rows=R, generator=gen, value_strategy="degree")
            else:
                run_rollout_fused(env, policy, T, buffer, generator=gen, critic=critic if mode == "critic" else None)
            env.sync()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        return T * B / dt

    runs = {"fused_critic": [], "fused_no_values": [], "degree": []}
    modes = {"fused_critic": "critic", "fused_no_values": "none", "degree": "degree"}
    for _ in range(a.pairs):
        for key, mode in modes.items():
            runs[key].append(one_run(mode))
    out = {"bench": "value_model_rollout", "device": name, "dist": a.dist, "batch": B, "steps": T, "obs_rows": R, "hidden": a.hidden, "pool": a.pool,
           "pairs": a.pairs}
    for key, v in runs.items():
        out[key] = {"env_steps_per_s": float(np.median(v)), "min": min(v), "max": max(v)}
    out["critic_over_degree"] = out["fused_critic"]["env_steps_per_s"] / out["degree"]["env_steps_per_s"]
    out["critic_over_no_values"] = out["fused_critic"]["env_steps_per_s"] / out["fused_no_values"]["env_steps_per_s"]
    print(json.dumps(out), flush=True)


if a.part in ("all", "values", "fit"):
    torch.manual_seed(a.seed)
    critic = PMLPValue(a.cols, a.hidden, pool=a.pool, deep_kernels=len(a.hidden) == 2).cuda()
    buf, gen = recorded_block()
    if a.part in ("all", "values"):
        part_values(buf, critic)
    if a.part in ("all", "fit"):
        part_fit(buf, critic, gen)
    del buf
    torch.cuda.empty_cache()
if a.part in ("all", "rollout"):
    part_rollout()
