"""env-steps/s of a policy rollout that records the baseline value of every state it visits (pg.py:451-475 with --value_model
degree: env.value('degree', gamma) before every step), the host in the loop against the device-side path:
    sync     env.values() each step (settles the handle, one blocking copy), copied into buffer.values[t] — only calls that
             exist without bbx_values_device, so this mode measures any commit
    device   run_rollout(..., value_strategy="degree"): bbx_values_device straight into the buffer's row, rollouts of the
             clones overlapping the steps that follow (ring depth: --ring n sets BBX_VALUE_RING, 1 removes the overlap)
One command alternates the modes (--mode both, the default) for --pairs pairs — with --rings 1,2,4 every pair also runs the
device mode at those depths — each run a fresh batch, a full warm-up rollout, then T timed steps on the host clock around work
that ends in env.sync() and torch.cuda.synchronize().  Prints one JSON line per run, then the finish() times of the torch
loop and of the GAE kernel on the last buffer, then a summary line.
    python scripts/bench_values_rollout.py [--mode both|sync|device] [--ring N] [--rings 1,2,4] [--pairs 5] [--batch 4096] [--steps 256]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from deepgroebner_amd import VecLeadMonomialsEnv
from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, run_rollout

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="both", choices=["both", "sync", "device"])
ap.add_argument("--ring", type=int, default=0, help="BBX_VALUE_RING of the device mode (0: the library's default)")
ap.add_argument("--rings", default="", help="comma-separated depths every pair runs in device mode besides --ring")
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--dist", default="3-20-10-weighted")
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--steps", type=int, default=256)
ap.add_argument("--hidden", type=int, default=128)
ap.add_argument("--obs-rows", type=int, default=256)
a = ap.parse_args()
B, T, R = a.batch, a.steps, a.obs_rows
dev = torch.device("cuda", torch.cuda.current_device())


def make_env(ring):
    old = os.environ.get("BBX_VALUE_RING")
    if ring:
        os.environ["BBX_VALUE_RING"] = str(ring)                 # (read when the handle is created)
    try:
        env = VecLeadMonomialsEnv(a.dist, batch=B, k=2)
    finally:
        if ring:
            if old is None:
                os.environ.pop("BBX_VALUE_RING", None)
            else:
                os.environ["BBX_VALUE_RING"] = old
    env.seed(np.arange(B) + 1000); env.seed_agent(np.arange(B)); env.reset()
    env.accounting(False)
    return env


@torch.no_grad()
def rollout_sync(env, policy, buffer, gen):
    """run_rollout's loop (one library call per vector step) with env.values() in front of every step."""
    stream = torch.cuda.current_stream()
    obs = torch.empty((B, R, env.cols), dtype=torch.int32, device=dev)
    rew = torch.zeros(B, dtype=torch.float64, device=dev); done = torch.zeros(B, dtype=torch.uint8, device=dev)
    rows = torch.zeros(B, dtype=torch.int32, device=dev); act = torch.zeros(B, dtype=torch.int32, device=dev)
    logp = torch.zeros(B, dtype=torch.float32, device=dev)
    env.rollout_device("first", 0, False, stream.cuda_stream, rew, done, rows, obs, R, True, False)
    env.sync()
    w = policy._fused_weights()
    u_all = torch.rand((T, B), device=dev, generator=gen)
    for t in range(T):
        buffer.rows[t].copy_(rows)
        buffer.values[t].copy_(torch.from_numpy(env.values("degree", buffer.gam)))
        env.policy_step_device(w["prepared"], w["hidden"], u_all[t], act, logp, rew, done, rows, obs, R, 2, stream.cuda_stream)
        buffer.actions[t].copy_(act); buffer.logprobs[t].copy_(logp); buffer.rewards[t].copy_(rew); buffer.dones[t].copy_(done)
        buffer.t += 1
    env.sync()


def one_run(mode, ring, policy):
    env = make_env(ring if mode == "device" else 0)
    gen = torch.Generator(device=dev); gen.manual_seed(7)
    buffer = None
    for timed in (False, True):                                  # a full warm-up rollout, then the timed one
        buffer = DeviceTrajectoryBuffer(T, B)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "sync":
            rollout_sync(env, policy, buffer, gen)
        else:
            run_rollout(env, policy, T, buffer, obs_rows=R, generator=gen, value_strategy="degree")
        env.sync()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return T * B / dt, dt, buffer


def timed_ms(fn, repeats=3):
    best = float("inf")
    for _ in range(repeats + 1):                                 # (the first call warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


torch.manual_seed(1)
policy = PMLPPolicy(2 * int(a.dist.split("-")[0]) * 2, (a.hidden,)).to(dev)   # (cols = 2 nvars k)
configs = []
if a.mode in ("both", "sync"):
    configs.append(("sync", 0))
if a.mode in ("both", "device"):
    configs.append(("device", a.ring))
    configs += [("device", int(r)) for r in a.rings.split(",") if r]
runs, last = {}, None
for pair in range(a.pairs):
    for mode, ring in configs:
        rate, dt, buf = one_run(mode, ring, policy)
        key = mode if mode == "sync" else "device_ring%s" % (ring or "default")
        runs.setdefault(key, []).append(rate)
        last = buf
        print(json.dumps({"mode": mode, "ring": ring or "default", "pair": pair, "env_steps_per_s": rate, "rollout_ms": dt * 1e3,
                          "dist": a.dist, "batch": B, "steps": T}), flush=True)
fin = {}
if hasattr(last, "_finish_torch"):
    fin = {"finish_torch_ms": timed_ms(last._finish_torch), "finish_kernel_ms": timed_ms(last.finish)}
else:
    fin = {"finish_torch_ms": timed_ms(last.finish)}
print(json.dumps(dict(fin, steps=T, batch=B)), flush=True)
summary = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v), "spread": max(v) - min(v)} for k, v in runs.items()}
print(json.dumps({"summary": summary}))
