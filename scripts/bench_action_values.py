"""Action values per second of VecLeadMonomialsEnv.action_values('degree') (bbx_action_values: one clone per (environment,
pair), a forced first step, the strategy's rollouts) next to the Python loop it replaces — per action index up to the
tallest pair set: copy() of the whole batch, one step() without auto-reset, values() — on the same states, in one session.
Each figure is the median of five with min and max; the two blocks are compared with == before anything is timed.
    python scripts/bench_action_values.py [--dists 3-20-10-weighted 5-10-5-uniform] [--batch 4096] [--steps 5]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from deepgroebner_amd import VecLeadMonomialsEnv

ap = argparse.ArgumentParser()
ap.add_argument("--dists", nargs="+", default=["3-20-10-weighted", "5-10-5-uniform"])
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--steps", type=int, default=5, help="random-agent steps before the states are valued")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--gamma", type=float, default=0.99)
a = ap.parse_args()
B = a.batch


def loop(env, strategy, gamma, R):
    """What a caller had to write before the call existed."""
    rows = env.rows
    q = np.full((B, R), np.nan)
    for act in range(R):
        t = env.copy()
        _, r, _, _ = t.step(np.maximum(np.minimum(act, rows - 1), 0).astype(np.int32), auto_reset=False)
        v = t.values(strategy, gamma)
        live = act < rows
        q[live, act] = (r + gamma * v)[live]
    return q


def timed(f):
    ts = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


for dist in a.dists:
    env = VecLeadMonomialsEnv(dist, batch=B, k=2)
    env.seed(np.arange(B) + 1000); env.seed_agent(np.arange(B)); env.reset()
    env.rollout("random", a.steps, auto_reset=True)
    R, total = int(env.rows.max()), int(env.rows.sum())
    got = env.action_values("degree", a.gamma)                      # warm-up of both (allocations, code objects) and the check
    want = loop(env, "degree", a.gamma, R)
    assert np.array_equal(got, want, equal_nan=True), dist
    call = timed(lambda: env.action_values("degree", a.gamma))
    py = timed(lambda: loop(env, "degree", a.gamma, R))
    chunk = env.action_values_chunk(0)
    out = {"dist": dist, "batch": B, "walked": a.steps, "action_values": total, "tallest_pair_set": R, "chunk": chunk,
           "passes": -(-total // chunk)}
    for name, (med, lo, hi) in (("call", call), ("loop", py)):
        out[name] = {"values_per_s": total / med, "ms": med * 1e3, "ms_min": lo * 1e3, "ms_max": hi * 1e3}
    out["loop_over_call"] = py[0] / call[0]
    print(json.dumps(out))
