"""What bootstrapping the buffer's tail (run_rollout_fused(..., critic=..., bootstrap=True), bbx_gae_bootstrap_device) changes and
what it costs; one JSON line per case.

    python scripts/bench_bootstrap.py [--case all|DIST:B:T[:ROWS] ...] [--hidden 128]

Cases (default): 3-20-10-weighted with B = 4096 and T in {64, 128, 256}; 5-10-5-uniform with B = 1024 and T = 256.  A PMLP(--hidden)
policy and a PMLP(--hidden) critic, both untrained from a fixed seed; k = 2; blocks of --obs-rows 256 rows (5-10-5-uniform: 2048,
the most the policy kernels score — its pair sets pass 256 rows within the first 256 steps).  A pair set that outgrows the block
is BBX_E_CAPACITY: behind the windows it ends the following (`followed`, `follow_stopped_by`), inside them the case prints
`not_measured` with the library's message.

Per case, on one batch of environments seeded 1000 .. 1000 + B - 1:
  rollout 1   T steps from reset() with bootstrap=True          window "from_reset"
  rollout 2   T more steps into the same buffer                  window "continued"
  then --follow more steps without states, so that the episodes the windows cut are followed to their ends.
For each window (COUNTS: deterministic for fixed seeds):
  share_used        steps get_index() returns / (T B), with the bootstrap and — the same buffer with last_values = None — without
  share_complete    steps finish() marks complete / (T B) without the bootstrap (with it: 1)
  mean_episode_length   over the steps used, the length of the episode each belongs to (its first step to its done flag, both known:
                    everything is recorded from reset(); an episode still running after --follow steps counts with the steps seen,
                    and `censored_steps` says how many used steps that concerns), with and without the bootstrap
Timings (device events or the host clock around work that ends in a synchronise; five alternating repeats, median [min, max]):
  finish_ms   on the window-2 buffer, per call over --calls 20 calls back to back: bbx_gae_device; bbx_gae_bootstrap_device with both
              optional pointers NULL (the same kernel: must lie inside the old entry's own spread); with last values and lambda-returns;
              the order of the three rotates from repeat to repeat
  rollout_ms  one run_rollout_fused call of T steps with bootstrap=True against the same call without it, on two copies of the
              environments in the same state with the same draws (env.copy()), the order alternating; beside it the bootstrap's own
              part timed alone (the zero-step launch, its wait, one critic launch over [B] states)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from deepgroebner_amd import _ffi
from deepgroebner_amd import rollout as ro
from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, PMLPValue, run_rollout_fused

DEFAULT = ["3-20-10-weighted:4096:64", "3-20-10-weighted:4096:128", "3-20-10-weighted:4096:256", "5-10-5-uniform:1024:256:2048"]
ap = argparse.ArgumentParser()
ap.add_argument("--case", nargs="+", default=["all"], help="DIST:B:T or DIST:B:T:ROWS, or all")
ap.add_argument("--hidden", type=int, default=128)
ap.add_argument("--obs-rows", type=int, default=256)
ap.add_argument("--follow", type=int, default=4096, help="steps the environments are followed behind the windows")
ap.add_argument("--repeats", type=int, default=5, help="alternating repeats per timing (at least 5)")
ap.add_argument("--calls", type=int, default=20, help="finish: calls per repeat")
a = ap.parse_args()
if a.repeats < 5:
    ap.error("--repeats must be at least 5")
if not torch.cuda.is_available():
    sys.exit("bench_bootstrap: no GPU (there is no CPU fall-back for a measurement)")
dev = torch.device("cuda", torch.cuda.current_device())
name = torch.cuda.get_device_name(0)


def note(*what):
    print(*what, file=sys.stderr, flush=True)


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def gen(seed):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    return g


def episode_spans(dones):
    """dones bool [N, B] from reset() on -> (first step, last step or -1 where the episode is still running at N) per entry."""
    N, B = dones.shape
    t = np.arange(N)[:, None]
    end = np.minimum.accumulate(np.where(dones, t, N)[::-1], axis=0)[::-1]
    prev = np.maximum.accumulate(np.where(dones, t, -1), axis=0)          # the last done flag at or before t
    start = np.vstack([np.zeros((1, B), dtype=prev.dtype), prev[:-1] + 1])
    return start, np.where(end < N, end, -1)


def used_mask(buf, T, B):
    m = np.zeros(T * B, dtype=bool)
    m[buf.get_index(None)[0].cpu().numpy()] = True
    return m.reshape(T, B)


def window_counts(buf, T, B):
    """The masks of one window: used with the bootstrap, used and complete without it (the same buffer, last_values = None)."""
    last = buf.last_values
    assert last is not None
    boot = used_mask(buf, T, B)
    assert bool(buf.complete.all())
    ro._set_last_values(buf, None)
    plain = used_mask(buf, T, B)
    comp = buf.complete.cpu().numpy().astype(bool)
    ro._set_last_values(buf, last)
    return {"boot": boot, "plain": plain, "complete": comp, "rows_gt_1": (buf.rows[:T] != 1).cpu().numpy()}


def window_report(masks, length, censored, T, B):
    out = {"steps": T * B, "share_complete_plain": float(masks["complete"].mean()), "share_more_than_one_row": float(masks["rows_gt_1"].mean())}
    for key in ("boot", "plain"):
        m = masks[key]
        out["used_" + key] = int(m.sum())
        out["share_used_" + key] = float(m.mean())
        out["mean_episode_length_" + key] = float(length[m].mean()) if m.any() else None
        out["censored_steps_" + key] = int(censored[m].sum())
    return out


def time_finish(buf, T, B):
    """Per-call times of the three ways through the GAE kernel on the same buffer, alternating."""
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    r, v, d = buf.rewards[:T], buf.values[:T], buf.dones[:T]
    ret = torch.empty_like(r); adv = torch.empty_like(r); lret = torch.empty_like(r); comp = torch.empty_like(d)
    last = buf.last_values
    dll = _ffi.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g, l = float(buf.gam), float(buf.lam)
    ways = {"gae_device": lambda: dll.bbx_gae_device(p(r), p(v), p(d), T, B, g, l, p(ret), p(adv), p(comp), s),
            "bootstrap_null_null": lambda: dll.bbx_gae_bootstrap_device(p(r), p(v), p(d), T, B, g, l, None, p(ret), p(adv), p(comp), None, s),
            "bootstrap_last_lambda": lambda: dll.bbx_gae_bootstrap_device(p(r), p(v), p(d), T, B, g, l, p(last), p(ret), p(adv), p(comp), p(lret), s)}
    times = {k: [] for k in ways}
    for k, fn in ways.items():
        for _ in range(a.calls):
            _ffi.check(fn())
    torch.cuda.synchronize()
    names = list(ways)
    for rep in range(a.repeats):
        for k in names[rep % 3:] + names[:rep % 3]:            # (each way follows each other way in turn)
            fn = ways[k]
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record(); e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.calls)
    out = {k: spread(v) for k, v in times.items()}
    old = out["gae_device"]
    out["null_null_inside_old_spread"] = old["min_ms"] <= out["bootstrap_null_null"]["median_ms"] <= old["max_ms"]
    out["last_lambda_over_old"] = out["bootstrap_last_lambda"]["median_ms"] / old["median_ms"]
    out["calls_per_repeat"] = a.calls
    return out


def time_rollout(env, policy, critic, buf, T, R):
    """One fused rollout call with and without the bootstrap from the same state with the same draws; the bootstrap's part alone."""
    times = {"bootstrap": [], "plain": []}
    stream = torch.cuda.current_stream()
    for rep in range(a.repeats + 1):                          # (the first pair warms up)
        order = ("bootstrap", "plain") if rep % 2 else ("plain", "bootstrap")
        twin = env.copy()
        for key in order:
            e = env if key == "bootstrap" else twin
            buf.t = 0
            g = gen(100 + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_rollout_fused(e, policy, T, buf, generator=g, critic=critic, bootstrap=key == "bootstrap")
            e.sync()
            torch.cuda.synchronize()
            if rep:
                times[key].append((time.perf_counter() - t0) * 1e3)
        del twin
    alone = []
    for rep in range(a.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ro._critic_last_values(env, critic, R, stream)
        torch.cuda.synchronize()
        if rep:
            alone.append((time.perf_counter() - t0) * 1e3)
    out = {k: spread(v) for k, v in times.items()}
    out["bootstrap_minus_plain_median_ms"] = out["bootstrap"]["median_ms"] - out["plain"]["median_ms"]
    out["bootstrap_part_alone"] = spread(alone)
    return out


def run_case(dist, B, T, R):
    from deepgroebner_amd import VecLeadMonomialsEnv
    cols = 2 * int(dist.split("-")[0]) * 2                      # (cols = 2 nvars k)
    torch.manual_seed(1)
    policy = PMLPPolicy(cols, (a.hidden,)).to(dev)
    critic = PMLPValue(cols, (a.hidden,)).to(dev)
    env = VecLeadMonomialsEnv(dist, batch=B, k=2)
    env.seed(np.arange(B) + 1000); env.seed_agent(np.arange(B)); env.reset()
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(R, cols))
    dones, masks = [], []
    for w in range(2):
        buf.t = 0
        run_rollout_fused(env, policy, T, buf, generator=gen(7 + w), critic=critic, bootstrap=True)
        dones.append(buf.dones[:T].cpu().numpy().astype(bool))
        masks.append(window_counts(buf, T, B))
        note(dist, B, T, "window", w, "recorded")
    finish = time_finish(buf, T, B)
    note(dist, B, T, "finish timed")
    twin = env.copy()                                          # the windows' environments, followed to the ends of their episodes
    follow = DeviceTrajectoryBuffer(a.follow, B)
    stopped = None
    g = gen(9)
    while follow.t < a.follow:                                 # (in chunks: a pair set that outgrows the block ends the following, not the case)
        before = follow.t
        try:
            run_rollout_fused(twin, policy, min(256, a.follow - before), follow, obs_rows=R, generator=g)
        except _ffi.BbxError as ex:
            stopped = str(ex)
            follow.t = before                                  # (the chunk that failed is not used)
            break
    dones.append(follow.dones[:follow.t].cpu().numpy().astype(bool))
    followed = follow.t
    del twin, follow
    note(dist, B, T, "followed", followed, stopped or "")
    every = np.concatenate(dones)
    start, end = episode_spans(every)
    censored = end < 0
    length = np.where(censored, every.shape[0], end + 1) - start
    out = {"bench": "bootstrap", "device": name, "dist": dist, "batch": B, "steps": T, "obs_rows": R, "hidden": a.hidden, "followed": followed,
           "follow_stopped_by": stopped, "episodes_finished_in_windows": int(every[:2 * T].sum()),
           "from_reset": window_report(masks[0], length[:T], censored[:T], T, B),
           "continued": window_report(masks[1], length[T:2 * T], censored[T:2 * T], T, B),
           "finish": finish}
    try:
        out["rollout"] = time_rollout(env, policy, critic, buf, T, R)
    except _ffi.BbxError as ex:
        out["rollout"] = {"not_measured": str(ex)}
    print(json.dumps(out), flush=True)
    del buf, env
    torch.cuda.empty_cache()


cases = DEFAULT if a.case == ["all"] else a.case
for c in cases:
    dist, B, T, R = (c.split(":") + [a.obs_rows])[:4]
    try:
        run_case(dist, int(B), int(T), int(R))
    except _ffi.BbxError as ex:                                # (a case that cannot be measured says so)
        print(json.dumps({"bench": "bootstrap", "device": name, "dist": dist, "batch": int(B), "steps": int(T), "obs_rows": int(R), "not_measured": str(ex)}),
              flush=True)
        torch.cuda.empty_cache()
