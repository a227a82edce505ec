"""Experiment: the wave timeline of the step kernel.  Every wave of the launch records where it ran (HW_ID, XCC_ID), when it
entered and when it had taken every step issued; the sixteen waves of four CUs also the time of every 64th step (100 MHz clock).
Normal launches or one persistent session.  Library built from scripts/patches/wave_timeline_debug.patch with -DBBX_DRIFT_DEBUG.
    [JOIN=1] [PREROLL=n] [KEY=steps|time:SHIFT] [OUT=file.npz] python scripts/exp_drift.py MODE TOTAL K
KEY says how the build under test keys its priority rotation (for the equal-priority share): on the wave's own steps,
((t >> 6) + quarter) & 3, or on time, bbx_prio_phase with that slot shift."""
import os, sys, time, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from deepgroebner_amd import VecLeadMonomialsEnv, _ffi
mode, total, K = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
key = os.environ.get("KEY", "steps")
B, R = 4096, 512
env = VecLeadMonomialsEnv("3-20-10-weighted", batch=B, k=2)
env.seed(np.arange(B) + 1000); env.seed_agent(np.arange(B)); env.reset(); env.accounting(False)
obs = torch.empty((B, R, env.cols), dtype=torch.int32, device="cuda")
rew = torch.zeros(B, dtype=torch.float64, device="cuda"); done = torch.zeros(B, dtype=torch.uint8, device="cuda"); rows = torch.zeros(B, dtype=torch.int32, device="cuda")
s = torch.cuda.current_stream()
env.persistent(True); env.persistent(mode == "persistent")          # (allocates the block the samples go to)
def launch(n):
    env.rollout_device("random", n, True, s.cuda_stream, rew, done, rows, obs, R, False, True)
pre = int(os.environ.get("PREROLL", "0"))
if pre:                                                    # the batch in its steady state, this launch shape warm (as bench.py does)
    launch(pre); env.sync(); launch(K); env.sync()
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
torch.cuda.synchronize()
t0 = time.perf_counter()
ev0.record(s)
for i in range(total // K):
    launch(K)
if os.environ.get("JOIN"):
    env.join(s.cuda_stream)
ev1.record(s)
t_issue = time.perf_counter() - t0
env.sync(); torch.cuda.synchronize(); dt = time.perf_counter() - t0
print("%s K=%d total %d steps: host %.1f us (issue %.1f us), %.3f us/step; events %.1f us" % (mode, K, total, dt * 1e6, t_issue * 1e6, dt / total * 1e6, ev0.elapsed_time(ev1) * 1e3), env.session_stats())
dll = C.CDLL(_ffi.LIB_PATH)
dll.bbx_session_debug.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
out = np.zeros(4 * 4096 + 64 * 512 // 2, dtype=np.uint64)
assert dll.bbx_session_debug(env._h, out.ctypes.data_as(C.c_void_p), len(out)) == 0
rec = out[:4 * 4096].reshape(4096, 4)
samples = out[4 * 4096:].view(np.uint32).reshape(64, 512).astype(np.int64)
if os.environ.get("OUT"):
    np.savez_compressed(os.environ["OUT"], rec=rec, samples=samples)
hw = (rec[:, 0] & np.uint64(0xffffffff)).astype(np.int64); xcc = (rec[:, 0] >> np.uint64(32)).astype(np.int64) & 15
slot, simd, cu, sh, se = hw & 15, (hw >> 4) & 3, (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7
cuid = ((xcc * 8 + se) * 2 + sh) * 16 + cu
simdid = cuid * 4 + simd
t_in, t_fin = rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64)
s0, s1 = (rec[:, 3] & np.uint64(0xffffffff)).astype(np.int64), (rec[:, 3] >> np.uint64(32)).astype(np.int64)
ok = t_fin > 0
print("waves with a finish record: %d of %d; steps taken by them: %s" % (ok.sum(), B, np.unique((s1 - s0)[ok])))
base = t_in.min()
launch_ticks = t_fin[ok].max() - base
q = np.arange(B) >> 10
fin = (t_fin - base) / 100.0                               # us
print("launch: first entry -> last finish %.1f us; entries spread over %.1f us" % (launch_ticks / 100.0, (t_in.max() - base) / 100.0))
print("spread = (last finish - median finish) / launch = %.2f %%   (last - 90th percentile: %.2f %%, median - first: %.2f %%)" % (
    100 * (fin[ok].max() - np.median(fin[ok])) / (launch_ticks / 100.0), 100 * (fin[ok].max() - np.percentile(fin[ok], 90)) / (launch_ticks / 100.0),
    100 * (np.median(fin[ok]) - fin[ok].min()) / (launch_ticks / 100.0)))
for k in range(4):
    m = ok & (q == k)
    print("quarter %d: finish min / median / max %.1f / %.1f / %.1f us; entry median %.1f us" % (k, fin[m].min(), np.median(fin[m]), fin[m].max(), np.median((t_in[m] - base) / 100.0)))
# which quarters share a SIMD, and the finish by age rank (order of entry) among a SIMD's waves
sets, by_rank, n_cu = {}, [[] for _ in range(8)], len(np.unique(cuid))
for sid in np.unique(simdid):
    w = np.flatnonzero(simdid == sid)
    sets[tuple(sorted(q[w]))] = sets.get(tuple(sorted(q[w])), 0) + 1
    for r, e in enumerate(w[np.argsort(t_in[w], kind="stable")]):
        if ok[e] and r < 8:
            by_rank[r].append(fin[e])
print("distinct CUs %d, SIMDs %d; quarters on one SIMD (multiset: count): %s" % (n_cu, len(np.unique(simdid)), dict(sorted(sets.items(), key=lambda kv: -kv[1])[:6])))
print("finish by age rank on the SIMD (median us): " + " ".join("%d: %.1f" % (r, np.median(v)) for r, v in enumerate(by_rank) if v))
# the sampled waves: share of the launch during which two waves of a SIMD hold the same priority
wave_env = np.array([(w >> 4) * 1024 + (((w >> 2) & 3)) * 4 + (w & 3) for w in range(64)])
shift = int(key.split(":")[1]) if key.startswith("time") else None
looks_of = []                                            # per sampled wave: (times of its looks, priority from each look on)
for w in range(64):
    e = wave_env[w]
    idx = np.array([i for i in range((s0[e] >> 6) + 1, (s1[e] >> 6) + 1) if samples[w, i & 511]], dtype=np.int64)
    tk = samples[w, idx & 511] if len(idx) else np.zeros(0, dtype=np.int64)
    looks_of.append((tk, ((idx if shift is None else (tk >> shift)) + (e >> 10)) & 3))
def prio_at(w, t):                                       # priority of sampled wave w at tick t (low 32 bits), from its own looks
    tk, pr = looks_of[w]
    i = int(np.searchsorted(tk, t, side="right")) - 1
    return int(pr[i]) if i >= 0 else None                   # None: before the wave's first look (the priority the wave started with: 0)
groups = {}
for w in range(64):
    groups.setdefault(simdid[wave_env[w]], []).append(w)
same = tot = 0
lo, hi = int(t_in[wave_env].max() & 0xffffffff), int(t_fin[wave_env][ok[wave_env]].min() & 0xffffffff)
for t in np.linspace(lo, hi, 400).astype(np.int64):
    for g in groups.values():
        pr = [prio_at(w, t) for w in g]
        pr = [0 if p is None else p for p in pr]
        tot += 1; same += len(set(pr)) < len(pr)
print("sampled waves: %d SIMDs with %s waves each; share of (SIMD, time) samples with two waves at equal priority: %.1f %% (key %s)" % (
    len(groups), sorted(set(len(g) for g in groups.values())), 100.0 * same / max(tot, 1), key))
for w in (0, 16, 32, 48):
    e = wave_env[w]
    looks = np.array([samples[w, i & 511] for i in range((s0[e] >> 6) + 1, (s1[e] >> 6) + 1)])
    if len(looks) > 1:
        print("env %4d (SIMD %d): us per step between looks: median %.3f, min %.3f, max %.3f" % (e, simdid[e], np.median(np.diff(looks)) / 6400.0, np.diff(looks).min() / 6400.0, np.diff(looks).max() / 6400.0))
