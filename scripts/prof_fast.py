"""Diagnostic (BBX_PROF_BUILD library only, BBX_PROF=1): per-phase cycle shares of the fast class's step loop at the
benchmark's shape (one kernel per launch, the random agent, the observation after every step), with the reset split into
drawing the ideal and installing it.
usage: BBX_PROF=1 prof_fast.py [DIST [BATCH [STEPS...]]]      (defaults: 3-20-10-weighted 4096 1024 20)"""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from deepgroebner_amd import VecLeadMonomialsEnv, _ffi
dist = sys.argv[1] if len(sys.argv) > 1 else "3-20-10-weighted"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
steps = [int(a) for a in sys.argv[3:]] or [1024, 20]
if not os.environ.get("BBX_PROF"):
    raise SystemExit("set BBX_PROF=1 (and use a library built with BBX_PROF_BUILD)")
lib = _ffi.lib()
if not hasattr(lib, "bbx_fast_prof_read"):
    raise SystemExit("libbbx.so was not built with BBX_PROF_BUILD")
names = {0: "loop top", 6: "reset: draw", 7: "reset: install", 1: "agent + pair removal", 2: "S-polynomial", 3: "reduce",
         4: "add_poly (pair update, insert)", 5: "observation + bookkeeping"}
for T in steps:
    env = VecLeadMonomialsEnv(dist, batch=B, k=2)
    env.seed(np.arange(B) + 1000); env.seed_agent(np.arange(B)); env.reset()
    acc = (C.c_ulonglong * 8)()
    obs = torch.empty((B, 512, env.cols), dtype=torch.int32, device="cuda")
    rew = torch.zeros(B, dtype=torch.float64, device="cuda"); done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(B, dtype=torch.int32, device="cuda")
    env.rollout_device("random", T, True, torch.cuda.current_stream().cuda_stream, rew, done, rows, obs, 512, False, True); env.sync()   # (warm-up)
    lib.bbx_fast_prof_read(acc, 1)
    t0 = time.perf_counter()
    env.rollout_device("random", T, True, torch.cuda.current_stream().cuda_stream, rew, done, rows, obs, 512, False, True); env.sync()
    dt = time.perf_counter() - t0
    lib.bbx_fast_prof_read(acc, 1)
    a = np.array(list(acc), dtype=np.float64)
    tot = a.sum()
    print("%s B=%d K=%d: %.4f s (stamped kernel) = %.1f M env-steps/s; %.0f ticks per env-step" % (dist, B, T, dt, B * T / dt / 1e6, tot / B / T))
    for i, n in names.items():
        print("  %-32s %6.2f %%  %8.1f ticks/env-step" % (n, 100 * a[i] / tot, a[i] / B / T))
    print("  %-32s %6.2f %%" % ("loop top + reset (slots 0 + 6 + 7)", 100 * (a[0] + a[6] + a[7]) / tot))
