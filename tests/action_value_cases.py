"""References for bbx_action_values (tests/test_action_values_cpu.py, tests/test_action_values_gpu.py); importable without
a GPU.

The definition, for environment e with n_e pairs and a < n_e:

    c = copy of environment e;  (r, done) = c.step(a)          # no auto-reset
    Q[e][a] = r + gamma * c.value(strategy, gamma)              # value of a finished environment is 0.0

with the product and the sum rounded one after the other in float64 — numpy's `r + gamma * v` on float64 arrays, Python's
on floats.  Three restatements of it: on the library's own copy / step / values (the twin: calls the suite already holds to
the oracle), on the CPU oracle's Env (independent of the library), and a numpy model of the pass plan."""
import ctypes as C

import numpy as np


def call(env, strategy="degree", gamma=0.99, max_rows=None, rewards=True, dones=True):
    """bbx_action_values through the C ABI -> (rc, q, rewards, dones, rows); the blocks start out as garbage the call must
    overwrite (-7.0 / -7.0 / 9)."""
    from deepgroebner_amd import _ffi
    R = max(1, int(env.rows.max())) if max_rows is None else int(max_rows)
    q = np.full((env.batch, max(R, 1)), -7.0, dtype=np.float64)
    r = np.full((env.batch, max(R, 1)), -7.0, dtype=np.float64) if rewards else None
    d = np.full((env.batch, max(R, 1)), 9, dtype=np.uint8) if dones else None
    rows = np.full(env.batch, -3, dtype=np.int32)
    rc = _ffi.lib().bbx_action_values(env._h, strategy.encode(), float(gamma), R, _ffi.ptr(q), _ffi.ptr(r), _ffi.ptr(d), _ffi.ptr(rows))
    return rc, q, r, d, rows


def twin_action_values(env, strategy, gamma, R):
    """The loop the call replaces, on a VecLeadMonomialsEnv whose `rows` are current: per action index a copy of the whole
    batch, one step without auto-reset (environments with fewer pairs repeat their last action, finished ones take action 0
    and stay finished; both are masked out), one values() -> (q, rewards, dones, rows): [B, R] float64 / float64 / uint8 with
    NaN / NaN / 0 where a >= rows[e], and the full pair counts."""
    B = env.batch
    rows = env.rows.astype(np.int32).copy()
    q = np.full((B, R), np.nan); rew = np.full((B, R), np.nan); done = np.zeros((B, R), dtype=np.uint8)
    for a in range(min(R, int(rows.max()) if B else 0)):
        t = env.copy()
        _, r, d, _ = t.step(np.maximum(np.minimum(a, rows - 1), 0).astype(np.int32), auto_reset=False)
        v = t.values(strategy, gamma)
        live = a < rows
        q[live, a] = (np.asarray(r, dtype=np.float64) + np.float64(gamma) * np.asarray(v, dtype=np.float64))[live]
        rew[live, a] = np.asarray(r, dtype=np.float64)[live]
        done[live, a] = np.asarray(d).astype(np.uint8)[live]
    return q, rew, done, rows


def oracle_action_values(o, strategy, gamma, limit=None):
    """The definition on one oracle environment (oracle.ffi.Env: copy, step, value) -> (q [n], rewards [n], dones [n]) for
    its first n = min(nP, limit) actions."""
    n = o.nP if limit is None else min(o.nP, int(limit))
    q = np.zeros(n); rew = np.zeros(n); done = np.zeros(n, dtype=np.uint8)
    for a in range(n):
        c = o.copy()
        r = float(c.step(a))
        v = float(c.value(strategy, gamma)) if c.nP > 0 else 0.0
        q[a] = np.float64(r) + np.float64(gamma) * np.float64(v)
        rew[a] = r; done[a] = 1 if c.nP == 0 else 0
    return q, rew, done


def same_block(got, want):
    """== on doubles where `want` holds a number, NaN exactly where `want` holds NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])


def plan_model(counts, chunk):
    """The pass plan: the flat list of sum(counts) positions cut into contiguous ranges of at most `chunk` -> first[npasses + 1]."""
    total = int(np.sum(np.asarray(counts, dtype=np.int64)))
    first = list(range(0, total, chunk))
    return np.asarray(first + [total], dtype=np.int32)


def plan(counts, chunk, cap=None):
    """bbx_action_values_plan -> (rc, first[:npasses + 1]); cap None: room to spare."""
    from deepgroebner_amd import _ffi
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    room = int(counts.sum()) // max(chunk, 1) + 8 if cap is None else cap
    first = np.full(max(room, 1), -1, dtype=np.int32)
    n = C.c_int32(-1)
    rc = _ffi.lib().bbx_action_values_plan(_ffi.ptr(counts), len(counts), int(chunk), _ffi.ptr(first), int(room), C.byref(n))
    return rc, (first[:n.value + 1].copy() if rc == 0 else None)
