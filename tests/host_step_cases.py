"""TEST INFRASTRUCTURE — the cases of the host-stepped interface above 64 environments (bbx_step_obs, bbx_reset with a mask,
bbx_obs on the device-buffer side of bbx_create's `zero_copy = batch <= 64`) and their mirror on the oracle.  Plain module, no
fixtures: tests/test_host_step_cases_cpu.py runs every case through the oracle alone and asserts what makes it mean something
(episodes that end, neighbours with different row counts, the steps at which the observation block has to be enlarged),
tests/test_host_step_large_gpu.py runs the same cases on the device and compares every output of every call.

A case is: distribution, batch, k, first seed (environment e is seeded seed0 + e), step count, auto-reset, and — for all but the
recorded trajectory of GROW_BOTH — the action rule (5 * t + e) % rows."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "dist batch k seed0 steps auto_reset elimination rewards")


def case(dist, batch, k, steps, auto_reset, seed0=70, elimination="gebauermoeller", rewards="additions"):
    return Case(dist, batch, k, seed0, steps, auto_reset, elimination, rewards)


# bbx_obs_offsets_kernel: one workgroup of 1024 threads, thread t owns the per = ceil(B / 1024) environments from t * per on
SCAN_THREADS = 1024
# rows per environment of the padded observation block of a new handle (bbx_step_obs); enlarged by doubling
BLOCK_ROWS = 128

# Steps and ragged observations across the partition boundaries of the offsets kernel: 65 is the smallest batch on the
# device-buffer side, at 1024 every scan thread owns one environment, at 1025 two (the last thread that has any owns one,
# half the threads none), at 2050 three (the last one owns one of three).  One of them with k = 1: another column count.
SCAN = {
    "B65": case("3-20-10-weighted", 65, 2, 80, True),
    "B65_k1": case("3-20-10-weighted", 65, 1, 80, True),
    "B1024": case("3-20-10-weighted", 1024, 2, 40, True),
    "B1025": case("3-20-10-weighted", 1025, 2, 40, True),
    "B2050": case("3-20-10-weighted", 2050, 2, 32, True),
}
SCAN_LEAN = ("B65", "B1025")          # these also with accounting off: the lean kernel variants
# The wide class (a fixed ideal, one workgroup per environment) with more workgroups than compute units: its launches are two
# kernels (BbxParams::wide_tail).  Every environment starts from the same ideal; the action rule makes them diverge.
WIDE = case("cyclic-6", 300, 1, 16, True)
# bbx_step / bbx_step_autoreset (no observation in the call) with bbx_obs in between
PLAIN = {"B65": case("3-20-10-weighted", 65, 2, 70, False), "B1025": case("3-20-10-weighted", 1025, 2, 30, True)}
PLAIN_OBS_EVERY = 5
# The register/LDS class with a working copy of 16 basis elements: environments that outgrow it are handed to the HBM-resident
# pass inside the host step (BBX_ST_SPILL, finish()), which then writes their outputs and observation rows; with and without
# auto-reset (finished environments with a basis beyond the class next to live ones)
SPILL = {"auto": case("3-8-6-uniform", 65, 2, 60, True), "finish": case("3-8-6-uniform", 65, 2, 60, False)}
SPILL_CAPS = {"lds_max_basis": 16}
# No auto-reset: environments finish one by one (empty slices between live neighbours) until the whole block is empty
FINISH = case("3-20-10-weighted", 65, 2, 200, False)
FINISH_ALL_DONE_AT = 136              # the step (0-based) after which the total row count is 0
FINISH_RESET_EVERY = 12               # every so many steps: reset(mask) of every other finished environment
FINISH_WITH_RESETS = (21, 184)          # (environments reset that way, steps until the block is empty) of the GPU test's run
# Growth inside a step call: ONE environment passes 128 rows, later 256, while all others stay small
GROW_STEP = case("5-10-5-uniform", 66, 2, 120, True)
GROW_STEP_AT = {128: 41, 256: 102}    # threshold -> the step (0-based) whose result first exceeds it
# Growth inside reset(): every environment starts with more rows than the first block holds
GROW_RESET = case("3-20-140-weighted", 66, 2, 6, True)
# bbx_obs and bbx_step_obs sharing the device block: pair sets go from 19 to above 50
SHARED = {"B65": case("3-20-10-weighted", 65, 2, 48, True), "B1025": case("3-20-10-weighted", 1025, 2, 30, True)}
# Records and observation block enlarged in the same call: the trajectory of
# test_step_with_observation_when_the_records_and_the_observation_block_grow_in_the_same_call in environments 0..4 (same seeds,
# same action stream, same masked resets); environments 5..64 take row 0 and are never reset
GROW_BOTH = case("5-3-3-0.5-uniform", 65, 2, 27, False, seed0=867467, elimination="lcm")
GROW_BOTH_RECORDED = 5
MAX_POLY_TERMS = 4096                 # starting max_poly_terms of the general class (create_common)
# Errors and copies
ERROR = case("3-20-10-weighted", 65, 2, 12, True)
COPY = case("3-20-140-weighted", 66, 2, 8, True)


def per_thread(batch):
    return (batch + SCAN_THREADS - 1) // SCAN_THREADS


class OracleBatch:
    """One oracle environment per environment of the batch, stepped the way the device steps a batch: a finished environment
    that is stepped without auto-reset stays as it is and reports (0.0, done, 0 rows)."""

    def __init__(self, bo, c, oracles=None):
        self.c, self.B = c, c.batch
        self.episodes = 0
        if oracles is not None:
            self.o = oracles
            return
        self.o = []
        for e in range(self.B):
            o = bo.env(c.dist, elimination=c.elimination, rewards=c.rewards)
            o.seed(c.seed0 + e)
            o.reset()
            self.o.append(o)

    def copy(self):
        return OracleBatch(None, self.c, [o.copy() for o in self.o])

    def rows(self):
        return np.array([o.nP for o in self.o], dtype=np.int32)

    def offsets(self):
        return np.concatenate([[0], np.cumsum(self.rows())]).astype(np.int32)

    def actions(self, t):
        return np.array([(5 * t + e) % max(o.nP, 1) for e, o in enumerate(self.o)], dtype=np.int32)

    def step(self, actions, auto_reset=None, skip=()):
        """-> (rewards float64 [B], dones bool [B]); with auto-reset a finished environment starts its next episode here.
        skip: environments that do not take the step (their action was refused)."""
        auto_reset = self.c.auto_reset if auto_reset is None else auto_reset
        rewards, dones = np.zeros(self.B, dtype=np.float64), np.ones(self.B, dtype=bool)
        for e, o in enumerate(self.o):
            if o.nP == 0 or e in skip:
                continue
            rewards[e] = o.step(int(actions[e]))
            dones[e] = o.nP == 0
            if dones[e]:
                self.episodes += 1
                if auto_reset:
                    o.reset()
        return rewards, dones

    def reset(self, mask=None):
        for e, o in enumerate(self.o):
            if mask is None or mask[e]:
                o.reset()

    def obs(self, e):
        return self.o[e].obs(self.c.k)


def finish_reset_mask(t, rows):
    """FINISH: at every FINISH_RESET_EVERY-th step, every other finished environment (none at the other steps)."""
    mask = np.zeros(len(rows), dtype=np.uint8)
    if t % FINISH_RESET_EVERY == FINISH_RESET_EVERY - 1 and t < 60:
        fin = np.flatnonzero(rows == 0)
        mask[fin[::2]] = 1
    return mask


def shared_capacities(rows):
    """SHARED: rows per environment of the device block before the run (observations(max_rows = rows.max() + 1) after the
    reset made it that small) and after each step (doubled until the tallest pair set fits); rows: [steps + 1, B]."""
    caps = [int(rows[0].max()) + 1]
    for r in rows[1:]:
        cap = caps[-1]
        while cap < int(r.max()):
            cap *= 2
        caps.append(cap)
    return caps


def shared_probe_rows(t, rows, cap):
    """SHARED: max_rows of the padded observation taken after step t (0: none) — below the block's capacity, no row cut."""
    return cap - 1 if t % 6 == 5 and int(rows.max()) < cap else 0


class GrowBothDriver:
    """Actions and masked resets of GROW_BOTH: environments 0..4 consume the random stream exactly as the recorded test does."""

    def __init__(self):
        self.rng = np.random.default_rng(GROW_BOTH.seed0)

    def actions(self, ob):
        acts = np.zeros(ob.B, dtype=np.int32)
        for e in range(GROW_BOTH_RECORDED):
            acts[e] = self.rng.integers(0, max(1, ob.o[e].nP))
        return acts

    def reset_mask(self, ob, live):
        mask = np.zeros(ob.B, dtype=np.uint8)
        for e in range(GROW_BOTH_RECORDED):
            if live[e] and ob.o[e].nP == 0 and self.rng.random() < 0.7:
                mask[e] = 1
        return mask
