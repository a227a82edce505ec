"""The fast class's step loop tests ONE value per step for everything rare (t_event in bbx_fast.h: the issued steps exhausted,
the 64-step housekeeping, a reset, a mailbox publication).  The situations in which that control can go wrong are events that
coincide: an episode that ends on the last step before a multiple of 64, or on the first after it, or on the last step a
launch issued.  tests/test_step_events_gpu.py runs the kernels on the seeds below; this file asserts, on the oracle alone,
that those seeds really produce the situations (found by a search over seeds 3000..3399, fixed here)."""
import functools

import numpy as np

from oracle import ffi
from oracle.trace import run_trace
from tests.oracle_walk import agent_seeds                    # (the twins import it from here)

K = 2
# consecutive launches: they begin and end at t % 64 of 0, 1, 63 and 64
SCHEDULE = (1, 62, 1, 1, 63, 64, 65, 2, 127)
ENDS = tuple(int(x) for x in np.cumsum(SCHEDULE))
TRACED_SEEDS = {"3-20-10-weighted": (3009, 3014, 3043, 3012, 3037, 3023, 3020, 3081),
                "3-2-10-uniform": (3002, 3003, 3006, 3009, 3011, 3020, 3014, 3010)}
# without auto-reset: (seeds, launch lengths); the first launch ends exactly with the first environment's episode
NO_RESET = {"3-20-10-weighted": ((3000, 3001, 3002, 3003, 3004, 3005, 3006, 3007), (51, 60)),
            "3-2-10-uniform": ((3002, 3003, 3000, 3001, 3004, 3005, 3006, 3007), (12, 10))}
# a register/LDS class capped at 16 basis elements (caps={"lds_max_basis": 16}): environments leave it mid-launch
LEAVE_SEEDS, LEAVE_LAUNCHES, LEAVE_CAP = (3000, 3001, 3002, 3003, 3004, 3005), (100, 100, 100), 16
MAILBOX_SEED, MAILBOX_STEPS = 77, 130


@functools.lru_cache(maxsize=None)
def traces(dist, seeds, T):
    """oracle.trace.run_trace of every seed under the hash agent with auto-reset, T steps."""
    bo = ffi.load("bo")
    out = []
    for s, a in zip(seeds, agent_seeds(seeds)):
        o = bo.env(dist)
        o.seed(s)
        out.append(run_trace(o, K, T, "hash", agent_seed=a))
    return out


@functools.lru_cache(maxsize=None)
def walks(dist, seeds, launches, auto_reset):
    """What every launch of `launches` steps leaves, per environment: a list (one entry per launch) of dicts with the steps the
    launch took, the last step's reward, the done flag, the row count and the observation the caller finds afterwards (the NEW
    episode's under auto-reset; without it a finished environment stops and keeps done = 1, no rows)."""
    bo = ffi.load("bo")
    out = []
    for s, a in zip(seeds, agent_seeds(seeds)):
        o = bo.env(dist)
        o.seed(s)
        o.reset()
        t, recs = 0, []
        for n in launches:
            taken, reward, done = 0, None, o.nP == 0
            for _ in range(n):
                if o.nP == 0:
                    break
                reward = o.step(ffi.agent_action(a, t, o.nP))
                t += 1
                taken += 1
                done = o.nP == 0
                if done and auto_reset:
                    o.reset()
            recs.append({"steps": taken, "reward": reward, "done": bool(done), "rows": o.nP, "obs": o.obs(K).copy(), "total": t})
        out.append(recs)
    return out


def episode_ends(tr):
    return [int(t) for t in np.flatnonzero(tr["done"])]


def test_schedule_meets_every_phase():
    begins = [0] + list(ENDS[:-1])
    assert {b % 64 for b in begins} >= {0, 1, 63} and {e % 64 for e in ENDS} >= {0, 1, 63}
    assert 64 in ENDS and 64 in begins and any(b % 64 and (b // 64 != (b + n) // 64) for b, n in zip(begins, SCHEDULE))


def test_traced_seeds_end_episodes_on_the_phase_and_on_the_last_issued_step():
    for dist, seeds in TRACED_SEEDS.items():
        assert 6 <= len(seeds) <= 64
        ends = [episode_ends(tr) for tr in traces(dist, seeds, ENDS[-1])]
        assert any(t % 64 == 63 for e in ends for t in e), dist       # the step that ends the episode also completes a block of 64
        assert any(t % 64 == 0 for e in ends for t in e), dist        # ... or is the first of one
        last = [(i, t) for i, e in enumerate(ends) for t in e if t + 1 in ENDS]
        assert last, dist                                             # a launch's last issued step ends an episode
        assert any((t + 1) % 64 == 0 for _, t in last), dist          # ... and all three at once
        for i, t in last:                                             # what the caller finds is the new episode's
            rec = walks(dist, seeds, SCHEDULE, True)[i][ENDS.index(t + 1)]
            assert rec["done"] and rec["rows"] > 0 and len(rec["obs"]) == rec["rows"]
        assert all(len(e) >= 2 for e in ends), dist


def test_walk_agrees_with_the_trace():
    for dist, seeds in TRACED_SEEDS.items():
        for tr, recs in zip(traces(dist, seeds, ENDS[-1]), walks(dist, seeds, SCHEDULE, True)):
            for end, rec in zip(ENDS, recs):
                assert rec["total"] == end and rec["reward"] == tr["reward"][end - 1] and rec["done"] == bool(tr["done"][end - 1])
                if not rec["done"]:
                    assert rec["rows"] == tr["nP"][end - 1]


def test_no_reset_seeds_finish_inside_at_and_after_the_first_launch():
    for dist, (seeds, launches) in NO_RESET.items():
        recs = walks(dist, seeds, launches, False)
        first = [r[0] for r in recs]
        assert first[0]["steps"] == launches[0] and first[0]["done"] and first[0]["rows"] == 0     # ends with its last issued step
        assert sum(r["done"] and r["steps"] < launches[0] for r in first) >= 2                       # finished with steps still issued
        assert sum(not r["done"] for r in first) >= 2                                                # still running
        second = [r[1] for r in recs]
        assert all(r["done"] for r in second)
        assert all(b["steps"] == 0 for a, b in zip(first, second) if a["done"])                      # the finished take no further steps
        assert any(0 < b["steps"] < launches[1] for b in second)


def test_leave_seeds_outgrow_the_capped_class_and_come_back():
    T = sum(LEAVE_LAUNCHES)
    for tr in traces("3-20-10-weighted", LEAVE_SEEDS, T):
        nG, ends = tr["nG"], episode_ends(tr)
        over = np.flatnonzero(nG > LEAVE_CAP)
        assert len(over) and len(ends) >= 2
        assert any(t > over[0] for t in ends)                         # an episode that left the class ends inside the run
        assert any(nG[t + 1] <= LEAVE_CAP for t in ends if t + 1 < T)  # ... and the next one starts inside it again
    begins = np.cumsum((0,) + LEAVE_LAUNCHES[:-1])
    assert any(tr["nG"][b - 1] > LEAVE_CAP for tr in traces("3-20-10-weighted", LEAVE_SEEDS, T) for b in begins[1:])   # a launch begins outside


def test_mailbox_seed_ends_episodes_inside_the_session():
    bo = ffi.load("bo")
    o = bo.env("3-20-10-weighted")
    o.seed(MAILBOX_SEED)
    o.reset()
    ends = []
    for t in range(MAILBOX_STEPS):
        o.step(ffi.agent_hash(1, t) % o.nP)
        if o.nP == 0:
            ends.append(t)
            o.reset()
    assert len([t for t in ends if t >= 5]) >= 2, ends               # (the session begins with the fifth step in a row)
