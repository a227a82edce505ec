"""Shared cases of the episode step limit tests (bbx_episode_limit) and the limited walk they are compared with.

The oracle knows no limit: the cap on episode length lives in the reference's Python loop around env.step() (pg.py), and so it
does here — limited_walk() steps a `bo.env` with a step counter of its own and resets it where the rule of bbx_common.h
(bbx_episode_end / bbx_episode_counted, restated below in plain Python) says so, recording what oracle/trace.py's run_trace
records, with done = (end != 0).

A case: distribution, creation caps (the kernel class), seeds, limits, steps.  The seeds were found by a search over the
oracle and are pinned here; tests/test_episode_limit_cpu.py asserts that they show, within the case's steps: a cut; an ordinary
end; (fast, binomial) an ordinary end on exactly the limit-th step of an episode; and that the case's last limit is larger than
every episode."""
import functools

import numpy as np

from oracle import ffi
from oracle.trace import fnv64, poly_words
from tests.oracle_walk import agent_seeds

K = 2
# class -> dist, caps, seeds (one environment each), limits (the last: larger than every episode), steps per walk
# (unlimited first episodes under the hash agent — fast: seed 3033 takes 20 steps, 3052 22, 3015 23, 3013 24, the other four
# more than 48; general: 3027 takes 3, 3006 9, 3000 13, 3007 26; wide: 3009 takes 11, 3002 12, 3001 14, 3000 19.
# 5-10-5-uniform: of seeds 3000..3599 none ends an episode within 60 steps under the hash, first, last or Degree agent and
# the shortest under the hash agent is seed 3559's, 122 steps: the case's mid-size limit, and why it walks 150 steps, not a few
# dozen)
CASES = {
    "fast": {"dist": "3-20-10-weighted", "caps": None, "seeds": (3033, 3052, 3015, 3013, 3000, 3001, 3004, 3005), "limits": (1, 2, 20, 1000),
             "steps": 48},
    "binom_hbm": {"dist": "5-10-5-uniform", "caps": None, "seeds": (3559, 3000, 3001, 3002), "limits": (1, 2, 122, 100000), "steps": 150},
    "general": {"dist": "3-5-4-0.5-uniform", "caps": None, "seeds": (3000, 3006, 3027, 3007), "limits": (1, 2, 10, 100000), "steps": 36},
    "wide": {"dist": "cyclic-4", "caps": None, "seeds": (3000, 3001, 3002, 3009), "limits": (1, 2, 12, 100000), "steps": 30},
    # the same ideals on the general class: what the existing wide tests tell the classes apart by (the launch planner puts
    # fixed ideals into the wide class unless wide_waves = -1 says otherwise)
    "wide_off": {"dist": "cyclic-4", "caps": {"wide_waves": -1}, "seeds": (3000, 3001, 3002, 3009), "limits": (12,), "steps": 30},
}
EXACT_END = ("fast", "binom_hbm")           # cases that must show an ordinary end on exactly the limit-th step
PIECE = 7                                   # traced launches of 7 steps: launches begin inside episodes


def episode_end(nP, episode_steps, limit):
    """bbx_episode_end (bbx_common.h), restated."""
    if nP == 0:
        return 1
    return 2 if limit > 0 and episode_steps >= limit else 0


def episode_counted(end, episode_steps, limit, auto_reset):
    """bbx_episode_counted (bbx_common.h), restated."""
    return end == 1 or (end == 2 and (auto_reset or episode_steps == limit))


class Walk:
    """One environment on the oracle with the header's counters: step(action) -> (reward, end)."""

    def __init__(self, dist, seed, limit, auto_reset=True):
        self.o = ffi.load("bo").env(dist)
        self.o.seed(seed)
        self.o.reset()
        self.limit, self.auto_reset = limit, auto_reset
        self.episode_steps = self.episodes = self.truncations = self.t = 0

    def step(self, action):
        r = self.o.step(action)
        self.t += 1
        self.episode_steps += 1
        end = episode_end(self.o.nP, self.episode_steps, self.limit)
        if episode_counted(end, self.episode_steps, self.limit, self.auto_reset):
            self.episodes += 1
            self.truncations += int(end == 2)
        return r, end

    def after(self, end):
        """what follows a step: the reset the rule asks for"""
        if end and self.auto_reset:
            self.o.reset()
            self.episode_steps = 0


def limited_walk(dist, seed, agent_seed, limit, nsteps, actions=None):
    """run_trace's record of `nsteps` steps under auto-reset with the episode step limit `limit` (0: off): the hash agent, or the
    given actions.  Per step the state BEHIND the step (before the reset that may follow), done = end != 0 and `end` itself;
    `episode_len`: the lengths of the episodes that ended; the final state, observation and counters."""
    w = Walk(dist, seed, limit)
    o = w.o
    rec = {key: [] for key in ("action", "reward", "nP", "nG", "obs_hash", "pairs_hash", "newpoly_hash", "done", "end", "rows_before")}
    lens = []
    for t in range(nsteps):
        a = int(actions[t]) if actions is not None else ffi.agent_action(agent_seed, t, o.nP)
        nG0 = o.nG
        rec["rows_before"].append(o.nP)
        r, end = w.step(a)
        rec["action"].append(a); rec["reward"].append(r); rec["nP"].append(o.nP); rec["nG"].append(o.nG)
        rec["obs_hash"].append(fnv64(o.obs(K))); rec["pairs_hash"].append(fnv64(o.pairs()))
        rec["newpoly_hash"].append(fnv64(poly_words(*o.poly(o.nG - 1))) if o.nG > nG0 else 0)
        rec["done"].append(int(end != 0)); rec["end"].append(end)
        if end:
            lens.append(w.episode_steps)
        w.after(end)
    out = {"action": np.array(rec["action"], dtype=np.int32), "reward": np.array(rec["reward"], dtype=np.float64),
           "nP": np.array(rec["nP"], dtype=np.int32), "nG": np.array(rec["nG"], dtype=np.int32),
           "done": np.array(rec["done"], dtype=np.int8), "end": np.array(rec["end"], dtype=np.int8),
           "rows_before": np.array(rec["rows_before"], dtype=np.int32),
           "obs_hash": np.array(rec["obs_hash"], dtype=np.uint64), "pairs_hash": np.array(rec["pairs_hash"], dtype=np.uint64),
           "newpoly_hash": np.array(rec["newpoly_hash"], dtype=np.uint64), "episode_len": np.array(lens, dtype=np.int32)}
    out["final_pairs"] = o.pairs().astype(np.int32)
    out["final_order"] = o.reducer_order().astype(np.int32)
    words = [poly_words(*o.poly(i)) for i in range(o.nG)]
    out["final_basis"] = np.concatenate(words) if words else np.zeros(0, dtype=np.int32)
    out["final_obs"] = o.obs(K)
    out["episodes"], out["truncations"], out["episode_steps"] = w.episodes, w.truncations, w.episode_steps
    return out


@functools.lru_cache(maxsize=None)
def case_walks(name, limit, nsteps=None):
    """limited_walk of every seed of a case under the hash agent (computed once, shared; never modified)."""
    c = CASES[name]
    return [limited_walk(c["dist"], s, a, limit, nsteps or c["steps"]) for s, a in zip(c["seeds"], agent_seeds(c["seeds"]))]
