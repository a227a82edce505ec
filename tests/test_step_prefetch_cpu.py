"""The front of a fast-class step: the pair is chosen from the register copy of the first 64 pairs (or from the list beyond
it), and lead monomial, tail monomial and working word of both members are read in one go.  What the step finds there was
left by the step before — a reset's new pair list, the register copy shifted by a zero reduction, an element appended a moment
ago, a pair list that has just grown past the register copy, a new block of agent hashes at a multiple of 64 — or by the launch
before, and a kernel that fetches any of it ahead of time has to get every one of these right.
tests/test_step_prefetch_gpu.py runs the headline shape on the seeds below; this file asserts, on the oracle alone, that each
seed really shows its situation (found by `search()` over seeds 3000 .. 7095, 320 steps each, fixed here: a seed that stops
showing its case fails the test, it is never skipped)."""
import functools

import numpy as np

from tests import oracle_walk as ow
from tests.test_step_events_cpu import K, agent_seeds, walks

DIST = "3-20-10-weighted"
T = 320                                              # steps per environment in every case
# launches chained by the GPU test: 1, 2, 63, 64 and 65 steps begin and end on both sides of the 64-step hash block
LAUNCHES = (1, 2, 63, 64, 65, 125)
assert sum(LAUNCHES) == T
LEAVE_CAP = 16                                       # caps={"lds_max_basis": 16}: the capacity test in front of a step sends environments away
SEARCH_SEEDS = range(3000, 3000 + 4096)

# case -> seeds that show it (the GPU test runs the union as one batch)
CASE_SEEDS = {
    "reset_then_step": (3000, 3001, 3002),
    "zero_reduction_then_pair_behind_it": (3000, 3001, 3002),
    "insertion_then_pair_with_the_new_element": (3000, 3001, 3002),
    "beyond_64_pairs_and_back": (3167, 3295, 3428),
    "hash_blocks_64_and_128": (3000, 3001, 3002),
    "leaves_the_class_at_the_capacity_test": (3000, 3001, 3002),
}


@functools.lru_cache(maxsize=None)
def walk(seed, steps=T):
    """The oracle under the hash agent with auto-reset, one dict of arrays: per step t the row count the step found (nP0), the
    action, the pair (i, j) it selected, |G| before and after, the row count it left (0: the episode ended, a reset follows)."""
    rec = {k: np.zeros(steps, dtype=np.int64) for k in ("nP0", "action", "i", "j", "nG0", "nG1", "nP1", "first_nP")}

    def left(o, t):                                  # (the new episode's row count: what the step behind a reset finds)
        if t and rec["nP1"][t - 1] == 0:
            rec["first_nP"][t - 1] = o.nP

    def before(o, t, act):
        left(o, t)
        rec["nP0"][t], rec["action"][t], rec["nG0"][t] = o.nP, act, o.nG
        rec["i"][t], rec["j"][t] = o.pairs()[act]

    def after(o, t, act, reward):
        rec["nG1"][t], rec["nP1"][t] = o.nG, o.nP

    left(ow.walk(DIST, seed, agent_seeds([seed])[0], steps, (before, after))[0], steps)
    return rec


def shows(case, w):
    """Steps t at which the walk `w` shows `case` (the situation concerns step t + 1, prepared by step t)."""
    nxt = slice(1, None)
    cur = slice(0, -1)
    done, zero = w["nP1"] == 0, (w["nG1"] == w["nG0"]) & (w["nP1"] > 0)
    ins = (w["nG1"] == w["nG0"] + 1) & (w["nP1"] > 0)
    if case == "reset_then_step":                    # the step behind a reset selects from the NEW list: its row count is the reset's
        return np.flatnonzero(done[cur] & (w["nP0"][nxt] == w["first_nP"][cur]) & (w["nP0"][nxt] > 0))
    if case == "zero_reduction_then_pair_behind_it":  # all pairs in the register copy, which the removal shifted at and behind `action`
        return np.flatnonzero(zero[cur] & (w["nP0"][cur] <= 64) & (w["action"][nxt] >= w["action"][cur]))
    if case == "insertion_then_pair_with_the_new_element":
        g = w["nG0"][cur]
        return np.flatnonzero(ins[cur] & ((w["i"][nxt] == g) | (w["j"][nxt] == g)))
    # (beyond 64 rows: step t leaves more than 64 pairs and step t + 1 selects one that is not in the register copy.  That step t
    # is also the very step that took the list across 64 happens for none of the 4096 seeds within 320 steps — the list is
    # beyond 64 rows for a handful of steps per thousand episodes — and changes nothing for the kernel, which sees |P| and the action.)
    if case == "beyond_64_pairs_and_back":           # the list has passed 64 rows and step t + 1 selects a pair beyond the register copy, ...
        up = np.flatnonzero((w["nP0"][nxt] > 64) & (w["action"][nxt] >= 64))
        # ... and the same episode later shrinks to 64 rows or fewer while it still has pairs
        back = np.flatnonzero((w["nP0"] > 64) & (w["nP1"] <= 64) & (w["nP1"] > 0))
        ends = np.flatnonzero(done)
        return np.array([t for t in up if any(b > t and not any(t < e < b for e in ends) for b in back)], dtype=np.int64)
    if case == "hash_blocks_64_and_128":             # steps 63 | 64 and 127 | 128 are plain steps of one episode (no reset in between)
        return np.array([63, 127] if not (done[63] or done[127]) else [], dtype=np.int64)
    if case == "leaves_the_class_at_the_capacity_test":   # |G| + 1 > cap in front of step t + 1, which step t (an insertion) prepared
        return np.flatnonzero(ins[cur] & (w["nG1"][cur] == LEAVE_CAP))
    raise KeyError(case)


def search(limit=4):
    """Seeds of SEARCH_SEEDS showing each case (the first `limit`): how CASE_SEEDS was found."""
    found = {c: [] for c in CASE_SEEDS}
    for s in SEARCH_SEEDS:
        w = walk(s)
        for c in found:
            if len(found[c]) < limit and len(shows(c, w)):
                found[c].append(s)
        walk.cache_clear()
        if all(len(v) >= limit for v in found.values()):
            break
    return found


def all_seeds():
    return tuple(sorted({s for v in CASE_SEEDS.values() for s in v}))


def test_every_case_has_seeds_that_show_it():
    for case, seeds in CASE_SEEDS.items():
        assert seeds, "no seed of %d..%d shows %r within %d steps" % (SEARCH_SEEDS[0], SEARCH_SEEDS[-1], case, T)
        for s in seeds:
            assert len(shows(case, walk(s))), (case, s)
    assert 1 <= len(all_seeds()) <= 256


def test_case_steps_fall_inside_and_across_launches():
    """The launches end at 1, 3, 66, 130, 195 and 320: among the seeds some case step t -> t + 1 lies inside a launch and some
    crosses from one launch into the next (the step prepared by the last step of a launch is the first of the next)."""
    ends = set(int(x) for x in np.cumsum(LAUNCHES))
    inside = across = 0
    for case, seeds in CASE_SEEDS.items():
        for s in seeds:
            for t in shows(case, walk(s)):
                if int(t) + 1 in ends:
                    across += 1
                else:
                    inside += 1
    assert inside and across, (inside, across)
    assert {e % 64 for e in ends} >= {1, 2, 3} and 64 in LAUNCHES and 63 in LAUNCHES and 65 in LAUNCHES


def test_walk_agrees_with_the_launch_records():
    """walks() of the events tests (what every launch leaves for the caller) follows the same steps."""
    seeds = all_seeds()
    recs = walks(DIST, seeds, LAUNCHES, True)
    for s, r in zip(seeds, recs):
        w = walk(s)
        for end, rec in zip(np.cumsum(LAUNCHES), r):
            last = int(end) - 1
            assert rec["total"] == end and rec["done"] == bool(w["nP1"][last] == 0)
            assert rec["rows"] == (w["first_nP"][last] if w["nP1"][last] == 0 else w["nP1"][last])


def test_sugar_bound_is_out_of_reach_of_the_class():
    """BBX_ST_DEG_OVERFLOW on the fast class needs a selected pair whose S-polynomial sugar passes 65535.  The class only takes
    ideals in at most 3 variables drawn from a distribution name (fixed ideals go to the wide class), and a name bounds the
    generators' degree by its middle number; over a walk the sugar stays within a small multiple of it.  Measured here: the
    largest degree a selected pair's lcm reaches on the seeds of this file — four orders of magnitude below the bound, so the
    refusal cannot be produced through the API and its path was checked by reading."""
    def degree(o, t, act):
        i, j = o.pairs()[act]
        li, lj = o.poly(int(i))[1][0], o.poly(int(j))[1][0]
        return max(int(np.maximum(li, lj).sum()), o.poly_sugar(int(i)), o.poly_sugar(int(j)))

    worst = max(d for s in all_seeds()[:4] for d, _ in ow.walk(DIST, s, agent_seeds([s])[0], T, (degree, None))[3])
    assert 0 < worst < 65535 // 100, worst
