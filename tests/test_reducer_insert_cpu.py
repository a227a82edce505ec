"""An insertion of the fast class puts the new element into the six reducer-order register arrays in place (f_insert6,
bbx_fast.h: the lanes beyond the position take their lower neighbour's word, the position's lane takes the new one) and
drops the selected pair in the same pass that compacts the old pairs.  This file asserts, on the
oracle alone, that the seeds tests/test_reducer_insert_gpu.py runs reach every situation those two have to get right:
  the new element enters the reducer order at position 0, at the end (position = |G|) and strictly inside, each with and
    without a tail (six situations);
  an insertion takes |G| from 63 to 64, where the update changes from the one-bank to the two-bank form;
  an inserting step selects the pair at index 0 and at index |P| - 1, with |P| < 64 and with |P| exactly 64 (four).
All eleven are here; tests/test_update_thresholds_gpu.py and tests/test_pair_compaction_gpu.py pin neighbouring thresholds
(|G| and |P| across 64 and 128, lists beyond 64 pairs) and are not relied on.  Ideal seeds 1000 .. 12999 with agent seed =
ideal seed - 993 were searched, 256 steps each: an element without a tail entering at the end showed on 45 of them, |P| = 64
with the first pair selected on 4, with the last on 2.  A seed that stops showing its situation fails the test."""
import functools

import numpy as np

from tests import oracle_walk as ow

DIST, K, T = "3-20-10-weighted", 2, 256
SEEDS = ((1000, 7), (1016, 23), (1028, 35), (1168, 175), (1274, 281), (1464, 471), (5198, 4205), (11922, 10929))
SITUATIONS = ("front_tail", "front_notail", "end_tail", "end_notail", "inside_tail", "inside_notail", "g63to64",
              "first_lt64", "last_lt64", "first_eq64", "last_eq64")
# situation -> ((ideal seed, agent seed), step) as the search reported them, re-asserted below
KNOWN = {"end_notail": (((1168, 175), 2), ((1274, 281), 62)), "g63to64": (((1016, 23), 61), ((1028, 35), 83), ((1274, 281), 195)),
         "first_eq64": (((1464, 471), 136), ((5198, 4205), 124)), "last_eq64": (((11922, 10929), 102),),
         "end_tail": (((1016, 23), 1), ((1028, 35), 0)), "front_notail": (((1000, 7), 34),), "inside_notail": (((1000, 7), 33),)}
LAUNCH = 16                                                  # the GPU test compares the state every LAUNCH steps
CUT = 32                                                     # ... and starts value() and policy rollouts every CUT steps


class Inserts:
    """walk()'s observer: where every insertion puts the new element and which pair its step selected, and the state the
    run stands in after every LAUNCH and CUT steps — left(o, t), the state t steps leave with a reset done, which is what
    the next step's before hook sees."""

    def __init__(self):
        self.seen = {k: [] for k in SITUATIONS}
        self.states, self.cuts = [], []

    def left(self, o, t):
        if t and t % LAUNCH == 0:
            self.states.append(ow.snapshot(o))
        if t and t % CUT == 0:
            self.cuts.append(o.copy())

    def before(self, o, t, a):
        self.left(o, t)
        self.nP, self.g = o.nP, o.nG

    def after(self, o, t, a, reward):
        nP, g, seen = self.nP, self.g, self.seen
        if o.nG == g + 1:                                        # an insertion: the new element is basis index g
            pos = int(np.flatnonzero(o.reducer_order() == g)[0])
            where = "front" if pos == 0 else ("end" if pos == g else "inside")
            seen[where + ("_tail" if len(o.poly(g)[0]) > 1 else "_notail")].append(t)
            if g == 63:
                seen["g63to64"].append(t)
            if nP < 64 and a == 0:
                seen["first_lt64"].append(t)
            if 1 < nP < 64 and a == nP - 1:
                seen["last_lt64"].append(t)
            if nP == 64 and a == 0:
                seen["first_eq64"].append(t)
            if nP == 64 and a == 63:
                seen["last_eq64"].append(t)


@functools.lru_cache(maxsize=None)
def walk(seed, aseed, nsteps=T):
    """nsteps steps of the hash agent with auto-reset on the oracle: ({situation: steps that show it}, [the state
    (oracle_walk.Snapshot: basis words, pair list, reducer order) after every LAUNCH steps], the environment as it stands
    afterwards, [a copy of the environment after every CUT steps])."""
    ins = Inserts()
    o = ow.walk(DIST, seed, aseed, nsteps, ins)[0]
    ins.left(o, nsteps)
    return ins.seen, ins.states, o, ins.cuts


def test_every_situation_is_reached():
    assert len(SEEDS) == len(set(SEEDS)) == 8 and T % LAUNCH == 0 and CUT % LAUNCH == 0
    shown = {k: [sa for sa in SEEDS if walk(*sa)[0][k]] for k in SITUATIONS}
    assert all(shown[k] for k in SITUATIONS), {k: len(v) for k, v in shown.items()}
    # the common ones on every seed, the rare ones where the search found them
    for k in ("front_tail", "front_notail", "inside_tail", "inside_notail", "first_lt64", "last_lt64"):
        assert len(shown[k]) == 8, (k, shown[k])
    for k, where in KNOWN.items():
        for sa, t in where:
            assert t in walk(*sa)[0][k], (k, sa, t, walk(*sa)[0][k])


def test_rare_situations_fall_inside_a_launch_too():
    """The GPU test chains launches of LAUNCH steps; an insertion at the last step of a launch is followed by a write-back,
    one inside a launch by a step of the same kernel on the registers it left.  Every situation shows inside a launch."""
    for k in SITUATIONS:
        steps = [t for sa in SEEDS for t in walk(*sa)[0][k]]
        assert any((t + 1) % LAUNCH for t in steps), (k, steps)


def test_value_rollouts_from_the_cuts_meet_the_thresholds():
    """The GPU test runs value() from the state after every CUT steps.  Under 'first' (pair 0 at every step, to the end of the
    episode) those rollouts are simulated here: the value kernel inserts at the front and inside, with and without a tail,
    takes |G| from 63 to 64 and selects the first of exactly 64 pairs in an inserting step.  (It meets no insertion at the
    end and cannot select a last pair: the policy rollouts and the lean kernels are what stands for those.)"""
    met = {k: 0 for k in SITUATIONS}
    for sa in SEEDS:
        for cut in walk(*sa)[3]:
            o = cut.copy()
            while o.nP > 0:
                nP, g = o.nP, o.nG
                o.step(0)
                if o.nG == g + 1:
                    pos = int(np.flatnonzero(o.reducer_order() == g)[0])
                    where = "front" if pos == 0 else ("end" if pos == g else "inside")
                    met[where + ("_tail" if len(o.poly(g)[0]) > 1 else "_notail")] += 1
                    met["g63to64"] += int(g == 63)
                    met["first_eq64"] += int(nP == 64)
                    met["first_lt64"] += int(nP < 64)
    for k in ("front_tail", "front_notail", "inside_tail", "inside_notail", "g63to64", "first_eq64", "first_lt64"):
        assert met[k] >= 8, (k, met)
