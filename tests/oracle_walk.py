"""The one walk of the hash agent on the oracle that the fast-class tests share.  Every tests/test_X_cpu.py proves on the
oracle that its fixed seeds reach the events X is about, and tests/test_X_gpu.py runs the kernels on those seeds; both go
through walk() here and differ only in the observer they hand it.  Nothing in this module needs a device or torch."""
import collections

import numpy as np

from oracle import ffi
from oracle.trace import poly_words


def agent_seeds(seeds):
    """the agent seeds of the step-events, prefetch and compaction tests: ideal seed - 2993"""
    return [s - 2993 for s in seeds]


def grevlex_key(e):
    # larger degree is greater; at equal degree the SMALLER exponent of the last variable wins (and so on down)
    return (int(sum(e)),) + tuple(-int(x) for x in reversed(e))


Snapshot = collections.namedtuple("Snapshot", "nG words pairs order")


def snapshot(o):
    """What a state comparison needs of an oracle environment, detached from it: |G|, the basis as one stream of
    oracle.trace.poly_words, the pair list, the reducer order."""
    return Snapshot(o.nG, np.concatenate([poly_words(*o.poly(i)) for i in range(o.nG)]), o.pairs(), o.reducer_order())


def fresh(dist, seed):
    """an oracle environment of `dist`, seeded and reset"""
    o = ffi.load("bo").env(dist)
    o.seed(seed)
    o.reset()
    return o


def walk(dist, seed, aseed, nsteps, observe=None):
    """nsteps steps of the hash agent with auto-reset on the oracle: (the environment as it stands afterwards, per-step
    rewards, per-step done flags, observed).

    observe is an object with methods before(o, t, action) and after(o, t, action, reward), or a pair (before, after) of
    such callables; either may be missing (None).  before sees the state the step selects from; after sees the state the
    step left BEFORE a reset replaces it, so o.nP == 0 there says that the episode has just ended.  observed[t] is
    (what before returned, what after returned) of step t; an observer that carries more than that from step to step keeps
    it itself.  The state a step leaves once a reset has happened is what the next step's before hook sees (and, for the
    last step, the environment returned)."""
    if observe is None or isinstance(observe, tuple):
        before, after = observe or (None, None)
    else:
        before, after = getattr(observe, "before", None), getattr(observe, "after", None)
    o = fresh(dist, seed)
    rewards, dones, observed = [], [], []
    for t in range(nsteps):
        a = ffi.agent_action(aseed, t, o.nP)
        b = before(o, t, a) if before else None
        r = o.step(a)
        observed.append((b, after(o, t, a, r) if after else None))
        rewards.append(r)
        dones.append(o.nP == 0)
        if o.nP == 0:
            o.reset()
    return o, np.array(rewards), np.array(dones), observed
