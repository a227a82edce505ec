"""The entry / exit protocol of the step kernels, the same for every kernel class: one seeded batch goes through
one sequence of calls on every forced class, and after EVERY call the outputs a caller sees (rewards, dones, rows) and the
header fields behind stats() — steps, additions, episodes, zero reductions, status, queue head, basis size: everything but the
algorithmic bytes — must equal the oracle's and those of the class's default kernels.  The output arrays carry sentinel
values into every call, so that a word nobody wrote shows.

The calls: reset; a launch without steps; 6 counter-hash steps without auto-reset; host steps (action 0, no auto-reset) until
every environment has finished — the calls after an environment finished take the `no step in this launch` paths —; Degree
and seeded std::random rollouts with auto-reset on the finished batch (nothing to take: no reset is pending); then, after
another reset, the same rollouts with work to do, the std::random one in two launches (the engine's state goes through the
header); values().

Seeds (checked against the oracle in test_seeds_reach_the_hand_off, no GPU): with SEED0 = 50965 every environment of the
3-8-6-uniform batch but 0 and 10 grows a basis of more than 16 elements in its first episode (17 .. 56: the sixteen reach
16 17 28 17 19 31 27 41 23 37 16 27 34 17 56 37), beyond the 16 of the `lds_max_basis: 16` classes, so those hand
environments to the HBM-resident pass; the first episodes end after 100 host steps."""
import numpy as np
import pytest

from oracle import ffi
from oracle.trace import degree_action, run_trace

SEED0, STD_SEED0, K, GAMMA = 50965, 4242, 2, 0.99
BINOMIAL = ("3-8-6-uniform", 16)
FIXED = ("cyclic-4", 4)
# the forced classes; the first of each group is the reference the others are compared with
CASES = {
    "binom_default": (BINOMIAL, None),                                        # register/LDS-resident (fast) class
    "binom_hbm": (BINOMIAL, {"lds_max_basis": -1}),                           # HBM-resident binomial class
    "binom_handoff": (BINOMIAL, {"lds_max_basis": 16}),                       # fast class handing over to the HBM-resident one
    "general_staged": (BINOMIAL, {"general_class": 1}),                       # general class, LDS-staged
    "general_handoff": (BINOMIAL, {"general_class": 1, "lds_max_basis": 16}),  # ... handing over to its HBM-resident kernel
    "wide_default": (FIXED, None),                                            # wide class
    "wide_3waves": (FIXED, {"wide_waves": 3}),
    "wide_off": (FIXED, {"wide_waves": -1}),                                  # the same ideals on the general class
}
HANDOFF_BASIS = 16
STAT_COLS = [0, 1, 2, 3, 4, 5, 7]                                             # (6: algorithmic bytes, class-dependent by design)


def std_choice(x, n):
    """choice() of the reference's seeded Random selection: minstd_rand0 and libstdc++'s uniform_int_distribution(0, n - 1)
    (std_choice, bbx_device.h) -> (row, new engine state)."""
    scaling = 2147483645 // n
    while True:
        x = x * 16807 % 2147483647
        if x - 1 < n * scaling:
            return (x - 1) // scaling, x


class Model:
    """One environment of the batch on the oracle, with the counters of its header."""

    def __init__(self, dist, seed, agent_seed, std_seed):
        self.o = ffi.load("bo").env(dist)
        self.o.seed(seed)
        self.agent_seed, self.t = agent_seed, 0
        self.rng = std_seed % 2147483647 or 1
        self.steps = self.adds = self.episodes = self.zero = 0
        self.need_reset = True
        self.max_basis = 0

    def took(self, reward, basis_before):
        self.steps += 1; self.adds += int(-reward); self.t += 1
        self.zero += int(self.o.nG == basis_before)
        self.max_basis = max(self.max_basis, self.o.nG)
        done = self.o.nP == 0
        self.episodes += int(done)
        return done

    def launch(self, agent, nsteps, auto_reset, action=0):
        """The step loop of one launch -> (reward, done, rows) as the caller finds them."""
        o, reward, done_last = self.o, 0.0, False
        while True:
            if self.need_reset:
                o.reset(); self.need_reset = False
            if nsteps <= 0 or o.nP == 0:
                break
            if agent == "random":
                a = ffi.agent_action(self.agent_seed, self.t, o.nP)
            elif agent == "random_std":
                a, self.rng = std_choice(self.rng, o.nP)
            else:
                a = degree_action(o) if agent == "degree" else action
            basis_before = o.nG
            reward = o.step(a)
            done_last = self.took(reward, basis_before)
            nsteps -= 1
            self.need_reset = done_last and auto_reset
        return reward, int(done_last or (o.nP == 0 and not self.need_reset)), o.nP

    def degree_rollout_after_reset(self, nsteps):
        """reset() and a Degree rollout with auto-reset in one: oracle.trace.run_trace -> (reward, done, rows)."""
        tr = run_trace(self.o.copy(), K, nsteps, "degree")                     # (resets first, and behind every finished episode)
        self.need_reset = True
        res = self.launch("degree", nsteps, True)
        assert len(tr["reward"]) == nsteps and res[:2] == (float(tr["reward"][-1]), int(tr["done"][-1]))
        assert res[2] == (self.o.nP if tr["done"][-1] else int(tr["nP"][-1])) and (self.o.obs(K) == tr["final_obs"]).all()
        return res

    def stats(self):
        return [self.steps, self.adds, self.episodes, self.zero, 0, self.o.nG]


def _models(dist, B):
    return [Model(dist, SEED0 + e, e, STD_SEED0 + e) for e in range(B)]


def _oracle_calls(dist, B):
    """What every call of the sequence leaves, from the oracle: a list of (label, rewards, dones, rows, stats[B, 6])."""
    ms, out = _models(dist, B), []

    def record(label, res):
        out.append((label, [r[0] for r in res], [r[1] for r in res], [r[2] for r in res], [m.stats() for m in ms]))

    record("no steps", [m.launch("first", 0, False) for m in ms])             # (reset() and the launch without steps: one state)
    record("hash 6", [m.launch("random", 6, False) for m in ms])
    while True:
        before = [m.o.nP == 0 for m in ms]
        record("host step", [m.launch("external", 1, False) for m in ms])
        if all(before):
            break
    record("degree 40, finished", [m.launch("degree", 40, True) for m in ms])
    record("std random 3, finished", [m.launch("random_std", 3, True) for m in ms])
    record("degree 40", [m.degree_rollout_after_reset(40) for m in ms])
    for n in (3, 2):
        record("std random %d" % n, [m.launch("random_std", n, True) for m in ms])
    values = [m.o.value("degree", GAMMA) for m in ms]
    return out, values, max(m.max_basis for m in ms)


_ORACLE, _GPU = {}, {}


def oracle_calls(dist, B):
    if (dist, B) not in _ORACLE:                                              # (once per batch, shared by its classes)
        _ORACLE[dist, B] = _oracle_calls(dist, B)
    return _ORACLE[dist, B]


def _gpu_calls(dist, B, caps):
    """The same sequence on the device -> (calls as (label, rewards, dones, rows, stats[B, 7]), values, largest basis seen)."""
    from deepgroebner_amd import VecLeadMonomialsEnv, _ffi
    env = VecLeadMonomialsEnv(dist, batch=B, k=K, caps=caps)
    env.seed(np.arange(B) + SEED0); env.seed_agent(np.arange(B)); env.seed_strategy(np.arange(B) + STD_SEED0)
    L, out, big = _ffi.lib(), [], 0

    def call(label, fn):
        nonlocal big
        rew = np.full(B, 7.0); done = np.full(B, 9, dtype=np.uint8); rows = np.full(B, -5, dtype=np.int32)   # sentinels
        _ffi.check(fn(rew, done, rows))
        st = env.stats()
        big = max(big, int(st[:, 7].max()))
        out.append((label, rew.tolist(), done.tolist(), rows.tolist(), st[:, STAT_COLS].tolist()))
        env.rows[:] = rows

    def rollout(agent, n, auto_reset):
        return lambda rew, done, rows: L.bbx_rollout(env._h, _ffi.AGENTS[agent], n, int(auto_reset), _ffi.ptr(rew), _ffi.ptr(done), _ffi.ptr(rows))

    acts = np.zeros(B, dtype=np.int32)
    env.reset()
    call("no steps", rollout("first", 0, False))
    call("hash 6", rollout("random", 6, False))
    for _ in range(400):
        before = env.rows == 0
        call("host step", lambda rew, done, rows: L.bbx_step(env._h, _ffi.ptr(acts), _ffi.ptr(rew), _ffi.ptr(done), _ffi.ptr(rows)))
        if before.all():
            break
    call("degree 40, finished", rollout("degree", 40, True))
    call("std random 3, finished", rollout("random_std", 3, True))
    env.reset()
    call("degree 40", rollout("degree", 40, True))
    for n in (3, 2):
        call("std random %d" % n, rollout("random_std", n, True))
    return out, env.values("degree", GAMMA).tolist(), big


def test_seeds_reach_the_hand_off():
    """The recorded seeds: some environment of the binomial batch outgrows the 16 basis elements of the small LDS classes."""
    dist, B = BINOMIAL
    assert oracle_calls(dist, B)[2] > HANDOFF_BASIS


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_step_protocol_same_in_every_class(case):
    (dist, B), caps = CASES[case]
    want, want_values, _ = oracle_calls(dist, B)
    got, values, big = _gpu_calls(dist, B, caps)
    assert [c[0] for c in got] == [c[0] for c in want]                        # the same calls (as many host steps)
    for (label, rew, done, rows, st), (_, wrew, wdone, wrows, wst) in zip(got, want):
        assert rew == wrew, (case, label, "rewards")
        assert done == wdone, (case, label, "dones")
        assert rows == wrows, (case, label, "rows")
        # oracle: steps, additions, episodes, zero reductions, status OK, basis size (the queue head: against the reference class)
        assert [s[:5] + s[6:] for s in st] == wst, (case, label, "stats")
    assert values == want_values, (case, "values")
    if caps and caps.get("lds_max_basis") == HANDOFF_BASIS:
        assert big > HANDOFF_BASIS                                            # (the hand-off occurred)
    ref = next(c for c in CASES if CASES[c][0] == (dist, B))
    if case == ref:
        _GPU[ref] = (got, values)
    else:
        if ref not in _GPU:
            _GPU[ref] = _gpu_calls(dist, B, CASES[ref][1])[:2]
        assert (got, values) == _GPU[ref], (case, "differs from", ref)       # everything, the queue head included
