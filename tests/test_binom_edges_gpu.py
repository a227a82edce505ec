"""The binomial class of the step kernel (binom_body, bin_add_poly, merge2: csrc/bbx_binom.h) on the cases of
tests/binom_cases.py: reductions whose reducer lies in the last register chunk of the scan, in the memory part behind it, or
nowhere although the basis is larger than the register part (sort_reducers=False on bases of 200 to 510 generators, and one
sorted case), and the coefficient and merge edges — members and reducers without a tail, tails and reduction products that
meet on one monomial with and without cancelling, new elements with lead coefficient 1 and p - 1 — on 8-, 16- and 32-byte
monomials (and the two lead coefficients once more on 5-10-5-uniform, the benchmark's second distribution).
tests/test_binom_edges_cpu.py asserts without a device that the seeds show these situations at the pinned steps.

Every comparison is exact against the oracle.  Per case, with the batch equal to the case's seed pairs: one traced launch
step for step, traced launches of 7 steps (launches then begin inside an episode, on the deep cases with a basis beyond the
register part), the lean kernels through device buffers in two launches, value() rollouts before and after, and for the
deep-reducer cases the general class, which has a reducer scan of its own."""
import functools

import numpy as np
import pytest

from oracle import ffi
from oracle.trace import poly_words, run_trace
from tests import binom_cases as bc

pytestmark = pytest.mark.gpu
K = bc.K
KEYS = (("action", "action"), ("reward", "reward"), ("rows", "nP"), ("basis_size", "nG"), ("done", "done"), ("obs_hash", "obs_hash"),
        ("pairs_hash", "pairs_hash"), ("newpoly_hash", "newpoly_hash"))
NAMES = sorted(bc.CASES)
DEEP = [n for n in NAMES if bc.CASES[n].group.startswith("deep")]


@functools.lru_cache(maxsize=None)
def oracle_traces(name):
    """run_trace of every environment of the case: computed once, shared by the traced tests of all classes"""
    c = bc.CASES[name]
    bo = ffi.load("bo")
    out = []
    for s, a in c.seeds:
        o = bo.env(c.dist, **dict(c.opts))
        o.seed(s)
        out.append(run_trace(o, K, c.steps, "hash", agent_seed=a))
    return out


def make_env(name, caps="case", trace=0):
    from deepgroebner_amd import VecLeadMonomialsEnv
    c = bc.CASES[name]
    env = VecLeadMonomialsEnv(c.dist, batch=len(c.seeds), k=K, caps=(c.caps if caps == "case" else caps), **dict(c.opts))
    env.seed(np.array([s for s, _ in c.seeds]))
    env.seed_agent(np.array([a for _, a in c.seeds]))
    if trace:
        env.trace_enable(trace)
    env.reset()
    return env


def state_words(basis, pairs, order):
    return np.concatenate([poly_words(c, x) for c, x in basis] + [np.asarray(pairs, np.int32).ravel(), np.asarray(order, np.int32)])


def same_state(env, name, where):
    """basis term for term, pair list and reducer order of every environment against the oracle walk's final state"""
    for e in range(len(bc.CASES[name].seeds)):
        o = bc.case_walk(name, e).env
        basis, pairs, order = env.state(e)
        assert len(basis) == o.nG, (name, where, e)
        got = np.concatenate([poly_words(c, x) for c, x in basis])
        want = np.concatenate([poly_words(*o.poly(i)) for i in range(o.nG)])
        assert np.array_equal(got, want), (name, where, e, "basis")
        assert np.array_equal(pairs, o.pairs()), (name, where, e, "pairs")
        assert np.array_equal(order, o.reducer_order()), (name, where, e, "reducer order")


def check_traced(name, chunk, caps="case"):
    c = bc.CASES[name]
    T = c.steps
    chunk = chunk or T
    env = make_env(name, caps, trace=chunk)
    got = [[] for _ in c.seeds]
    for t0 in range(0, T, chunk):                            # (every launch writes its trace from slot 0)
        n = min(chunk, T - t0)
        rew, done, rows = env.rollout("random", n, auto_reset=True)
        for e in range(len(c.seeds)):
            got[e].append(env.trace_read(e, 0, n))
    for e, want in enumerate(oracle_traces(name)):
        g = np.concatenate(got[e])
        for key, wkey in KEYS:
            w = np.asarray(want[wkey])
            same = g[key].astype(w.dtype) == w
            assert same.all(), (name, chunk, "environment", e, key, "first difference at step", int(np.flatnonzero(~same)[0]))
        assert np.array_equal(state_words(*env.state(e)), np.concatenate([want["final_basis"], want["final_pairs"].ravel(), want["final_order"]])), \
            (name, chunk, e, "final state")
        assert rew[e] == want["reward"][-1] and bool(done[e]) == bool(want["done"][-1]) and rows[e] == len(want["final_pairs"]), (name, chunk, e)
    same_state(env, name, ("traced", chunk))                 # (the two oracle walks describe the same run)
    obs = env.observations()
    for e, want in enumerate(oracle_traces(name)):
        assert np.array_equal(obs[e], want["final_obs"]), (name, chunk, e, "observation")
    assert (env.stats()[:, 4] == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_one_traced_launch(name):
    check_traced(name, 0)


@pytest.mark.parametrize("name", NAMES)
def test_traced_launches_of_7_steps(name):
    check_traced(name, 7)


@pytest.mark.parametrize("name", DEEP)
def test_general_class_one_traced_launch(name):
    """The general class on the same binomial ideals: wave_reduce (csrc/bbx_device.h) scans the reducers itself."""
    check_traced(name, 0, caps=bc.GENERAL)


@pytest.mark.parametrize("name", NAMES)
def test_lean_kernels_through_device_buffers(name):
    """The production variant (no accounting, no tracing) on device buffers, the observation block written at every step, in
    two launches: final state, outputs, the block, and the step, addition and episode counters against the oracle walk."""
    import torch
    c = bc.CASES[name]
    B, T = len(c.seeds), c.steps
    walks = [bc.case_walk(name, e) for e in range(B)]
    R = max(max(int(tr["nP"].max()), int(tr["init"][1])) for tr in oracle_traces(name)) + 1   # (no step's rows are cut)
    env = make_env(name)
    env.accounting(False)
    s = torch.cuda.current_stream().cuda_stream
    obs = torch.zeros((B, R, env.cols), dtype=torch.int32, device="cuda")
    rew = torch.zeros(B, dtype=torch.float64, device="cuda"); done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(B, dtype=torch.int32, device="cuda")
    for n in (T // 2, T - T // 2):
        env.rollout_device("random", n, True, s, rew, done, rows, obs, R, False, True)
    env.sync(); torch.cuda.synchronize()
    st = env.stats()
    assert (st[:, 0] == T).all() and (st[:, 4] == 0).all(), (name, st)
    same_state(env, name, "lean")
    rew, done, rows, obs = rew.cpu().numpy(), done.cpu().numpy(), rows.cpu().numpy(), obs.cpu().numpy()
    for e, w in enumerate(walks):
        o = w.env
        assert rew[e] == w.rewards[-1] and bool(done[e]) == bool(w.dones[-1]) and rows[e] == o.nP, (name, e)
        assert st[e, 1] == int(np.sum(-w.rewards)) and st[e, 2] == int(w.dones.sum()), (name, e, st[e])
        assert np.array_equal(obs[e, :o.nP], o.obs(K)), (name, e, "observation block")


@pytest.mark.parametrize("name", NAMES)
def test_values_before_and_after_the_rollout(name):
    """value() rollouts under "degree" and "first" from the reset state and from the state after the case's steps; the batch
    itself stays where the oracle is."""
    c = bc.CASES[name]
    env = make_env(name)
    bo = ffi.load("bo")
    for nsteps in (0, c.steps):
        if nsteps:
            env.rollout("random", nsteps, auto_reset=True)
        for strategy in ("degree", "first"):
            got = env.values(strategy, 0.99)
            for e, (s, a) in enumerate(c.seeds):
                if nsteps:
                    o = bc.case_walk(name, e).env
                else:
                    o = bo.env(c.dist, **dict(c.opts)); o.seed(s); o.reset()
                assert got[e] == o.value(strategy, 0.99), (name, nsteps, strategy, e)
    same_state(env, name, "valued")
