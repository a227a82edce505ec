"""New basis elements with lead coefficient 1 and 32002 (the two ends of the inverse table the fast class reads 1/LC from,
bbx_fast.h add_poly) through every kernel of the class a rollout can take: the traced kernel step for step, the lean headline
kernel as single launches and inside a persistent session, and the value kernel.  Eight environments, 128 steps; basis, reducer
order, pair list, rewards and observation against the oracle.  tests/test_lead_coef_cpu.py asserts that the seeds produce
those elements and that later steps use them."""
import numpy as np
import pytest

from oracle import ffi
from oracle.trace import poly_words, run_trace
from tests.test_lead_coef_cpu import DIST, K, SEEDS, T, walk

pytestmark = pytest.mark.gpu
KEYS = (("action", "action"), ("reward", "reward"), ("rows", "nP"), ("basis_size", "nG"), ("done", "done"), ("obs_hash", "obs_hash"),
        ("pairs_hash", "pairs_hash"), ("newpoly_hash", "newpoly_hash"))
B = len(SEEDS)


def _env(trace=0):
    from deepgroebner_amd import VecLeadMonomialsEnv
    env = VecLeadMonomialsEnv(DIST, batch=B, k=K)
    env.seed(np.array([s for s, _ in SEEDS]))
    env.seed_agent(np.array([a for _, a in SEEDS]))
    if trace:
        env.trace_enable(trace)
    env.reset()
    return env


def _same_state(env, where):
    """basis term for term, pair list and reducer order of every environment against the oracle after T steps"""
    for e, sa in enumerate(SEEDS):
        o = walk(*sa)[0]
        basis, pairs, order = env.state(e)
        assert len(basis) == o.nG, (where, e)
        got = np.concatenate([poly_words(c, x) for c, x in basis])
        want = np.concatenate([poly_words(*o.poly(i)) for i in range(o.nG)])
        assert np.array_equal(got, want), (where, e, "basis")
        assert np.array_equal(pairs, o.pairs()), (where, e, "pairs")
        assert np.array_equal(order, o.reducer_order()), (where, e, "reducer order")


def test_traced_rollout_step_for_step():
    env = _env(trace=T)
    rew, done, rows = env.rollout("random", T, auto_reset=True)
    bo = ffi.load("bo")
    for e, (s, a) in enumerate(SEEDS):
        o = bo.env(DIST)
        o.seed(s)
        want = run_trace(o, K, T, "hash", agent_seed=a)
        got = env.trace_read(e, 0, T)
        for key, wkey in KEYS:
            w = np.asarray(want[wkey])
            g = got[key].astype(w.dtype)
            assert np.array_equal(g, w), (e, key, "first difference at step", int(np.flatnonzero(g != w)[0]))
        assert rew[e] == want["reward"][-1] and bool(done[e]) == bool(want["done"][-1]) and rows[e] == walk(s, a)[0].nP, e
    _same_state(env, "traced")
    obs = env.observations()
    for e, sa in enumerate(SEEDS):
        assert np.array_equal(obs[e], walk(*sa)[0].obs(K)), e


@pytest.mark.parametrize("persistent", (False, True))
def test_headline_rollout_device(persistent):
    """The lean headline shape (hash agent, rewards / dones / rows buffers, the observation written after every step) as two
    launches of 64 steps and as one persistent session of two calls."""
    import torch
    R = 256
    env = _env()
    env.accounting(False)
    env.persistent(persistent)
    s = torch.cuda.current_stream().cuda_stream
    obs = torch.zeros((B, R, env.cols), dtype=torch.int32, device="cuda")
    rew = torch.zeros(B, dtype=torch.float64, device="cuda"); done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(B, dtype=torch.int32, device="cuda")
    for n in (T // 2, T - T // 2):
        env.rollout_device("random", n, True, s, rew, done, rows, obs, R, False, True)
    env.sync()
    if persistent:
        assert env.session_stats()["sessions"] >= 1, env.session_stats()
    st = env.stats()
    assert (st[:, 0] == T).all() and (st[:, 4] == 0).all(), st
    _same_state(env, ("headline", persistent))
    rew, done, rows, obs = rew.cpu().numpy(), done.cpu().numpy(), rows.cpu().numpy(), obs.cpu().numpy()
    for e, sa in enumerate(SEEDS):
        o, rewards, dones, ins = walk(*sa)
        assert rew[e] == rewards[-1] and bool(done[e]) == bool(dones[-1]) and rows[e] == o.nP, e
        assert st[e, 1] == int(np.sum(-rewards)) and st[e, 2] == int(dones.sum()), (e, st[e])
        assert np.array_equal(obs[e, :o.nP], o.obs(K)), e


def test_values_before_and_after_the_rollout():
    """value() rollouts (the class's value kernel) from the reset state and from the state 128 steps later"""
    env = _env()
    bo = ffi.load("bo")
    for nsteps in (0, T):
        if nsteps:
            env.rollout("random", nsteps, auto_reset=True)
        for strategy in ("degree", "first"):
            got = env.values(strategy, 0.99)
            for e, (s, a) in enumerate(SEEDS):
                if nsteps:
                    o = walk(s, a)[0]
                else:
                    o = bo.env(DIST); o.seed(s); o.reset()
                assert got[e] == o.value(strategy, 0.99), (nsteps, strategy, e)
    _same_state(env, "valued")
