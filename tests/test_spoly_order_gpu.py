"""The S-polynomial's two scaled tails ordered by the reduction loop's own scalar code (FA_ORDER, bbx_fast.h) instead of a
merge on the vector unit, through every kernel of the fast class: traced step for step, lean headline (single launches
and a persistent session), generic lean (obs_fill), value, one-layer policy rollout.  Eight environments, 256 steps; the
seeds select pairs of every kind the ordering has to tell apart — first tail leading, second leading, equal monomials
with a non-zero and with a zero sum, either member or both without a tail (tests/test_spoly_order_cpu.py asserts that).
Everything against the oracle: per step on the traced kernel, state (basis term for term, pair list, reducer order) and
outputs on the lean ones."""
import numpy as np
import pytest

from oracle import ffi
from oracle.trace import poly_words, run_trace
from tests import policy_cases as pc
from tests.test_spoly_order_cpu import DIST, K, SEEDS, T, walk

pytestmark = pytest.mark.gpu
KEYS = (("action", "action"), ("reward", "reward"), ("rows", "nP"), ("basis_size", "nG"), ("done", "done"), ("obs_hash", "obs_hash"),
        ("pairs_hash", "pairs_hash"), ("newpoly_hash", "newpoly_hash"))
B = len(SEEDS)
R = 256


def _env(trace=0):
    from deepgroebner_amd import VecLeadMonomialsEnv
    env = VecLeadMonomialsEnv(DIST, batch=B, k=K)
    env.seed(np.array([s for s, _ in SEEDS]))
    env.seed_agent(np.array([a for _, a in SEEDS]))
    if trace:
        env.trace_enable(trace)
    env.reset()
    return env


def _same(env, e, o, where):
    basis, pairs, order = env.state(e)
    assert len(basis) == o.nG, (where, e)
    got = np.concatenate([poly_words(c, x) for c, x in basis])
    want = np.concatenate([poly_words(*o.poly(i)) for i in range(o.nG)])
    assert np.array_equal(got, want), (where, e, "basis")
    assert np.array_equal(pairs, o.pairs()), (where, e, "pairs")
    assert np.array_equal(order, o.reducer_order()), (where, e, "reducer order")


def _same_state(env, where):
    for e, sa in enumerate(SEEDS):
        _same(env, e, walk(*sa)[0], where)


def _buffers(n):
    import torch
    return (torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"),
            torch.zeros(n, dtype=torch.int32, device="cuda"), torch.full((n, R, 4 * 3), -1, dtype=torch.int32, device="cuda"))


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


@pytest.mark.parametrize("kernel", ("headline", "headline-session", "generic"))
def test_lean_rollout_device(kernel):
    """The lean headline shape (hash agent, the observation written after every step, no fill) as four launches of 64 steps
    and as one persistent session of four calls; with obs_fill on the launcher takes the generic lean kernel instead."""
    import torch
    env = _env()
    env.accounting(False)
    env.persistent(kernel == "headline-session")
    s = torch.cuda.current_stream().cuda_stream
    rew, done, rows, obs = _buffers(B)
    for _ in range(4):
        env.rollout_device("random", T // 4, True, s, rew, done, rows, obs, R, kernel == "generic", True)
    env.sync()
    if kernel == "headline-session":
        assert env.session_stats()["sessions"] >= 1, env.session_stats()
    st = env.stats()
    assert (st[:, 0] == T).all() and (st[:, 4] == 0).all(), st
    _same_state(env, kernel)
    got_rew, got_done, got_rows, got_obs = (x.cpu().numpy() for x in (rew, done, rows, obs))
    for e, sa in enumerate(SEEDS):
        o, rewards, dones, _ = walk(*sa)
        assert got_rew[e] == rewards[-1] and bool(got_done[e]) == bool(dones[-1]) and got_rows[e] == o.nP, e
        assert np.array_equal(got_obs[e, :o.nP], o.obs(K)), e
        # additions (1 + reductions per step) and episodes over the whole run
        assert st[e, 1] == int(np.sum(-rewards)) and st[e, 2] == int(dones.sum()), (e, st[e])
    if kernel == "generic":                                  # (the fill: -1 behind the live rows)
        assert all((got_obs[e, got_rows[e]:] == -1).all() for e in range(B))


def test_values_after_the_rollout():
    """value() rollouts (the class's value kernel: to the end of the episode under a fixed strategy) from the state 256
    steps in"""
    env = _env()
    env.rollout("random", T, auto_reset=True)
    for strategy in ("degree", "first"):
        got = env.values(strategy, 0.99)
        for e, sa in enumerate(SEEDS):
            assert got[e] == walk(*sa)[0].value(strategy, 0.99), (strategy, e)
    _same_state(env, "valued")


def test_policy_rollout_one_layer():
    """bbx_policy_rollout_device with a one-layer policy of 64 hidden units, 64 steps: the environments — replayed on the
    oracle with the actions the kernel drew — step for step: observation, row count, reward, done flag; the state afterwards."""
    import torch
    nT = 64
    env = _env()
    env.accounting(False)
    w = pc.make_weights(env.cols, (64,), 1611)
    pol = pc.to_policy(w, "cuda")
    p = pol._fused_weights()
    s = torch.cuda.current_stream().cuda_stream
    u = torch.rand((nT, B), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1612))
    A = torch.zeros((nT, B), dtype=torch.int32, device="cuda"); L = torch.zeros((nT, B), dtype=torch.float32, device="cuda")
    Rw = torch.zeros((nT, B), dtype=torch.float64, device="cuda"); D = torch.zeros((nT, B), dtype=torch.uint8, device="cuda")
    N = torch.zeros((nT, B), dtype=torch.int32, device="cuda")
    O = torch.full((nT, B, R, env.cols), -1, dtype=torch.int32, device="cuda")
    env.policy_rollout_device(p["prepared"], p["hidden"], nT, u, A, L, Rw, D, N, O, R, B * R * env.cols, s)
    env.sync(); torch.cuda.synchronize()
    acts, rews, dones = A.cpu().numpy(), Rw.cpu().numpy(), D.cpu().numpy()
    obs, rows = O.cpu().numpy(), N.cpu().numpy()
    bo = ffi.load("bo")
    assert env.stats()[:, 4].max() == 0
    for e, (seed, _) in enumerate(SEEDS):
        o = bo.env(DIST); o.seed(seed); o.reset()
        for t in range(nT):
            assert rows[t, e] == o.nP and np.array_equal(obs[t, e, :o.nP], o.obs(K)), (e, t)
            assert 0 <= acts[t, e] < o.nP, (e, t)
            r = o.step(int(acts[t, e]))
            assert rews[t, e] == r and bool(dones[t, e]) == (o.nP == 0), (e, t)
            if o.nP == 0:
                o.reset()
        _same(env, e, o, "policy rollout")
