"""The peel by one keyed wave minimum per bucket (add_poly, bbx_fast.h) through every kernel of the fast class: traced, lean
headline (single launches and a persistent session), generic lean (obs_fill), value, one-layer policy rollout.  Eight
environments whose 256 steps under the hash agent show, each of them, every insertion tests/test_peel_keyed_min_cpu.py lists:
several buckets at one degree, a bucket with a coprime member, a bucket of three and more equal lcms, six and more buckets, an
insertion that emits nothing, and insertions into 64 and more elements (the two-bank copy).  The lean run is cut into launches
of 16 steps, and after EVERY launch the basis term for term, the pair list and the reducer order of every environment are
compared with the oracle's — a pair emitted for the wrong member of a bucket, or a bucket left in, shows within 16 steps of
where it happened.  The value and the policy kernel choose their own pairs: they start from the state after every 32 steps of
that run (bases of 64 and more elements among them) and are held to the oracle replayed with their actions (state term for
term) or run with their strategy (value)."""
import numpy as np
import pytest

from oracle.trace import poly_words
from tests import policy_cases as pc
from tests.test_peel_keyed_min_cpu import CUT, DIST, K, LAUNCH, SEEDS, T, walk

pytestmark = pytest.mark.gpu
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


def _check(env, launch, where):
    for e, sa in enumerate(SEEDS):
        words, pairs, order = walk(*sa)[1][launch]
        basis, got_pairs, got_order = env.state(e)
        got = np.concatenate([poly_words(c, x) for c, x in basis])
        assert np.array_equal(got_order, order), (where, e, "reducer order after step", (launch + 1) * LAUNCH)
        assert np.array_equal(got_pairs, pairs), (where, e, "pairs after step", (launch + 1) * LAUNCH)
        assert np.array_equal(got, words), (where, e, "basis after step", (launch + 1) * LAUNCH)


@pytest.mark.parametrize("kernel", ("headline", "headline-session", "generic"))
def test_state_after_every_short_launch(kernel):
    import torch
    env = _env()
    env.accounting(False)
    env.persistent(kernel == "headline-session")
    s = torch.cuda.current_stream().cuda_stream
    rew = torch.zeros(B, dtype=torch.float64, device="cuda"); done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(B, dtype=torch.int32, device="cuda")
    obs = torch.full((B, R, 4 * 3), -1, dtype=torch.int32, device="cuda")
    for launch in range(T // LAUNCH):
        env.rollout_device("random", LAUNCH, True, s, rew, done, rows, obs, R, kernel == "generic", True)
        env.sync()
        _check(env, launch, kernel)
    st = env.stats()
    assert (st[:, 0] == T).all() and (st[:, 4] == 0).all(), st
    got_rows, got_obs = rows.cpu().numpy(), obs.cpu().numpy()
    for e, sa in enumerate(SEEDS):
        o = walk(*sa)[2]
        assert got_rows[e] == o.nP and np.array_equal(got_obs[e, :min(o.nP, R)], o.obs(K)[:R]), e


def test_traced_rollout_in_one_launch():
    """The same 256 steps as ONE launch of the traced kernel: every insertion is followed by a step on the registers it left."""
    from oracle import ffi
    from oracle.trace import run_trace
    env = _env(trace=T)
    env.rollout("random", T, auto_reset=True)
    bo = ffi.load("bo")
    for e, (s, a) in enumerate(SEEDS):
        o = bo.env(DIST)
        o.seed(s)
        want = run_trace(o, K, T, "hash", agent_seed=a)
        got = env.trace_read(e, 0, T)
        for key, wkey in (("action", "action"), ("reward", "reward"), ("rows", "nP"), ("basis_size", "nG"), ("done", "done"),
                          ("obs_hash", "obs_hash"), ("pairs_hash", "pairs_hash"), ("newpoly_hash", "newpoly_hash")):
            w = np.asarray(want[wkey])
            g = got[key].astype(w.dtype)
            assert np.array_equal(g, w), (e, key, "first difference at step", int(np.flatnonzero(g != w)[0]))
    _check(env, T // LAUNCH - 1, "traced")


def _same(env, e, o, where):
    basis, pairs, order = env.state(e)
    assert len(basis) == o.nG, (where, e)
    assert np.array_equal(order, o.reducer_order()), (where, e, "reducer order")
    assert np.array_equal(pairs, o.pairs()), (where, e, "pairs")
    got = np.concatenate([poly_words(c, x) for c, x in basis])
    assert np.array_equal(got, np.concatenate([poly_words(*o.poly(i)) for i in range(o.nG)])), (where, e, "basis")


def test_values_from_every_cut():
    """value() rollouts (the class's value kernel) under 'first' and 'degree' from the state after every 32 steps: each runs
    its episode to the end on a copy of the state — bases of 64 and more elements among them — and returns what the oracle's
    value() returns from the same state; the batch itself is where the oracle is."""
    env = _env()
    for c in range(T // CUT):
        env.rollout("random", CUT, auto_reset=True)
        for strategy in ("first", "degree"):
            got = env.values(strategy, 0.99)
            for e, sa in enumerate(SEEDS):
                assert got[e] == walk(*sa)[3][c].value(strategy, 0.99), (c, strategy, e)
    _check(env, T // LAUNCH - 1, "valued")


@pytest.mark.parametrize("start", (0, 64, 128, 192))
def test_policy_rollout_from_a_cut(start):
    """bbx_policy_rollout_device with a one-layer policy of 64 hidden units, 48 steps from the state `start` hash-agent steps
    in: the environments — replayed on the oracle with the actions the kernel drew — step for step (row count, observation,
    reward, done flag), and the state afterwards: basis, pair list, reducer order."""
    import torch
    nT = 48
    env = _env()
    env.accounting(False)
    if start:
        env.rollout("random", start, auto_reset=True)
    w = pc.make_weights(env.cols, (64,), 2521)
    pol = pc.to_policy(w, "cuda")
    p = pol._fused_weights()
    s = torch.cuda.current_stream().cuda_stream
    u = torch.rand((nT, B), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2522 + start))
    A = torch.zeros((nT, B), dtype=torch.int32, device="cuda"); L = torch.zeros((nT, B), dtype=torch.float32, device="cuda")
    Rw = torch.zeros((nT, B), dtype=torch.float64, device="cuda"); D = torch.zeros((nT, B), dtype=torch.uint8, device="cuda")
    N = torch.zeros((nT, B), dtype=torch.int32, device="cuda")
    O = torch.full((nT, B, R, env.cols), -1, dtype=torch.int32, device="cuda")
    env.policy_rollout_device(p["prepared"], p["hidden"], nT, u, A, L, Rw, D, N, O, R, B * R * env.cols, s)
    env.sync(); torch.cuda.synchronize()
    acts, rews, dones, obs, rows = A.cpu().numpy(), Rw.cpu().numpy(), D.cpu().numpy(), O.cpu().numpy(), N.cpu().numpy()
    assert env.stats()[:, 4].max() == 0
    inserted = 0
    for e, sa in enumerate(SEEDS):
        if start:
            o = walk(*sa)[3][start // CUT - 1].copy()
        else:
            from oracle import ffi
            o = ffi.load("bo").env(DIST); o.seed(sa[0]); o.reset()
        for t in range(nT):
            assert rows[t, e] == o.nP and np.array_equal(obs[t, e, :min(o.nP, R)], o.obs(K)[:R]), (e, t)
            assert 0 <= acts[t, e] < o.nP, (e, t)
            nG = o.nG
            r = o.step(int(acts[t, e]))
            inserted += int(o.nG == nG + 1)
            assert rews[t, e] == r and bool(dones[t, e]) == (o.nP == 0), (e, t)
            if o.nP == 0:
                o.reset()
        _same(env, e, o, ("policy rollout", start))
    assert inserted >= B                                      # (the rollout is about insertions: there are many)
