"""The fast class's working copy of a basis element's info (bbx_fast.h: gi[] holds tc/lc and -tc/lc, the S-polynomial's two
coefficients, formed when the element enters; gc[] keeps the record's word lc | tc << 16 for the write-back) through every
kernel of the class: traced, lean headline (single launches and a persistent session), generic lean, value, policy rollout
(the two-bank layout), with the class capped so that records travel to the HBM-resident class and back, from records the
class did not just write (copy(), clone_envs), and beyond 128 reducers, where the reducer words are rebuilt from gc[].
Eight environments, 128 steps; the seeds select elements without a tail as first and as second member of a pair and pairs
of two scaled elements with tails (tests/test_spoly_coef_cpu.py asserts that).  Everything against the oracle; the basis
term for term after each run is what shows that gc[] restores lead and tail coefficient."""
import numpy as np
import pytest

from oracle import ffi
from oracle.trace import poly_words, run_trace
from tests import policy_cases as pc
from tests.test_spoly_coef_cpu import DIST, K, SEEDS, T, walk

pytestmark = pytest.mark.gpu
KEYS = (("action", "action"), ("reward", "reward"), ("rows", "nP"), ("basis_size", "nG"), ("done", "done"), ("obs_hash", "obs_hash"),
        ("pairs_hash", "pairs_hash"), ("newpoly_hash", "newpoly_hash"))
B = len(SEEDS)
CAPS = (None, {"lds_max_basis": 16})          # the second: records written by the class are read by the HBM-resident one and handed back
CAP_IDS = ("default", "lds16")
R = 256


def _env(trace=0, caps=None, extra=()):
    from deepgroebner_amd import VecLeadMonomialsEnv
    seeds = list(SEEDS) + list(extra)
    env = VecLeadMonomialsEnv(DIST, batch=len(seeds), k=K, caps=caps)
    env.seed(np.array([s for s, _ in seeds]))
    env.seed_agent(np.array([a for _, a in seeds]))
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


def _same_state(env, where, envs=range(B)):
    """basis term for term, pair list and reducer order against the oracle after T steps (environment e runs SEEDS[e % B])"""
    for e in envs:
        _same(env, e, walk(*SEEDS[e % B])[0], where)


def _buffers(n):
    import torch
    return (torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"),
            torch.zeros(n, dtype=torch.int32, device="cuda"), torch.full((n, R, 4 * 3), -1, dtype=torch.int32, device="cuda"))


def _same_outputs(bufs, envs=range(B)):
    rew, done, rows, obs = (x.cpu().numpy() for x in bufs)
    for e in envs:
        o, rewards, dones, _, _ = walk(*SEEDS[e % B])
        assert rew[e] == rewards[-1] and bool(done[e]) == bool(dones[-1]) and rows[e] == o.nP, e
        assert np.array_equal(obs[e, :o.nP], o.obs(K)), e


@pytest.mark.parametrize("caps", CAPS, ids=CAP_IDS)
def test_traced_rollout_step_for_step(caps):
    env = _env(trace=T, caps=caps)
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


@pytest.mark.parametrize("caps", CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("kernel", ("headline", "headline-session", "generic"))
def test_lean_rollout_device(kernel, caps):
    """The lean headline shape (hash agent, the observation written after every step, no fill) as two launches of 64 steps and
    as one persistent session of two calls; with obs_fill on the launcher takes the generic lean kernel instead."""
    import torch
    env = _env(caps=caps)
    env.accounting(False)
    env.persistent(kernel == "headline-session")
    s = torch.cuda.current_stream().cuda_stream
    rew, done, rows, obs = bufs = _buffers(B)
    for n in (T // 2, T - T // 2):
        env.rollout_device("random", n, True, s, rew, done, rows, obs, R, kernel == "generic", True)
    env.sync()
    if kernel == "headline-session":
        assert env.session_stats()["sessions"] >= 1, env.session_stats()
    st = env.stats()
    assert (st[:, 0] == T).all() and (st[:, 4] == 0).all(), st
    _same_state(env, (kernel, caps))
    _same_outputs(bufs)
    for e, sa in enumerate(SEEDS):
        o, rewards, dones, _, _ = walk(*sa)
        assert st[e, 1] == int(np.sum(-rewards)) and st[e, 2] == int(dones.sum()), (e, st[e])
    if kernel == "generic":                                  # (the fill: -1 behind the live rows)
        got, nrows = obs.cpu().numpy(), rows.cpu().numpy()
        assert all((got[e, nrows[e]:] == -1).all() for e in range(B))


@pytest.mark.parametrize("caps", CAPS, ids=CAP_IDS)
def test_values_before_and_after_the_rollout(caps):
    """value() rollouts (the class's value kernel) from the reset state and from the state 128 steps later"""
    env = _env(caps=caps)
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
    _same_state(env, ("valued", caps))


CUT = 40


def test_copy_taken_mid_episode():
    """copy() at step 40: the copy stages records in that it never wrote; both batches stepped on to 128."""
    import torch
    env = _env()
    env.accounting(False)
    s = torch.cuda.current_stream().cuda_stream
    ebufs, tbufs = _buffers(B), _buffers(B)
    env.rollout_device("random", CUT, True, s, *ebufs, R, False, True)
    env.sync()
    for e, sa in enumerate(SEEDS):
        _same(env, e, walk(sa[0], sa[1], CUT)[0], "at the cut")
    twin = env.copy()
    twin.accounting(False)
    for batch, bufs in ((env, ebufs), (twin, tbufs)):
        batch.rollout_device("random", T - CUT, True, s, *bufs, R, False, True)
        batch.sync()
    for batch, bufs, name in ((env, ebufs, "source"), (twin, tbufs, "copy")):
        _same_state(batch, name)
        _same_outputs(bufs)


def test_clones_taken_mid_episode():
    """clone_envs at step 40 over eight environments that ran other ideals: source and clone stepped on to 128."""
    import torch
    env = _env(extra=[(s + 400, a + 400) for s, a in SEEDS])
    env.accounting(False)
    s = torch.cuda.current_stream().cuda_stream
    bufs = _buffers(2 * B)
    env.rollout_device("random", CUT, True, s, *bufs, R, False, True)
    env.sync()
    env.clone_envs(list(range(B)), list(range(B, 2 * B)))
    for e in range(2 * B):
        _same(env, e, walk(*SEEDS[e % B], CUT)[0], "cloned")
    env.rollout_device("random", T - CUT, True, s, *bufs, R, False, True)
    env.sync()
    _same_state(env, "clones", range(2 * B))
    _same_outputs(bufs, range(2 * B))


@pytest.mark.parametrize("persistent", (False, True))
def test_reducers_beyond_the_registers(persistent):
    """3-20-140-weighted: 140 generators, so reducers 128.. exist as an order only and their words (tc | -tc/lc << 16) are
    rebuilt from gc[] and gi[] — in the reduction when one of them divides, and at every write-back.  Two environments, 16
    steps in launches of 4; state (reducer order included) and observation against the oracle."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    dist, nB, nT, rows_cap = "3-20-140-weighted", 2, 16, 2048
    bo = ffi.load("bo")
    env = VecLeadMonomialsEnv(dist, batch=nB, k=K)
    env.seed(np.arange(nB) + 700); env.seed_agent(np.arange(nB)); env.reset()
    env.accounting(False)
    env.persistent(persistent)
    s = torch.cuda.current_stream().cuda_stream
    rew = torch.zeros(nB, dtype=torch.float64, device="cuda"); done = torch.zeros(nB, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(nB, dtype=torch.int32, device="cuda")
    obs = torch.zeros((nB, rows_cap, env.cols), dtype=torch.int32, device="cuda")
    for _ in range(nT // 4):
        env.rollout_device("random", 4, True, s, rew, done, rows, obs, rows_cap, False, True)
    env.sync()
    assert (env.stats()[:, 4] == 0).all(), env.stats()
    got_rows, got_obs, got_rew = rows.cpu().numpy(), obs.cpu().numpy(), rew.cpu().numpy()
    for e in range(nB):
        o = bo.env(dist); o.seed(700 + e); o.reset()
        assert o.nG > 128
        for t in range(nT):
            r = o.step(ffi.agent_action(e, t, o.nP))
            assert o.nP > 0                                  # (no episode of these ends within 16 steps)
        _same(env, e, o, ("beyond the registers", persistent))
        assert got_rew[e] == r and got_rows[e] == o.nP and o.nP <= rows_cap
        assert np.array_equal(got_obs[e, :o.nP], o.obs(K)), e


def test_policy_rollout_two_bank_layout():
    """bbx_policy_rollout_device with a one-layer policy of 64 hidden units (the class's two-bank LDS layout), 32 steps: the
    draws against the float64 reference and the torch module, the environments — replayed on the oracle with the actions the
    kernel drew — step for step: observation, row count, reward, done flag; the state afterwards."""
    import torch
    nT = 32
    env = _env()
    env.accounting(False)
    w = pc.make_weights(env.cols, (64,), 911)
    pol = pc.to_policy(w, "cuda")
    p = pol._fused_weights()
    s = torch.cuda.current_stream().cuda_stream
    u = torch.rand((nT, B), device="cuda", generator=torch.Generator(device="cuda").manual_seed(912))
    A = torch.zeros((nT, B), dtype=torch.int32, device="cuda"); L = torch.zeros((nT, B), dtype=torch.float32, device="cuda")
    Rw = torch.zeros((nT, B), dtype=torch.float64, device="cuda"); D = torch.zeros((nT, B), dtype=torch.uint8, device="cuda")
    N = torch.zeros((nT, B), dtype=torch.int32, device="cuda")
    O = torch.full((nT, B, R, env.cols), -1, dtype=torch.int32, device="cuda")
    env.policy_rollout_device(p["prepared"], p["hidden"], nT, u, A, L, Rw, D, N, O, R, B * R * env.cols, s)
    env.sync(); torch.cuda.synchronize()
    for t in range(nT):                                      # the torch path, as tests/test_rollout.py holds the per-step kernel to it
        a_t, l_t = pol.act_torch(O[t], N[t], u[t])
        assert int((A[t] != a_t).sum()) <= 1 and torch.allclose(L[t][A[t] == a_t], l_t[A[t] == a_t], atol=5e-4, rtol=1e-4), t
    obs, rows = O.reshape(nT * B, R, env.cols).cpu().numpy(), N.reshape(-1).cpu().numpy()
    uu, a, l = u.reshape(-1).cpu().numpy(), A.reshape(-1).cpu().numpy(), L.reshape(-1).cpu().numpy()
    ref = pc.reference(w, obs, rows)
    band = pc.check_draws(w, obs, rows, uu, a, l, ref=ref, what="two-bank rollout")
    assert band <= pc.near_boundary(ref, uu), band
    acts, rews, dones = A.cpu().numpy(), Rw.cpu().numpy(), D.cpu().numpy()
    obs, rows = obs.reshape(nT, B, R, env.cols), rows.reshape(nT, B)
    bo = ffi.load("bo")
    assert env.stats()[:, 4].max() == 0
    for e, (seed, _) in enumerate(SEEDS):
        o = bo.env(DIST); o.seed(seed); o.reset()
        for t in range(nT):
            assert rows[t, e] == o.nP and np.array_equal(obs[t, e, :o.nP], o.obs(K)), (e, t)
            r = o.step(int(acts[t, e]))
            assert rews[t, e] == r and bool(dones[t, e]) == (o.nP == 0), (e, t)
            if o.nP == 0:
                o.reset()
        _same(env, e, o, "policy rollout")
