"""The episode step limit inside the step kernels (bbx_episode_limit): every kernel class against the limited walk on the oracle
(tests/episode_limit_cases.py; tests/test_episode_limit_cpu.py asserts that the pinned seeds show cuts, ordinary ends, ordinary
ends on exactly the limit-th step and a limit that never bites).  Traced launches field for field; the lean kernels through
device buffers; the fused policy rollouts by replaying the actions they recorded; sessions and the host mailbox; limits that
change nothing or change under a running episode; the value calls, which ignore the limit; copies and clones; evaluate_policy."""
import numpy as np
import pytest

from oracle import ffi
from oracle.trace import poly_words
from tests.action_value_cases import call as av_call, oracle_action_values, same_block
from tests.episode_limit_cases import CASES, K, PIECE, Walk, agent_seeds, case_walks, limited_walk
from tests.fast_harness import KEYS, assert_trace_equal, make_env, rollout_buffers, stream

pytestmark = pytest.mark.gpu
CASE_LIMITS = [(name, limit) for name in CASES for limit in CASES[name]["limits"]]
GAMMA = 0.99


def _env(name, limit, trace=0, lean=False):
    c = CASES[name]
    return make_env(c["dist"], c["seeds"], K, caps=c["caps"], trace=trace, lean=lean and "before reset", agent=agent_seeds(c["seeds"]),
                    max_episode_length=limit or None)


def _same_end(env, want, where):
    """final state (basis, pairs, reducer order), observation, episode_counts() and the steps of the running episode"""
    obs = env.observations(max_rows=max(1, max(len(w["final_pairs"]) for w in want)))   # (the padded block: env.rows may be out of date)
    ep, tr = env.episode_counts()
    for e, w in enumerate(want):
        basis, pairs, order = env.state(e)
        assert np.array_equal(pairs, w["final_pairs"]) and np.array_equal(order, w["final_order"]), where + (e, "pairs / reducer order")
        words = [poly_words(c, x) for c, x in basis]
        assert np.array_equal(np.concatenate(words) if words else np.zeros(0, np.int32), w["final_basis"]), where + (e, "basis")
        n = len(w["final_pairs"])
        assert np.array_equal(np.asarray(obs[e])[:n].reshape(n, -1), w["final_obs"].reshape(n, -1)), where + (e, "observation")
        assert (int(ep[e]), int(tr[e])) == (w["episodes"], w["truncations"]), where + (e, "episodes / truncations", int(ep[e]), int(tr[e]))
    assert np.array_equal(env.stats()[:, 2], ep)              # bbx_stats' episode column is the same counter


@pytest.mark.parametrize("name,limit", CASE_LIMITS)
def test_traced_launches(name, limit):
    """One traced launch of the case's steps, and the same steps in traced launches of 7 (launches begin inside episodes, the
    count crosses launches): every trace field, the final state, the observation and the counters against the walk."""
    T = CASES[name]["steps"]
    want = case_walks(name, limit)
    env = _env(name, limit, trace=T)
    env.rollout("random", T, auto_reset=True)
    for e, w in enumerate(want):
        assert_trace_equal(env.trace_read(e, 0, T), w, KEYS, (name, limit, "one launch", e), 0, T)
    _same_end(env, want, (name, limit, "one launch"))
    env = _env(name, limit, trace=PIECE)
    for t0 in range(0, T, PIECE):
        n = min(PIECE, T - t0)
        env.rollout("random", n, auto_reset=True)
        for e, w in enumerate(want):
            assert_trace_equal(env.trace_read(e, 0, n), w, KEYS, (name, limit, "launches of 7", e), t0, n)
    _same_end(env, want, (name, limit, "launches of 7"))


@pytest.mark.parametrize("name,limit", CASE_LIMITS)
def test_lean_launches_through_device_buffers(name, limit):
    """The lean kernels (no trace, no accounting; with a limit set the fast class runs its general lean kernel, not the headline
    one) in two launches on caller buffers, the observation written at every step: rewards, dones, rows and the observation
    behind each launch, then the final state and the counters."""
    T = CASES[name]["steps"]
    B, R = len(CASES[name]["seeds"]), 1024
    env = _env(name, limit, lean=True)
    s = stream()
    rew, done, rows, obs = rollout_buffers(B, R, env.cols, fill=0)
    n1 = T // 2 + 1
    for upto, n in ((n1, n1), (T, T - n1)):
        env.rollout_device("random", n, True, s, rew, done, rows, obs, R, False, True)
        env.sync()
        want = case_walks(name, limit, upto)
        for e, w in enumerate(want):
            nP = len(w["final_pairs"])
            assert int(rows[e]) == nP and float(rew[e]) == w["reward"][-1] and int(done[e]) == w["done"][-1], (name, limit, upto, e)
            assert np.array_equal(obs[e, :nP].cpu().numpy(), w["final_obs"].reshape(nP, -1)), (name, limit, upto, e, "observation")
    assert set(done.cpu().numpy().tolist()) <= {0, 1}
    _same_end(env, case_walks(name, limit, T), (name, limit, "lean"))


def _policy(cols, hidden, seed):
    import torch
    from deepgroebner_amd.rollout import PMLPPolicy
    torch.manual_seed(seed)
    policy = PMLPPolicy(cols, list(hidden)).cuda()
    with torch.no_grad():
        for lin in list(policy.embedding) + [policy.deciding]:
            lin.weight.mul_(0.3)
    return policy


@pytest.mark.parametrize("name,hidden", [("fast", (64,)), ("fast", (64, 64)), ("binom_hbm", (64,))])
def test_fused_policy_rollouts_replayed_on_the_walk(name, hidden):
    """bbx_policy_rollout_device / bbx_policy2_rollout_device with the case's mid-size limit, in two launches: the actions the
    call recorded are replayed on the limited walk — per-step rewards, dones and rows, the final state and the counters must be
    the walk's, whatever the policy's arithmetic made of its logits."""
    import torch
    c = CASES[name]
    T, B, limit = c["steps"], len(c["seeds"]), c["limits"][-2]
    env = _env(name, limit, lean=True)
    policy = _policy(env.cols, hidden, 5)
    s = stream()
    u = torch.rand((T, B), device="cuda")
    A = torch.zeros((T, B), dtype=torch.int32, device="cuda"); L = torch.zeros((T, B), dtype=torch.float32, device="cuda")
    Rw = torch.zeros((T, B), dtype=torch.float64, device="cuda"); D = torch.full((T, B), 9, dtype=torch.uint8, device="cuda")
    N = torch.zeros((T, B), dtype=torch.int32, device="cuda")
    if len(hidden) == 1:
        w = policy._fused_weights()
        go = lambda a, b: env.policy_rollout_device(w["prepared"], w["hidden"], b - a, u[a:b], A[a:b], L[a:b], Rw[a:b], D[a:b], N[a:b], None, 1024, 0, s)
    else:
        w = policy._deep_weights()
        go = lambda a, b: env.policy2_rollout_device(w["prepared"], w["hidden"][0], w["hidden"][1], b - a, u[a:b], A[a:b], L[a:b], Rw[a:b], D[a:b],
                                                     N[a:b], None, 1024, 0, s)
    cut = T // 3 + 1
    go(0, cut); env.sync()
    go(cut, T); env.sync()
    acts = A.cpu().numpy()
    want = [limited_walk(c["dist"], seed, 0, limit, T, actions=acts[:, e]) for e, seed in enumerate(c["seeds"])]
    for e, wk in enumerate(want):
        assert np.array_equal(N[:, e].cpu().numpy(), wk["rows_before"]), (name, hidden, e, "rows")
        assert np.array_equal(Rw[:, e].cpu().numpy(), wk["reward"]), (name, hidden, e, "rewards")
        assert np.array_equal(D[:, e].cpu().numpy(), wk["done"].astype(np.uint8)), (name, hidden, e, "dones")
    assert sum(int((wk["end"] == 2).sum()) for wk in want) > 0          # the limit did cut episodes of this rollout
    _same_end(env, want, (name, hidden))


def test_session_calls_equal_separate_launches():
    """bbx_persistent(1): six rollout_device calls of 20 steps with limit 3 against the same calls as separate launches, bit for
    bit, and both against the walk's counters."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    dist, B, R, limit, calls = "3-20-10-weighted", 64, 256, 3, [20] * 6
    seeds = tuple(range(3000, 3000 + B))
    s = stream()
    outs = []
    for persistent in (True, False):
        env = VecLeadMonomialsEnv(dist, batch=B, k=K, max_episode_length=limit)
        env.seed(np.array(seeds)); env.seed_agent(np.array(agent_seeds(seeds))); env.accounting(False); env.reset()
        env.persistent(persistent)
        rew, done, rows, obs = rollout_buffers(B, R, env.cols, fill=0)
        for n in calls:
            env.rollout_device("random", n, True, s, rew, done, rows, obs, R, False, True)
        env.sync()
        if persistent:
            assert env.session_stats()["sessions"] >= 1, env.session_stats()
        live = (torch.arange(R, device="cuda")[None, :] < rows[:, None]).cpu().numpy()
        ep, tr = env.episode_counts()
        outs.append([rew.cpu().numpy(), done.cpu().numpy(), rows.cpu().numpy(), obs.cpu().numpy()[live], np.delete(env.stats(), 6, axis=1), ep, tr])
    for a, b, what in zip(outs[0], outs[1], ("rewards", "dones", "rows", "observations", "stats", "episodes", "truncations")):
        assert np.array_equal(a, b), what
    for e in (0, 1, B - 1):
        w = limited_walk(dist, seeds[e], agent_seeds(seeds)[e], limit, sum(calls))
        assert (int(outs[0][5][e]), int(outs[0][6][e])) == (w["episodes"], w["truncations"]) and w["truncations"] > 0, e


MBOX_SEEDS, MBOX_LIMIT, MBOX_STEPS = (3000, 3001), 7, 20


def _mailbox_env(auto_reset):
    from deepgroebner_amd import VecLeadMonomialsEnv
    dist = "3-20-10-weighted"
    env = VecLeadMonomialsEnv(dist, batch=len(MBOX_SEEDS), k=K, max_episode_length=MBOX_LIMIT)
    env.seed(np.array(MBOX_SEEDS)); env.accounting(False)
    states = env.reset()
    return env, states, [Walk(dist, s, MBOX_LIMIT, auto_reset) for s in MBOX_SEEDS]


def test_mailbox_loop_with_auto_reset():
    """20 step() calls on a batch of two with limit 7 (a loop of host steps becomes a mailbox session on the resident kernel):
    reward, done, rows and the observation of every step against the walk — behind a cut, the new episode's."""
    env, states, walks = _mailbox_env(True)
    for t in range(MBOX_STEPS):
        acts = [ffi.agent_hash(e + 1, t) % w.o.nP for e, w in enumerate(walks)]
        states, rew, done, infos = env.step(np.array(acts, dtype=np.int32), auto_reset=True)
        for e, w in enumerate(walks):
            r, end = w.step(acts[e])
            assert rew[e] == r and bool(done[e]) == (end != 0), (t, e)
            w.after(end)
            assert int(env.rows[e]) == w.o.nP and np.array_equal(states[e], w.o.obs(K)), (t, e)
            assert infos[e] == {}
    assert all(w.truncations >= 2 for w in walks)
    ep, tr = env.episode_counts()
    assert [(int(a), int(b)) for a, b in zip(ep, tr)] == [(w.episodes, w.truncations) for w in walks]
    assert env.session_stats()["sessions"] >= 1, env.session_stats()


def test_mailbox_loop_without_auto_reset():
    """The same loop without auto-reset: the 7th step reports done with {"truncated": True}, stepping on keeps reporting done,
    the state is the one the steps leave, and the counters moved once."""
    env, states, walks = _mailbox_env(False)
    for t in range(12):
        acts = [ffi.agent_hash(e + 1, t) % w.o.nP for e, w in enumerate(walks)]
        states, rew, done, infos = env.step(np.array(acts, dtype=np.int32), auto_reset=False)
        for e, w in enumerate(walks):
            r, end = w.step(acts[e])
            assert w.o.nP > 0 and end == (2 if t + 1 >= MBOX_LIMIT else 0)                   # (the seeds: no ordinary end in these steps)
            assert rew[e] == r and bool(done[e]) == (t + 1 >= MBOX_LIMIT), (t, e)
            assert infos[e] == ({"truncated": True} if t + 1 >= MBOX_LIMIT else {}), (t, e, infos[e])
            assert int(env.rows[e]) == w.o.nP and np.array_equal(states[e], w.o.obs(K)), (t, e)
    ep, tr = env.episode_counts()
    assert ep.tolist() == [1, 1] and tr.tolist() == [1, 1] and all((w.episodes, w.truncations) == (1, 1) for w in walks)


@pytest.mark.parametrize("name", [n for n in CASES if len(CASES[n]["limits"]) > 1])
def test_a_limit_larger_than_every_episode_changes_nothing(name):
    T = CASES[name]["steps"]
    free, off = _env(name, CASES[name]["limits"][-1], trace=T), _env(name, 0, trace=T)
    free.rollout("random", T, auto_reset=True); off.rollout("random", T, auto_reset=True)
    for e in range(len(CASES[name]["seeds"])):
        assert free.trace_read(e, 0, T).tobytes() == off.trace_read(e, 0, T).tobytes(), (name, e)
    assert np.array_equal(np.delete(free.stats(), 6, axis=1), np.delete(off.stats(), 6, axis=1))
    assert free.episode_counts()[1].sum() == 0 and off.episode_counts()[1].sum() == 0


@pytest.mark.parametrize("name", ["fast", "general"])
def test_lowering_the_limit_under_a_running_episode(name):
    """10 steps under a limit nothing reaches, then limit 4: an episode that has 4 steps or more is cut at its next step."""
    c = CASES[name]
    n1, n2, low = 10, 9, 4
    env = _env(name, 1000, trace=n1)
    walks = [Walk(c["dist"], s, 1000) for s in c["seeds"]]
    recs = [[] for _ in walks]
    t = 0
    for n, limit in ((n1, 1000), (n2, low)):
        assert env.episode_limit(limit) == 1000              # (the value it had: set at creation, unchanged by the first call)
        env.rollout("random", n, auto_reset=True)
        for e, (w, a) in enumerate(zip(walks, agent_seeds(c["seeds"]))):
            w.limit = limit
            got = env.trace_read(e, 0, n)
            for i in range(n):
                over = w.episode_steps >= low
                r, end = w.step(ffi.agent_action(a, t + i, w.o.nP))
                assert (float(got["reward"][i]), int(got["rows"][i]), int(got["done"][i])) == (r, w.o.nP, int(end != 0)), (name, e, t + i)
                if limit == low and i == 0 and over and w.o.nP:
                    assert end == 2
                    recs[e].append(t + i)
                w.after(end)
        t += n
    assert any(recs), name                                   # some environment entered the second launch past the new limit
    ep, tr = env.episode_counts()
    assert [(int(a), int(b)) for a, b in zip(ep, tr)] == [(w.episodes, w.truncations) for w in walks]


def test_a_limit_set_behind_headline_launches_counts_from_there():
    """The headline-shaped lean kernels keep no step count per episode: a limit set after such a launch starts the episodes
    under way at count 0 (include/bbx.h), whatever the header held — the walk does the same."""
    c = CASES["fast"]
    B, R, n1, n2, limit = len(c["seeds"]), 256, 30, 13, 5
    env = _env("fast", 0, lean=True)
    s = stream()
    rew, done, rows, obs = rollout_buffers(B, R, env.cols, fill=0)
    env.rollout_device("random", n1, True, s, rew, done, rows, obs, R, False, True)      # the headline shape, limit off
    env.sync()
    assert env.episode_limit(limit) is None
    env.rollout_device("random", n2, True, s, rew, done, rows, obs, R, False, True)
    env.sync()
    ep, tr = env.episode_counts()
    for e, (seed, a) in enumerate(zip(c["seeds"], agent_seeds(c["seeds"]))):
        w = Walk(c["dist"], seed, 0)
        for t in range(n1 + n2):
            if t == n1:
                w.limit, w.episode_steps = limit, 0
            end = w.step(ffi.agent_action(a, t, w.o.nP))[1]
            w.after(end)
        assert (int(ep[e]), int(tr[e]), int(rows[e]), int(done[e])) == (w.episodes, w.truncations, w.o.nP, int(end != 0)), e
        assert np.array_equal(env.state(e)[1], w.o.pairs()), e
    assert tr.sum() > 0


def test_value_calls_ignore_the_limit_and_copies_carry_it():
    """values('degree') and action_values('degree') with a limit set are the oracle's unlimited values and leave the counters
    alone; copy() carries count and limit, clone_envs the count."""
    name, limit, n1, n2 = "fast", 5, 13, 11
    c = CASES[name]
    env = _env(name, limit)
    env.rollout("random", n1, auto_reset=True)
    walks = [Walk(c["dist"], s, limit) for s in c["seeds"]]
    for w, a in zip(walks, agent_seeds(c["seeds"])):
        for t in range(n1):
            w.after(w.step(ffi.agent_action(a, t, w.o.nP))[1])
    before = env.episode_counts()
    assert np.array_equal(env.values("degree", GAMMA), np.array([w.o.value("degree", GAMMA) for w in walks]))
    rc, q, r, d, rows = av_call(env, "degree", GAMMA)
    assert rc == 0
    for e, w in enumerate(walks):
        wq, wr, wd = oracle_action_values(w.o, "degree", GAMMA)
        n = w.o.nP
        assert rows[e] == n and same_block(q[e, :n], wq) and np.array_equal(r[e, :n], wr) and np.array_equal(d[e, :n], wd), e
    after = env.episode_counts()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert [(int(a), int(b)) for a, b in zip(*after)] == [(w.episodes, w.truncations) for w in walks]
    twin = env.copy()
    assert twin.episode_limit(limit) == limit                # the handle's limit came with the copy
    env.clone_envs([0], [1])                                  # environment 1 becomes environment 0, count and all
    walks[1] = None
    for h in (env, twin):
        h.rollout("random", n2, auto_reset=True)
    for e, (w, a) in enumerate(zip(list(walks), agent_seeds(c["seeds"]))):
        if w is None:
            continue
        for t in range(n1, n1 + n2):
            w.after(w.step(ffi.agent_action(a, t, w.o.nP))[1])
    ep, tr = env.episode_counts()
    tep, ttr = twin.episode_counts()
    for e, w in enumerate(walks):
        if w is None:
            assert (int(ep[1]), int(tr[1])) == (int(ep[0]), int(tr[0])) and np.array_equal(env.state(1)[1], env.state(0)[1])
            continue
        assert (int(ep[e]), int(tr[e])) == (w.episodes, w.truncations), e
        assert np.array_equal(env.state(e)[1], w.o.pairs()), e
        if e != 1:
            assert (int(tep[e]), int(ttr[e])) == (w.episodes, w.truncations) and np.array_equal(twin.state(e)[1], w.o.pairs()), e
    assert tr.sum() > 0


def test_evaluate_policy_with_a_cap():
    """evaluate_policy(..., max_episode_length=L): no length above L, some episode cut at L, the handle's limit restored."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    from deepgroebner_amd.rollout import evaluate_policy
    B, L = 16, 6
    env = VecLeadMonomialsEnv("3-20-10-weighted", batch=B, k=K)
    env.seed(np.arange(B) + 50)
    assert env.episode_limit(11) is None
    ev = evaluate_policy(env, _policy(env.cols, (64,), 1), 3, chunk=16, max_episode_length=L)
    lengths = ev.lengths.cpu().numpy()
    assert ev.complete and lengths.shape == (B, 3) and (lengths >= 1).all() and (lengths <= L).all() and (lengths == L).any()
    assert torch.isfinite(ev.returns).all()
    assert env.episode_limit(None) == 11                      # restored
    assert env.episode_counts()[1].sum() > 0
