"""The fast class's step loop has one test per step for everything rare (t_event in bbx_fast.h): the issued steps exhausted,
the 64-step housekeeping (hash refill, priority rotation, time slice), a reset, a mailbox publication.  Here the kernels run
where those events coincide — launches that begin and end on every phase of the 64-step block, episodes that end on the
block's last and first step and on a launch's last issued step, environments that finish or leave the class with steps still
issued, sessions whose calls cross 64 and 128 at different offsets, the host mailbox — against the oracle step for step
(traced kernels) or through counters, final states and outputs (lean kernels).  tests/test_step_events_cpu.py asserts that the
seeds produce these situations."""
import numpy as np
import pytest

from oracle import ffi
from oracle.trace import fnv64, run_trace
from tests.test_gpu_parity import _state_words
from tests.test_step_events_cpu import (ENDS, K, LEAVE_LAUNCHES, LEAVE_SEEDS, MAILBOX_SEED, MAILBOX_STEPS, NO_RESET, SCHEDULE,
                                        TRACED_SEEDS, agent_seeds, traces, walks)
from tests.fast_harness import KEYS, assert_trace_equal, make_env, rollout_buffers, stream

pytestmark = pytest.mark.gpu


def _env(dist, seeds, **kw):
    return make_env(dist, seeds, K, agent=agent_seeds(seeds), **kw)


def _same_outputs(env, out, recs, where):
    """rewards / dones / rows of a host rollout and the observation blocks behind it against the oracle's walk."""
    rew, done, rows = out
    obs = env.observations()
    for e, rec in enumerate(recs):
        if rec["steps"]:
            assert rew[e] == rec["reward"], where + (e, "reward")
        assert bool(done[e]) == rec["done"] and rows[e] == rec["rows"], where + (e, "done / rows", bool(done[e]), rows[e], rec["done"], rec["rows"])
        assert np.array_equal(obs[e][:rec["rows"]].reshape(-1, 6 * K), rec["obs"].reshape(-1, 6 * K)), where + (e, "observation")


@pytest.mark.parametrize("dist", sorted(TRACED_SEEDS))
def test_launch_lengths_against_the_64_step_phase(dist):
    """Consecutive traced launches of 1, 62, 1, 1, 63, 64, 65, 2 and 127 steps: every step against the oracle, and behind every
    launch what the caller finds — with the new episode's rows and observation where the last issued step ended one."""
    seeds = TRACED_SEEDS[dist]
    env = _env(dist, seeds, trace=max(SCHEDULE))
    want, recs = traces(dist, seeds, ENDS[-1]), walks(dist, seeds, SCHEDULE, True)
    t0 = 0
    for i, n in enumerate(SCHEDULE):
        out = env.rollout("random", n, auto_reset=True)
        for e in range(len(seeds)):
            assert_trace_equal(env.trace_read(e, 0, n), want[e], KEYS, (dist, "launch", i, "environment", e), t0, n)
        _same_outputs(env, out, [r[i] for r in recs], (dist, "launch", i))
        t0 += n
    assert (env.stats()[:, 0] == ENDS[-1]).all()
    for e in range(len(seeds)):
        assert np.array_equal(env.state(e)[1], want[e]["final_pairs"]) and np.array_equal(env.state(e)[2], want[e]["final_order"]), (dist, e)


@pytest.mark.parametrize("dist", sorted(NO_RESET))
def test_no_auto_reset_traced(dist):
    """Environments finish in the middle of a launch with steps still issued (one of them with the launch's last step): they
    take no further steps, in that launch or the next, and leave done = 1 with zero rows."""
    seeds, launches = NO_RESET[dist]
    env = _env(dist, seeds, trace=max(launches))
    recs = walks(dist, seeds, launches, False)
    bo = ffi.load("bo")
    want = []
    for s, a in zip(seeds, agent_seeds(seeds)):
        o = bo.env(dist); o.seed(s)
        want.append(run_trace(o, K, 0, "hash", agent_seed=a, until_done=True))
    t0 = [0] * len(seeds)
    for i, n in enumerate(launches):
        out = env.rollout("random", n, auto_reset=False)
        for e in range(len(seeds)):
            took = recs[e][i]["steps"]
            assert_trace_equal(env.trace_read(e, 0, max(took, 1))[:took], want[e], KEYS, (dist, "launch", i, "environment", e), t0[e], took)
            t0[e] += took
        _same_outputs(env, out, [r[i] for r in recs], (dist, "launch", i))
        assert np.array_equal(env.stats()[:, 0], np.array([r[i]["total"] for r in recs])), (dist, i)
    assert np.array_equal(env.stats()[:, 0], np.array([len(w["action"]) for w in want]))
    assert (env.stats()[:, 2] == 1).all() and (env.rows == 0).all()


def _lean_check(env, want):
    st = env.stats()
    assert (st[:, 4] == 0).all(), st[:, 4]
    for key, col in (("steps", 0), ("additions", 1), ("episodes", 2), ("zero_reductions", 3), ("nG", 7)):
        assert np.array_equal(st[:, col], np.array([r[key] for r in want])), (key, st[:, col], [r[key] for r in want])
    for e in range(len(want)):
        basis, pairs, order = env.state(e)
        assert fnv64(_state_words(basis, pairs, order)) == want[e]["state_hash"], e


@pytest.mark.parametrize("dist", sorted(NO_RESET))
def test_no_auto_reset_lean(dist):
    import torch
    seeds, launches = NO_RESET[dist]
    B = len(seeds)
    env = _env(dist, seeds, lean=True)
    recs = walks(dist, seeds, launches, False)
    rows = torch.zeros(B, dtype=torch.int32, device="cuda"); done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    s = stream()
    bo = ffi.load("bo")
    total = 0
    for i, n in enumerate(launches):
        env.rollout_device("random", n, False, s, dones=done, rows=rows)
        env.sync()
        total += n
        assert np.array_equal(rows.cpu().numpy(), np.array([r[i]["rows"] for r in recs])), (dist, i)
        assert np.array_equal(done.cpu().numpy().astype(bool), np.array([r[i]["done"] for r in recs])), (dist, i)
        _lean_check(env, bo.run_random_many(dist, K, seeds, agent_seeds(seeds), total, False, 0))
        assert np.array_equal(env.stats()[:, 0], np.array([r[i]["total"] for r in recs])), (dist, i)


def test_leaving_the_class_in_the_middle_of_a_launch():
    """A register/LDS class capped at 16 basis elements, launches of 100 steps: the hand-off to the binomial pass where an
    environment outgrows the class, and its return when the episode ends, step for step."""
    dist, T = "3-20-10-weighted", sum(LEAVE_LAUNCHES)
    env = _env(dist, LEAVE_SEEDS, caps={"lds_max_basis": 16}, trace=max(LEAVE_LAUNCHES))
    want, recs = traces(dist, LEAVE_SEEDS, T), walks(dist, LEAVE_SEEDS, LEAVE_LAUNCHES, True)
    t0 = 0
    for i, n in enumerate(LEAVE_LAUNCHES):
        out = env.rollout("random", n, auto_reset=True)
        for e in range(len(LEAVE_SEEDS)):
            assert_trace_equal(env.trace_read(e, 0, n), want[e], KEYS, ("launch", i, "environment", e), t0, n)
        _same_outputs(env, out, [r[i] for r in recs], ("launch", i))
        t0 += n
    assert (env.stats()[:, 0] == T).all()


SESSIONS = {"10x20": [20] * 10, "3x64": [64] * 3, "70x1": [1] * 70, "1x200": [200]}


@pytest.mark.parametrize("name", sorted(SESSIONS))
def test_persistent_sessions_across_the_phase(name):
    """The lean headline shape (hash agent, the observation written after every step, rows / rewards / dones buffers) in
    persistent sessions whose calls cross 64 and 128 at different offsets, one with a join in the middle: counters, final
    states and row counts are the oracle's, and every output equals that of the same calls as separate launches."""
    import torch
    dist, B, R = "3-20-10-weighted", 64, 256
    calls = SESSIONS[name]
    seeds = tuple(range(3000, 3000 + B))
    bo = ffi.load("bo")
    want = bo.run_random_many(dist, K, seeds, agent_seeds(seeds), sum(calls), True, 0)
    s = stream()
    outs = []
    for persistent in (True, False):
        env = _env(dist, seeds, lean=True, persistent=persistent)
        rew, done, rows, obs = rollout_buffers(B, R, env.cols, fill=0)
        for i, n in enumerate(calls):
            env.rollout_device("random", n, True, s, rew, done, rows, obs, R, False, True)
            if name == "10x20" and i == 4:                     # (100 steps issued: the join falls between 64 and 128)
                env.join(s)
        env.sync()
        if persistent:
            assert env.session_stats()["sessions"] >= 1, env.session_stats()
        _lean_check(env, want)
        assert np.array_equal(rows.cpu().numpy(), np.array([r["nP"] for r in want]))
        live = (torch.arange(R, device="cuda")[None, :] < rows[:, None]).cpu().numpy()
        outs.append([rew.cpu().numpy(), done.cpu().numpy(), rows.cpu().numpy(), obs.cpu().numpy()[live], np.delete(env.stats(), 6, axis=1)])
    for a, b, what in zip(outs[0], outs[1], ("rewards", "dones", "rows", "observations", "stats")):
        assert np.array_equal(a, b), (name, what)


def test_host_mailbox_steps():
    """One environment stepped from the host with plain step() calls: the instantiation whose every loop top has duties (the
    per-step publication).  Reward, done flag and row count of each of 130 steps against the oracle."""
    from deepgroebner_amd import VecLeadMonomialsEnv
    bo = ffi.load("bo")
    dist = "3-20-10-weighted"
    env = VecLeadMonomialsEnv(dist, batch=1, k=K)
    env.seed(np.array([MAILBOX_SEED])); env.accounting(False)
    states = env.reset()
    o = bo.env(dist); o.seed(MAILBOX_SEED); o.reset()
    for t in range(MAILBOX_STEPS):
        assert len(states[0]) == o.nP, t
        a = ffi.agent_hash(1, t) % o.nP
        states, rew, done, _ = env.step(np.array([a], dtype=np.int32), auto_reset=True)
        assert rew[0] == o.step(a), t
        assert bool(done[0]) == (o.nP == 0), t
        if o.nP == 0:
            o.reset()
        assert int(env.rows[0]) == o.nP and np.array_equal(states[0], o.obs(K)), t
    ss = env.session_stats()
    assert ss["sessions"] >= 1 and ss["joined"] > MAILBOX_STEPS // 2, ss
