"""The headline shape (hash agent, 3 variables, k = 2, the observation written after every step, auto-reset) through
rollout_device, as bench.py drives it, on the seeds of tests/test_step_prefetch_cpu.py: every seed shows one of the situations
in which a step's front — pair selection and operand reads — depends on what the step or the launch before it left (a reset, a
shifted register copy of the pair list, an element appended a moment ago, more than 64 pairs, a new hash block, the capacity
test).  Persistent sessions and one kernel per launch; final states, counters, rewards, dones, rows and the observation block
against the oracle, exactly."""
import numpy as np
import pytest

from oracle import ffi
from tests.test_step_events_cpu import K, agent_seeds, walks
from tests.test_step_events_gpu import _env, _lean_check
from tests.test_step_prefetch_cpu import CASE_SEEDS, DIST, LAUNCHES, LEAVE_CAP, T, all_seeds
from tests.fast_harness import rollout_buffers, stream

pytestmark = pytest.mark.gpu
R = 128                                              # rows of the caller's observation block (|P| stays below on these seeds)


def _same_as_walk(bufs, recs, where):
    """rewards / dones / rows / observation rows of the caller's buffers against what the oracle's walk says the launch left."""
    rew, done, rows, obs = (x.cpu().numpy() for x in bufs)
    for e, rec in enumerate(recs):
        assert rows[e] == rec["rows"] and bool(done[e]) == rec["done"], where + (e, "rows / done", rows[e], bool(done[e]), rec["rows"], rec["done"])
        assert rew[e] == rec["reward"], where + (e, "reward", rew[e], rec["reward"])
        assert rec["rows"] <= R
        assert np.array_equal(obs[e, :rec["rows"]], rec["obs"].reshape(-1, 6 * K)), where + (e, "observation")


def _run(seeds, caps, persistent, joins):
    """LAUNCHES as consecutive rollout_device calls; outputs are compared wherever the stream is joined (one kernel per launch:
    behind every call)."""
    assert seeds and len(seeds) <= 256
    bo = ffi.load("bo")
    recs = walks(DIST, seeds, LAUNCHES, True)
    s = stream()
    env = _env(DIST, seeds, caps=caps, lean=True, persistent=persistent)
    bufs = rollout_buffers(len(seeds), R, env.cols, fill=-7)
    total = 0
    for i, n in enumerate(LAUNCHES):
        env.rollout_device("random", n, True, s, *bufs, R, False, True)
        total += n
        if not persistent or i in joins:
            if persistent:
                env.join(s)
            env.sync()
            _same_as_walk(bufs, [r[i] for r in recs], ("persistent" if persistent else "launches", "call", i))
            _lean_check(env, bo.run_random_many(DIST, K, seeds, agent_seeds(seeds), total, True, 0))
    env.sync()
    assert total == T
    _same_as_walk(bufs, [r[-1] for r in recs], ("persistent" if persistent else "launches", "end"))
    _lean_check(env, bo.run_random_many(DIST, K, seeds, agent_seeds(seeds), T, True, 0))
    return env


@pytest.mark.parametrize("persistent", [True, False], ids=["session", "launches"])
def test_case_seeds_chained_launches(persistent):
    """Launches of 1, 2, 63, 64, 65 and 125 steps on all case seeds.  In a session the calls are queued behind each other — the
    waves poll for more steps and carry on — with joins behind the third and the fifth call (a stop, then a new session)."""
    env = _run(all_seeds(), None, persistent, joins=(2, 4))
    if persistent:
        assert env.session_stats()["sessions"] >= 1, env.session_stats()


@pytest.mark.parametrize("persistent", [True, False], ids=["session", "launches"])
def test_leaving_the_class_at_the_capacity_test(persistent):
    """A class capped at 16 basis elements: the capacity test in front of a step sends the environment to the HBM-resident
    pass with the record as the oracle has it before that step — the pass continues from it, so any difference shows in the
    states, counters and outputs compared here."""
    _run(CASE_SEEDS["leaves_the_class_at_the_capacity_test"], {"lds_max_basis": LEAVE_CAP}, persistent, joins=(3,))
