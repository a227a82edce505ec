"""The harness of the fast-class twins held to itself, without a device: the state comparison of tests/fast_harness.py must
pass on a batch that IS the oracle's state and fail, naming the part, on each single mutation of it; same_doubles must
reject NaN and shape mismatch; the shared walk of tests/oracle_walk.py must take the steps of a loop written out here."""
import numpy as np
import pytest

from oracle import ffi
from tests import oracle_walk as ow
from tests.fast_harness import assert_same_state, assert_same_states, assert_trace_equal, same_doubles
from tests.test_spoly_order_cpu import KINDS, KNOWN_FIRST, selected_kind

DIST, SEED, ASEED = "3-20-10-weighted", 1000, 7


class Batch:
    """what assert_same_state reads of a VecLeadMonomialsEnv: state(e) -> (basis as [(coefficients, exponents)], pairs, order)"""

    def __init__(self, o):
        self.basis = [tuple(np.array(x) for x in o.poly(i)) for i in range(o.nG)]
        self.pairs, self.order = np.array(o.pairs()), np.array(o.reducer_order())

    def state(self, e):
        return self.basis, self.pairs, self.order


@pytest.fixture()
def oracle():
    return ow.walk(DIST, SEED, ASEED, 16)[0]


def test_the_oracles_own_state_passes(oracle):
    assert oracle.nG >= 4 and oracle.nP >= 2
    assert_same_state(Batch(oracle), 0, oracle, "own")
    assert_same_state(Batch(oracle), 0, ow.snapshot(oracle), "own snapshot")
    assert_same_states(Batch(oracle), [(SEED, ASEED)], lambda s, a: ow.walk(DIST, s, a, 16), "own walk")


def _coefficient(b):
    b.basis[1][0][0] = (int(b.basis[1][0][0]) + 1) % 32003


def _pairs(b):
    assert not np.array_equal(b.pairs[0], b.pairs[1])
    b.pairs[[0, 1]] = b.pairs[[1, 0]]


def _order(b):
    b.order[[0, 1]] = b.order[[1, 0]]


def _dropped(b):
    del b.basis[-1]


@pytest.mark.parametrize("mutate,part", ((_coefficient, "basis"), (_pairs, "pairs"), (_order, "reducer order"), (_dropped, None)),
                         ids=("coefficient", "pair", "reducer-order", "dropped-element"))
def test_every_single_mutation_fails_and_names_its_part(oracle, mutate, part):
    b = Batch(oracle)
    mutate(b)
    with pytest.raises(AssertionError) as ei:
        assert_same_state(b, 3, oracle, "mutated")
    parts = [p for p in ("basis", "pairs", "reducer order") if repr(p) in str(ei.value)]
    assert "'mutated', 3" in str(ei.value) and parts == ([part] if part else []), str(ei.value)   # (a lost element: (where, e) alone)


def test_trace_comparison_names_field_and_step():
    want = {"action": np.arange(8), "reward": -np.ones(8)}
    keys = (("action", "action"), ("reward", "reward"))
    got = {"action": np.arange(2, 6, dtype=np.int32), "reward": -np.ones(4, dtype=np.float32)}
    assert_trace_equal(got, want, keys, 0, 2, 4)
    got["reward"][3] = -2
    with pytest.raises(AssertionError) as ei:
        assert_trace_equal(got, want, keys, ("launch", 1), 2, 4)
    assert "'launch', 1, 'reward', 'first difference at step', 5" in str(ei.value), str(ei.value)


def test_same_doubles():
    a = np.array([1.0, -2.5, 0.0])
    assert same_doubles(a, a.copy()) and same_doubles(a, [1.0, -2.5, 0.0]) and same_doubles(np.zeros(0), np.zeros(0))
    assert not same_doubles(a, a + np.array([0.0, 0.0, 1e-300]))
    assert not same_doubles(np.array([1.0, np.nan]), np.array([1.0, np.nan]))          # NaN nowhere, not even on both sides
    assert not same_doubles(a, a[:2]) and not same_doubles(a, a[None, :]) and not same_doubles(a[:0], a)


class Recorder:
    def __init__(self):
        self.calls = []

    def before(self, o, t, action):
        self.calls.append(("before", t, action, o.nP, o.nG))
        return o.nP

    def after(self, o, t, action, reward):
        self.calls.append(("after", t, action, reward, o.nP, o.nG))
        return o.nG


def test_walk_takes_the_steps_of_a_loop_written_out():
    T = 200
    rec = Recorder()
    o, rewards, dones, observed = ow.walk(DIST, SEED, ASEED, T, rec)
    w = ffi.load("bo").env(DIST)
    w.seed(SEED)
    w.reset()
    calls, want_rewards, want_dones, want_observed = [], [], [], []
    for t in range(T):
        a = ffi.agent_action(ASEED, t, w.nP)
        calls.append(("before", t, a, w.nP, w.nG))
        nP = w.nP
        r = w.step(a)
        calls.append(("after", t, a, r, w.nP, w.nG))              # (before the reset: an episode's last step shows 0 rows)
        want_observed.append((nP, w.nG))
        want_rewards.append(r)
        want_dones.append(w.nP == 0)
        if w.nP == 0:
            w.reset()
    assert rec.calls == calls and observed == want_observed
    assert rewards.tolist() == want_rewards and dones.tolist() == want_dones and sum(want_dones) >= 2
    assert any(c[0] == "after" and c[4] == 0 for c in calls)
    assert (o.nP, o.nG) == (w.nP, w.nG)
    assert_same_state(Batch(o), 0, w, "written out")
    # callables in place of an object, either missing; no observer at all
    o2, rewards2, dones2, observed2 = ow.walk(DIST, SEED, ASEED, T, (None, lambda o, t, a, r: r))
    assert [x for _, x in observed2] == want_rewards and all(b is None for b, _ in observed2)
    assert ow.walk(DIST, SEED, ASEED, T)[3] == [(None, None)] * T
    assert rewards2.tolist() == want_rewards and dones2.tolist() == want_dones and (o2.nP, o2.nG) == (w.nP, w.nG)


def test_pair_kind_observer_reproduces_the_known_first_occurrences():
    kinds = [k for k, _ in ow.walk(DIST, SEED, ASEED, 256, (selected_kind, None))[3]]
    assert {k: kinds.index(k) for k in KINDS} == KNOWN_FIRST


def test_grevlex_key_and_agent_seeds():
    assert ow.grevlex_key((1, 0, 0)) > ow.grevlex_key((0, 1, 0)) > ow.grevlex_key((0, 0, 1))      # x > y > z at one degree
    assert ow.grevlex_key((0, 0, 2)) > ow.grevlex_key((1, 0, 0)) and ow.grevlex_key((1, 1, 0)) > ow.grevlex_key((1, 0, 1))
    assert ow.agent_seeds((3000, 3009)) == [7, 16]
