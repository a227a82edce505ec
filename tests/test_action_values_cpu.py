"""bbx_action_values without a GPU: the pass planner (a pure host function of libbbx) against its numpy model, and the
definition itself on the CPU oracle — the identities it must satisfy, so that the references the GPU tests compare against
(tests/action_value_cases.py) are themselves checked."""
import numpy as np
import pytest

import __graft_entry__ as graft
from oracle import ffi
from tests import action_value_cases as A


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


PLANS = [
    ("all counts zero", [0, 0, 0, 0], 5),
    ("one environment taller than the chunk", [2, 23, 1], 7),
    ("chunk 1", [3, 0, 2, 4], 1),
    ("chunk equal to the total", [3, 0, 2, 4], 9),
    ("chunk one below the total", [3, 0, 2, 4], 8),
    ("chunk one above the total", [3, 0, 2, 4], 10),
    ("B = 1", [11], 4),
    ("B = 1, empty", [0], 4),
    ("passes that begin and end inside environments", [5, 5, 5, 5], 3),
]


@pytest.mark.parametrize("name,counts,chunk", PLANS, ids=[p[0] for p in PLANS])
def test_pass_plan_equals_the_model(name, counts, chunk):
    want = A.plan_model(counts, chunk)
    rc, first = A.plan(counts, chunk)
    assert rc == 0 and np.array_equal(first, want), (name, first, want)
    # what the call relies on: contiguous, ascending, no pass above the chunk, none empty, the whole list covered
    sizes = np.diff(first)
    assert first[0] == 0 and first[-1] == sum(counts) and (sizes > 0).all() and (sizes <= chunk).all()
    assert len(sizes) == -(-sum(counts) // chunk)
    # exactly enough room is enough; one element less is BBX_E_CAPACITY
    rc, again = A.plan(counts, chunk, cap=len(want))
    assert rc == 0 and np.array_equal(again, want)
    rc, _ = A.plan(counts, chunk, cap=len(want) - 1)
    assert rc == -3, name


def test_pass_plan_refuses_bad_arguments():
    from deepgroebner_amd import _ffi
    assert A.plan([1, 2], 0)[0] == -1                      # chunk < 1
    assert A.plan([1, -2], 3)[0] == -1                     # a negative count
    first = np.zeros(4, dtype=np.int32)
    assert _ffi.lib().bbx_action_values_plan(None, 2, 3, _ffi.ptr(first), 4, None) == -1


def _walked_states(dist, seed, steps=40):
    """The states of one oracle episode under the counter-hash agent, each a fresh copy."""
    bo = ffi.load("bo")
    o = bo.env(dist); o.seed(seed); o.reset()
    t = 0
    while o.nP > 0 and t < steps:
        yield o.copy()
        o.step(ffi.agent_action(seed, t, o.nP)); t += 1


def test_definition_identities_on_the_oracle():
    """Two identities of Q[a] = r + gamma * value(state behind a), on the episodes of a small ideal distribution:

    terminal: where every action ends the episode, Q[a] is the step's reward — == on doubles (r + gamma * 0.0 is r);
    one pair: where the state has one pair, no strategy has a choice in its first step, so Q[0] is value(strategy) of the
      state itself.  NOT bit for bit in general: value() accumulates r0 + gamma r1 + gamma^2 r2 + ... term by term, Q[0] is
      r0 + gamma * (r1 + gamma r2 + ...), and the two round differently.  At gamma = 1 every term is a small negative integer
      and both are exact: ==.  At gamma = 0.99 each evaluation is N <= S steps (S = the undiscounted |return|: every reward is
      <= -1) of at most 3 operations whose operands are bounded by S, each rounding by at most 2^-53 S: |Q[0] - value| <= 6 S^2 2^-53,
      asserted with 8.

    (max_a Q[a] >= value('degree') need not hold — Degree is a heuristic, not a maximiser over first actions — and is not asserted.)"""
    terminal = one_pair = 0
    for seed in (0, 1, 3, 4):
        for o in _walked_states("2-4-3-uniform", seed):
            for strategy in ("degree", "normal", "first"):
                q, rew, done = A.oracle_action_values(o, strategy, 0.99)
                assert not np.isnan(q).any() and len(q) == o.nP
                if done.all():
                    terminal += 1
                    assert np.array_equal(q, rew), (seed, strategy)
                if o.nP == 1:
                    one_pair += 1
                    q1, _, _ = A.oracle_action_values(o, strategy, 1.0)
                    assert q1[0] == o.value(strategy, 1.0), (seed, strategy)       # exact: integers
                    S = abs(o.value(strategy, 1.0))
                    assert abs(q[0] - o.value(strategy, 0.99)) <= 8.0 * S * S * 2.0 ** -53, (seed, strategy)
    assert terminal >= 3 and one_pair >= 6, (terminal, one_pair)   # both identities were met, under every strategy


def test_best_actions_takes_the_first_maximum_over_the_numbers():
    from deepgroebner_amd.buchberger import best_actions
    nan = np.nan
    block = np.array([[-5.0, -3.0, -3.0, nan],      # a tie: the first of the two
                      [nan, nan, nan, nan],         # no pair: 0
                      [-9.0, nan, nan, nan],
                      [-4.0, -7.0, -2.0, -2.0]])
    got = best_actions(block)
    assert got.dtype == np.int32 and got.tolist() == [1, 0, 0, 2]
    assert best_actions(np.array([-1.0, -1.0])).tolist() == [0]
