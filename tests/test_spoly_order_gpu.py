"""The S-polynomial's two scaled tails ordered by the reduction loop's own scalar code (FA_ORDER, bbx_fast.h) instead of a
merge on the vector unit, through every kernel of the fast class: traced step for step, lean headline (single launches
and a persistent session), generic lean (obs_fill), value, one-layer policy rollout.  Eight environments, 256 steps; the
seeds select pairs of every kind the ordering has to tell apart — first tail leading, second leading, equal monomials
with a non-zero and with a zero sum, either member or both without a tail (tests/test_spoly_order_cpu.py asserts that).
Everything against the oracle: per step on the traced kernel, state (basis term for term, pair list, reducer order) and
outputs on the lean ones."""
import pytest

from tests.test_spoly_order_cpu import DIST, K, SEEDS, T, walk
from tests.fast_harness import KERNELS, check_lean_rollout, check_policy_rollout_one_layer, check_traced_rollout, check_values_after_rollout

pytestmark = pytest.mark.gpu


def test_traced_rollout_step_for_step():
    check_traced_rollout(DIST, SEEDS, K, T, walk)


@pytest.mark.parametrize("kernel", KERNELS)
def test_lean_rollout_device(kernel):
    """The lean headline shape (hash agent, the observation written after every step, no fill) as four launches of 64 steps
    and as one persistent session of four calls; with obs_fill on the launcher takes the generic lean kernel instead."""
    check_lean_rollout(kernel, [T // 4] * 4, DIST, SEEDS, K, walk)


def test_values_after_the_rollout():
    """value() rollouts (the class's value kernel: to the end of the episode under a fixed strategy) from the state 256
    steps in"""
    check_values_after_rollout(DIST, SEEDS, K, (T,), lambda s, a, n: walk(s, a)[0])


def test_policy_rollout_one_layer():
    """bbx_policy_rollout_device with a one-layer policy of 64 hidden units, 64 steps: the environments — replayed on the
    oracle with the actions the kernel drew — step for step: observation, row count, reward, done flag; the state afterwards."""
    check_policy_rollout_one_layer(DIST, SEEDS, K, 64, 1611, 1612)
