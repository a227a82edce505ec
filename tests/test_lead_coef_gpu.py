"""New basis elements with lead coefficient 1 and 32002 (the two ends of the inverse table the fast class reads 1/LC from,
bbx_fast.h add_poly) through every kernel of the class a rollout can take: the traced kernel step for step, the lean headline
kernel as single launches and inside a persistent session, and the value kernel.  Eight environments, 128 steps; basis, reducer
order, pair list, rewards and observation against the oracle.  tests/test_lead_coef_cpu.py asserts that the seeds produce
those elements and that later steps use them."""
import pytest

from tests.test_lead_coef_cpu import DIST, K, SEEDS, T, walk
from tests.fast_harness import check_lean_rollout, check_traced_rollout, check_values_after_rollout

pytestmark = pytest.mark.gpu


def test_traced_rollout_step_for_step():
    check_traced_rollout(DIST, SEEDS, K, T, walk)


@pytest.mark.parametrize("persistent", (False, True))
def test_headline_rollout_device(persistent):
    """The lean headline shape (hash agent, rewards / dones / rows buffers, the observation written after every step) as two
    launches of 64 steps and as one persistent session of two calls."""
    check_lean_rollout("headline-session" if persistent else "headline", (T // 2, T - T // 2), DIST, SEEDS, K, walk)


def test_values_before_and_after_the_rollout():
    """value() rollouts (the class's value kernel) from the reset state and from the state 128 steps later"""
    check_values_after_rollout(DIST, SEEDS, K, (0, T), lambda s, a, n: walk(s, a)[0])
