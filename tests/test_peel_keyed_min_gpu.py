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
import pytest

from tests.test_peel_keyed_min_cpu import CUT, DIST, K, LAUNCH, SEEDS, T, walk
from tests.fast_harness import (KERNELS, check_policy_rollout_one_layer, check_state_after_every_launch, check_traced_rollout,
                                check_values_after_rollout)

pytestmark = pytest.mark.gpu


def states(seed, aseed):
    return walk(seed, aseed)[1]


def final(seed, aseed):
    return walk(seed, aseed)[2]


def at_cut(seed, aseed, nsteps):
    return walk(seed, aseed)[3][nsteps // CUT - 1]


@pytest.mark.parametrize("kernel", KERNELS)
def test_state_after_every_short_launch(kernel):
    check_state_after_every_launch(kernel, LAUNCH, DIST, SEEDS, K, T, states, final)


def test_traced_rollout_in_one_launch():
    """The same 256 steps as ONE launch of the traced kernel: every insertion is followed by a step on the registers it left."""
    check_traced_rollout(DIST, SEEDS, K, T, lambda s, a: (final(s, a),))


def test_values_from_every_cut():
    """value() rollouts (the class's value kernel) under 'first' and 'degree' from the state after every 32 steps: each runs
    its episode to the end on a copy of the state — bases of 64 and more elements among them — and returns what the oracle's
    value() returns from the same state; the batch itself is where the oracle is."""
    check_values_after_rollout(DIST, SEEDS, K, range(CUT, T + 1, CUT), at_cut, strategies=("first", "degree"))


@pytest.mark.parametrize("start", (0, 64, 128, 192))
def test_policy_rollout_from_a_cut(start):
    """bbx_policy_rollout_device with a one-layer policy of 64 hidden units, 48 steps from the state `start` hash-agent steps
    in: the environments — replayed on the oracle with the actions the kernel drew — step for step (row count, observation,
    reward, done flag), and the state afterwards: basis, pair list, reducer order."""
    inserted = check_policy_rollout_one_layer(DIST, SEEDS, K, 48, 2521, 2522 + start, start, lambda s, a: at_cut(s, a, start))
    assert inserted >= len(SEEDS)                            # (the rollout is about insertions: there are many)
