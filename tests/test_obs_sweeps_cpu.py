"""The headline observation writer of the fast class (write_obs32, bbx_fast.h) covers 32 rows per trip as two interleaved
sweeps of 16 while more than 16 rows remain and ends with ONE sweep of 16 when at most 16 remain.  This file asserts, on the
oracle alone, that the batch tests/test_obs_sweeps_gpu.py steps shows the row counts at which the writer changes its path —
exactly 1, 16, 17, 32, 33, 48 and 49 rows — at the (environment, step) pairs pinned here, and a count above the cut block of
the truncation case.  32 environments (ideal seed 1000 + e, agent seed 7 + e), 48 steps of the hash agent with auto-reset
(160 steps were searched: 49 rows show 7 times among them, 48 rows 15 times; the pairs chosen share four steps); a pair that
stops showing its count fails the test."""
import functools

import numpy as np

from tests import oracle_walk as ow

DIST, K, B, T = "3-20-10-weighted", 2, 32, 48
SEEDS = tuple((1000 + e, 7 + e) for e in range(B))
COUNTS = (1, 16, 17, 32, 33, 48, 49)
# row count -> (environment, step): the observation after that step of that environment has exactly that many rows
CASES = {1: (4, 45), 16: (1, 43), 17: (9, 45), 32: (3, 41), 33: (3, 45), 48: (16, 44), 49: (16, 45)}
CUT_ROWS = 20                                                # the truncation case: a block of 20 rows per environment
CUT_STEP = 45                                                # ... read after this step, where some environments have more


@functools.lru_cache(maxsize=None)
def walk(e):
    """T steps of environment e on the oracle: ([row count after every step], [observation after every step]) — what a
    launch that ends with that step leaves in the environment's block (after a step that ends an episode: the new ideal's)."""
    # (what a step leaves once a reset has happened is what the next step's before hook sees, and the last: the final state)
    o, _, _, seen = ow.walk(DIST, *SEEDS[e], T, (lambda o, t, a: (o.nP, o.obs(K)), None))
    left = [b for b, _ in seen[1:]] + [(o.nP, o.obs(K))]
    return [n for n, _ in left], [rows for _, rows in left]


def boundaries():
    """the steps after which the GPU test reads the blocks, ascending"""
    return sorted({t for _, t in CASES.values()})


def test_every_row_count_is_shown_where_pinned():
    assert set(CASES) == set(COUNTS)
    for c, (e, t) in CASES.items():
        assert walk(e)[0][t] == c, (c, e, t, walk(e)[0][t])
        assert walk(e)[1][t].shape == (c, 4 * 3)


def test_the_cut_block_is_smaller_than_some_observations_and_larger_than_others():
    rows = [walk(e)[0][CUT_STEP] for e in range(B)]
    assert max(rows) > CUT_ROWS + 16 and min(rows) < CUT_ROWS and any(CUT_ROWS < r <= CUT_ROWS + 12 for r in rows), rows


def test_both_ends_of_the_writer_are_common():
    """At most 16 rows left behind the 32-row trips (the single sweep) and more than 16 (another trip) both occur at every
    boundary the GPU test reads: all 32 blocks are compared there, not only the pinned one."""
    for t in boundaries():
        rows = np.array([walk(e)[0][t] for e in range(B)])
        tail = (rows - 1) % 32 + 1
        assert (tail <= 16).sum() >= 4 and (tail > 16).sum() >= 4, (t, rows)
