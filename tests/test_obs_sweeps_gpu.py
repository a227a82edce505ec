"""The headline observation writer (write_obs32, bbx_fast.h: trips of 32 rows, then one sweep of 16 for a rest of at most 16)
at the row counts where it changes its path: exactly 1, 16, 17, 32, 33, 48 and 49 rows, at the (environment, step) pairs
tests/test_obs_sweeps_cpu.py pins on the oracle.  32 environments are stepped to just before each of those steps; the block
is then overwritten with a sentinel and ONE step is launched, so that what the block holds afterwards is what that step's
observation wrote: every row of every environment is compared with the oracle's observation, and every row beyond the
environment's count must still hold the sentinel — nothing past the live part is stored (with obs_fill, the generic kernel:
the -1 padding instead).  Lean headline kernel as launches and as a persistent session, generic lean kernel, the cut block
(obs_rows smaller than |P|: the first obs_rows rows and the truncation error), and the one-layer policy rollout, whose
per-step blocks are each held to the oracle replayed with the kernel's actions."""
import numpy as np
import pytest

from tests.test_obs_sweeps_cpu import B, CASES, CUT_ROWS, CUT_STEP, DIST, K, SEEDS, boundaries, walk
from tests.fast_harness import KERNELS, make_env, policy_rollout, replay_policy_rollout, rollout_buffers, stream

pytestmark = pytest.mark.gpu
R = 80                                                       # rows per block: above every count of the run (69 at most in 160 steps)
SENT = -7


@pytest.mark.parametrize("kernel", KERNELS)
def test_blocks_at_the_pinned_row_counts(kernel):
    import torch
    env = make_env(DIST, SEEDS, K, lean=True, persistent=kernel == "headline-session")
    s = stream()
    rew, done, rows, obs = rollout_buffers(B, R, env.cols, fill=SENT)
    generic = kernel == "generic"
    at, shown = 0, set()
    for t in boundaries():
        if t > at:
            env.rollout_device("random", t - at, True, s, rew, done, rows, obs, R, generic, True)
            env.sync()
        obs.fill_(SENT)
        torch.cuda.synchronize()
        env.rollout_device("random", 1, True, s, rew, done, rows, obs, R, generic, True)
        env.sync()
        at = t + 1
        got_rows, got = rows.cpu().numpy(), obs.cpu().numpy()
        for e in range(B):
            n, want = walk(e)[0][t], walk(e)[1][t]
            assert got_rows[e] == n, (kernel, t, e)
            assert np.array_equal(got[e, :n], want), (kernel, t, e, n, "rows of the observation")
            assert (got[e, n:] == (-1 if generic else SENT)).all(), (kernel, t, e, n, "rows beyond the count")
            shown.update(c for c, et in CASES.items() if et == (e, t) and n == c)
    assert shown == set(CASES), shown
    assert (env.stats()[:, 4] == 0).all()


def test_cut_block_keeps_its_first_rows_and_reports_the_rest():
    """obs_rows = 20 where environments have up to 49 rows: the first 20 rows of those, all rows of the others, the sentinel
    beyond them and in a spare block behind the last environment's; the call that waits for the launch reports the rows lost."""
    from deepgroebner_amd import _ffi
    env = make_env(DIST, SEEDS, K, lean=True)
    s = stream()
    rew, done, rows, big = rollout_buffers(B, R, env.cols, fill=SENT)
    env.rollout_device("random", CUT_STEP, True, s, rew, done, rows, big, R, False, True)
    env.sync()
    small = rollout_buffers(B, CUT_ROWS, env.cols, fill=SENT, blocks=B + 1)[3]
    env.rollout_device("random", 1, True, s, rew, done, rows, small, CUT_ROWS, False, True)
    with pytest.raises(_ffi.BbxError) as ei:
        env.sync()
    assert "more rows" in str(ei.value), ei.value
    got_rows, got = rows.cpu().numpy(), small.cpu().numpy()
    cut = 0
    for e in range(B):
        n, want = walk(e)[0][CUT_STEP], walk(e)[1][CUT_STEP]
        m = min(n, CUT_ROWS)
        cut += int(n > CUT_ROWS)
        assert got_rows[e] == n, e
        assert np.array_equal(got[e, :m], want[:m]) and (got[e, m:] == SENT).all(), (e, n)
    assert cut >= 4 and (got[B] == SENT).all()


def test_policy_rollout_blocks_step_by_step():
    """bbx_policy_rollout_device, one hidden layer of 64 units, 24 steps: the block of every step (written before the step, from
    the state the policy scores) is the oracle's observation, replayed with the actions the kernel drew, and keeps the sentinel
    beyond its rows."""
    nT = 24
    env = make_env(DIST, SEEDS, K, lean=True)
    out = {key: x.cpu().numpy() for key, x in policy_rollout(env, 64, 2531, nT, 2532, R, fill=SENT)[2].items()}
    obs, rows = out["obs"], out["rows"]
    replay_policy_rollout(DIST, SEEDS, K, out["acts"], out["rews"], out["dones"], obs, rows)   # (rows[t, e] is the oracle's count)
    tails = set()
    for e in range(B):
        for t in range(nT):
            n = rows[t, e]
            assert (obs[t, e, n:] == SENT).all(), (e, t, n)
            tails.add((n - 1) % 32 < 16)
    assert tails == {True, False}                               # (a rest of at most 16 rows and a longer one both occurred)
