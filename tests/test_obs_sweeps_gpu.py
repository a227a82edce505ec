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

from tests import policy_cases as pc
from tests.test_obs_sweeps_cpu import B, CASES, CUT_ROWS, CUT_STEP, DIST, K, SEEDS, boundaries, walk

pytestmark = pytest.mark.gpu
R = 80                                                       # rows per block: above every count of the run (69 at most in 160 steps)
SENT = -7


def _env():
    from deepgroebner_amd import VecLeadMonomialsEnv
    env = VecLeadMonomialsEnv(DIST, batch=B, k=K)
    env.seed(np.array([s for s, _ in SEEDS]))
    env.seed_agent(np.array([a for _, a in SEEDS]))
    env.reset()
    env.accounting(False)
    return env


def _bufs(rows_per_block, blocks=B):
    import torch
    return (torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda"),
            torch.zeros(B, dtype=torch.int32, device="cuda"), torch.full((blocks, rows_per_block, 4 * 3), SENT, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("kernel", ("headline", "headline-session", "generic"))
def test_blocks_at_the_pinned_row_counts(kernel):
    import torch
    env = _env()
    env.persistent(kernel == "headline-session")
    s = torch.cuda.current_stream().cuda_stream
    rew, done, rows, obs = _bufs(R)
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
    import torch
    from deepgroebner_amd import _ffi
    env = _env()
    s = torch.cuda.current_stream().cuda_stream
    rew, done, rows, big = _bufs(R)
    env.rollout_device("random", CUT_STEP, True, s, rew, done, rows, big, R, False, True)
    env.sync()
    _, _, _, small = _bufs(CUT_ROWS, B + 1)
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
    import torch
    from oracle import ffi
    nT = 24
    env = _env()
    w = pc.make_weights(env.cols, (64,), 2531)
    p = pc.to_policy(w, "cuda")._fused_weights()
    s = torch.cuda.current_stream().cuda_stream
    u = torch.rand((nT, B), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2532))
    A = torch.zeros((nT, B), dtype=torch.int32, device="cuda"); L = torch.zeros((nT, B), dtype=torch.float32, device="cuda")
    Rw = torch.zeros((nT, B), dtype=torch.float64, device="cuda"); D = torch.zeros((nT, B), dtype=torch.uint8, device="cuda")
    N = torch.zeros((nT, B), dtype=torch.int32, device="cuda")
    O = torch.full((nT, B, R, env.cols), SENT, dtype=torch.int32, device="cuda")
    env.policy_rollout_device(p["prepared"], p["hidden"], nT, u, A, L, Rw, D, N, O, R, B * R * env.cols, s)
    env.sync(); torch.cuda.synchronize()
    acts, obs, rows = A.cpu().numpy(), O.cpu().numpy(), N.cpu().numpy()
    assert env.stats()[:, 4].max() == 0
    tails = set()
    for e, (seed, _) in enumerate(SEEDS):
        o = ffi.load("bo").env(DIST); o.seed(seed); o.reset()
        for t in range(nT):
            n = o.nP
            assert rows[t, e] == n and np.array_equal(obs[t, e, :n], o.obs(K)), (e, t)
            assert (obs[t, e, n:] == SENT).all(), (e, t, n)
            tails.add((n - 1) % 32 < 16)
            o.step(int(acts[t, e]))
            if o.nP == 0:
                o.reset()
    assert tails == {True, False}                               # (a rest of at most 16 rows and a longer one both occurred)
