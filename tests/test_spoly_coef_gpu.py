"""The fast class's working copy of a basis element's info (bbx_fast.h: gi[] holds tc/lc and -tc/lc, the S-polynomial's two
coefficients, formed when the element enters; gc[] keeps the record's word lc | tc << 16 for the write-back) through every
kernel of the class: traced, lean headline (single launches and a persistent session), generic lean, value, policy rollout
(the two-bank layout), with the class capped so that records travel to the HBM-resident class and back, from records the
class did not just write (copy(), clone_envs), and beyond 128 reducers, where the reducer words are rebuilt from gc[].
Eight environments, 128 steps; the seeds select elements without a tail as first and as second member of a pair and pairs
of two scaled elements with tails (tests/test_spoly_coef_cpu.py asserts that).  Everything against the oracle; the basis
term for term after each run is what shows that gc[] restores lead and tail coefficient."""
import numpy as np
import pytest

from oracle import ffi
from tests import policy_cases as pc
from tests.test_spoly_coef_cpu import DIST, K, SEEDS, T, walk
from tests.fast_harness import (KERNELS, assert_same_outputs, assert_same_state, assert_same_states, check_lean_rollout, check_traced_rollout,
                                check_values_after_rollout, make_env, policy_rollout, replay_policy_rollout, rollout_buffers, stream)

pytestmark = pytest.mark.gpu
B = len(SEEDS)
CAPS = (None, {"lds_max_basis": 16})          # the second: records written by the class are read by the HBM-resident one and handed back
CAP_IDS = ("default", "lds16")
R = 256


@pytest.mark.parametrize("caps", CAPS, ids=CAP_IDS)
def test_traced_rollout_step_for_step(caps):
    check_traced_rollout(DIST, SEEDS, K, T, walk, caps=caps)


@pytest.mark.parametrize("caps", CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_lean_rollout_device(kernel, caps):
    """The lean headline shape (hash agent, the observation written after every step, no fill) as two launches of 64 steps and
    as one persistent session of two calls; with obs_fill on the launcher takes the generic lean kernel instead."""
    check_lean_rollout(kernel, (T // 2, T - T // 2), DIST, SEEDS, K, walk, caps=caps)


@pytest.mark.parametrize("caps", CAPS, ids=CAP_IDS)
def test_values_before_and_after_the_rollout(caps):
    """value() rollouts (the class's value kernel) from the reset state and from the state 128 steps later"""
    check_values_after_rollout(DIST, SEEDS, K, (0, T), lambda s, a, n: walk(s, a)[0], caps=caps)


CUT = 40


def test_copy_taken_mid_episode():
    """copy() at step 40: the copy stages records in that it never wrote; both batches stepped on to 128."""
    env = make_env(DIST, SEEDS, K, lean=True)
    s = stream()
    ebufs, tbufs = rollout_buffers(B, R, env.cols), rollout_buffers(B, R, env.cols)
    env.rollout_device("random", CUT, True, s, *ebufs, R, False, True)
    env.sync()
    assert_same_states(env, SEEDS, lambda seed, aseed: walk(seed, aseed, CUT), "at the cut")
    twin = env.copy()
    twin.accounting(False)
    for batch, bufs in ((env, ebufs), (twin, tbufs)):
        batch.rollout_device("random", T - CUT, True, s, *bufs, R, False, True)
        batch.sync()
    for batch, bufs, name in ((env, ebufs, "source"), (twin, tbufs, "copy")):
        assert_same_states(batch, SEEDS, walk, name)
        assert_same_outputs(bufs, SEEDS, walk, K)


def test_clones_taken_mid_episode():
    """clone_envs at step 40 over eight environments that ran other ideals: source and clone stepped on to 128."""
    env = make_env(DIST, list(SEEDS) + [(s + 400, a + 400) for s, a in SEEDS], K, lean=True)
    s = stream()
    bufs = rollout_buffers(2 * B, R, env.cols)
    env.rollout_device("random", CUT, True, s, *bufs, R, False, True)
    env.sync()
    env.clone_envs(list(range(B)), list(range(B, 2 * B)))
    assert_same_states(env, SEEDS * 2, lambda seed, aseed: walk(seed, aseed, CUT), "cloned")
    env.rollout_device("random", T - CUT, True, s, *bufs, R, False, True)
    env.sync()
    assert_same_states(env, SEEDS * 2, walk, "clones")
    assert_same_outputs(bufs, SEEDS * 2, walk, K)


@pytest.mark.parametrize("persistent", (False, True))
def test_reducers_beyond_the_registers(persistent):
    """3-20-140-weighted: 140 generators, so reducers 128.. exist as an order only and their words (tc | -tc/lc << 16) are
    rebuilt from gc[] and gi[] — in the reduction when one of them divides, and at every write-back.  Two environments, 16
    steps in launches of 4; state (reducer order included) and observation against the oracle."""
    dist, nB, nT, rows_cap = "3-20-140-weighted", 2, 16, 2048
    bo = ffi.load("bo")
    env = make_env(dist, [(700 + e, e) for e in range(nB)], K, lean=True, persistent=persistent)
    rew, done, rows, obs = rollout_buffers(nB, rows_cap, env.cols, fill=0)
    for _ in range(nT // 4):
        env.rollout_device("random", 4, True, stream(), rew, done, rows, obs, rows_cap, False, True)
    env.sync()
    assert (env.stats()[:, 4] == 0).all(), env.stats()
    got_rows, got_obs, got_rew = rows.cpu().numpy(), obs.cpu().numpy(), rew.cpu().numpy()
    for e in range(nB):
        o = bo.env(dist); o.seed(700 + e); o.reset()
        assert o.nG > 128
        for t in range(nT):
            r = o.step(ffi.agent_action(e, t, o.nP))
            assert o.nP > 0                                  # (no episode of these ends within 16 steps)
        assert_same_state(env, e, o, ("beyond the registers", persistent))
        assert got_rew[e] == r and got_rows[e] == o.nP and o.nP <= rows_cap
        assert np.array_equal(got_obs[e, :o.nP], o.obs(K)), e


def test_policy_rollout_two_bank_layout():
    """bbx_policy_rollout_device with a one-layer policy of 64 hidden units (the class's two-bank LDS layout), 32 steps: the
    draws against the float64 reference and the torch module, the environments — replayed on the oracle with the actions the
    kernel drew — step for step: observation, row count, reward, done flag; the state afterwards."""
    import torch
    nT = 32
    env = make_env(DIST, SEEDS, K, lean=True)
    w, pol, out = policy_rollout(env, 64, 911, nT, 912, R)
    u, A, L, O, N = out["u"], out["acts"], out["logp"], out["obs"], out["rows"]
    for t in range(nT):                                      # the torch path, as tests/test_rollout.py holds the per-step kernel to it
        a_t, l_t = pol.act_torch(O[t], N[t], u[t])
        assert int((A[t] != a_t).sum()) <= 1 and torch.allclose(L[t][A[t] == a_t], l_t[A[t] == a_t], atol=5e-4, rtol=1e-4), t
    obs, rows = O.reshape(nT * B, R, env.cols).cpu().numpy(), N.reshape(-1).cpu().numpy()
    uu, a, l = u.reshape(-1).cpu().numpy(), A.reshape(-1).cpu().numpy(), L.reshape(-1).cpu().numpy()
    ref = pc.reference(w, obs, rows)
    band = pc.check_draws(w, obs, rows, uu, a, l, ref=ref, what="two-bank rollout")
    assert band <= pc.near_boundary(ref, uu), band
    finals, _ = replay_policy_rollout(DIST, SEEDS, K, A.cpu().numpy(), out["rews"].cpu().numpy(), out["dones"].cpu().numpy(),
                                      obs.reshape(nT, B, R, env.cols), rows.reshape(nT, B))
    for e, o in enumerate(finals):
        assert_same_state(env, e, o, "policy rollout")
