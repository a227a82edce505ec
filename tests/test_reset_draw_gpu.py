"""The fast class draws a reset's ideal across the lanes (gen_ideal_lanes in bbx_device.h) where the one-pass install runs,
and one generator after another where a generator takes a rejection or a retrial, beyond 11 generators and under tight
capacities.  Either way the trajectory must be the oracle's step for step — actions, rewards, pair sets, observations, new
basis elements — episode after episode, so that every reset along the way is checked; the lean kernels (other
instantiations of the same body) through their counters and final states."""
import numpy as np
import pytest

from oracle import ffi
from oracle.trace import fnv64, run_trace
from tests.test_gpu_parity import _state_words
from tests.test_reset_draw_cpu import M, rejection_states

pytestmark = pytest.mark.gpu
DISTS = ["3-20-10-weighted", "3-20-10-weighted-homog", "3-20-10-weighted-pure", "3-20-10-weighted-consts", "3-20-11-weighted",
         "3-20-10-maximum", "3-2-10-uniform", "2-5-4-uniform"]


def _check(dist, sort_input=False, caps=None, seeds=None, B=6, T=200, k=2):
    from deepgroebner_amd import VecLeadMonomialsEnv
    seeds = np.arange(B) + 2000 if seeds is None else np.asarray(seeds)
    env = VecLeadMonomialsEnv(dist, batch=B, k=k, sort_input=sort_input, caps=caps)
    env.seed(seeds)
    env.seed_agent(np.arange(B) + 7)
    env.trace_enable(T)
    env.reset()
    env.rollout("random", T, auto_reset=True)
    bo = ffi.load("bo")
    for e in range(B):
        o = bo.env(dist, sort_input=sort_input)
        o.seed(int(seeds[e]))
        want = run_trace(o, k, T, "hash", agent_seed=e + 7)
        got = env.trace_read(e, 0, T)
        for key, wkey in (("action", "action"), ("reward", "reward"), ("rows", "nP"), ("basis_size", "nG"), ("obs_hash", "obs_hash"),
                          ("pairs_hash", "pairs_hash"), ("newpoly_hash", "newpoly_hash")):
            assert np.array_equal(got[key], want[wkey]), (dist, sort_input, caps, e, key)
        episodes = int(np.count_nonzero(np.asarray(want["nG"])[1:] < np.asarray(want["nG"])[:-1]))
        assert episodes >= 2, ("too few resets of this environment inside the rollout to say anything about them", dist, sort_input, e, episodes)


@pytest.mark.parametrize("sort_input", [False, True])
@pytest.mark.parametrize("dist", DISTS)
def test_lane_parallel_draw_matches_the_oracle(dist, sort_input):
    # (episodes of -pure and -maximum last 100-200 steps: 600 steps for two resets in every environment)
    _check(dist, sort_input=sort_input, T=600 if dist in ("3-20-10-weighted-pure", "3-20-10-maximum") else 200)


@pytest.mark.parametrize("sort_input", [False, True])
def test_constructed_rejections_take_the_sequential_draw(sort_input):
    """Engine states that put a raw past its bound at the coefficient draw, at a monomial draw and at the last generator's
    last draw (tests/test_reset_draw_cpu.py): as the seed itself, and 70 raws earlier, so that the reset after an ideal drawn
    across the lanes starts from it."""
    states = rejection_states(10, 7)
    back = pow(16807, -70, M)
    seeds = [s for what in ("coefficient", "choice", "last-draw") for s in (states[what], states[what] * back % M)]
    _check("3-20-10-weighted", sort_input=sort_input, seeds=seeds)


@pytest.mark.parametrize("sort_input", [False, True])
def test_twelve_generators_keep_the_sequential_draw(sort_input):
    _check("3-20-12-weighted", sort_input=sort_input)


@pytest.mark.parametrize("sort_input", [False, True])
def test_tight_caps_keep_the_sequential_draw(sort_input):
    # |P| <= 32 in the fast class: 10 generators need up to 55 pairs, so neither the one-pass install nor the batch may run
    _check("3-20-10-weighted", sort_input=sort_input, caps={"lds_max_basis": 16})


def _check_lean(env, want):
    st = env.stats()
    assert (st[:, 4] == 0).all(), st[:, 4]
    for key, col in (("steps", 0), ("additions", 1), ("episodes", 2), ("zero_reductions", 3), ("nG", 7)):
        assert np.array_equal(st[:, col], np.array([r[key] for r in want])), key
    for e in range(len(want)):
        basis, pairs, order = env.state(e)
        assert fnv64(_state_words(basis, pairs, order)) == want[e]["state_hash"], e


@pytest.mark.parametrize("persistent", [False, True])
@pytest.mark.parametrize("dist", ["3-20-10-weighted", "3-2-10-uniform"])
def test_lean_kernels(dist, persistent):
    """The timed kernels: one kernel per launch (300 steps), and a persistent session of 3 x 100 steps."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    B, T = 64, 300
    bo = ffi.load("bo")
    want = bo.run_random_many(dist, 2, range(1000, 1000 + B), range(B), T, True, 0)
    assert min(r["episodes"] for r in want) >= 2
    env = VecLeadMonomialsEnv(dist, batch=B, k=2)
    env.seed(np.arange(B) + 1000); env.seed_agent(np.arange(B)); env.reset(); env.accounting(False)
    rows = torch.zeros(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if persistent:
        env.persistent(True)
        for _ in range(3):
            env.rollout_device("random", T // 3, True, s, rows=rows)
        env.sync()
        assert env.session_stats()["sessions"] >= 1
    else:
        env.rollout_device("random", T, True, s, rows=rows)
        env.sync()
    _check_lean(env, want)
    assert np.array_equal(rows.cpu().numpy(), np.array([r["nP"] for r in want]))
