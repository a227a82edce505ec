"""The fast class installs a device-drawn ideal of at most 11 generators in one pass (install_ideal in bbx_fast.h) and
falls back to inserting generator after generator beyond that or under tight capacities.  Both must give the oracle's
trajectory step for step: actions, rewards, pair sets, observations, new basis elements — episode after episode, so
that every reset along the way is checked."""
import numpy as np
import pytest

from oracle import ffi
from oracle.trace import run_trace


def _check(dist, sort_input=False, caps=None, B=6, T=160, k=2, host_gen=False, monkeypatch=None):
    from deepgroebner_amd import VecLeadMonomialsEnv
    if host_gen:
        monkeypatch.setenv("BBX_HOST_GEN", "1")
    env = VecLeadMonomialsEnv(dist, batch=B, k=k, sort_input=sort_input, caps=caps)
    env.seed(np.arange(B) + 2000)
    env.seed_agent(np.arange(B) + 7)
    env.trace_enable(T)
    env.reset()
    env.rollout("random", T, auto_reset=True)
    bo = ffi.load("bo")
    episodes = 0
    for e in range(B):
        o = bo.env(dist, sort_input=sort_input)
        o.seed(2000 + e)
        want = run_trace(o, k, T, "hash", agent_seed=e + 7)
        got = env.trace_read(e, 0, T)
        for key, wkey in (("action", "action"), ("reward", "reward"), ("rows", "nP"), ("basis_size", "nG"), ("obs_hash", "obs_hash"),
                          ("pairs_hash", "pairs_hash"), ("newpoly_hash", "newpoly_hash")):
            assert np.array_equal(got[key], want[wkey]), (dist, sort_input, caps, e, key)
        episodes += int(np.count_nonzero(np.asarray(want["nG"])[1:] < np.asarray(want["nG"])[:-1]))
    assert episodes >= 2, "too few resets inside the rollout to say anything about them"


@pytest.mark.gpu
@pytest.mark.parametrize("sort_input", [False, True])
@pytest.mark.parametrize("n", [2, 3, 5, 8, 10, 11, 12, 15])
def test_one_pass_and_sequential_install_match_the_oracle(n, sort_input):
    _check("3-20-%d-weighted" % n, sort_input=sort_input)


@pytest.mark.gpu
@pytest.mark.parametrize("dist", ["3-20-10-uniform", "3-10-6-uniform"])
def test_uniform_distributions(dist):
    _check(dist)


@pytest.mark.gpu
@pytest.mark.parametrize("sort_input", [False, True])
def test_tight_caps_take_the_sequential_install(sort_input):
    # |P| <= 32 in the fast class: 10 generators need up to 55 pairs, so the one-pass install may not run
    _check("3-20-10-weighted", sort_input=sort_input, caps={"lds_max_basis": 16})


@pytest.mark.gpu
def test_host_queued_ideals(monkeypatch):
    # (ideals from the host queue keep the sequential install)
    _check("3-20-10-weighted", host_gen=True, monkeypatch=monkeypatch)
