"""value() / values() / values_device() from bases whose generator lead monomials tie: the path of the clone's tie flag,
bbx_value_resort_kernel (the device restatement of libstdc++'s std::sort, then the rebuilt reducer-order arrays of both
record layouts) and the step kernels of every class that start from the rebuilt order.  Every value is == the oracle's
double; the cases (tests/value_tie_cases.py) are states where a rollout from the environment's own, stable, reducer order
gives another value, so a resort that is skipped, wrong or ignored fails here.  The control group of 16-element bases is
the one place where the two orders are the same."""
import time

import numpy as np
import pytest

import __graft_entry__ as graft
from oracle import ffi
from tests import value_tie_cases as V
from tests.fast_harness import same_doubles, stream

pytestmark = pytest.mark.gpu

OBS_ROWS = 1024


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


@pytest.fixture(scope="module")
def groups():
    return V.build()


def _make(grp, caps=None):
    """The group's handle at the valued state: seeded, reset, the recorded actions walked; checked against the oracle's state."""
    from deepgroebner_amd import VecLeadMonomialsEnv
    B = grp.batch
    env = VecLeadMonomialsEnv(grp.ctor, batch=B, k=2, caps=grp.caps if caps is None else caps, sort_input=grp.sort_input)
    if not grp.listed:
        env.seed(np.asarray(grp.seeds, dtype=np.int64))
    env.seed_agent(np.arange(B))
    env.reset()
    for acts in grp.actions:
        env.step(np.asarray(acts, dtype=np.int32))
    assert env.rows.tolist() == [o.nP for o in grp.envs], grp.name
    for e in (0, B - 1):
        basis, pairs, order = env.state(e)
        assert len(basis) == grp.envs[e].nG and np.array_equal(pairs, grp.envs[e].pairs()), (grp.name, e)
        assert all(np.array_equal(c, wc) and np.array_equal(x, wx) for (c, x), (wc, wx) in zip(basis, grp.envs[e].basis())), (grp.name, e)
    return env


def _values_device(env, strategy, gamma=0.99, seeds=None):
    import torch
    out = torch.full((env.batch,), -1.0, dtype=torch.float64, device="cuda")
    s = None if seeds is None else torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.int64)).cuda()
    env.values_device(out, strategy, gamma, s, stream())
    env.sync()
    return out.cpu().numpy()


def _reducer_orders(env, grp):
    return [np.array_equal(env.state(e)[2], grp.envs[e].reducer_order()) for e in range(grp.batch)]


@pytest.mark.parametrize("name", V.GROUP_NAMES)
def test_values_from_tied_bases_equal_the_oracle(groups, name):
    t0 = time.perf_counter()
    grp = groups[name]
    B = grp.batch
    env = _make(grp)
    twin = env.copy()                                        # never valued: what the state must still be afterwards
    obs0, stats0 = env.observations(OBS_ROWS), env.stats()
    bad, compared = [], 0
    for s in V.STRATEGIES:
        want = np.asarray(grp.want[s])
        got = env.values(s, 0.99)
        dev = _values_device(env, s, 0.99)
        wrong = np.flatnonzero(got != want).tolist()
        print(name, s, "values: environments that differ", wrong, "values_device:", np.flatnonzero(dev != want).tolist())
        compared += len(got)
        if not same_doubles(got, want):
            bad.append(("values", s, wrong))
        if not same_doubles(dev, want):
            bad.append(("values_device", s, np.flatnonzero(dev != want).tolist()))
    assert compared == B * len(V.STRATEGIES) == 5 * len(grp.envs)      # nothing skipped, nothing tolerated
    for e in (1, B - 1):                                     # the single-environment call
        for s in ("degree", "first"):
            v = env.value(e, s, 0.99)
            if not v == grp.want[s][e]:
                bad.append(("value", s, e))
    if not same_doubles(env.values("degree", 0.9), grp.want09):
        bad.append(("values", "degree, gamma 0.9"))
    if not same_doubles(_values_device(env, "degree", 0.9), grp.want09):
        bad.append(("values_device", "degree, gamma 0.9"))
    assert not bad, (name, bad)
    # the valued environments are untouched, their reducer order is still the stable one
    assert np.array_equal(env.observations(OBS_ROWS), obs0) and np.array_equal(env.stats(), stats0), name
    assert np.array_equal(obs0, twin.observations(OBS_ROWS)), name
    assert all(_reducer_orders(env, grp)), name
    for _ in range(3):
        a, b = env.rollout("random", 1, auto_reset=True), twin.rollout("random", 1, auto_reset=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
        assert np.array_equal(env.observations(OBS_ROWS), twin.observations(OBS_ROWS)), name
    assert np.array_equal(env.stats(), twin.stats()), name
    print(name, "wall time %.2f s" % (time.perf_counter() - t0))


RANDOM = ("fast|3-3-20-uniform", "fast_spill|3-5-18-maximum", "binom_hbm|5-2-24-weighted", "general|3-3-20-0.5-uniform", "listed_mixed",
          "listed_16_plus_one_step_general")


@pytest.mark.parametrize("name", RANDOM)
def test_seeded_random_rollouts_from_tied_bases(groups, name):
    """value('random') under buchberger(G, P, Random, seed) from the oracle's state; seeds 0, 2^31 - 1 and -1 exercise
    seed -> engine state.  Random selection draws pairs, the reducers still start from std::sort's order."""
    bo = ffi.load("bo")
    grp = groups[name]
    B = grp.batch
    env = _make(grp)
    seeds = np.random.default_rng(12).integers(-2 ** 31, 2 ** 31 - 1, size=B)
    seeds[:3] = (0, 2147483647, -1)

    def ret(e, selection, seed=None, mode=True):
        G, P = grp.states[e]
        st = bo.buchberger(G, P, selection=selection, seed=None if seed is None else int(seed), sort_reducers=mode, want_basis=False)[1]
        assert st["polynomial_additions"] <= V.MAX_ADDITIONS         # (checked on the CPU before anything is launched)
        return st["discounted_return"]
    want = [ret(e, "random", seeds[e]) for e in range(B)]
    mutant = [ret(e, "random", seeds[e], 2) for e in range(B)]
    print(name, "random: the stable-order mutant differs on", [e for e in range(B) if mutant[e] != want[e]])
    assert same_doubles(env.values("random", 0.99, seeds=seeds), want), name
    assert same_doubles(_values_device(env, "random", 0.99, seeds), want), name


@pytest.mark.parametrize("name", V.SAMPLE)
def test_sample_with_explicit_seeds_from_tied_bases(groups, name):
    """'sample': the best of the Degree rollout and 100 seeded Random ones, every one from std::sort's order (the CPU test
    shows that the best of the stable-order mutant's rollouts is another number for some environment of either group)."""
    grp = groups[name]
    env = _make(grp)
    seeds = V.sample_seeds(grp.batch)
    want = V.sample_values(ffi.load("bo"), grp, seeds)            # (bounded on the CPU before anything is launched)
    assert same_doubles(env.values("sample", 0.99, seeds=seeds), want), name
    assert all(_reducer_orders(env, grp)), name


@pytest.mark.parametrize("name", V.GROWTH)
def test_value_rollouts_from_tied_bases_that_outgrow_the_records(groups, name):
    """Capacities so tight that the rollouts must outgrow the records (the basis capacity is the largest valued basis; the
    oracle says how far the rollouts go beyond it): values() starts again on enlarged records, values_device() carries its
    waiting clones over at the wait.  After either, the order must still be std::sort's: the values are the oracle's."""
    grp = groups[name]
    caps, cap, peak = V.growth_caps(grp, "degree")
    env = _make(grp, caps)
    twin = env.copy()
    before = twin.capacities()
    print(name, "caps", caps, "the rollouts reach", peak, "elements; capacities before", before)
    assert before["max_basis"] == cap < peak
    got = twin.values("degree", 0.99)
    after = twin.capacities()
    assert after["grown"] > before["grown"], (before, after)
    assert same_doubles(got, grp.want["degree"]), (name, "values", np.flatnonzero(got != np.asarray(grp.want["degree"])).tolist())
    assert env.capacities() == before
    dev = _values_device(env, "degree", 0.99)
    assert same_doubles(dev, grp.want["degree"]), (name, "values_device", np.flatnonzero(dev != np.asarray(grp.want["degree"])).tolist())
    assert env.capacities()["grown"] > before["grown"], (before, env.capacities())
    for s in ("normal", "first"):                            # (the clone ring follows the new layout)
        assert same_doubles(_values_device(env, s, 0.99), grp.want[s]), (name, s)
        assert same_doubles(twin.values(s, 0.99), grp.want[s]), (name, s)
    assert all(_reducer_orders(env, grp)), name
    assert np.array_equal(env.observations(OBS_ROWS), twin.observations(OBS_ROWS)) and np.array_equal(env.stats(), twin.stats())
