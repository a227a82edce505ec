"""The cases of tests/value_tie_cases.py, checked on the CPU with the oracle alone: every environment is a state in which
buchberger()'s std::sort of the reducers and the environment's stable order differ, and one whose value a rollout from the
stable order (the oracle's mutant mode sort_reducers=2) gets wrong; the oracle additions the cases rest on."""
import time

import numpy as np
import pytest

from tests import value_tie_cases as V


@pytest.fixture(scope="module")
def groups(bo):
    t0 = time.perf_counter()
    V.build.cache_clear()                                     # (time a real build, not another module's cached one)
    g = V.build()
    return g, time.perf_counter() - t0


def test_build_takes_a_few_seconds(groups):
    _, seconds = groups
    print("case build: %.2f s" % seconds)
    assert seconds < 10.0


def test_every_group_has_its_environments(groups):
    g, _ = groups
    for name, grp in g.items():
        assert V.MIN_ENVS <= grp.batch <= 32, name
        assert all(len(a) == grp.batch for a in grp.actions) and len(grp.actions) <= 3, name
        assert all(len(grp.want[s]) == grp.batch for s in V.STRATEGIES) and len(grp.want09) == grp.batch, name
        assert grp.max_additions <= V.MAX_ADDITIONS, name
        assert not np.isnan([grp.want[s] for s in V.STRATEGIES]).any(), name
    # every kernel class and shape the cases are there for
    need = ["fast|3-3-20-uniform", "fast|3-5-18-maximum", "fast_spill|3-3-20-uniform", "binom_hbm_w2|3-5-18-maximum",
            "general_class|3-3-20-uniform", "binom_hbm|4-2-20-uniform", "binom_hbm|5-2-24-weighted", "binom_hbm|8-2-24-uniform",
            "general|3-3-20-0.5-uniform", "general|4-2-18-0.5-uniform", "listed_mixed", "listed_mixed_general",
            "listed_16_plus_one_step", "listed_16_control", "fast_sort_input|3-3-20-uniform", "listed_sort_input", "listed_heapsort"]
    assert not [n for n in need if n not in g]
    assert sorted(len(F) for F in g["listed_mixed"].ctor)[:4] == [17, 18, 19, 24] and {32, 33, 64}.issubset({len(F) for F in g["listed_mixed"].ctor})
    for name in ("listed_mixed", "listed_sort_input", "listed_16_plus_one_step"):
        for F in g[name].ctor:                                # tie groups of 2 to 5 generators, 2 to 4 terms
            leads = [f[0][1] for f in F]
            sizes = {leads.count(m) for m in set(leads)}
            assert max(sizes) >= 2 and max(sizes) <= 5 and all(2 <= len(f) <= 4 for f in F), name
            assert any(f[0][0] != 1 for f in F), name         # lead coefficients other than 1


def test_tie_size_and_order_conditions(groups, bo):
    g, _ = groups
    for name, grp in g.items():
        for e, (G, P) in enumerate(grp.states):
            ngen = len(grp.ctor[e]) if grp.listed else int(grp.ctor.split("-")[2])
            assert V.has_generator_tie(G, ngen), (name, e)
            assert len(P) > 0 and len(G) == grp.envs[e].nG, (name, e)
            std, stable = bo.sort_order(G), V.stable_order(G)
            assert np.array_equal(stable, grp.envs[e].reducer_order()), (name, e)     # the environment keeps the stable order
            assert sorted(std.tolist()) == list(range(len(G))), (name, e)
            if grp.control:
                assert len(G) == 16 and np.array_equal(std, stable), (name, e)
            else:
                assert len(G) > 16 and not np.array_equal(std, stable), (name, e)
                assert grp.order_differs[e] and grp.tie[e], (name, e)


def test_the_stable_order_mutant_gets_every_environment_wrong(groups, bo):
    g, _ = groups
    for name, grp in g.items():
        wrong = 0
        for e, (G, P) in enumerate(grp.states):
            for s in V.PROBED:
                true = bo.buchberger(G, P, selection=s, sort_reducers=True, want_basis=False)[1]["discounted_return"]
                mutant = bo.buchberger(G, P, selection=s, sort_reducers=2, want_basis=False)[1]["discounted_return"]
                # sort_reducers=1 through bo.buchberger reproduces the environment's value()
                assert true == grp.want[s][e] == grp.true_probe[s][e] == grp.envs[e].value(s, 0.99), (name, e, s)
                assert mutant == grp.mutant[s][e], (name, e, s)
                assert (mutant != true) == (s in grp.sensitive[e]), (name, e, s)
            wrong += bool(grp.sensitive[e])
            assert grp.want["env"][e] == grp.want["first"][e], (name, e)
        if grp.control:
            assert wrong == 0, name                           # 16 elements: the orders agree, and so do the values
        else:
            assert wrong == grp.batch >= V.MIN_ENVS, (name, wrong)


def test_mutant_mode_is_the_environment_order_and_leaves_the_other_modes_alone(groups, bo):
    """sort_reducers=2 starts from gord_insert_sorted of every element in basis order; an environment built with it values
    its clones from its own order.  0 and 1 behave as before: 1 equals the environment's value(), 0 (basis order) is a third
    answer on at least one case."""
    g, _ = groups
    grp = g["fast|3-3-20-uniform"]
    third = 0
    for e in range(grp.batch):
        o = grp.oracle_env(bo, e, sort_reducers=2)
        o.reset()
        for t in range(len(grp.actions)):
            o.step(grp.actions[t][e])
        assert np.array_equal(o.reducer_order(), grp.envs[e].reducer_order())
        G, P = grp.states[e]
        for s in V.PROBED:
            assert o.value(s, 0.99) == grp.mutant[s][e]
            unsorted = bo.buchberger(G, P, selection=s, sort_reducers=False, want_basis=False)[1]["discounted_return"]
            third += unsorted not in (grp.mutant[s][e], grp.true_probe[s][e])
    assert third > 0


def test_heapsort_fallback_is_entered_by_the_oracle_on_the_killer_case(groups, bo):
    g, _ = groups
    grp = g["listed_heapsort"]
    for e, (G, P) in enumerate(grp.states):
        n = len(G)
        entered, depth = V.enters_heapsort(bo, G)
        print("listed_heapsort env %d: %d elements, depth limit %d, deepest level %d, heapsort %s" % (e, n, 2 * (n.bit_length() - 1), depth, entered))
        assert entered and depth == 2 * (n.bit_length() - 1)
        bo.stat_sort(True)                                    # the statistic is per rollout too: cleared, then set by value()
        grp.envs[e].value("degree", 0.99)
        assert bo.stat_sort(True)[0] > 0
    # and an ordinary case does not: the statistic tells the two apart
    G, _ = g["listed_mixed"].states[4]
    assert len(G) == 64 and V.enters_heapsort(bo, G) == (False, V.enters_heapsort(bo, G)[1])
    assert V.enters_heapsort(bo, G)[1] < 12


def test_sample_of_the_mutant_is_another_number(groups, bo):
    g, _ = groups
    for name in V.SAMPLE:
        seeds = V.sample_seeds(g[name].batch)
        true, mutant = V.sample_values(bo, g[name], seeds), V.sample_values(bo, g[name], seeds, sort_reducers=2)
        print(name, "sample: the mutant differs on", [e for e in range(g[name].batch) if true[e] != mutant[e]])
        assert any(t != m for t, m in zip(true, mutant)), name


def test_growth_caps_come_from_the_oracle(groups):
    g, _ = groups
    for name in V.GROWTH:
        caps, cap, peak = V.growth_caps(g[name], "degree")
        print(name, caps, "largest basis reached", peak)
        assert cap % 2 == 0 and cap >= max(len(G) for G, _ in g[name].states) and peak > cap
