"""The cases of tests/test_update_thresholds_gpu.py through the oracle alone: every case still crosses the threshold it is
there for, and the degree-limit rollouts select no pair beyond the limit — so a case that stops reaching its point fails on
a machine without a GPU, too."""
import pytest

from oracle import ffi
from tests import alg_cases as ac
from tests import test_update_thresholds_gpu as ut


@pytest.mark.parametrize("name", sorted(ut.CASES))
def test_every_case_crosses_its_threshold_on_the_oracle(name):
    ut.assert_point(name)
    for w in ut.oracle_traces(name):
        assert len(w["nG"]) == ut.CASES[name][1]


@pytest.mark.parametrize("nv", (3, 4, 8))
def test_seeded_random_rollouts_of_the_degree_limit_ideals_select_nothing_beyond_the_limit(bo, nv):
    _, F = ac.degree_limit_ideals()[nv]
    for e in range(3):
        o = bo.env(fixed=F); o.reset()
        for t in range(6):
            assert o.nP > 0
            i, j = o.pairs()[ffi.agent_action(11 + e, t, o.nP)]
            assert ac.pair_sugar(o, i, j) <= 65535, (e, t)
            o.step(ffi.agent_action(11 + e, t, o.nP))
