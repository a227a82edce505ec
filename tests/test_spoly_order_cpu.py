"""The lean kernels of the fast class no longer put the S-polynomial's two scaled tails in order on the vector unit: they
enter the reduction loop's assembly as they come and are ordered by the loop's own exchange code (FA_ORDER, bbx_fast.h),
which until now only ever saw the new term of a reduction round next to the old tail term.  This file asserts, on the
oracle alone, that the seeds tests/test_spoly_order_gpu.py runs select pairs of every kind that code has to tell apart:
both members with tails and the first scaled tail leading, the second leading, equal monomials with a non-zero and with
a zero coefficient sum (h = 0 before any reduction), the first member without a tail, the second without one, neither
with one.  (Ideal seeds 1000 .. 12999 with agent seed = ideal seed - 993 were searched, 256 steps each: 4798 of them show
all seven; eight are fixed here.  A seed that stops showing a kind fails the test, it is never skipped.)"""
import functools

import numpy as np

from tests import oracle_walk as ow

DIST, K, T, P = "3-20-10-weighted", 2, 256, 32003
SEEDS = ((1000, 7), (1001, 8), (1002, 9), (1003, 10), (1006, 13), (1010, 17), (1012, 19), (1015, 22))
KINDS = ("first_leads", "second_leads", "nonzero_sum", "zero_sum", "first_tailless", "second_tailless", "both_tailless")
# first occurrences the search reported for (1000, 7), re-asserted below
KNOWN_FIRST = {"first_leads": 0, "second_leads": 1, "zero_sum": 8, "second_tailless": 41, "both_tailless": 48, "nonzero_sum": 144,
               "first_tailless": 209}


def pair_kind(o, i, j):
    """What the S-polynomial of basis elements i, j is made of (buchberger.cpp:18-21 on binomials): the lead terms cancel,
    a = (tc_i / lc_i) tail_i lcm / LM_i and b = -(tc_j / lc_j) tail_j lcm / LM_j remain."""
    (ci, ei), (cj, ej) = o.poly(int(i)), o.poly(int(j))
    ti, tj = len(ci) > 1, len(cj) > 1
    if not ti or not tj:
        return "both_tailless" if not ti and not tj else ("first_tailless" if not ti else "second_tailless")
    lcm = np.maximum(ei[0], ej[0])
    am, bm = ei[1] + lcm - ei[0], ej[1] + lcm - ej[0]
    if ow.grevlex_key(am) != ow.grevlex_key(bm):
        return "first_leads" if ow.grevlex_key(am) > ow.grevlex_key(bm) else "second_leads"
    ac = int(ci[1]) * pow(int(ci[0]), P - 2, P) % P
    bc = (P - int(cj[1]) * pow(int(cj[0]), P - 2, P) % P) % P
    return "zero_sum" if (ac + bc) % P == 0 else "nonzero_sum"


def selected_kind(o, t, action):
    """walk()'s before hook: the kind of the pair the step selects"""
    return pair_kind(o, *o.pairs()[action])


@functools.lru_cache(maxsize=None)
def walk(seed, aseed, nsteps=T):
    """nsteps steps of the hash agent with auto-reset on the oracle: (the environment as it stands afterwards, per-step
    rewards, done flags, the kind of every selected pair)."""
    o, rewards, dones, seen = ow.walk(DIST, seed, aseed, nsteps, (selected_kind, None))
    return o, rewards, dones, [kind for kind, _ in seen]


def test_every_seed_selects_pairs_of_every_kind():
    assert len(SEEDS) == len(set(SEEDS)) == 8
    for sa in SEEDS:
        _, _, dones, kinds = walk(*sa)
        assert set(kinds) == set(KINDS), (sa, sorted(set(KINDS) - set(kinds)))
        assert dones.sum() >= 1, sa                              # episodes end inside the run: resets install new ideals


def test_first_occurrences_on_the_first_seed():
    kinds = walk(*SEEDS[0])[3]
    assert {k: kinds.index(k) for k in KINDS} == KNOWN_FIRST


def test_a_zero_sum_ends_the_step_without_a_reduction():
    """h = 0 before any reduction: the step adds nothing to the basis and counts one addition (reward -1)."""
    seen = ow.walk(DIST, *SEEDS[0], T, (lambda o, t, a: (pair_kind(o, *o.pairs()[a]), o.nG), lambda o, t, a, r: (o.nG, r)))[3]
    zero = [(t, nG, after) for t, ((kind, nG), after) in enumerate(seen) if kind == "zero_sum"]
    for t, nG, after in zero:
        assert after == (nG, -1.0), t
    assert len(zero) >= 1
