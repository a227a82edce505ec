"""The closed form behind the fast class's one-pass install of a reset's ideal (install_ideal in bbx_fast.h), restated in
numpy and held against the oracle: n sequential Gebauer-Moeller updates (bo_update) from an empty basis must leave
exactly the pairs — same pairs, same order — that the closed form keeps, and the reducer order is the stable sort of
the generators by lead monomial."""
import numpy as np
import pytest

from oracle import ffi
from tests.oracle_walk import grevlex_key

NV = 3


def _lcm(a, b):
    return np.maximum(a, b)


def closed_form_pairs(L):
    """L: [n, NV] lead exponents in insertion order -> the final pair list [(i, j)] in lane order j(j-1)/2 + i."""
    n = len(L)
    out = []
    for j in range(1, n):
        for i in range(j):
            Lij = _lcm(L[i], L[j])
            keep = True
            for k in range(n):
                Lkj = _lcm(L[k], L[j])
                eq = bool((Lkj == Lij).all())
                if k < j:
                    if ((Lkj <= Lij).all() and not eq) or (eq and (k < i or not np.minimum(L[k], L[j]).any())):
                        keep = False
                elif k > j:
                    if (L[k] <= Lij).all() and not eq and not (Lij == _lcm(L[i], L[k])).all():
                        keep = False
            if keep:
                out.append((i, j))
    return out


def closed_form_rank(L):
    """rank(f) = #{k : LM_k < LM_f} + #{k < f : LM_k == LM_f} (std::upper_bound insertion)."""
    keys = [grevlex_key(e) for e in L]
    return [sum(1 for k in range(len(L)) if keys[k] < keys[f]) + sum(1 for k in range(f) if keys[k] == keys[f]) for f in range(len(L))]


def sequential(bo, F):
    G, P = [], []
    for f in F:
        G, P = bo.update(G, P, f)
    return P


def _check_ideal(bo, F):
    L = np.array([f[0][1][:NV] for f in F], dtype=np.int64)
    assert closed_form_pairs(L) == sequential(bo, F)
    want = sorted(range(len(F)), key=lambda f: grevlex_key(L[f]))          # stable sort by lead monomial
    rank = closed_form_rank(L)
    assert [want.index(f) for f in range(len(F))] == rank


def _ideals(bo, dist, count, seed):
    g = bo.generator(dist)
    g.seed(seed)
    return [g.next() for _ in range(count)]


@pytest.mark.parametrize("dist,count", [("3-20-10-weighted", 4000)] +
                         [("3-20-%d-%s" % (n, kind), 400) for kind in ("weighted", "uniform") for n in range(1, 12)])
def test_closed_form_equals_sequential_updates(dist, count):
    bo = ffi.load("bo")
    for F in _ideals(bo, dist, count, 12345):
        _check_ideal(bo, F)


def _binomial(lead, tail):
    return [(1, tuple(lead) + (0,) * (8 - len(lead))), (7, tuple(tail) + (0,) * (8 - len(tail)))]


HARD = {
    "equal leads": [((2, 1, 0), (0, 0, 1)), ((2, 1, 0), (1, 0, 0)), ((2, 1, 0), (0, 1, 0)), ((1, 1, 1), (0, 0, 0))],
    "coprime leads": [((3, 0, 0), (0, 0, 0)), ((0, 2, 0), (0, 0, 1)), ((0, 0, 4), (1, 0, 0)), ((1, 1, 0), (0, 0, 0))],
    "equal lcms in one bucket": [((2, 0, 0), (0, 0, 0)), ((0, 2, 0), (0, 0, 0)), ((2, 2, 0), (0, 0, 1)), ((1, 2, 0), (0, 0, 0)),
                                 ((2, 1, 0), (0, 0, 0)), ((2, 2, 1), (0, 0, 0))],
    "divisibility chain": [((1, 0, 0), (0, 0, 0)), ((2, 0, 0), (0, 1, 0)), ((3, 0, 0), (0, 0, 1)), ((3, 1, 0), (0, 0, 0)),
                           ((3, 1, 1), (0, 0, 0)), ((4, 1, 1), (0, 0, 0))],
    "eleven generators": [((a, b, c), (0, 0, 0)) for a, b, c in
                          [(3, 0, 0), (0, 3, 0), (0, 0, 3), (1, 1, 1), (2, 1, 0), (1, 2, 0), (0, 1, 2), (2, 0, 1), (1, 1, 1), (3, 1, 0), (0, 3, 1)]],
}


@pytest.mark.parametrize("name", sorted(HARD))
def test_closed_form_hard_cases(name):
    bo = ffi.load("bo")
    gens = HARD[name]
    rng = np.random.default_rng(len(name))
    for trial in range(40):                              # every case in a few insertion orders
        order = list(range(len(gens))) if trial == 0 else list(rng.permutation(len(gens)))
        _check_ideal(bo, [_binomial(*gens[o]) for o in order])
