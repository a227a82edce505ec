"""The case builders of tests/alg_cases.py through the oracle alone: every condition that makes the device cases of
tests/test_alg_parity.py mean something is asserted here, so a case that silently degenerates fails on a machine without a GPU."""
import numpy as np
import pytest

from tests import alg_cases as ac

NVS = (3, 4, 7, 8)


@pytest.mark.parametrize("nv", NVS)
def test_merge_totals_and_lengths_are_the_planned_ones(bo, nv):
    """A.n + B.n hits every planned value exactly, in both layouts; the oracle's sums have the planted lengths; the shifted
    pairs put a cancelling pair on positions 183 / 184 and 11 591 / 11 592 of the merged sequence."""
    cases = ac.binop_cases(nv, False) + ac.binop_cases(nv, True)
    assert sorted({c[3] for c in cases}) == sorted(ac.MERGE_TOTALS)
    for kind in ("disjoint", "shared"):
        assert [c[3] for c in cases if c[0].startswith(kind)] == list(ac.MERGE_TOTALS)
    for label, A, B, total, nsum in cases + ac.boundary_cases(nv):
        assert len(A) + len(B) == total, label
        assert len(bo.binop("poly_add", A, B)) == nsum, label
        assert max(len(e) for _, e in A + B) == 8 and max(max(i for i, x in enumerate(e) if x) for _, e in A + B if any(e)) == nv - 1, label
    for label, A, B, total, nsum in cases:
        if label.startswith("shared"):
            assert {e for _, e in B} <= {e for _, e in A} and len(bo.binop("poly_sub", A, B)) == nsum, label
        else:
            assert not ({e for _, e in A} & {e for _, e in B}), label
    by = {c[0]: c for c in ac.boundary_cases(nv)}
    assert by["planted-all"][4] == 0 and bo.binop("poly_add", by["planted-all"][1], by["planted-all"][2]) == []
    assert 0 < by["planted-half"][4] < len(by["planted-half"][1])
    assert (len(by["zero-right"][1]) > 5000 and by["zero-right"][2] == []) and (len(by["zero-left"][2]) > 5000 and by["zero-left"][1] == [])
    for label, cancel in (("shifted-241", (ac.MT,)), ("shifted-11801", (ac.MT, ac.BATCH_TILES * ac.MT))):
        _, A, B, _, _ = by[label]
        merged = sorted([(ac.lead_key([t]), 0, t) for t in A] + [(ac.lead_key([t]), 1, t) for t in B], key=lambda r: (tuple(-x for x in r[0]), r[1]))
        for p in range(2, len(merged), 2):                  # every even position holds the B copy of the monomial in front of it
            (ka, sa, ta), (kb, sb, tb) = merged[p - 1], merged[p]
            assert (sa, sb) == (0, 1) and ta[1] == tb[1], (label, p)
            assert ((ta[0] + tb[0]) % ac.P == 0) == (p in cancel), (label, p)


def test_term_limit_case_has_exactly_the_limit_and_one_more(bo):
    A, B, t = ac.term_limit_case()
    assert len(bo.binop("poly_add", A, B)) == 65535
    assert len(bo.binop("poly_add", A, bo.binop("poly_add", B, t))) == 65536


@pytest.mark.parametrize("nv", (3, 8))
@pytest.mark.parametrize("n", ac.TIE_SIZES)
def test_tie_bases_tie_and_keep_what_divisibility_says(bo, nv, n):
    """At least half of the elements share their lead monomial with another one; minimalize keeps 8 or more elements (a
    basis of fewer than 16 elements cannot both tie half of them and keep 8: there, and with all lead monomials equal, it keeps
    one per distinct minimal lead monomial); the kept lead monomials are exactly the minimal ones under divisibility, found
    without any sort, and every kept polynomial is one of the inputs."""
    for order, G in ac.tie_cases(nv, n).items():
        leads = [g[0][1] for g in G]
        assert all(any(e) for e in leads)
        if n >= 2:
            assert 2 * sum(1 for e in leads if leads.count(e) > 1) >= n, order
        kept = bo.minimalize(G)
        want = ac.minimal_leads(G)
        assert sorted(g[0][1] for g in kept) == sorted(want), order
        assert all(g in G for g in kept), order
        if order == "all-equal":
            assert len(set(leads)) == 1 and len(kept) == 1
        elif n >= 16:
            assert len(kept) >= 8, order
    if n >= 33:                                              # some elements lead with a proper multiple: minimalize has to discard them
        G = ac.tie_cases(nv, n)["given"]
        assert len(ac.minimal_leads(G)) < len({g[0][1] for g in G})


@pytest.mark.parametrize("nv", (3, 8))
def test_update_cases_drop_emit_and_share_buckets(bo, nv):
    """Under Gebauer-Moeller, every case with 64 or more elements and 255 or more old pairs: the oracle drops an old pair, emits
    a new one, and meets a bucket of two or more equal lcms with a member coprime to f."""
    cases = ac.update_cases(nv)
    assert sorted({len(G) for _, G, _, _ in cases}) == [0, 1, 63, 64, 65, 128, 129, 512, 513, 700]
    assert sorted({len(Pl) for _, _, Pl, _ in cases}) == [0, 1, 255, 256, 257, 3000]
    for label, G, Pl, f in cases:
        assert len(set(Pl)) == len(Pl) and all(0 <= i < j < len(G) for i, j in Pl), label
        if label == "constant-f":
            assert not any(f[0][1])
            continue
        if len(G) < 64 or len(Pl) < 255:
            continue
        G2, P2 = bo.update(G, Pl, f, "gebauermoeller")
        old = [p for p in P2 if p[1] < len(G)]
        new = [p for p in P2 if p[1] == len(G)]
        dropped, cp_buckets = ac.gm_facts(G, Pl, f)
        assert len(old) < len(Pl) and len(Pl) - len(old) == dropped, label
        assert len(new) >= 1 and len(G2) == len(G) + 1, label
        assert cp_buckets >= 1, label


@pytest.mark.parametrize("nv", (3, 4, 8))
def test_degree_limit_ideals_are_within_the_limits_and_their_lcms_are_not(bo, nv):
    """Generators within the documented limits; lcm(0, 2) beyond 65 535, a proper multiple of lcm(1, 2), which is not; for 4
    and 8 variables the low halves of two different words of the packed lcm sum past 65 535.  The reference's update drops
    the pair (0, 2) — under Gebauer-Moeller only — and an environment's first six steps under the first-pair rule select no
    pair whose sugar passes the limit while the basis keeps meeting lcms that do."""
    n, F = ac.degree_limit_ideals()[nv]
    assert n == nv and all(max(e) <= 65535 and sum(e) <= 65535 for f in F for _, e in f)
    assert [bo.polylist([f]).get(0) for f in ac.padded(F)] == ac.padded(F)           # (terms in descending order as written)
    lm = [f[0][1] for f in F]
    big, small = ac.lcm_degree(lm[0], lm[2]), ac.lcm_degree(lm[1], lm[2])
    assert big > 65535 >= small and ac.lcm_degree(lm[0], lm[1]) <= 65535
    l02, l12 = [max(x, y) for x, y in zip(lm[0], lm[2])], [max(x, y) for x, y in zip(lm[1], lm[2])]
    assert l02 != l12 and all(x <= y for x, y in zip(l12, l02))
    assert (big & 0xffff) < small                                                      # a 16-bit degree would order them the other way
    if nv > 3:
        words = [ac.pad(l02)[2 * w] for w in range(4)]                                 # the low halves of the words
        assert sum(1 for x in words if x >= 30000) == 2 and sum(words[:-1] if nv == 4 else words) > 65535
    G = ac.padded(F)
    assert bo.update(G[:2], [(0, 1)], G[2], "gebauermoeller")[1] == [(0, 1), (1, 2)]
    for elim in ("lcm", "none"):
        assert bo.update(G[:2], [(0, 1)], G[2], elim)[1] == [(0, 1), (0, 2), (1, 2)]
    o = bo.env(fixed=F); o.reset()
    assert o.nG == 3 and o.pairs().tolist() == [[0, 1], [1, 2]]
    beyond = 0
    for t in range(6):
        assert o.nP > 0
        i, j = o.pairs()[0]
        assert ac.pair_sugar(o, i, j) <= 65535, t
        nG = o.nG
        o.step(0)
        if o.nG > nG:
            new = [int(x) for x in o.poly(nG)[1][0]]
            beyond += sum(1 for g in range(nG) if ac.lcm_degree([int(x) for x in o.poly(g)[1][0]], new) > 65535)
    assert beyond >= 3


def test_hard_limit_ideal_has_one_pair_beyond_the_limit(bo):
    F = ac.hard_limit_ideal()
    o = bo.env(fixed=F); o.reset()
    assert o.pairs().tolist() == [[0, 1]] and ac.lcm_degree(F[0][0][1], F[1][0][1]) == 80001 and ac.pair_sugar(o, 0, 1) == 80001


@pytest.mark.parametrize("nv", NVS)
def test_reduce_and_interreduce_cases_do_work(bo, nv):
    """Several divisors divide the dividend's lead term; the growing case's intermediate results are many times its length;
    the interreduce basis is minimal, has 65 or more elements and its interreduction changes it."""
    rng = np.random.default_rng(7)
    for ndiv in (65, 128, 200):
        F, g = ac.reduce_case(bo, nv, ndiv, rng)
        assert sum(1 for f in F if all(x <= y for x, y in zip(f[0][1], g[0][1]))) >= 2 or ndiv == 65, ndiv
        r, steps = bo.reduce(g, F)
        assert steps >= 1
    F, g = ac.growing_reduce_case(bo, rng)
    bo.fn("stat_max_terms")(1)
    r, steps = bo.reduce(g, F)
    assert bo.fn("stat_max_terms")(1) > 8 * max(len(g), len(F[0])) and steps > 20
    G = ac.interreduce_case(nv)
    assert len(G) >= 65 and bo.minimalize(G) == G and min(len(g) for g in G) >= 25
    assert bo.interreduce(G) != G


def test_pair_set_is_distinct_and_in_range():
    rng = np.random.default_rng(3)
    for m, count in ((2, 1), (3, 3), (64, 255), (700, 3000), (78, 3003)):
        Pl = ac.pair_set(m, count, rng)
        assert len(Pl) == count == len(set(Pl)) and all(0 <= i < j < m for i, j in Pl)


def test_mirror_carries_sugars_through_operations(bo):
    """The mirror keeps a result's sugar (max of the operands') when the result feeds a later operation — the high-level
    wrappers of oracle/ffi.py rebuild their operands and would reset it to the lead term's degree."""
    x3, y, one = [(1, ac.pad((3,)))], [(1, ac.pad((0, 1)))], [(1, ac.pad(()))]
    m = ac.Mirror(bo, [x3 + y, x3, y + one])
    m.binop("sub", 0, 1)                                    # y, with sugar 3
    assert m.polys()[3] == y and m.sugars()[3] == 3
    m.binop("mul", 2, 3)                                    # y^2 + y: every term of y + 1 times (y with sugar 3): 1 + 3
    assert m.sugars()[4] == 4 and len(m.polys()[4]) == 2
    steps = m.reduce(4, 4)                                  # by [x^3 + y, x^3, y + 1, y]: y + 1 divides first
    assert steps >= 1 and len(m) == 6


def test_ref_agrees_where_it_is_available(bo):
    from oracle import ffi
    if not ffi.available("ref"):
        pytest.skip("the compiled reference is not on this machine")
    ref = ffi.load("ref")
    rng = np.random.default_rng(9)
    G = ac.tie_cases(3, 100)["given"]
    assert ref.minimalize(G) == bo.minimalize(G)
    _, G, Pl, f = ac.update_cases(3)[4]
    for elim in ("gebauermoeller", "lcm", "none"):
        assert ref.update(G, Pl, f, elim) == bo.update(G, Pl, f, elim)
    F, g = ac.reduce_case(bo, 4, 128, rng)
    assert ref.reduce(g, F) == bo.reduce(g, F)
