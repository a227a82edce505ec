"""The batched polynomial algebra on the device (bbx_alg_* through deepgroebner_amd.PolyLists; csrc/bbx_algebra.hip) against
the oracle at its edges: merge dispatch and tile boundaries, lists that grow in the middle of a batch, sugars, the three
updates beyond one ballot / one unrolled trip / the on-chip limit, minimalize among equal lead monomials, the 16-bit limits,
zero polynomials.  The cases are those of tests/alg_cases.py (tests/test_alg_cases_cpu.py checks that they are what they
claim to be); every comparison is of the WHOLE list with a mirrored oracle list — number of elements, every polynomial, every
sugar, step counts and pair lists in order — and exact."""
import numpy as np
import pytest

from tests import alg_cases as ac

pytestmark = pytest.mark.gpu
NVS = (3, 4, 7, 8)


def handle(bo, lists):
    from deepgroebner_amd import PolyLists
    return PolyLists(lists), [ac.Mirror(bo, l) for l in lists]


def check(L, mirrors, what):
    for k, m in enumerate(mirrors):
        diff = ac.same_state(L, k, m)
        assert diff is None, (what, diff)


def binop(L, mirrors, op, ij):
    ij = [tuple(ij)] * len(mirrors) if isinstance(ij[0], int) else ij
    L.binop(op, ij)
    for m, (i, j) in zip(mirrors, ij):
        m.binop(op, i, j)


def reduce(L, mirrors, args, what):
    steps = L.reduce(args)
    want = [m.reduce(g, nF) for m, (g, nF) in zip(mirrors, args)]
    assert [int(s) for s in steps] == want, (what, "steps")


# ---- binary operations ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("large", (False, True))
@pytest.mark.parametrize("nv", NVS)
def test_binops_at_every_merge_total(bo, nv, large):
    """add, sub, spoly (and mul, on the short ones) of every planned A.n + B.n — disjoint monomials and all monomials shared,
    one batch per number of variables (W = 2, 4, 4, 8), so that lists of very different lengths share a launch."""
    cases = ac.binop_cases(nv, large)
    if large:
        cases = cases + [c for c in ac.boundary_cases(nv) if c[1] and c[2]]
    L, mirrors = handle(bo, [[A, B] for _, A, B, _, _ in cases])
    for op in ("add", "sub", "spoly") + (() if large else ("mul",)):
        binop(L, mirrors, op, (0, 1))
    binop(L, mirrors, "sub", (1, 0))
    check(L, mirrors, [c[0] for c in cases])


@pytest.mark.parametrize("nv", NVS)
def test_zero_and_self_operands(bo, nv):
    """A zero polynomial on either side of more than 5 000 terms (the empty-operand branch of the merge dispatch) under +, -
    and *; f - f, f + (-f), spoly(f, f), f * f, 0 * 0."""
    rng = np.random.default_rng(30 + nv)
    big = ac.boundary_cases(nv)[2][1]
    f = ac.poly_from(bo, ac.monomial_pool(nv, 900), 150, rng)
    negf = [((ac.P - c) % ac.P, e) for c, e in f]
    L, mirrors = handle(bo, [[big, []], [f, negf]])
    for op in ("add", "sub", "mul"):
        binop(L, mirrors, op, [(0, 1), (0, 1)])            # f + (-f) = 0, f - (-f), f * (-f)
        binop(L, mirrors, op, [(1, 0), (1, 0)])
        binop(L, mirrors, op, [(1, 1), (0, 0)])            # 0 op 0; f op f
    binop(L, mirrors, "spoly", [(0, 0), (0, 0)])
    check(L, mirrors, "zero / self")
    assert L.get(0)[2] == big and L.get(1)[2] == [] and L.get(1)[-1] == []


@pytest.mark.parametrize("nv", NVS)
def test_products(bo, nv):
    """A single-term operand on either side; a 200 x 200 product of sparse polynomials, whose intermediate sums outgrow the
    record's scratch polynomials several times (2 x 200 terms at creation, tens of thousands in the end)."""
    rng = np.random.default_rng(40 + nv)
    pool = ac.monomial_pool(nv, 30000)
    f, g = ac.poly_from(bo, pool, 200, rng), ac.poly_from(bo, pool, 200, rng)
    one = [(int(rng.integers(1, ac.P)), pool[777])]
    L, mirrors = handle(bo, [[f, g], [f, one], [one, one]])
    binop(L, mirrors, "mul", (0, 1))
    binop(L, mirrors, "mul", (1, 0))
    check(L, mirrors, "products")
    assert len(L.get(0)[2]) > 16 * 400


@pytest.mark.parametrize("batch,nv", ((1, 3), (3, 4), (4, 7), (5, 8), (257, 3)))
def test_uneven_batch_only_one_list_grows(bo, batch, nv):
    """One list three orders of magnitude larger than the rest: only it runs out of room and has the operation again, the
    others must neither be appended to twice nor lose an element when the records are laid out anew."""
    rng = np.random.default_rng(50 + batch)
    pool = ac.monomial_pool(nv, 60000)
    small = [[ac.poly_from(bo, pool[:200], 5, rng), ac.poly_from(bo, pool[:200], 3, rng)] for _ in range(min(batch, 6))]
    lists = [small[k % len(small)] for k in range(batch)]
    lists[batch // 2] = [ac.poly_from(bo, pool, 5000, rng), ac.poly_from(bo, pool[:5000], 3, rng)]
    L, mirrors = handle(bo, lists)
    binop(L, mirrors, "mul", (0, 1))
    binop(L, mirrors, "add", (2, 0))
    reduce(L, mirrors, [(2, 2)] * batch, "uneven")
    check(L, mirrors, "uneven batch of %d" % batch)
    assert len(L.get(batch // 2)[2]) > 2 * 5000


@pytest.mark.parametrize("nv", NVS)
def test_chain_of_operations_on_one_handle(bo, nv):
    """36 random operations on one handle, results feeding later operands (with the sugars they were given), the whole
    state against the mirror after every one."""
    rng = np.random.default_rng(60 + nv)
    pool = ac.monomial_pool(nv, 400)
    lists = [[ac.poly_from(bo, pool, int(rng.integers(1, 30)), rng) for _ in range(4)] for _ in range(3)]
    L, mirrors = handle(bo, lists)
    for step in range(36):
        op = ("add", "sub", "mul", "spoly", "reduce")[int(rng.integers(0, 5))]
        args = []
        for m in mirrors:
            n = len(m)
            sizes = [m.nterms(i) for i in range(n)]
            if op == "reduce":
                args.append((int(rng.integers(0, n)), int(rng.integers(0, n + 1))))
                continue
            ok = [i for i in range(n) if (op != "spoly" or sizes[i] > 0) and (op != "mul" or sizes[i] <= 60)]
            args.append((ok[int(rng.integers(0, len(ok)))], ok[int(rng.integers(0, len(ok)))]))
        if op == "reduce":
            reduce(L, mirrors, args, (step, op, args))
        else:
            binop(L, mirrors, op, args)
        check(L, mirrors, (step, op, args))


# ---- limits ------------------------------------------------------------------------------------------------------------------------

def refused(L, mirrors, call, mirror_call, bad, follow):
    """`call` must be refused because of list `bad`.  Afterwards every list reads back as what is on the device: the refused
    one unchanged, the others with their result or unchanged — and consistently so: the valid operation `follow` (per-list
    (op, i, j)) on the handle gives the oracle's lists.  A host mirror of the sizes that went stale on the failure path would
    show the others unchanged here and with TWO new elements after `follow`."""
    from deepgroebner_amd._ffi import BbxError
    before = [len(m) for m in mirrors]
    with pytest.raises(BbxError):
        call()
    sizes, _ = L.sizes()
    assert int(sizes[bad]) == before[bad]
    for k, m in enumerate(mirrors):
        assert int(sizes[k]) in ((before[k],) if k == bad else (before[k], before[k] + 1)), k
        if int(sizes[k]) == before[k] + 1:
            mirror_call(m)
    check(L, mirrors, "after the refused call")
    assert len({f[0] for f in follow}) == 1
    binop(L, mirrors, follow[0][0], [(i, j) for _, i, j in follow])
    check(L, mirrors, "after the call that followed the refused one")


def test_term_limit_and_the_lists_after_a_refused_call(bo):
    """A sum of exactly 65 535 terms is returned; one of 65 536 is refused (plen[] has 16 bits), and the handle stays usable and
    truthful about every list."""
    A, B, t = ac.term_limit_case()
    Bt = bo.binop("poly_add", B, t)
    a, b = A[:7], B[:5]
    L, mirrors = handle(bo, [[A, B]])
    binop(L, mirrors, "add", (0, 1))
    check(L, mirrors, "65535 terms")
    assert len(L.get(0)[2]) == 65535
    L, mirrors = handle(bo, [[a, b], [A, Bt], [b, a], [A, B]])
    refused(L, mirrors, lambda: L.binop("add", (0, 1)), lambda m: m.binop("add", 0, 1), 1,
            [("sub", 0, 1), ("sub", 0, 0), ("sub", 1, 0), ("sub", 0, 1)])


def test_exponent_above_16_bits_is_unsupported_at_create(bo):
    from deepgroebner_amd import PolyLists
    from deepgroebner_amd._ffi import BbxError
    L = PolyLists([[[(1, (65535, 0, 0))]]])
    assert L.get(0) == [[(1, ac.pad((65535,)))]] and L.sugars(0) == [65535]
    for e in ((65536, 0, 0), (0, 0, 0, 0, 0, 0, 0, 65536), (40000, 30000)):
        with pytest.raises(BbxError) as ex:
            PolyLists([[[(1, (1, 1))], [(5, e), (1, (0, 1))]]])
        assert ex.value.code == -5, e                        # BBX_E_UNSUPPORTED


def mono(v, e, nv=8):
    x = [0] * 8; x[v] = e
    return tuple(x)


@pytest.mark.parametrize("var", (0, 7))
def test_degree_and_sugar_limit(bo, var):
    """Degree / sugar of exactly 65 535 is returned by spoly, mul and reduce; 65 536 is refused, never wrapped.  var = 7: the
    only non-zero exponents sit in variable 8 (W = 8)."""
    one = (1, ac.pad(()))
    v2 = 1 if var == 0 else 6
    f = [(3, mono(var, 32768)), one]
    g_ok = [(5, mono(var if var == 7 else v2, 32767)), one]
    g_bad = [(5, mono(var if var == 7 else v2, 32768)), one]
    small = [[(2, mono(var, 2)), one], [(7, mono(var, 1))]]
    for op in ("mul", "spoly"):
        if op == "spoly" and var == 7:
            continue                                          # (one variable: the lcm is the larger power, nothing near the limit)
        L, mirrors = handle(bo, [[f, g_ok], small])
        binop(L, mirrors, op, (0, 1))
        check(L, mirrors, (op, "65535"))
        assert L.sugars(0)[2] == 65535
        L, mirrors = handle(bo, [small, [f, g_bad], small])
        refused(L, mirrors, lambda: L.binop(op, (0, 1)), lambda m: m.binop(op, 0, 1), 1, [("add", 0, 1), ("add", 0, 1), ("add", 1, 0)])
    if var == 7:
        L, mirrors = handle(bo, [[[(3, mono(7, 32768))], [(5, mono(7, 32767))]]])
        binop(L, mirrors, "mul", (0, 1))
        assert L.get(0)[2] == [(15, mono(7, 65535))] and L.sugars(0)[2] == 65535
        return
    # reduce: a divisor whose sugar (60 000, left by a cancelled lead term) is far above its degree
    for e, ok in ((5535, True), (5536, False)):
        a = [(1, mono(0, 60000)), (1, mono(1, 5535)), (1, mono(2, 1))]
        b = [(1, mono(0, 60000))]
        M = list(mono(1, 5535)); M[2] = e
        p = [(1, mono(0, 20000)), (1, tuple(M))]
        q = [(ac.P - 1, mono(0, 20000)), one]
        lists = [[a, b, p, q], [small[0], small[1], small[0], small[1]]]
        L, mirrors = handle(bo, lists)
        binop(L, mirrors, "sub", (0, 1))                     # x1^5535 + x2 with sugar 60 000
        binop(L, mirrors, "add", (2, 3))                     # x1^5535 x2^e + 1
        check(L, mirrors, "reduce operands")
        assert L.sugars(0)[4] == 60000
        if ok:
            reduce(L, mirrors, [(5, 5), (5, 5)], "sugar 65535")
            check(L, mirrors, "sugar 65535")
            assert L.sugars(0)[6] == 65535
        else:
            refused(L, mirrors, lambda: L.reduce([(5, 5), (5, 5)]), lambda m: m.reduce(5, 5), 0, [("add", 0, 1), ("add", 0, 1)])


@pytest.mark.parametrize("elimination", ("gebauermoeller", "lcm", "none"))
@pytest.mark.parametrize("nv", (3, 4, 8))
def test_update_with_lcms_beyond_the_degree_limit(bo, nv, elimination):
    """Generators within the limits whose lcm(0, 2) has degree 70 000 (3 variables) or 66 100 (4 and 8 variables: the low halves
    of two words of the packed lcm sum past 65 535) and is a proper multiple of lcm(1, 2): the reference's pair list in order
    — (0, 2) leaves under Gebauer-Moeller and stays under the other two —, beside a small list in the same batch."""
    F = ac.padded(ac.degree_limit_ideals()[nv][1])
    small = [[(2, mono(nv - 1, 2)), (1, ac.pad(()))], [(7, mono(0, 1))], [(1, mono(0, 1)), (3, mono(nv - 1, 1))]]
    L, mirrors = handle(bo, [F, small])
    got = L.update([[(0, 1)], [(0, 1)]], elimination)
    want = [m.update([(0, 1)], elimination) for m in mirrors]
    assert want[0] == ([(0, 1), (1, 2)] if elimination == "gebauermoeller" else [(0, 1), (0, 2), (1, 2)])
    assert got == want, (nv, elimination, got)
    check(L, mirrors, "update leaves the lists as they are")


# ---- reduce ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nv", NVS)
def test_reduce_cases(bo, nv):
    """nF = 0; the dividend among its divisors; 65, 128 and 200 divisors of which several divide the same term (the first in
    list order wins); a constant divisor; zero polynomials among the divisors (expected: the oracle without them); a short
    dividend whose intermediate results outgrow the scratch polynomials; a 2 000-term dividend."""
    rng = np.random.default_rng(70 + nv)
    lists, args, names = [], [], []

    def case(name, F, g, gi=None, nF=None):
        lists.append(list(F) + [g]); names.append(name)
        args.append((len(F) if gi is None else gi, len(F) if nF is None else nF))
    for ndiv in (65, 128, 200):
        F, g = ac.reduce_case(bo, nv, ndiv, rng)
        case("%d divisors" % ndiv, F, g)
    F, g = ac.reduce_case(bo, nv, 65, rng)
    case("nF = 0", F, g, nF=0)
    case("dividend among the divisors", F, g, nF=len(F) + 1)
    case("dividend is divisor 3", F, g, gi=3)
    F, g = ac.reduce_case(bo, nv, 70, rng, constant_divisor=True)
    case("constant divisor", F, g)
    F, g = ac.reduce_case(bo, nv, 130, rng, zero_at=(0, 5, 63, 64, 129))
    case("zero divisors", F, g)
    F, g = ac.growing_reduce_case(bo, rng)
    case("growing", F, g)
    F, g = ac.reduce_case(bo, nv, 200, rng, dividend_terms=2000)
    case("2000-term dividend", F, g)
    L, mirrors = handle(bo, lists)
    reduce(L, mirrors, args, names)
    check(L, mirrors, names)
    assert L.get(names.index("nF = 0"))[-1] == lists[names.index("nF = 0")][-1]


# ---- update ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("elimination", ("gebauermoeller", "lcm", "none"))
@pytest.mark.parametrize("nv", (3, 8))
def test_update_beyond_one_ballot_and_one_trip(bo, nv, elimination):
    """m = 0 .. 700 basis elements and |P| = 0 .. 3 000 old pairs in ONE batch (lists of different sizes: only some force the
    pair set to grow before the launch), lead monomials from a small pool (shared lcm buckets, members coprime to f), a
    constant f: the pair lists in order, and the lists themselves."""
    cases = ac.update_cases(nv)
    L, mirrors = handle(bo, [list(G) + [f] for _, G, _, f in cases])
    got = L.update([Pl for _, _, Pl, _ in cases], elimination)
    for k, (label, G, Pl, f) in enumerate(cases):
        assert got[k] == mirrors[k].update(Pl, elimination), (label, elimination)
    check(L, mirrors, "update leaves the lists as they are")
    binop(L, mirrors, "add", [(len(m) - 1, len(m) - 1) for m in mirrors])      # (the handle is as usable as before)
    check(L, mirrors, "after update")


# ---- minimalize / interreduce ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nv", (3, 8))
def test_minimalize_among_equal_lead_monomials(bo, nv):
    """Tie bases of 1 .. 700 elements as given, ascending, descending and with all lead monomials equal: which of the
    elements with equal lead monomials survives is what libstdc++'s introsort leaves first (insertion sort up to 16 elements,
    the partition loop above).  Then interreduce of the minimal bases."""
    names, lists = [], []
    for n in ac.TIE_SIZES:
        for order, G in ac.tie_cases(nv, n).items():
            names.append((n, order)); lists.append(G)
    L, mirrors = handle(bo, lists)
    L.minimalize()
    for m in mirrors:
        m.minimalize()
    check(L, mirrors, names)
    L.interreduce()
    for m in mirrors:
        m.interreduce()
    check(L, mirrors, names)


@pytest.mark.parametrize("nv", NVS)
def test_interreduce_of_minimal_bases(bo, nv):
    """The oracle's minimal bases of 65 or more elements with tails of dozens of terms, other elements' lead monomials among them."""
    G = ac.interreduce_case(nv)
    L, mirrors = handle(bo, [G, G[:70], list(reversed(G))])
    L.interreduce()
    for m in mirrors:
        m.interreduce()
    check(L, mirrors, "interreduce")
    L.minimalize()
    for m in mirrors:
        m.minimalize()
    check(L, mirrors, "minimalize of a reduced basis")


@pytest.mark.parametrize("nv", (4, 8))
def test_free_functions_cut_to_the_ring(bo, nv):
    """minimalize / interreduce / reduce_many / spoly_many with exponent tuples of the ring's width (4 and 8 variables)."""
    from deepgroebner_amd import interreduce, minimalize, reduce_many, spoly_many
    rng = np.random.default_rng(90 + nv)
    cut = lambda f: [(c, e[:nv]) for c, e in f]
    G = ac.tie_cases(nv, 33)["given"]
    assert minimalize([cut(g) for g in G]) == [cut(g) for g in bo.minimalize(G)]
    M = ac.interreduce_case(nv)
    assert interreduce([cut(g) for g in M]) == [cut(g) for g in bo.interreduce(M)]
    F, g = ac.reduce_case(bo, nv, 65, rng)
    F2, g2 = ac.reduce_case(bo, nv, 8, rng)
    got = reduce_many([(cut(g), [cut(f) for f in F]), (cut(g2), [cut(f) for f in F2])])
    for (r, st), (gg, FF) in zip(got, ((g, F), (g2, F2))):
        wr, ws = bo.reduce(gg, FF)
        assert r == cut(wr) and st == {"steps": ws}
    pairs = [(F[0], F[1]), (g, g2), (M[0], M[1])]
    got = spoly_many([(cut(a), cut(b)) for a, b in pairs])
    assert got == [cut(bo.spoly(a, b)) for a, b in pairs]
