"""TEST INFRASTRUCTURE — deterministic case builders for the batched polynomial algebra (bbx_alg_*, csrc/bbx_algebra.hip)
and a mirror of a device-resident list on the oracle.  Plain module, no fixtures: tests/test_alg_cases_cpu.py runs every
builder through the oracle alone and asserts what makes a case mean something, tests/test_alg_parity.py and
scripts/fuzz_algebra.py run the same cases on the device.  Everything is exact arithmetic over GF(32003).

Term lists are [(coefficient, exponent tuple of 8 slots), ...] in descending grevlex order, normalised through
bo.polylist([...]).get(0) like the random sweep of tests/test_hip_known_answers.py does."""
import functools

import numpy as np

P = 32003
NV = 8
MT = 184                          # positions per merge tile (csrc/bbx_device.h)
BATCH_TILES = 63                  # tiles per partition batch of wave_merge_tiled: 63 * 184 = 11 592 positions
# A.n + B.n of the binary-operation cases: around the dispatch threshold (64), one / two tile boundaries, the second
# partition batch, and two lengths far beyond it
MERGE_TOTALS = (63, 64, 65, MT, MT + 1, 2 * MT, 2 * MT + 1, BATCH_TILES * MT, BATCH_TILES * MT + 1, 2 * BATCH_TILES * MT + 1, 40000)
TIE_SIZES = (1, 2, 16, 17, 18, 33, 100, 700)
# (m basis elements, |P| old pairs): every m of {0, 1, 63, 64, 65, 128, 129, 512, 513, 700} and every |P| of
# {0, 1, 255, 256, 257, 3000} (m = 0, 1 admit no pair (i, j), i < j < m)
UPDATE_SHAPES = ((0, 0), (1, 0), (63, 1), (64, 255), (65, 256), (128, 257), (129, 3000), (512, 256), (513, 257), (700, 3000))


def pad(e):
    return tuple(int(x) for x in e) + (0,) * (NV - len(e))


def _of_degree(nv, d):
    if nv == 1:
        yield (d,)
        return
    for e in range(d + 1):
        for rest in _of_degree(nv - 1, d - e):
            yield (e,) + rest


@functools.lru_cache(maxsize=None)
def monomial_pool(nv, count, min_degree=0):
    """The first `count` monomials in `nv` variables by increasing degree (from min_degree), as 8-slot tuples."""
    out, d, zeros = [], min_degree, (0,) * (NV - nv)
    while len(out) < count:
        out.extend(e + zeros for e in _of_degree(nv, d))
        d += 1
    return tuple(out[:count])


def normalise(bo, terms):
    return bo.polylist([list(terms)]).get(0)


def coefs(rng, n):
    return [int(c) for c in rng.integers(1, P, size=n)]


def poly_from(bo, monos, n, rng):
    """n distinct monomials of the pool `monos`, coefficients in 1..32002."""
    idx = rng.choice(len(monos), size=n, replace=False)
    return normalise(bo, list(zip(coefs(rng, n), (monos[int(i)] for i in idx))))


def disjoint_pair(bo, nv, na, nb, rng):
    """Two polynomials of na and nb terms without a common monomial, interleaved at random in the order."""
    pool = monomial_pool(nv, na + nb + 7)
    idx = rng.permutation(len(pool))
    A = normalise(bo, list(zip(coefs(rng, na), (pool[int(i)] for i in idx[:na]))))
    B = normalise(bo, list(zip(coefs(rng, nb), (pool[int(i)] for i in idx[na:na + nb]))))
    return A, B


def shared_pair(bo, nv, n, rng, extra=0):
    """Two polynomials on the SAME n monomials (A has `extra` more of its own), no coefficient pair summing or subtracting
    to zero: A + B and A - B have n + extra terms."""
    pool = monomial_pool(nv, n + extra + 5)
    idx = rng.permutation(len(pool))
    ca = coefs(rng, n + extra)
    cb = []
    for c in ca[:n]:
        b = int(rng.integers(1, P))
        while (b + c) % P == 0 or b == c:
            b = int(rng.integers(1, P))
        cb.append(b)
    A = normalise(bo, list(zip(ca, (pool[int(i)] for i in idx[:n + extra]))))
    B = normalise(bo, list(zip(cb, (pool[int(i)] for i in idx[:n]))))
    return A, B


def planted_cancellation(bo, A, share, rng, nfresh=0, nv=3):
    """B = -A on a random `share` of A's terms plus `nfresh` terms on monomials A does not have
    -> (B, len(A + B)): the length of the sum is known in advance."""
    ncancel = int(round(share * len(A)))
    hit = rng.choice(len(A), size=ncancel, replace=False) if ncancel else []
    terms = [((P - A[int(i)][0]) % P, A[int(i)][1]) for i in hit]
    have = {e for _, e in A}
    fresh = [e for e in monomial_pool(nv, len(A) + nfresh + 3) if e not in have][:nfresh]
    terms += list(zip(coefs(rng, nfresh), fresh))
    return normalise(bo, terms), len(A) - ncancel + nfresh


def shifted_pairs(bo, S, rng, cancel_positions=()):
    """A = [one larger monomial] + S, B = S.  In the merged sequence of A and B (ties: the A term first) position 0 is the
    larger monomial and positions 2k + 1, 2k + 2 are the two copies of S[k], so every tile boundary at an even position falls
    between the two copies of one monomial.  cancel_positions: even positions p whose pair (p - 1, p) cancels exactly;
    every other pair sums to a non-zero coefficient -> (A, B, len(A + B))."""
    S = [t[1] for t in normalise(bo, [(1, e) for e in S])]
    big = list(S[0]); big[0] += 1                          # x0 * S[0]: larger than every monomial of S
    ca, cb = coefs(rng, len(S)), []
    cancel = {(p - 2) // 2 for p in cancel_positions}
    assert all(p % 2 == 0 and 0 <= (p - 2) // 2 < len(S) for p in cancel_positions)
    for k, c in enumerate(ca):
        b = P - c
        if k not in cancel:
            b = int(rng.integers(1, P))
            while (b + c) % P == 0:
                b = int(rng.integers(1, P))
        cb.append(b)
    A = normalise(bo, [(int(rng.integers(1, P)), tuple(big))] + list(zip(ca, S)))
    B = normalise(bo, list(zip(cb, S)))
    return A, B, 1 + len(S) - len(cancel)


def tie_basis(bo, nv, n, rng, pool_size=None, tails=2, multiples=True):
    """n polynomials whose lead monomials come from a small pool without the constant monomial, so that many are equal:
    the pool is an antichain (monomials of one degree, each used again and again) and, from n = 33 on, a quarter of the
    elements lead with a proper multiple of a pool monomial, which minimalize has to discard.  Tails are lower-degree
    terms that tell elements with equal lead monomials apart."""
    if pool_size is None:
        pool_size = max(1, min(n // 2, 12))
    deg = 1
    while len(list(_of_degree(nv, deg))) < 24:
        deg += 1
    anti = [pad(e) for e in _of_degree(nv, deg)][::2][:pool_size]     # (every second one of a degree with 24 or more)
    leads = [anti[k % len(anti)] for k in range(n)]
    if multiples and n >= 33:
        for k in range(3, n, 4):
            e = list(leads[k]); e[int(rng.integers(0, nv))] += 1
            leads[k] = tuple(e)
    leads = [leads[int(i)] for i in rng.permutation(n)]
    lower = monomial_pool(nv, 1 + nv + (nv * (nv + 1) // 2 if deg > 2 else 0))   # degrees 0..2, all below the leads'
    out = []
    for k, lead in enumerate(leads):
        nt = int(rng.integers(1, tails + 1)) if tails else 0
        idx = rng.choice(len(lower), size=nt, replace=False) if nt else []
        out.append(normalise(bo, [(int(rng.integers(1, P)), lead)] + list(zip(coefs(rng, nt), (lower[int(i)] for i in idx)))))
    return out


def lead_key(f):
    """Sort key of the lead monomial in ascending grevlex order."""
    e = f[0][1]
    return (sum(e),) + tuple(-x for x in reversed(e))


def tie_orders(bo, G):
    """The orders in which a tie basis is fed to minimalize: as given, ascending, descending (Python's stable sort)."""
    return {"given": list(G), "ascending": sorted(G, key=lead_key), "descending": sorted(G, key=lead_key, reverse=True)}


def pair_set(m, count, rng):
    """`count` distinct pairs (i, j), i < j < m, in random order."""
    total = m * (m - 1) // 2
    assert count <= total
    idx = rng.choice(total, size=count, replace=False).astype(np.int64) if count else np.zeros(0, dtype=np.int64)
    j = ((1 + np.sqrt(1 + 8 * idx.astype(np.float64))) / 2).astype(np.int64)
    j = np.where(j * (j - 1) // 2 > idx, j - 1, j)
    j = np.where((j + 1) * j // 2 <= idx, j + 1, j)
    i = idx - j * (j - 1) // 2
    return [(int(a), int(b)) for a, b in zip(i, j)]


def update_case(bo, nv, m, npairs, rng, constant_f=False):
    """(G, P, f) for update(): m basis elements whose lead monomials come from the monomials of degree 1..3 (shared lcm
    buckets), f's lead monomial x0 * x1, so that the pure powers of the other variables are coprime to f while e.g.
    x0 * x2^2 has the lcm of x2^2: buckets of equal lcms with a coprime member."""
    pool = monomial_pool(nv, 1 + nv + nv * (nv + 1) // 2 + nv * (nv + 1) * (nv + 2) // 6)[1:]
    G = []
    for k in range(m):
        lead = pool[int(rng.integers(0, len(pool)))]
        G.append(normalise(bo, [(int(rng.integers(1, P)), lead), (int(rng.integers(1, P)), pad(()))]))
    if constant_f:
        f = [(int(rng.integers(1, P)), pad(()))]
    else:
        f = normalise(bo, [(int(rng.integers(1, P)), pad((1, 1))), (int(rng.integers(1, P)), pad((0, 0, 1)))])
    return G, pair_set(m, npairs, rng), f


def gm_facts(G, Pl, f):
    """What the Gebauer-Moeller update of (G, Pl) by f meets, computed from the definition on exponent tuples:
    (old pairs dropped, buckets of two or more equal lcms that hold a member coprime to f)."""
    lmf = f[0][1]
    lm = [g[0][1] for g in G]
    lcm = lambda a, b: tuple(max(x, y) for x, y in zip(a, b))
    dropped = 0
    for i, j in Pl:
        l = lcm(lm[i], lm[j])
        if all(x >= y for x, y in zip(l, lmf)) and l != lcm(lm[i], lmf) and l != lcm(lm[j], lmf):
            dropped += 1
    buckets = {}
    for a in lm:
        buckets.setdefault(lcm(a, lmf), []).append(all(min(x, y) == 0 for x, y in zip(a, lmf)))
    return dropped, sum(1 for v in buckets.values() if len(v) >= 2 and any(v))


def minimal_leads(G):
    """The minimal elements of the set of lead monomials under divisibility — independently of any sort."""
    leads = {g[0][1] for g in G}
    return {a for a in leads if not any(b != a and all(x <= y for x, y in zip(b, a)) for b in leads)}


def reduce_case(bo, nv, ndiv, rng, dividend_terms=40, zero_at=(), constant_divisor=False):
    """(F, g): ndiv divisors whose lead monomials come from a small pool (several divide the same term: the first in list
    order must win) and a dividend g; zero_at: positions of F that hold the zero polynomial."""
    leads = monomial_pool(nv, 40, 2)
    lower = monomial_pool(nv, 1 + nv)
    F = []
    for k in range(ndiv):
        if k in zero_at:
            F.append([])
            continue
        lead = leads[int(rng.integers(0, len(leads)))]
        nt = int(rng.integers(0, 3))
        idx = rng.choice(len(lower), size=nt, replace=False) if nt else []
        F.append(normalise(bo, [(int(rng.integers(1, P)), lead)] + list(zip(coefs(rng, nt), (lower[int(i)] for i in idx)))))
    if constant_divisor:
        F[ndiv // 2] = [(int(rng.integers(1, P)), pad(()))]
    g = poly_from(bo, monomial_pool(nv, 4 * dividend_terms + 50), dividend_terms, rng)
    return F, g


def growing_reduce_case(bo, rng, nterms=12):
    """A short dividend whose intermediate results are far longer than it: the single divisor x0^2 + (21 lower
    terms in five other variables) turns every power of x0 into a product with that tail."""
    tail = [e for e in monomial_pool(6, 1 + 6 + 21) if e[0] == 0]      # degrees 0..2 in x1..x5: all below x0^2
    f = normalise(bo, [(1, pad((2,)))] + list(zip(coefs(rng, len(tail)), tail)))
    g = normalise(bo, list(zip(coefs(rng, nterms), (pad((7 - k % 3, k // 3, k % 2)) for k in range(nterms)))))
    return [f], g


class Mirror:
    """One device list mirrored on the oracle: the same operations in the same order on a std::vector<Polynomial>, sugars
    included (results feed later operands with the sugar they were given)."""

    BINOPS = {"add": "poly_add", "sub": "poly_sub", "mul": "poly_mul", "spoly": "spoly"}

    def __init__(self, bo, polys):
        self.bo = bo
        self.pl = bo.polylist(polys)

    def __len__(self):
        return len(self.pl)

    def nterms(self, i):
        return self.bo.fn("pl_nterms")(self.pl.h, i)

    def _prefix(self, n, drop_zero=False):
        out = self.bo.polylist()
        for i in range(n):
            if not (drop_zero and self.nterms(i) == 0):
                self.bo.fn("pl_copy")(self.pl.h, i, out.h)
        return out

    def binop(self, op, i, j):
        self.bo.fn(self.BINOPS[op])(self.pl.h, int(i), int(j), self.pl.h)

    def reduce(self, g, nF):
        """Element g by the elements [0, nF), zero polynomials left out (the reference would dereference their lead term)."""
        F = self._prefix(nF, drop_zero=True)
        return self.bo.fn("reduce")(self.pl.h, int(g), F.h, self.pl.h)

    def update(self, pairs, elimination):
        """The last element joins the ones before it: the new pair list (the list itself stays as it is)."""
        from oracle import ffi
        m = len(self) - 1
        G = self._prefix(m)
        buf = np.zeros((len(pairs) + m + 1, 2), dtype=np.int32)
        if len(pairs):
            buf[:len(pairs)] = np.asarray(pairs, dtype=np.int32)
        n = self.bo.fn("update")(G.h, buf.ctypes.data_as(ffi._ip), len(pairs), self.pl.h, m, ffi.ELIM[elimination])
        return [(int(a), int(b)) for a, b in buf[:n]]

    def minimalize(self):
        out = self.bo.polylist()
        self.bo.fn("minimalize")(self.pl.h, out.h)
        self.pl = out

    def interreduce(self):
        out = self.bo.polylist()
        self.bo.fn("interreduce")(self.pl.h, out.h)
        self.pl = out

    def polys(self):
        return self.pl.all()

    def sugars(self):
        return [self.pl.sugar(i) for i in range(len(self.pl))]


def same_state(L, k, mirror):
    """The whole of device list k against its mirror: number of elements, every polynomial, every sugar -> None or a
    description of the first difference."""
    got, want = L.get(k), mirror.polys()
    if len(got) != len(want):
        return "list %d: %d elements on the device, %d on the oracle" % (k, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            t = next((t for t, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            return "list %d element %d: %d terms on the device, %d on the oracle, first difference at term %d" % (k, i, len(a), len(b), t)
    gs, ws = L.sugars(k), mirror.sugars()
    if gs != ws:
        i = next(i for i, (x, y) in enumerate(zip(gs, ws)) if x != y)
        return "list %d element %d: sugar %d on the device, %d on the oracle" % (k, i, gs[i], ws[i])
    sizes, tot = L.sizes()
    if int(sizes[k]) != len(want):
        return "list %d: sizes() reports %d elements, get() %d" % (k, int(sizes[k]), len(want))
    return None


# ---- the planned cases, shared by the CPU conditions and the device parity tests ---------------------------------------

@functools.lru_cache(maxsize=None)
def binop_cases(nv, large):
    """[(label, A, B, A.n + B.n planned, len(A + B) planned)]: every MERGE_TOTALS value at or below 2 MT + 1 (large False)
    or above (large True), once with disjoint monomials (uneven split) and once with all monomials shared."""
    from oracle import ffi
    bo = ffi.load("bo")
    rng = np.random.default_rng(1000 + nv + (50 if large else 0))
    out = []
    for total in MERGE_TOTALS:
        if (total > 2 * MT + 1) != large:
            continue
        na = max(1, total // 3)
        A, B = disjoint_pair(bo, nv, na, total - na, rng)
        out.append(("disjoint-%d" % total, A, B, total, total))
        A, B = shared_pair(bo, nv, total // 2, rng, extra=total % 2)
        out.append(("shared-%d" % total, A, B, total, total // 2 + total % 2))
    return out


@functools.lru_cache(maxsize=None)
def boundary_cases(nv):
    """shifted_pairs with a cancelling pair exactly on the first tile boundary (positions 183 / 184) and on the boundary
    between the two partition batches (11 591 / 11 592); a zero polynomial on either side of more than 5 000 terms; planted
    partial and total cancellation."""
    from oracle import ffi
    bo = ffi.load("bo")
    rng = np.random.default_rng(2000 + nv)
    out = []
    A, B, n = shifted_pairs(bo, monomial_pool(nv, 120), rng, cancel_positions=(MT,))
    out.append(("shifted-241", A, B, 241, n))
    A, B, n = shifted_pairs(bo, monomial_pool(nv, 5900), rng, cancel_positions=(MT, BATCH_TILES * MT))
    out.append(("shifted-11801", A, B, 11801, n))
    big = poly_from(bo, monomial_pool(nv, 6000), 5003, rng)
    out.append(("zero-right", big, [], 5003, 5003))
    out.append(("zero-left", [], big, 5003, 5003))
    A = poly_from(bo, monomial_pool(nv, 4000), 3000, rng)
    B, n = planted_cancellation(bo, A, 0.5, rng, nfresh=100, nv=nv)
    out.append(("planted-half", A, B, 4600, n))
    B, n = planted_cancellation(bo, A, 1.0, rng, nv=nv)
    out.append(("planted-all", A, B, 6000, n))
    return out


@functools.lru_cache(maxsize=None)
def term_limit_case():
    """(A, B, t): A + B has exactly 65 535 terms (the most a polynomial can hold), A + (B + t) exactly 65 536."""
    from oracle import ffi
    bo = ffi.load("bo")
    rng = np.random.default_rng(3000)
    pool = monomial_pool(3, 65536)
    c = coefs(rng, 65536)
    A = normalise(bo, list(zip(c[:32768], pool[:65536:2])))
    B = normalise(bo, list(zip(c[32768:65535], pool[1:65535:2])))
    return A, B, [(c[65535], pool[65535])]


@functools.lru_cache(maxsize=None)
def tie_cases(nv, n):
    """{order name: basis}: a tie basis as given, ascending, descending, and one with all lead monomials equal."""
    from oracle import ffi
    bo = ffi.load("bo")
    rng = np.random.default_rng(4000 + 10 * n + nv)
    out = tie_orders(bo, tie_basis(bo, nv, n, rng))
    out["all-equal"] = tie_basis(bo, nv, n, rng, pool_size=1, multiples=False)
    return out


@functools.lru_cache(maxsize=None)
def update_cases(nv):
    """[(label, G, P, f)] for every UPDATE_SHAPES entry, and one with a constant f."""
    from oracle import ffi
    bo = ffi.load("bo")
    rng = np.random.default_rng(5000 + nv)
    out = [("m%d-p%d" % (m, k),) + update_case(bo, nv, m, k, rng) for m, k in UPDATE_SHAPES]
    out.append(("constant-f",) + update_case(bo, nv, 65, 256, rng, constant_f=True))
    return out


@functools.lru_cache(maxsize=None)
def interreduce_case(nv, n=280):
    """A minimal basis of 65 or more elements (the oracle's minimalize of a tie basis with long tails) for interreduce:
    tails of dozens of terms, among them other elements' lead monomials."""
    from oracle import ffi
    bo = ffi.load("bo")
    rng = np.random.default_rng(6000 + nv)
    deg = 1
    while len(list(_of_degree(nv, deg))) < 80:            # an antichain of 80 or more lead monomials
        deg += 1
    leads = [pad(e) for e in _of_degree(nv, deg)]
    lower = [e for e in monomial_pool(nv, 5000) if sum(e) <= deg][:600]   # (degree deg included: other elements' lead monomials)
    G = []
    for k in range(n):
        lead = leads[int(rng.integers(0, len(leads)))]
        cand = [e for e in lower if lead_key([(1, e)]) < lead_key([(1, lead)])]
        idx = rng.choice(len(cand), size=min(len(cand), int(rng.integers(24, 60))), replace=False)
        G.append(normalise(bo, [(int(rng.integers(1, P)), lead)] + list(zip(coefs(rng, len(idx)), (cand[int(i)] for i in idx)))))
    return bo.minimalize(G)


# ---- pair lcms whose degree passes 65 535 (the degree slot of a packed monomial has 16 bits) ----------------------------

def _mono(nv, **slots):
    e = [0] * nv
    for name, x in slots.items():
        e[int(name[1:])] = x
    return tuple(e)


def degree_limit_ideals():
    """{label: (nv, F)}: three generators within the limits (every exponent and degree at most 65 535) such that
    lcm(LM f0, LM f2) has a degree beyond 65 535 and is a proper multiple of lcm(LM f1, LM f2), which has not: Gebauer-Moeller
    drops the pair (0, 2).  An update that orders or compares the lcms by a 16-bit degree takes the large one for a small one,
    emits it first and keeps it.
      3 variables (8-byte monomials): degree 70 000 against 60 020.
      4 and 8 variables (16- and 32-byte monomials): degree 66 100 against 35 120, the two large exponents in the LOW halves of
      different 32-bit words (x0: word 0; x2 resp. x6: word 1 resp. 3), 35 000 + 31 000 > 65 535 — a sum of whole words
      carries into the high halves there."""
    out = {3: (3, [[(1, _mono(3, x0=1, x2=10000)), (1, _mono(3))],
                   [(1, _mono(3, x0=1, x2=20)), (1, _mono(3, x1=1))],
                   [(1, _mono(3, x0=30000, x1=30000)), (1, _mono(3, x2=1))]])}
    for nv, c, d in ((4, "x2", "x3"), (8, "x6", "x7")):
        out[nv] = (nv, [[(1, _mono(nv, x0=1, **{c: 31000})), (1, _mono(nv))],
                        [(1, _mono(nv, x0=1, **{c: 20})), (1, _mono(nv, x1=1))],
                        [(1, _mono(nv, x0=35000, **{d: 100})), (1, _mono(nv, **{c: 1}))]])
    return out


def hard_limit_ideal():
    """[x^40000 z + 1, y^40000 z + 1]: one pair, whose lcm has degree 80 001 — selecting it cannot be done in 16 bits."""
    return [[(1, (40000, 0, 1)), (1, (0, 0, 0))], [(1, (0, 40000, 1)), (1, (0, 0, 0))]]


def padded(F):
    return [[(c, pad(e)) for c, e in f] for f in F]


def lcm_degree(a, b):
    return sum(max(x, y) for x, y in zip(a, b))


def pair_sugar(o, i, j):
    """Sugar of the S-polynomial of the oracle environment's pair (i, j), from its basis (buchberger.cpp:18-21)."""
    li, lj = [int(x) for x in o.poly(int(i))[1][0]], [int(x) for x in o.poly(int(j))[1][0]]
    d = lcm_degree(li, lj)
    return max(o.poly_sugar(int(i)) + d - sum(li), o.poly_sugar(int(j)) + d - sum(lj))
