"""Randomised parity sweep of the batched polynomial algebra (test infrastructure, GPU box): deepgroebner_amd.PolyLists
(bbx_alg_*, csrc/bbx_algebra.hip) against a mirrored oracle state.  Every round draws a number of variables, a number of lists,
list shapes from the builders of tests/alg_cases.py (merge totals around the dispatch threshold and the tile / partition-batch
boundaries, shifted pairs with a cancelling pair on a boundary, zero operands, planted cancellation, tie bases, update cases
up to 700 elements and 3 000 pairs, divisor lists with zero polynomials, results at the 16-bit limits) and a random sequence
of operations over ONE handle; after every operation the WHOLE of every list — elements, terms, sugars — step counts and pair
lists are compared.
    python scripts/fuzz_algebra.py [ROUNDS] [SEED]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from deepgroebner_amd import PolyLists
from deepgroebner_amd._ffi import BbxError
from oracle import ffi
from tests import alg_cases as ac

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
bo = ffi.load("bo")
t0 = time.time(); nops = 0


def mismatch(tag, msg):
    print("MISMATCH %s: %s" % (tag, msg)); sys.exit(1)


def compare(tag, L, mirrors):
    for k, m in enumerate(mirrors):
        d = ac.same_state(L, k, m)
        if d:
            mismatch(tag, d)


def draw_pair(rng, nv, cap):
    """Two operands of one of the planned shapes, A.n + B.n at most about `cap`."""
    kind = rng.choice(["disjoint", "shared", "shifted", "zero", "planted", "short"])
    totals = [t for t in ac.MERGE_TOTALS if t <= cap]
    total = int(rng.choice(totals)) + int(rng.integers(-2, 3))
    if nv == 1:
        total = min(total, 400)
    if kind == "disjoint":
        return ac.disjoint_pair(bo, nv, max(1, int(rng.integers(1, total))), max(1, total // 2), rng)
    if kind == "shared":
        return ac.shared_pair(bo, nv, max(1, total // 2), rng, extra=int(rng.integers(0, 3)))
    if kind == "shifted":
        n = max(3, total // 2)
        bounds = [p for p in range(ac.MT, 2 * n, ac.MT) if p % 2 == 0]
        cancel = tuple(int(p) for p in rng.choice(bounds, size=min(len(bounds), 3), replace=False)) if bounds else ()
        return ac.shifted_pairs(bo, ac.monomial_pool(nv, n), rng, cancel_positions=cancel)[:2]
    if kind == "zero":
        f = ac.poly_from(bo, ac.monomial_pool(nv, total + 9), total, rng)
        return (f, []) if rng.random() < 0.5 else ([], f)
    if kind == "planted":
        A = ac.poly_from(bo, ac.monomial_pool(nv, total + 9), max(2, total // 2), rng)
        return A, ac.planted_cancellation(bo, A, float(rng.choice([0.1, 0.5, 1.0])), rng, nfresh=int(rng.integers(0, 40)), nv=nv)[0]
    pool = ac.monomial_pool(nv, 300)
    return ac.poly_from(bo, pool, int(rng.integers(1, 40)), rng), ac.poly_from(bo, pool, int(rng.integers(1, 40)), rng)


def round_binops(rng, nv, tag):
    global nops
    n = int(rng.choice([1, 3, 4, 5, 17, 257], p=[0.2, 0.2, 0.2, 0.2, 0.15, 0.05]))
    cap = 40000 if n <= 5 else (2000 if n <= 17 else 400)
    lists = [list(draw_pair(rng, nv, cap if k == 0 or rng.random() < 0.3 else 70)) for k in range(n)]
    L, mirrors = PolyLists(lists), [ac.Mirror(bo, l) for l in lists]
    for step in range(int(rng.integers(3, 9))):
        op = str(rng.choice(["add", "sub", "mul", "spoly", "reduce"]))
        args = []
        if op == "mul" and any(min(m.nterms(i) for i in range(len(m))) > 77 for m in mirrors):
            op = "add"                                                   # (products stay below 6 000 terms)
        for m in mirrors:
            sizes = [m.nterms(i) for i in range(len(m))]
            if op == "reduce":
                ok = [i for i in range(len(m)) if sizes[i] <= 3000] or [min(range(len(m)), key=lambda q: sizes[q])]
                args.append((ok[int(rng.integers(0, len(ok)))], int(rng.integers(0, len(m) + 1)) if max(sizes) <= 3000 else 0))
                continue
            ok = [i for i in range(len(m)) if (op != "spoly" or sizes[i] > 0) and (op != "mul" or sizes[i] <= 77)]
            if not ok:
                ok = [min(range(len(m)), key=lambda q: sizes[q])]
            i, j = ok[int(rng.integers(0, len(ok)))], ok[int(rng.integers(0, len(ok)))]
            if op != "mul" and sizes[i] + sizes[j] > 65000:         # (a result may hold 65 535 terms at the most)
                j = min(range(len(m)), key=lambda q: sizes[q])
                i = i if sizes[i] + sizes[j] <= 65000 else j
            args.append((i, j))
        if op in ("spoly", "mul") and any(mm.nterms(a) == 0 and op == "spoly" for mm, ab in zip(mirrors, args) for a in ab):
            op = "add"
        if op == "reduce":
            steps = L.reduce(args)
            want = [m.reduce(g, nF) for m, (g, nF) in zip(mirrors, args)]
            if [int(s) for s in steps] != want:
                mismatch(tag, "reduce %s: steps %s on the device, %s on the oracle" % (args, list(steps), want))
        else:
            L.binop(op, args)
            for m, (i, j) in zip(mirrors, args):
                m.binop(op, i, j)
        nops += 1
        compare("%s step %d %s %s" % (tag, step, op, args[:4]), L, mirrors)
    return "%d lists, sizes %s" % (n, [len(f) for f in lists[0]])


def round_reduce(rng, nv, tag):
    global nops
    lists, args = [], []
    for k in range(int(rng.integers(1, 6))):
        ndiv = int(rng.choice([1, 2, 63, 64, 65, 128, 200]))
        zero_at = tuple(int(z) for z in rng.integers(0, ndiv, size=int(rng.integers(0, 4)))) if rng.random() < 0.4 else ()
        F, g = ac.reduce_case(bo, max(nv, 2), ndiv, rng, dividend_terms=int(rng.choice([1, 12, 40, 300, 2000])), zero_at=zero_at,
                              constant_divisor=rng.random() < 0.15)
        if rng.random() < 0.15:
            F, g = ac.growing_reduce_case(bo, rng)
        lists.append(list(F) + [g])
        args.append((len(F), int(rng.choice([0, len(F), len(F) + 1, int(rng.integers(0, len(F) + 1))]))))
    L, mirrors = PolyLists(lists), [ac.Mirror(bo, l) for l in lists]
    steps = L.reduce(args)
    want = [m.reduce(g, nF) for m, (g, nF) in zip(mirrors, args)]
    if [int(s) for s in steps] != want:
        mismatch(tag, "reduce %s: steps %s on the device, %s on the oracle" % (args, list(steps), want))
    nops += 1
    compare(tag, L, mirrors)
    return "%d lists, steps %s" % (len(lists), want)


def round_update(rng, nv, tag):
    global nops
    nv = max(nv, 3)
    elim = str(rng.choice(["gebauermoeller", "gebauermoeller", "lcm", "none"]))
    cases = []
    for k in range(int(rng.integers(1, 5))):
        m = int(rng.choice([0, 1, 2, 63, 64, 65, 128, 129, 512, 513, 700, int(rng.integers(2, 300))]))
        npairs = min(int(rng.choice([0, 1, 255, 256, 257, 3000, int(rng.integers(0, 600))])), m * (m - 1) // 2)
        cases.append(ac.update_case(bo, nv, m, npairs, rng, constant_f=rng.random() < 0.1))
    L, mirrors = PolyLists([list(G) + [f] for G, _, f in cases]), [ac.Mirror(bo, list(G) + [f]) for G, _, f in cases]
    got = L.update([Pl for _, Pl, _ in cases], elim)
    for k, (G, Pl, f) in enumerate(cases):
        want = mirrors[k].update(Pl, elim)
        if got[k] != want:
            mismatch(tag, "update %s list %d (m = %d, |P| = %d): %d pairs on the device, %d on the oracle" % (elim, k, len(G), len(Pl), len(got[k]), len(want)))
    nops += 1
    compare(tag, L, mirrors)
    return "%s m %s |P| %s" % (elim, [len(G) for G, _, _ in cases], [len(Pl) for _, Pl, _ in cases])


def round_minimalize(rng, nv, tag):
    global nops
    nv = max(nv, 2)
    lists = []
    for k in range(int(rng.integers(1, 6))):
        n = int(rng.choice(list(ac.TIE_SIZES) + [int(rng.integers(1, 200))]))
        G = ac.tie_basis(bo, nv, n, rng, pool_size=int(rng.choice([1, 2, 5, 12])) if rng.random() < 0.5 else None, multiples=rng.random() < 0.7)
        lists.append(ac.tie_orders(bo, G)[str(rng.choice(["given", "ascending", "descending"]))])
    L, mirrors = PolyLists(lists), [ac.Mirror(bo, l) for l in lists]
    for op in ("minimalize", "interreduce"):
        getattr(L, op)()
        for m in mirrors:
            getattr(m, op)()
        nops += 1
        compare(tag + " " + op, L, mirrors)
    return "n %s -> %s" % ([len(l) for l in lists], [len(m) for m in mirrors])


def round_limits(rng, nv, tag):
    """A product at the degree limit (returned) or one above it (refused: the other lists must read back as what is on the
    device, and the handle must go on giving the oracle's answers)."""
    global nops
    v, w = int(rng.integers(0, nv)), int(rng.integers(0, nv))
    e = int(rng.integers(1, 65535))
    over = bool(rng.random() < 0.5)
    mono = lambda q, x: tuple(x if i == q else 0 for i in range(8))
    f = [(3, mono(v, e)), (1, mono(0, 0))]
    mw = list(mono(w, 65535 - e + (1 if over else 0)))
    g = [(5, tuple(mw)), (2, mono(0, 0))]
    small = [ac.poly_from(bo, ac.monomial_pool(nv, 50), 4, rng), ac.poly_from(bo, ac.monomial_pool(nv, 50), 3, rng)]
    lists = [small, [f, g], list(reversed(small))]
    L, mirrors = PolyLists(lists), [ac.Mirror(bo, l) for l in lists]
    try:
        L.binop("mul", (0, 1))
        refused = False
    except BbxError:
        refused = True
    if refused != over:
        mismatch(tag, "a product of sugar %d was %s" % (65535 + over, "refused" if refused else "returned"))
    sizes, _ = L.sizes()
    for k, m in enumerate(mirrors):
        if int(sizes[k]) == len(m) + 1 and not (over and k == 1):
            m.binop("mul", 0, 1)
    compare(tag + " after the product", L, mirrors)
    L.binop("add", (0, 1))
    for m in mirrors:
        m.binop("add", 0, 1)
    nops += 2
    compare(tag + " after the sum that followed", L, mirrors)
    return "sugar %d %s" % (65535 + over, "refused" if over else "returned")


KINDS = {"binops": round_binops, "reduce": round_reduce, "update": round_update, "minimalize": round_minimalize, "limits": round_limits}
for it in range(rounds):
    rng = np.random.default_rng([seed0, it])
    nv = int(rng.integers(1, 9))
    kind = str(rng.choice(["binops", "binops", "binops", "reduce", "update", "minimalize", "limits"]))
    tag = "seed %d round %d %s nv=%d" % (seed0, it, kind, nv)
    try:
        info = KINDS[kind](rng, nv, tag)
    except SystemExit:
        raise
    except Exception as ex:
        print("ERROR %s: %s: %s" % (tag, type(ex).__name__, str(ex)[:300])); sys.exit(1)
    print("ok %-44s %s" % (tag, info))
print("fuzz_algebra: %d rounds, %d operations, %.0f s, no mismatch" % (rounds, nops, time.time() - t0))
