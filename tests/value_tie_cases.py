"""Cases for value() rollouts from bases whose generator lead monomials tie (tests/test_value_ties_cpu.py checks the cases
themselves on the CPU, tests/test_value_ties_gpu.py runs them on the device).

buchberger() starts a rollout by std::sort-ing its reducers by lead monomial (buchberger.cpp:157-158); the environment keeps
its reducers in the STABLE order of upper_bound insertion.  The two orders differ only when two of the ideal's generators
have the same lead monomial and the basis has more than 16 elements (libstdc++'s std::sort is an insertion sort up to
there).  Every environment of every group below is such a state, AND one where the difference shows: the discounted return
of a rollout that starts from the stable order (the oracle's mutant mode sort_reducers=2, "the re-sort was forgotten")
differs from the true one for at least one of Degree, Normal and First.  The one exception is the control group of
16-element bases, where the two orders must be the same.

The search is deterministic (seeds 0, 1, 2, ... in order; hand-built ideals from random.Random(fixed seed)) and runs on the
oracle alone.  build() returns the groups by name; a group is one device handle.

Lead coefficients.  The generators of a distribution string are monic (the reference divides every generator by its lead
coefficient, ideals.cpp; so do the device generators), so a binomial record never holds a GENERATOR whose lead coefficient
is not 1.  Basis elements added by a step are not normalised (the C++ path keeps the remainder as reduce() left it), and
bbx_value_resort_kernel recomputes -tc/lc from ginfo for every element, generator or not.  The binomial groups therefore
walk one to three steps before valuing, and build() asserts that every binomial group that walks holds elements with a
lead coefficient other than 1.  Listed ideals (general record layout) keep the coefficients they are given: the hand-built
ones below have random lead coefficients.
"""
import functools
import random

import numpy as np

from oracle import ffi

STRATEGIES = ("degree", "normal", "sugar", "first", "env")   # 'env' selects First (std::map default, buchberger.cpp:342-349)
PROBED = ("degree", "normal", "first")                       # strategies bo.buchberger(G, P, ...) reproduces from a re-read basis
MAX_ADDITIONS = 20000                                        # per rollout: nothing near a hang can be built into a case
MIN_ENVS = 8
P_MOD = 32003


class Group:
    """One device handle: constructor argument, seeds, walk, caps and the oracle's answers for every environment."""

    def __init__(self, name, ctor, seeds, caps, sort_input, control=False):
        self.name, self.ctor, self.seeds, self.caps, self.sort_input, self.control = name, ctor, seeds, caps, sort_input, control
        self.actions = []        # [steps][B]: the action index every environment takes before it is valued
        self.envs = []           # the oracle environments, at the valued state
        self.states = []         # (G, P) re-read from them
        self.want = {}           # strategy -> [B] doubles at gamma 0.99, from the oracle ENVIRONMENT's value()
        self.want09 = []         # Degree at gamma 0.9
        self.mutant = {}         # strategy in PROBED -> [B] doubles of the stable-order mutant
        self.true_probe = {}     # strategy in PROBED -> [B] doubles of bo.buchberger(G, P, sort_reducers=1)
        self.sensitive = []      # per environment: the strategies of PROBED the mutant gets wrong
        self.tie, self.order_differs = [], []
        self.nonzero = {}        # strategy in PROBED -> [B] nonzero reductions of the true rollout (basis growth)
        self.max_additions = 0

    @property
    def batch(self):
        return len(self.envs)

    @property
    def listed(self):
        return not isinstance(self.ctor, str)

    def oracle_env(self, bo, e, sort_reducers=True):
        """A fresh oracle environment for environment e, before reset."""
        if self.listed:
            return bo.env(fixed=self.ctor[e], sort_input=self.sort_input, sort_reducers=sort_reducers)
        o = bo.env(self.ctor, sort_input=self.sort_input, sort_reducers=sort_reducers)
        o.seed(self.seeds[e])
        return o


def grevlex_key(e):
    """Ascending sort key of an exponent tuple in the reference's order (degree, then reverse lexicographic)."""
    return (sum(e),) + tuple(-x for x in reversed(e))


def read_state(o):
    G = [[(int(c), tuple(int(x) for x in ex)) for c, ex in zip(cs, es)] for cs, es in o.basis()]
    return G, [tuple(int(x) for x in p) for p in o.pairs()]


def stable_order(G):
    """The order upper_bound insertion of every element in basis order gives: stable by lead monomial."""
    return np.asarray(sorted(range(len(G)), key=lambda i: grevlex_key(G[i][0][1])), dtype=np.int32)


def has_generator_tie(G, ngen):
    leads = [G[i][0][1] for i in range(min(ngen, len(G)))]
    return len(set(leads)) < len(leads)


def probe(bo, o, ngen):
    """Everything the tests need to know about one valued state, or None when its rollouts are too long."""
    G, P = read_state(o)
    r = {"G": G, "P": P, "tie": has_generator_tie(G, ngen),
         "differs": not np.array_equal(bo.sort_order(G), stable_order(G)),
         "true": {}, "mutant": {}, "nonzero": {}, "adds": 0}
    for s in PROBED:
        for mode, key in ((1, "true"), (2, "mutant")):
            st = bo.buchberger(G, P, selection=s, sort_reducers=mode, want_basis=False)[1]
            r["adds"] = max(r["adds"], int(st["polynomial_additions"]))
            r[key][s] = st["discounted_return"]
            if mode == 1:
                r["nonzero"][s] = int(st["nonzero_reductions"])
    if r["adds"] > MAX_ADDITIONS:
        return None
    r["sensitive"] = tuple(s for s in PROBED if r["true"][s] != r["mutant"][s])
    return r


def _walk(o, seed, steps):
    """`steps` actions of the counter-hash agent; None when the episode ends on the way."""
    acts = []
    for t in range(steps):
        if o.nP == 0:
            return None
        a = ffi.agent_action(seed & 0xFFFFFFFF, t, o.nP)
        acts.append(a)
        o.step(a)
    return acts if o.nP > 0 else None


def _add(group, bo, o, acts, pr):
    group.envs.append(o)
    group.states.append((pr["G"], pr["P"]))
    for t, a in enumerate(acts):
        while len(group.actions) <= t:
            group.actions.append([])
        group.actions[t].append(a)
    for s in PROBED:
        group.mutant.setdefault(s, []).append(pr["mutant"][s])
        group.true_probe.setdefault(s, []).append(pr["true"][s])
        group.nonzero.setdefault(s, []).append(pr["nonzero"][s])
    group.sensitive.append(pr["sensitive"])
    group.tie.append(pr["tie"]); group.order_differs.append(pr["differs"])
    group.max_additions = max(group.max_additions, pr["adds"])


def _finish(group):
    for s in STRATEGIES:
        group.want[s] = [o.value(s, 0.99) for o in group.envs]
    group.want09 = [o.value("degree", 0.9) for o in group.envs]
    return group


def dist_group(bo, name, dist, steps, caps=None, sort_input=False, nenv=MIN_ENVS, seed_range=range(400)):
    """The first `nenv` seeds of `dist` whose state after `steps` actions is tied, larger than 16 and sensitive."""
    ngen = int(dist.split("-")[2])
    g = Group(name, dist, [], caps, sort_input)
    for seed in seed_range:
        o = bo.env(dist, sort_input=sort_input)
        o.seed(seed); o.reset()
        acts = _walk(o, seed, steps)
        if acts is None or o.nG <= 16:
            continue
        pr = probe(bo, o, ngen)
        if pr is None or not (pr["tie"] and pr["differs"] and pr["sensitive"]):
            continue
        g.seeds.append(seed)
        _add(g, bo, o, acts, pr)
        if g.batch == nenv:
            break
    assert g.batch >= MIN_ENVS, (name, g.batch)
    return _finish(g)


def with_caps(g, name, caps):
    """The same environments on another kernel class: everything but the name and the caps is shared."""
    h = Group.__new__(Group)
    h.__dict__.update(g.__dict__)
    h.name, h.caps = name, caps
    return h


# ---- hand-built ideals -------------------------------------------------------------------------------------------------
def monomials(nvars, max_degree, min_degree=1):
    """All monomials of `nvars` variables with min_degree <= degree <= max_degree, ascending."""
    out = []

    def rec(prefix, left):
        if len(prefix) == nvars - 1:
            out.append(tuple(prefix) + (left,))
            return
        for x in range(left + 1):
            rec(prefix + [x], left - x)
    for d in range(min_degree, max_degree + 1):
        rec([], d)
    return sorted(out, key=grevlex_key)


def tied_ideal(rng, nvars, ngen, lead_degrees=(2, 3)):
    """`ngen` generators of 2 to 4 terms whose leads come from a small pool, so that tie groups of 2 to 5 generators exist;
    random coefficients, the lead's included; every tail monomial has a smaller degree than the lead."""
    pool = [m for m in monomials(nvars, lead_degrees[1], lead_degrees[0])]
    rng.shuffle(pool)
    leads = []
    while len(leads) < ngen:
        m = pool[len(set(leads)) % len(pool)]
        leads += [m] * min(rng.randint(2, 5) if len(leads) < ngen - 1 else 1, ngen - len(leads))
    rng.shuffle(leads)
    F = []
    for lead in leads:
        lower = monomials(nvars, sum(lead) - 1, 0)
        tail = rng.sample(lower, min(rng.randint(1, 3), len(lower)))
        F.append([(rng.randint(1, P_MOD - 1), lead)] + [(rng.randint(1, P_MOD - 1), m) for m in sorted(tail, key=grevlex_key, reverse=True)])
    return F


def _first_nonzero_action(o):
    """The first action whose step adds an element to the basis (None: there is none)."""
    for a in range(o.nP):
        c = o.copy()
        n = c.nG
        c.step(a)
        if c.nG == n + 1 and c.nP > 0:
            return a
    return None


def listed_group(bo, name, counts, nvars, seed, caps=None, sort_input=False, steps=0, control=False, make=None, accept=None):
    """One hand-built ideal per entry of `counts` (its number of generators): the first draw of random.Random(seed) per entry
    that is tied, larger than 16 at the valued state and sensitive.  steps=1: valued after the first step that adds an element
    (the 16 -> 17 threshold).  control: kept for what it is (the caller asserts the orders agree)."""
    rng = random.Random(seed)
    g = Group(name, [], None, caps, sort_input, control)
    for ngen in counts:
        for _attempt in range(200):
            F = (make or tied_ideal)(rng, nvars, ngen)
            o = bo.env(fixed=F, sort_input=sort_input)
            o.reset()
            if o.nP == 0:
                continue
            acts = []
            if steps:
                a = _first_nonzero_action(o)
                if a is None:
                    continue
                acts = [a]
                o.step(a)
            pr = probe(bo, o, ngen)
            if pr is None:
                continue
            if not control and not (pr["tie"] and o.nG > 16 and pr["differs"] and pr["sensitive"]):
                continue
            if accept is not None and not accept(F, o, pr):
                continue
            g.ctor.append(F)
            _add(g, bo, o, acts, pr)
            break
        else:
            raise AssertionError("no ideal of %d generators found for %s" % (ngen, name))
    assert g.batch >= MIN_ENVS, (name, g.batch)
    return _finish(g)


def control_of(bo, g, name):
    """The ideals of the one-step group `g`, valued at reset (16 elements): the orders must agree there."""
    c = Group(name, g.ctor, None, g.caps, g.sort_input, control=True)
    for e, F in enumerate(g.ctor):
        o = bo.env(fixed=F, sort_input=g.sort_input)
        o.reset()
        _add(c, bo, o, [], probe(bo, o, len(F)))
    return _finish(c)


# ---- a generator order that drives libstdc++'s std::sort into its heapsort fallback ------------------------------------
def _introsort_partitions(n, less):
    """The quicksort part of libstdc++'s std::sort (bits/stl_algo.h __introsort_loop: pivot = median of first + 1, mid,
    last - 1, moved to first; __unguarded_partition; segments of 16 or fewer left alone) on range(n) with NO depth limit,
    so that an adversarial `less` shapes every level."""
    v = list(range(n))

    def swap(a, b):
        v[a], v[b] = v[b], v[a]

    def median_to_first(result, a, b, c):
        if less(v[a], v[b]):
            if less(v[b], v[c]): swap(result, b)
            elif less(v[a], v[c]): swap(result, c)
            else: swap(result, a)
        elif less(v[a], v[c]): swap(result, a)
        elif less(v[b], v[c]): swap(result, c)
        else: swap(result, b)

    def partition(first, last, pivot):
        while True:
            while less(v[first], v[pivot]): first += 1
            last -= 1
            while less(v[pivot], v[last]): last -= 1
            if not first < last:
                return first
            swap(first, last)
            first += 1
    stack = [(0, n)]
    while stack:
        first, last = stack.pop()
        while last - first > 16:
            mid = first + (last - first) // 2
            median_to_first(first, first + 1, mid, last - 1)
            cut = partition(first + 1, last, first)
            stack.append((cut, last))
            last = cut
    return v


def killer_ranks(n):
    """McIlroy's adversary ("A killer adversary for quicksort", 1999) against the partitions above: keys are decided as
    late as possible and the pivot candidate is frozen small, so nearly every partition splits off a handful of elements.
    Returns the rank (0 .. n-1, all distinct) of the element at every input position."""
    gas = n
    val = [gas] * n
    state = {"solid": 0, "candidate": 0}

    def freeze(x):
        val[x] = state["solid"]; state["solid"] += 1

    def less(x, y):
        if val[x] == gas and val[y] == gas:
            freeze(x if x == state["candidate"] else y)
        if val[x] == gas:
            state["candidate"] = x
        elif val[y] == gas:
            state["candidate"] = y
        return val[x] < val[y]
    _introsort_partitions(n, less)
    for x in range(n):
        if val[x] == gas:
            freeze(x)
    return val


def killer_ideal(rng, nvars, ngen):
    """Polynomials of 2 to 4 terms whose lead monomials, in basis order, are the adversary's input, except that about one rank in eight shares
    the monomial of the rank below it (the ties that flag the clone and let the two orders differ).  The ties blunt the
    adversary a little: the caller keeps only ideals on which the oracle's sort still enters the fallback.  Short tails of
    lower degree keep the rollout cheap."""
    ranks = killer_ranks(ngen)
    d = 2
    while len(monomials(nvars, d, d)) < ngen:        # leads of one degree: none divides another, every reducer matters
        d += 1
    ms = monomials(nvars, d, d)[:ngen]
    for r in sorted(rng.sample(range(1, ngen), ngen // 8)):
        ms[r] = ms[r - 1]
    F = []
    for r in ranks:
        lead = ms[r]
        lower = monomials(nvars, sum(lead) - 1, 0)
        tail = rng.sample(lower, min(rng.randint(1, 3), len(lower)))
        F.append([(rng.randint(1, P_MOD - 1), lead)] + [(rng.randint(1, P_MOD - 1), m) for m in sorted(tail, key=grevlex_key, reverse=True)])
    return F


def enters_heapsort(bo, G):
    bo.stat_sort(True)
    bo.sort_order(G)
    heapsorts, depth = bo.stat_sort(True)
    return heapsorts > 0, depth


# ---- growth ------------------------------------------------------------------------------------------------------------
def growth_caps(g, strategy, extra=None):
    """Capacities so tight that the value rollouts of `strategy` must outgrow the records: the basis capacity is the largest
    basis of the group at the valued state (made even, as the library does), and some rollout adds elements beyond it — the
    oracle's nonzero reductions say how many.  The pair capacity is left alone: the basis alone makes growth certain."""
    nG = [len(G) for G, _ in g.states]
    cap = max(nG) + (max(nG) & 1)
    peak = max(n + z for n, z in zip(nG, g.nonzero[strategy]))
    assert peak > cap, (g.name, cap, peak)
    caps = dict(g.caps or {}, max_basis=cap)
    caps.update(extra or {})
    return caps, cap, peak


@functools.lru_cache(maxsize=None)
def build():
    """Every group, by name.  Built once per process (a few seconds on the oracle) and shared, never modified."""
    bo = ffi.load("bo")
    groups = []
    # register/LDS binomial class, W = 2, and the same ideals on the classes that continue in or live in HBM
    for dist, steps in (("3-3-20-uniform", 1), ("3-5-18-maximum", 2)):
        g = dist_group(bo, "fast|" + dist, dist, steps)
        groups.append(g)
        groups.append(with_caps(g, "fast_spill|" + dist, {"lds_max_basis": 16}))
        groups.append(with_caps(g, "binom_hbm_w2|" + dist, {"lds_max_basis": -1}))
        groups.append(with_caps(g, "general_class|" + dist, {"general_class": 1}))
    groups.append(dist_group(bo, "fast_reset|3-3-20-uniform", "3-3-20-uniform", 0))
    groups.append(dist_group(bo, "fast_sort_input|3-3-20-uniform", "3-3-20-uniform", 1, sort_input=True))
    # binomial HBM class, W = 4 and W = 8
    for dist, steps in (("4-2-20-uniform", 1), ("5-2-24-weighted", 3), ("8-2-24-uniform", 2)):
        groups.append(dist_group(bo, "binom_hbm|" + dist, dist, steps))
    # general class from distribution strings
    for dist, steps in (("3-3-20-0.5-uniform", 1), ("4-2-18-0.5-uniform", 0)):
        groups.append(dist_group(bo, "general|" + dist, dist, steps))
    # listed ideals: wide class, and the same list on the general class
    mixed = listed_group(bo, "listed_mixed", (17, 18, 32, 33, 64, 80, 19, 24), 5, seed=1)
    groups.append(mixed)
    groups.append(with_caps(mixed, "listed_mixed_general", {"wide_waves": -1}))
    step17 = listed_group(bo, "listed_16_plus_one_step", (16,) * 8, 3, seed=2, steps=1)
    groups.append(step17)
    groups.append(with_caps(step17, "listed_16_plus_one_step_general", {"wide_waves": -1}))
    groups.append(control_of(bo, step17, "listed_16_control"))
    groups.append(listed_group(bo, "listed_sort_input", (17, 20, 33, 40, 18, 26, 64, 22), 4, seed=3, sort_input=True))
    heap = listed_group(bo, "listed_heapsort", (64, 65, 66, 67, 68, 69, 70, 64), 5, seed=4, make=killer_ideal,
                        accept=lambda F, o, pr: enters_heapsort(bo, pr["G"])[0])
    groups.append(heap)
    groups.append(with_caps(heap, "listed_heapsort_general", {"wide_waves": -1}))
    for g in groups:
        assert g.max_additions <= MAX_ADDITIONS, (g.name, g.max_additions)
        if not g.listed and "0.5" not in g.ctor and g.actions:       # binomial records that walked: non-monic elements
            assert any(f[0][0] != 1 for G, _ in g.states for f in G), g.name
    assert tuple(g.name for g in groups) == GROUP_NAMES
    return {g.name: g for g in groups}


# the groups build() returns, in its order (the GPU test's parameters: known without building anything)
GROUP_NAMES = tuple(c + "|" + d for d in ("3-3-20-uniform", "3-5-18-maximum") for c in ("fast", "fast_spill", "binom_hbm_w2", "general_class")) + (
    "fast_reset|3-3-20-uniform", "fast_sort_input|3-3-20-uniform", "binom_hbm|4-2-20-uniform", "binom_hbm|5-2-24-weighted",
    "binom_hbm|8-2-24-uniform", "general|3-3-20-0.5-uniform", "general|4-2-18-0.5-uniform", "listed_mixed", "listed_mixed_general",
    "listed_16_plus_one_step", "listed_16_plus_one_step_general", "listed_16_control", "listed_sort_input", "listed_heapsort",
    "listed_heapsort_general")
SAMPLE = ("fast|3-3-20-uniform", "listed_16_plus_one_step")     # 'sample' (best of Degree and 100 seeded Random rollouts)


def sample_seeds(batch):
    return np.random.default_rng(13).integers(0, 2 ** 31 - 1, size=(batch, 100))


def sample_values(bo, grp, seeds, sort_reducers=True):
    """What value('sample') must return with these seeds, from the re-read states; every rollout within MAX_ADDITIONS."""
    want = []
    for e, (G, P) in enumerate(grp.states):
        runs = [bo.buchberger(G, P, selection="random", seed=int(s), sort_reducers=sort_reducers, want_basis=False)[1] for s in seeds[e]]
        runs.append(bo.buchberger(G, P, selection="degree", sort_reducers=sort_reducers, want_basis=False)[1])
        assert max(r["polynomial_additions"] for r in runs) <= MAX_ADDITIONS
        want.append(max(r["discounted_return"] for r in runs))
    return want


GROWTH = ("fast|3-3-20-uniform", "general|3-3-20-0.5-uniform")
