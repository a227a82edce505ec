"""The binomial class of the step kernel (binom_body, bin_add_poly, merge2: csrc/bbx_binom.h) at its reduction and coefficient
edges: a float-free restatement of one binomial step on the oracle's state, the situations a step can show, and the cases —
distributions, options and pinned (ideal seed, agent seed) pairs — that tests/test_binom_edges_cpu.py holds to the oracle
and tests/test_binom_edges_gpu.py runs on the device.  numpy and the oracle only: importable without a GPU.

The restatement (restate_step) builds the S-polynomial of the selected pair from the two tails,
    a = tc_i/lc_i tm_i gamma/lm_i,   b = -tc_j/lc_j tm_j gamma/lm_j,   gamma = lcm(lm_i, lm_j),
merged as merge2 does (the larger monomial first by the oracle's mono_gt; equal monomials add, a zero sum drops the term), and
reduces it over reducer_order(): the first reducer whose lead divides LM(h) gives h <- h - (LT h / LT f) f, otherwise the lead
term moves to the remainder.  It returns the remainder, the reducer-order indices the rounds used and the situations shown:
    first_notail, second_notail, both_notail   which members of the selected pair have one term
    tails_meet_sum, tails_meet_cancel          the two S-polynomial tails land on one monomial; the sum is non-zero, or it is
                                               zero and h vanishes before any round
    red_meet_sum, red_meet_cancel              in a round the reducer's scaled tail lands on h's second term; non-zero / zero sum
    reducer_notail                             a round uses a reducer without a tail: only LT h goes
    r_second_after_reduction                   the remainder receives its second term after at least one round since its first
    new_notail, new_lc_one_tail, new_lc_pm1    the inserted element has one term; LC = 1 and a tail; LC = p - 1 = 32002
    found_in_memory                            a round's reducer has order index >= 64 SR of the class: the scan's memory part
    found_last_register_chunk                  ... index in [64 SR - 64, 64 SR): the last chunk scanned from registers
    miss_through_memory                        a round finds no reducer while |G| > 64 SR: the scan runs through all of memory
SR (8, 6, 3 chunks of 64 for 8-, 16- and 32-byte monomials: 512, 384, 192 reducers) is read from bbx_binom.h.

What the searches found (hash agent, agent seed = ideal seed - 993 unless a pair is taken from another test; every walk agreed
with the oracle's new element on every step):

Deep reducers, ideal seeds 1000..2999, sort_reducers=False:
    8-3-200-uniform, 60 steps     every seed finds reducers in memory; largest index 230; index 191 on 151 seeds, 192 on 149
    4-8-400-uniform, 60 steps     every seed; largest index 439; index 383 on 60 seeds, 384 on 66, both on 2091 and 2221 only
    3-20-510-weighted, 30 steps   1266 seeds (1000 is one, 1001 is not); largest index 519; index 511 on 1726 seeds, 512 on 1246
  Every unsorted case pins a round at exactly 64 SR - 1 and one at exactly 64 SR on both of its seeds.  Largest index of the
  pinned cases: deep-32-byte 225, deep-16-byte 424, deep-8-byte-hbm and deep-8-byte-staged 513, deep-32-byte-sorted 202.
The same seeds and steps with sort_reducers=True:
    8-3-200-uniform               218 of 2000 seeds reach the memory part (largest index 227, seed 2741), 133 show all three scan
                                  situations; index 191 on 16 seeds, 192 on 17, both on 2337 alone -> the case deep-32-byte-sorted
    4-8-400-uniform               largest index 347 (< 384): none
    3-20-510-weighted             largest index 214 (< 512): none

Coefficient and merge edges, ideal seeds 1000..20999, 128 steps; seeds of 20000 that show the rare situations:
    distribution                       new_lc_one_tail  new_lc_pm1  first_notail  tails_meet_sum  red_meet_sum  reducer_notail
    3-20-10-weighted                         29             33         19746          10992          19838         20000
    3-20-10-weighted, unsorted reducers      39             34         19552          10845          19986         20000
    4-5-4-uniform                            19             23          3928           2729           4399          5041
    5-10-5-uniform                           23             27           140             98            180           183
    8-3-4-weighted                           20             26          1364           2078           1027          2266
  edges-8-byte-hbm takes its pairs from tests/test_lead_coef_cpu.py (six) and tests/test_spoly_coef_cpu.py (two): they show the
  whole list.  Only 31 of the 20000 seeds of 5-10-5-uniform end an episode within 128 steps, and none of those inserts an
  element with LC = 1 and a tail or LC = 32002: in the 16-byte group these two are pinned on 4-5-4-uniform, everything else on
  both distributions.  Nothing is left out under the lead-coefficient rule: every group pins every situation of its list.
  5-10-5-uniform is the distribution whose kernel the benchmark runs, so the case lc-16-byte-5-10-5 runs seven of its seeds
  that do insert such elements (9 of the 20000 insert both kinds) — outside the four groups, since no episode ends in them."""
import collections
import functools
import os
import re

import numpy as np

from oracle import ffi

P = 32003
K = 2
WAVE = 64
HBM = {"lds_max_basis": -1}
GENERAL = {"general_class": 1, "lds_max_basis": -1}

PAIR_SITUATIONS = ("first_notail", "second_notail", "both_notail", "tails_meet_sum", "tails_meet_cancel")
ROUND_SITUATIONS = ("red_meet_sum", "red_meet_cancel", "reducer_notail", "r_second_after_reduction")
NEW_SITUATIONS = ("new_notail", "new_lc_one_tail", "new_lc_pm1")
SCAN_SITUATIONS = ("found_in_memory", "found_last_register_chunk", "miss_through_memory")
EDGE_SITUATIONS = PAIR_SITUATIONS + ROUND_SITUATIONS + NEW_SITUATIONS


@functools.lru_cache(maxsize=None)
def header_constants():
    """{monomial bytes: SR}: the chunks of 64 reducer lead monomials a reduction scans from registers, read from the
    kernel's header (not retyped)."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "deepgroebner_amd", "csrc", "bbx_binom.h")).read()
    m = re.search(r"constexpr int SR = W == 2 \? (\d+) : \(W == 4 \? (\d+) : (\d+)\);", text)
    return {8: int(m.group(1)), 16: int(m.group(2)), 32: int(m.group(3))}


def mono_bytes(dist):
    """bytes of a packed monomial of the distribution (bbx_api.cpp: W = 2, 4 or 8 words for up to 3, 7 and 8 variables)"""
    n = int(dist.split("-")[0])
    return 8 if n <= 3 else (16 if n <= 7 else 32)


def register_part(dist):
    """64 * SR: how many reducers (in reducer order) a round of the distribution's class scans from registers"""
    return WAVE * header_constants()[mono_bytes(dist)]


# ---- the restatement ---------------------------------------------------------------------------------------------------------
# A term is (coefficient in 1..p-1, exponent tuple of 8) or None (absent: a term with c == 0 in the kernel).

def _gt(bo, a, b):
    return bo.mono_gt(a, b)


def merge2(bo, x, y):
    """(x) + (y) for single optional terms, as merge2 of bbx_binom.h: (first, second, "sum" / "cancel" / None for whether the
    two met on one monomial)"""
    if x is None or y is None:
        return (x if x is not None else y), None, None
    if _gt(bo, x[1], y[1]):
        return x, y, None
    if _gt(bo, y[1], x[1]):
        return y, x, None
    c = (x[0] + y[0]) % P
    return ((c, x[1]) if c else None), None, ("sum" if c else "cancel")


def _inv(c):
    return pow(int(c), P - 2, P)


def _terms(poly):
    coef, exps = poly
    return [(int(c), tuple(int(v) for v in e)) for c, e in zip(coef, exps)]


def _mul(m, q):
    return tuple(a + b for a, b in zip(m, q))


def _div(m, q):
    return tuple(a - b for a, b in zip(m, q))


Step = collections.namedtuple("Step", "remainder used situations")


def restate_step(bo, basis, order, i, j, part):
    """One binomial step on the state before it.  basis: [[(c, exps), ...] per element] (one or two terms, lead first),
    order: the reducer order (basis indices), (i, j): the selected pair, part: 64 * SR of the class.
    Returns Step(remainder as a term list — [] when the S-polynomial reduces to zero —, the reducer-order indices the
    rounds used, the set of situations the step showed)."""
    sit = set()
    fi, fj = basis[i], basis[j]
    assert 1 <= len(fi) <= 2 and 1 <= len(fj) <= 2, "not a binomial basis"
    if len(fi) == 1:
        sit.add("first_notail")
    if len(fj) == 1:
        sit.add("second_notail")
    if len(fi) == 1 and len(fj) == 1:
        sit.add("both_notail")
    gamma = tuple(max(a, b) for a, b in zip(fi[0][1], fj[0][1]))
    a = b = None
    if len(fi) == 2:
        a = (fi[1][0] * _inv(fi[0][0]) % P, _mul(fi[1][1], _div(gamma, fi[0][1])))
    if len(fj) == 2:
        b = ((P - fj[1][0] * _inv(fj[0][0]) % P) % P, _mul(fj[1][1], _div(gamma, fj[0][1])))
    h0, h1, met = merge2(bo, a, b)
    if met:
        sit.add("tails_meet_" + met)
    leads = np.array([basis[g][0][1] for g in order], dtype=np.int64).reshape(len(order), ffi.NV)
    r, used = [], []
    rounds_since_first = 0
    while h0 is not None:
        hit = np.flatnonzero((leads <= np.array(h0[1], dtype=np.int64)).all(axis=1))
        if len(hit):
            idx = int(hit[0])
            f = basis[int(order[idx])]
            used.append(idx)
            if idx >= part:
                sit.add("found_in_memory")
            elif idx >= part - WAVE:
                sit.add("found_last_register_chunk")
            sb = None
            if len(f) == 2:
                kg = (P - f[1][0] * _inv(f[0][0]) % P) % P             # -tc / lc
                sb = (h0[0] * kg % P, _mul(f[1][1], _div(h0[1], f[0][1])))
            else:
                sit.add("reducer_notail")
            h0, h1, met = merge2(bo, h1, sb)
            if met:
                sit.add("red_meet_" + met)
            if r:
                rounds_since_first += 1
        else:
            if len(order) > part:
                sit.add("miss_through_memory")
            if r and rounds_since_first:
                sit.add("r_second_after_reduction")
            r.append(h0)
            assert len(r) <= 2, "a binomial reduced by binomials has at most two terms"
            h0, h1 = h1, None
    if r:
        if len(r) == 1:
            sit.add("new_notail")
        if len(r) == 2 and r[0][0] == 1:
            sit.add("new_lc_one_tail")
        if r[0][0] == P - 1:
            sit.add("new_lc_pm1")
    return Step(r, tuple(used), frozenset(sit))


Walk = collections.namedtuple("Walk", "env rewards dones steps new disagreements")


def walk_env(dist, opts, seed, aseed, nsteps, part=None):
    """nsteps steps of the hash agent with auto-reset on the oracle, every one restated from the state in front of it:
    Walk(the environment as it stands afterwards, per-step rewards, done flags, the restated Steps, the oracle's new element
    per step as a term list ([] when |G| did not change), the steps at which the two differ)."""
    bo = ffi.load("bo")
    part = register_part(dist) if part is None else part
    o = bo.env(dist, **opts)
    o.seed(seed)
    o.reset()
    basis = [_terms(o.poly(g)) for g in range(o.nG)]
    rewards, dones, steps, new, bad = [], [], [], [], []
    for t in range(nsteps):
        a = ffi.agent_action(aseed, t, o.nP)
        i, j = (int(v) for v in o.pairs()[a])
        st = restate_step(bo, basis, o.reducer_order(), i, j, part)
        nG0 = o.nG
        rewards.append(o.step(a))
        assert o.nG in (nG0, nG0 + 1)
        got = _terms(o.poly(nG0)) if o.nG > nG0 else []
        if got != st.remainder:
            bad.append(t)
        if got:
            basis.append(got)
        steps.append(st); new.append(got)
        dones.append(o.nP == 0)
        if o.nP == 0:
            o.reset()
            basis = [_terms(o.poly(g)) for g in range(o.nG)]
    return Walk(o, np.array(rewards), np.array(dones), steps, new, bad)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
# name -> Case.  opts: options of the environment (oracle and device alike), caps: the device handle's caps, K = 2 everywhere;
# seeds: (ideal seed, agent seed) pairs = the batch of the GPU tests; part: 64 * SR of the case's class; pins: situation ->
# ((index into seeds, step), ...) where the oracle's trajectory shows it (up to three seeds each, the first such step of each);
# index_pins: reducer-order index (part - 1 or part) -> the same, for rounds that used exactly that reducer; largest_index:
# the largest reducer-order index any round of the case uses.
Case = collections.namedtuple("Case", "group dist opts caps steps seeds part pins index_pins largest_index")

UNSORTED = {"sort_reducers": False}


def _case(group, dist, opts, caps, steps, seeds, spec, largest_index):
    """spec: "situation e:t e:t; ..." — "index-1" / "index+0" for the reducer-order indices 64 SR - 1 and 64 SR"""
    part = register_part(dist)
    pins, index_pins = {}, {}
    for item in spec.split(";"):
        name, *where = item.split()
        where = tuple(tuple(int(v) for v in w.split(":")) for w in where)
        if name.startswith("index"):
            index_pins[part + int(name[5:])] = where
        else:
            pins[name] = where
    return Case(group, dist, opts, caps, steps, seeds, part, pins, index_pins, largest_index)


CASES = {
    # ---- coefficient and merge edges: 128 steps with auto-reset, an episode ends inside every run
    # (six pairs of tests/test_lead_coef_cpu.py and two of tests/test_spoly_coef_cpu.py)
    "edges-8-byte-hbm": _case("edges-8-byte-hbm", "3-20-10-weighted", {}, HBM, 128,
        ((5012, 1012), (5015, 1015), (6048, 2048), (6549, 2549), (7694, 3694), (8077, 4077), (8711, 4711), (9694, 5694)),
        "first_notail 0:17 1:15 2:33; second_notail 0:9 1:7 2:39; both_notail 0:17 1:15 2:39; "
        "tails_meet_sum 0:20 1:4 3:122; tails_meet_cancel 0:3 1:60 2:9; red_meet_sum 0:7 1:66 2:22; "
        "red_meet_cancel 0:5 1:119 2:16; reducer_notail 0:10 1:8 2:35; r_second_after_reduction 0:2 1:5 2:7; "
        "new_notail 0:7 1:4 2:22; new_lc_one_tail 2:32 3:61 5:4; new_lc_pm1 4:93 5:13 6:67",
        25),
    "edges-8-byte-staged": _case("edges-8-byte-staged", "3-20-10-weighted", UNSORTED, None, 128,
        ((1801, 808), (2793, 1800), (3168, 2175), (3480, 2487), (4531, 3538), (10712, 9719), (15604, 14611), (16278, 15285)),
        "first_notail 0:48 1:64 2:44; second_notail 0:26 1:53 2:17; both_notail 0:48 1:64 2:44; "
        "tails_meet_sum 0:21 1:70 2:51; tails_meet_cancel 0:24 1:16 2:37; red_meet_sum 0:58 1:43 2:12; "
        "red_meet_cancel 0:12 1:34 2:18; reducer_notail 0:22 1:45 2:13; r_second_after_reduction 0:11 1:5 2:0; "
        "new_notail 0:21 1:43 2:12; new_lc_one_tail 1:103 2:1 3:49; new_lc_pm1 0:77 1:119 3:46",
        53),
    "edges-16-byte-4-5-4": _case("edges-16-byte", "4-5-4-uniform", {}, None, 128,
        ((1740, 747), (2956, 1963), (3376, 2383), (10860, 9867), (12021, 11028), (13868, 12875), (15561, 14568), (16652, 15659)),
        "first_notail 0:28 1:30 3:94; second_notail 0:19 1:19 3:84; both_notail 0:28 1:30 3:94; "
        "tails_meet_sum 0:94 1:16 3:89; tails_meet_cancel 0:5 1:5 2:15; red_meet_sum 0:18 1:21 3:83; "
        "red_meet_cancel 0:3 1:7 2:7; reducer_notail 0:20 1:23 3:84; r_second_after_reduction 0:1 1:46 2:3; "
        "new_notail 0:18 1:16 3:83; new_lc_one_tail 1:100 2:4 4:92; new_lc_pm1 0:102 2:6 3:61",
        26),
    "edges-16-byte-5-10-5": _case("edges-16-byte", "5-10-5-uniform", {}, None, 128,
        ((1193, 200), (7127, 6134), (7367, 6374), (8055, 7062), (9042, 8049), (13068, 12075), (13925, 12932), (17607, 16614)),
        "first_notail 0:87 1:25 2:4; second_notail 0:59 1:7 2:3; both_notail 0:87 1:25 2:4; tails_meet_sum 1:6 2:0 4:39; "
        "tails_meet_cancel 0:3 1:9 2:61; red_meet_sum 0:57 1:22 2:2; red_meet_cancel 0:4 1:4 2:71; "
        "reducer_notail 0:58 1:7 2:5; r_second_after_reduction 0:5 1:0 2:1; new_notail 0:57 1:6 2:0",
        62),
    "edges-32-byte": _case("edges-32-byte", "8-3-4-weighted", {}, None, 128,
        ((1093, 100), (1096, 103), (1174, 181), (1236, 243), (1242, 249), (10277, 9284), (10792, 9799), (18284, 17291)),
        "first_notail 0:45 1:113 3:99; second_notail 0:38 1:110 3:97; both_notail 0:51 1:113 3:99; "
        "tails_meet_sum 0:37 1:109 3:94; tails_meet_cancel 0:2 1:40 2:3; red_meet_sum 0:50 1:115 3:95; "
        "red_meet_cancel 0:4 1:3 2:2; reducer_notail 0:38 1:111 3:98; r_second_after_reduction 0:0 1:51 2:1; "
        "new_notail 0:37 1:109 3:94; new_lc_one_tail 2:15 5:4 6:83; new_lc_pm1 2:30 5:0 6:89",
        19),
    # ---- beyond the four groups: the lead-coefficient ends on the benchmark's second distribution, whose runs of 128 steps end
    # no episode where they show them (module docstring); value() from the final state then uses what was inserted
    "lc-16-byte-5-10-5": _case("lc-16-byte", "5-10-5-uniform", {}, None, 128,
        ((1244, 251), (3741, 2748), (8923, 7930), (9884, 8891), (13933, 12940), (16397, 15404), (17817, 16824)),
        "new_lc_one_tail 2:25 3:21 4:29 5:22; new_lc_pm1 0:14 1:7 3:8 4:3",
        80),
    # ---- deep reducers: no episode ends inside these runs, every launch after the first begins beyond the register part
    "deep-32-byte": _case("deep", "8-3-200-uniform", UNSORTED, None, 60,
        ((1032, 39), (1044, 51)),
        "found_in_memory 0:5 1:2; found_last_register_chunk 0:0 1:0; miss_through_memory 0:0 1:0; index-1 0:12 1:2; "
        "index+0 0:20 1:45",
        225),
    "deep-16-byte": _case("deep", "4-8-400-uniform", UNSORTED, None, 60,
        ((2091, 1098), (2221, 1228)),
        "found_in_memory 0:4 1:3; found_last_register_chunk 0:8 1:5; miss_through_memory 0:0 1:0; index-1 0:38 1:5; "
        "index+0 0:33 1:13",
        424),
    "deep-8-byte-hbm": _case("deep", "3-20-510-weighted", UNSORTED, HBM, 30,
        ((1000, 7), (1002, 9)),
        "found_in_memory 0:4 1:13; found_last_register_chunk 0:2 1:1; miss_through_memory 0:6 1:12; index-1 0:4 1:2; "
        "index+0 0:4 1:13",
        513),
    "deep-8-byte-staged": _case("deep", "3-20-510-weighted", UNSORTED, None, 30,
        ((1000, 7), (1002, 9)),
        "found_in_memory 0:4 1:13; found_last_register_chunk 0:2 1:1; miss_through_memory 0:6 1:12; index-1 0:4 1:2; "
        "index+0 0:4 1:13",
        513),
    "deep-32-byte-sorted": _case("deep", "8-3-200-uniform", {}, None, 60,
        ((2337, 1344), (2464, 1471)),
        "found_in_memory 0:1 1:1; found_last_register_chunk 0:1 1:4; miss_through_memory 0:0 1:0; index-1 0:17; "
        "index+0 0:1 1:1",
        202),
}
GROUPS = {}
for _name, _c in CASES.items():
    GROUPS.setdefault(_c.group, []).append(_name)
# group -> the situations of its list that no seed inside the search bound showed (only the two lead-coefficient ones may be)
LEFT_OUT = {}


@functools.lru_cache(maxsize=None)
def case_walk(name, e):
    """walk_env of environment e of the case: computed once, shared by every test that needs it (read-only: value() and the
    getters of the environment it holds do not change it)"""
    c = CASES[name]
    return walk_env(c.dist, dict(c.opts), c.seeds[e][0], c.seeds[e][1], c.steps, c.part)


def required(group):
    """the situations the group's cases must pin between them"""
    if group.startswith("lc"):
        return ("new_lc_one_tail", "new_lc_pm1")
    return SCAN_SITUATIONS if group.startswith("deep") else EDGE_SITUATIONS
