"""The Gebauer-Moeller peel of the fast class takes ONE wave minimum per bucket of equal minimal lcms, over the keys
degree << 8 | basis index (add_poly, bbx_fast.h; bbx_peel_key, bbx_common.h): the minimum names the next bucket and the member
that stands for it.  tests/peel_keyed_min_check.cpp runs that loop on the host, with the kernel's own key statements, against
the rule stated directly — built here with -fsanitize=address,undefined as a program of its own.  The second half asserts, on
the oracle alone, that the seeds tests/test_peel_keyed_min_gpu.py runs show the insertions the new loop has to get right:
  multi    two or more buckets at one degree (the peel by levels went through them in index order of a second loop);
  coprime  a bucket with a member whose lead monomial is coprime to the new one's: it emits nothing;
  triple   a bucket of three or more equal lcms: its smallest index is emitted;
  six      an insertion with at least six buckets;
  none     an insertion that emits no pair at all;
  g64      an insertion into a basis of 64 or more elements (the two-bank copy of the update).
Ideal seeds 1000 .. 3999 with agent seed = ideal seed - 993 were searched, 256 steps each; `none` and `g64` are the rare ones
(an insertion without a new pair on 414 of the 3000 seeds, |G| >= 64 on 385; the eight seeds here show both).  A seed that
stops showing its case fails the test."""
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import ffi
from tests import oracle_walk as ow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST, K, T = "3-20-10-weighted", 2, 256
LAUNCH, CUT = 16, 32
SITUATIONS = ("multi", "coprime", "triple", "six", "none", "g64")
SEEDS = ((1042, 49), (1131, 138), (1250, 257), (1274, 281), (1471, 478), (1506, 513), (1623, 630), (1751, 758))
# situation -> ((ideal seed, agent seed), step) as the search reported them, re-asserted below
KNOWN = {"none": (((1042, 49), 225), ((1131, 138), 17), ((1250, 257), 235), ((1274, 281), 78), ((1471, 478), 58), ((1506, 513), 60),
                  ((1623, 630), 34), ((1751, 758), 0)),
         "g64": (((1042, 49), 152), ((1131, 138), 166), ((1250, 257), 59), ((1274, 281), 196), ((1471, 478), 140), ((1506, 513), 133),
                 ((1623, 630), 150), ((1751, 758), 122))}
BOX_CASES = 2 * 27 * (27 + 378 + 3654 + 27405 + 169911)       # multisets of 1..5 of 27 monomials, two arrangements, 27 f
SEEDED_CASES = 255 * 4 * 3


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("peel_keyed_min") / "peel_keyed_min_check")
    csrc = os.path.join(ROOT, "deepgroebner_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, os.path.join(ROOT, "tests", "peel_keyed_min_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    rep = {ln.split()[0]: [int(v) for v in ln.split()[2::2]] for ln in p.stdout.splitlines() if " cases " in ln}
    rep["reach"] = dict(zip(*[iter([ln for ln in p.stdout.splitlines() if ln.startswith("reach:")][0].split()[1:])] * 2))
    return rep


def test_keyed_peel_emits_what_the_rule_says(report):
    assert report["box"] == [BOX_CASES, 0] and report["seeded"] == [SEEDED_CASES, 0], report
    assert report["keys"][0] > BOX_CASES and report["keys"][1] == 0, report       # every key named a live candidate of its index


def test_check_program_reaches_every_bank_and_the_degree_limit(report):
    r = {k: int(v) for k, v in report["reach"].items()}
    assert r["max_degree"] == 65535 and r["max_buckets"] >= 13, r                # (13: the most the workload showed)
    assert min(r["bank0"], r["bank1"], r["bank2"], r["bank3"]) > 0, r


def peel_shape(leads, f):
    """What the peel meets when an element with lead monomial f enters a basis with lead monomials `leads` (rows of exponents):
    (levels, buckets, the most buckets at one degree, the largest bucket, buckets with a coprime member, pairs emitted)."""
    L = np.maximum(leads, f[None, :])
    cp = (np.minimum(leads, f[None, :]).sum(1) == 0)
    n = len(L)
    div = (L[:, None, :] <= L[None, :, :]).all(2)                # div[j, i]: L_j | L_i
    same = (L[:, None, :] == L[None, :, :]).all(2)
    minimal = ~(div & ~same).any(0)
    seen, per_deg, biggest, with_cp, emitted = set(), {}, 0, 0, 0
    for i in range(n):
        if minimal[i] and tuple(L[i]) not in seen:
            seen.add(tuple(L[i]))
            members = same[i]
            per_deg[int(L[i].sum())] = per_deg.get(int(L[i].sum()), 0) + 1
            biggest = max(biggest, int(members.sum()))
            with_cp += int(cp[members].any())
            emitted += int(not cp[members].any())
    return len(per_deg), len(seen), max(per_deg.values()), biggest, with_cp, emitted


class Peels:
    """walk()'s observer: the shape of every insertion's peel, and the state the run stands in after every LAUNCH and CUT
    steps — left(o, t), the state t steps leave with a reset done, which is what the next step's before hook sees."""

    def __init__(self):
        self.seen = {k: [] for k in SITUATIONS}
        self.states, self.cuts, self.shapes, self.rows, self.leads = [], [], [], [], None

    def left(self, o, t):
        if t and t % LAUNCH == 0:
            self.states.append(ow.snapshot(o))
        if t and t % CUT == 0:
            self.cuts.append(o.copy())

    def before(self, o, t, action):
        self.left(o, t)
        if self.leads is None:                                   # (a new episode: the ideal's lead monomials)
            self.leads = [o.poly(i)[1][0] for i in range(o.nG)]
        self.g = o.nG

    def after(self, o, t, action, reward):
        g = self.g
        if o.nG == g + 1:                                        # an insertion: the new element is basis index g
            f = o.poly(g)[1][0]
            levels, buckets, widest, biggest, with_cp, emitted = peel_shape(np.array(self.leads), f)
            self.shapes.append((levels, buckets))
            self.leads.append(f)
            for k, shown in (("multi", widest >= 2), ("coprime", with_cp >= 1), ("triple", biggest >= 3), ("six", buckets >= 6),
                             ("none", emitted == 0), ("g64", g >= 64)):
                if shown:
                    self.seen[k].append(t)
        self.rows.append(o.nP)
        if o.nP == 0:
            self.leads = None


@functools.lru_cache(maxsize=None)
def walk(seed, aseed, nsteps=T):
    """nsteps steps of the hash agent with auto-reset on the oracle: ({situation: steps that show it}, [the state
    (oracle_walk.Snapshot: basis words, pair list, reducer order) after every LAUNCH steps], the environment as it stands
    afterwards, [a copy of the environment after every CUT steps], [(levels, buckets) of every insertion], [|P| after every
    step, before a reset])."""
    p = Peels()
    o = ow.walk(DIST, seed, aseed, nsteps, p)[0]
    p.left(o, nsteps)
    return p.seen, p.states, o, p.cuts, p.shapes, p.rows


def test_every_situation_is_reached():
    assert len(SEEDS) == len(set(SEEDS)) and T % LAUNCH == 0 and CUT % LAUNCH == 0
    shown = {k: [sa for sa in SEEDS if walk(*sa)[0][k]] for k in SITUATIONS}
    assert all(shown[k] for k in SITUATIONS), {k: len(v) for k, v in shown.items()}
    for k in SITUATIONS:                                         # these eight show every one of them
        assert len(shown[k]) == len(SEEDS) == 8, (k, shown[k])
    for k, where in KNOWN.items():
        for sa, t in where:
            assert t in walk(*sa)[0][k], (k, sa, t, walk(*sa)[0][k])


def test_rare_situations_fall_inside_a_launch_too():
    """The GPU test chains launches of LAUNCH steps; an insertion at the last step of a launch is followed by a write-back,
    one inside a launch by a step of the same kernel on the state it left.  Every situation shows inside a launch."""
    for k in SITUATIONS:
        steps = [t for sa in SEEDS for t in walk(*sa)[0][k]]
        assert any((t + 1) % LAUNCH for t in steps), (k, steps)


def test_the_emitted_count_is_the_growth_of_the_pair_list():
    """peel_shape's count of emitted pairs is the oracle's: |P| after an inserting step = what the update kept + emitted, so it
    is at least `emitted` — and exactly `emitted` when the step started from one pair (the selected one) — on every seed."""
    bo = ffi.load("bo")
    checked = 0
    for seed, aseed in SEEDS[:2]:
        o = bo.env(DIST); o.seed(seed); o.reset()
        for t in range(64):
            g, nP = o.nG, o.nP
            leads = np.array([o.poly(i)[1][0] for i in range(g)])
            o.step(ffi.agent_action(aseed, t, nP))
            if o.nG == g + 1:
                emitted = peel_shape(leads, o.poly(g)[1][0])[5]
                new = int((o.pairs()[:, 1] == g).sum())
                assert new == emitted, (seed, t, new, emitted)
                checked += 1
            if o.nP == 0:
                o.reset()
    assert checked >= 16
