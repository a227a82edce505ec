"""The fast class keeps, per basis element, the two coefficients an S-polynomial takes from it — tc/lc and -tc/lc, formed
once when the element enters (bbx_ginfo_hot, bbx_common.h) — instead of multiplying tc by 1/lc for both members of every
selected pair.  tests/spoly_coef_check.cpp drives the two helpers on the host — built here with
-fsanitize=address,undefined — over every lead coefficient against the formulas the step evaluated before.  The second half
asserts, on the oracle alone, that the seeds tests/test_spoly_coef_gpu.py runs reach the cases that change: elements
WITHOUT a tail (both coefficients 0) selected later as the first and as the second member of a pair, and pairs whose
members both have a tail and a lead coefficient other than 1 (ideal seeds 5000..5399 with agent seed = ideal seed - 4000
all select a single-term element within 128 steps; eight of them are fixed here)."""
import functools
import os
import subprocess

import pytest

from tests import oracle_walk as ow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST, K, T, P = "3-20-10-weighted", 2, 128, 32003
SEEDS = ((5001, 1001), (5012, 1012), (5015, 1015), (5019, 1019), (5041, 1041), (5082, 1082), (5091, 1091), (5118, 1118))
NTC = 64                                                     # tail coefficients per lead coefficient: 5 fixed + 59 seeded


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoly_coef") / "spoly_coef_check")
    csrc = os.path.join(ROOT, "deepgroebner_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, os.path.join(ROOT, "tests", "spoly_coef_check.cpp"),
                           os.path.join(csrc, "bbx_ideals.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    return {ln.split()[0]: [int(v) for v in ln.split()[2::2]] for ln in p.stdout.splitlines() if "cases" in ln}


@pytest.mark.parametrize("what,cases", (("inverse", P - 1), ("halves", (P - 1) * NTC), ("range", (P - 1) * NTC), ("zero", P - 1),
                                        ("roundtrip", (P - 1) * NTC), ("mulmod", (P - 1) * NTC)))
def test_working_word_of_every_lead_coefficient(report, what, cases):
    """halves: tc/lc and -tc/lc as the step formed them; range: both below p; zero: tc == 0 gives 0 | 0 and nothing else
    does; roundtrip: record word -> working word + kept word -> record word."""
    assert report[what] == [cases, 0], (what, report[what])


@functools.lru_cache(maxsize=None)
def walk(seed, aseed, nsteps=T):
    """nsteps steps of the hash agent with auto-reset on the oracle: (the environment as it stands afterwards, per-step
    rewards, done flags, the selections as (step, what the first member is, what the second is), the number of single-term
    insertions) — a member is "none" (no tail), "monic" (tail, lead coefficient 1) or "scaled" (tail, another one)."""
    def kind(o, g):
        c = o.poly(int(g))[0]
        return "none" if len(c) == 1 else ("monic" if c[0] == 1 else "scaled")

    def before(o, t, a):
        i, j = o.pairs()[a]
        return t, kind(o, i), kind(o, j), o.nG

    def after(o, t, a, r):                                   # a single-term element entered: the new one is the last
        return o.nG, len(o.poly(o.nG - 1)[0])

    o, rewards, dones, seen = ow.walk(DIST, seed, aseed, nsteps, (before, after))
    single = sum(int(nG1 > nG0 and terms == 1) for (_, _, _, nG0), (nG1, terms) in seen)
    return o, rewards, dones, [pick[:3] for pick, _ in seen], single


def test_seeds_select_elements_without_tail_on_both_sides():
    assert len(SEEDS) == len(set(SEEDS)) == 8
    first = second = both_scaled = 0
    for sa in SEEDS:
        _, _, dones, picks, single = walk(*sa)
        # (generators are binomials: a single-term element entered by a step of this run)
        assert single >= 1, sa
        assert any(a == "none" or b == "none" for _, a, b in picks), sa
        first += any(a == "none" for _, a, _ in picks)
        second += any(b == "none" for _, _, b in picks)
        both_scaled += any(a == "scaled" and b == "scaled" for _, a, b in picks)
        assert dones.sum() >= 1, sa                              # episodes end inside the run: resets install new ideals
    assert first >= 2 and second >= 2 and both_scaled >= 1, (first, second, both_scaled)
    # what the search found for these eight: every one of them has all three cases
    assert (first, second, both_scaled) == (8, 8, 8)
