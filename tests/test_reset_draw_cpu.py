"""The fast class draws a reset's ideal across the lanes (gen_ideal_lanes in bbx_device.h): all raw engine outputs of the
ideal in one jump-ahead step, generator f decoded by lane f from the raws a draw without rejections would have given it
(bbx_gen_decode in bbx_common.h, the one statement of it for kernel and host), and the sequential draw instead whenever a
generator deviates.  tests/reset_draw_check.cpp drives that decode on the host from a host-computed raw batch — built
here with -fsanitize=address,undefined — and holds it against the sequential generator (BinomialGen, bbx_ideals.cpp):
same generators, same engine state afterwards (the next ideal), over random and constructed engine states."""
import os
import subprocess

import pytest

from oracle import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 2 ** 31 - 1
DISTS = ["3-20-10-weighted", "3-20-10-weighted-homog", "3-20-10-weighted-pure", "3-20-10-weighted-consts", "3-20-11-weighted",
         "3-20-10-maximum", "3-2-10-uniform", "2-5-4-uniform"]
COUNT = 4000


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("reset_draw") / "reset_draw_check")
    csrc = os.path.join(ROOT, "deepgroebner_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, os.path.join(ROOT, "tests", "reset_draw_check.cpp"),
                           os.path.join(csrc, "bbx_ideals.cpp"), "-o", exe])
    p = subprocess.run([exe, str(COUNT)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    return [ln.split() for ln in p.stdout.splitlines()]


def test_jump_multipliers_are_engine_steps(report):
    """A_k x_0 mod m against k sequential engine steps, k = 1..128, from x_0 in {1, 2, m - 1} and 200 random states."""
    (line,) = [ln for ln in report if ln[0] == "jump"]
    assert int(line[2]) == 203 and int(line[4]) == 0, line


@pytest.mark.parametrize("dist", DISTS)
def test_batch_decode_equals_sequential_generator(report, dist):
    (line,) = [ln for ln in report if ln[0] == "dist" and ln[1] == dist]
    got = dict(zip(line[2::2], (int(v) for v in line[3::2])))
    flags_pure, homog = "pure" in dist, "homog" in dist
    assert got["stride"] == (0 if flags_pure else 1) + (2 if homog else 4) + 2
    assert got["mismatches"] == 0, line
    assert got["batch"] + got["fallback"] == COUNT
    assert got["batch"] > 0, "the batch path was never taken"
    if dist == "3-2-10-uniform":                             # six monomials of degree 2: equal monomials, hence the fallback, are common
        assert got["fallback"] > COUNT // 10 and got["batch"] > COUNT // 10, line
    if dist == "3-20-10-weighted":                           # the benchmark's distribution: the batch is the rule
        assert got["batch"] > COUNT * 9 // 10, line


def test_constructed_rejections(report):
    """Engine states x_0 = t / A_k that put a raw past the distribution's bound at the coefficient draw, at a monomial draw and
    at the last generator's last draw: the batch must deviate at exactly that generator; one below the bound it must not."""
    lines = [ln for ln in report if ln[0] == "reject"]
    assert not [ln for ln in lines if ln[-1] == "BAD"]
    for dist in DISTS:
        kinds = {ln[2]: ln[-1] for ln in lines if ln[1] == dist}
        want = {"choice", "last-draw"} | (set() if "pure" in dist else {"coefficient", "coefficient-at-past", "coefficient-below-past"})
        assert set(kinds) == want, (dist, kinds)
        if dist.startswith("3-20-"):                         # (in the small distributions an earlier generator deviates by chance)
            assert set(kinds.values()) == {"ok"}, (dist, kinds)


def rejection_states(npoly, stride, pure=False):
    """The constructed engine states, as the host program builds them (the GPU tests seed environments with them)."""
    at = {"choice": 3 * stride + stride - 1, "last-draw": npoly * stride}
    if not pure:
        at["coefficient"] = 2 * stride + 1
    return {what: (M - 1) * pow(16807, -k, M) % M for what, k in at.items()}


def test_constructed_states_against_the_oracle():
    """The same states through the oracle's generator: from a state R the sequential draw takes more raws than the stride
    allows — one more for a monomial draw; two more for the coefficient draw, whose replacement m - 16807 is past the bound
    again — and the state npoly * stride raws BEFORE R leads to R."""
    bo = ffi.load("bo")
    dist, npoly, stride = "3-20-10-weighted", 10, 7

    def first(state, skip=0):
        g = bo.generator(dist)
        g.seed(state % M)
        for _ in range(skip):
            g.next()
        return g.next()

    for what, R in rejection_states(npoly, stride).items():
        extra = 2 if what == "coefficient" else 1
        assert first(R, skip=1) == first(R * pow(16807, npoly * stride + extra, M)), what
        if what != "last-draw":                              # (there the next ideal's coefficient draw skips m - 1 and m - 16807 anyway)
            assert first(R, skip=1) != first(R * pow(16807, npoly * stride, M)), what
        assert first(R * pow(16807, -npoly * stride, M), skip=1) == first(R), what
