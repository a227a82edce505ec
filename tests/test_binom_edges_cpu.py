"""tests/binom_cases.py without a device: the restatement of the binomial step agrees with the oracle on every step of every
case, and the seeds tests/test_binom_edges_gpu.py runs show the situations they were chosen for at the steps pinned there."""
import pytest

from tests import binom_cases as bc

NAMES = sorted(bc.CASES)


def test_register_part_is_read_from_the_kernel_header():
    assert set(bc.header_constants()) == {8, 16, 32} and all(1 <= v <= 16 for v in bc.header_constants().values())
    assert bc.mono_bytes("3-20-10-weighted") == 8 and bc.mono_bytes("5-10-5-uniform") == 16 and bc.mono_bytes("4-5-4-uniform") == 16
    assert bc.mono_bytes("8-3-4-weighted") == 32
    for c in bc.CASES.values():
        assert c.part == bc.register_part(c.dist) == 64 * bc.header_constants()[bc.mono_bytes(c.dist)]


def test_merge2_of_the_restatement():
    from oracle import ffi
    bo = ffi.load("bo")
    hi, lo = (0, 2, 0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0, 0, 0)
    assert bo.mono_gt(hi, lo) and not bo.mono_gt(lo, hi)
    assert bc.merge2(bo, None, None) == (None, None, None)
    assert bc.merge2(bo, (5, lo), None) == ((5, lo), None, None) == bc.merge2(bo, None, (5, lo))
    assert bc.merge2(bo, (5, lo), (7, hi)) == ((7, hi), (5, lo), None) == bc.merge2(bo, (7, hi), (5, lo))
    assert bc.merge2(bo, (5, lo), (7, lo)) == ((12, lo), None, "sum")
    assert bc.merge2(bo, (5, lo), (bc.P - 5, lo)) == (None, None, "cancel")
    assert bc.merge2(bo, (bc.P - 1, lo), (2, lo)) == ((1, lo), None, "sum")


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_oracle_on_every_step(name):
    """remainder == the oracle's new element, term for term; |G| unchanged where it is zero (walk_env compares [] with [])"""
    c = bc.CASES[name]
    assert 2 <= len(c.seeds) <= 16 and len(set(c.seeds)) == len(c.seeds) and 30 <= c.steps <= 128
    for e in range(len(c.seeds)):
        w = bc.case_walk(name, e)
        assert len(w.steps) == len(w.new) == c.steps
        assert w.disagreements == [], (name, c.seeds[e], "steps", w.disagreements[:5])
        for st, new in zip(w.steps, w.new):
            assert st.remainder == new and len(new) <= 2
            assert all(0 < co < bc.P for co, _ in new)


@pytest.mark.parametrize("name", NAMES)
def test_pinned_steps_show_their_situations(name):
    c = bc.CASES[name]
    assert c.pins
    for sit, where in c.pins.items():
        assert sit in bc.EDGE_SITUATIONS + bc.SCAN_SITUATIONS and where
        for e, t in where:
            assert sit in bc.case_walk(name, e).steps[t].situations, (name, sit, c.seeds[e], "step", t)
    for idx, where in c.index_pins.items():
        assert idx in (c.part - 1, c.part) and where
        for e, t in where:
            assert idx in bc.case_walk(name, e).steps[t].used, (name, "reducer index", idx, c.seeds[e], "step", t)


@pytest.mark.parametrize("group", sorted(bc.GROUPS))
def test_every_group_covers_its_list(group):
    names = bc.GROUPS[group]
    pinned = set().union(*(bc.CASES[n].pins for n in names))
    want = set(bc.required(group)) - set(bc.LEFT_OUT.get(group, ()))
    assert want <= pinned, (group, sorted(want - pinned))
    assert set(bc.LEFT_OUT.get(group, ())) <= {"new_lc_one_tail", "new_lc_pm1"}       # (nothing else may be left out)
    for n in names:                                          # the largest reducer-order index a round of the case uses
        c = bc.CASES[n]
        assert max(max(st.used, default=-1) for e in range(len(c.seeds)) for st in bc.case_walk(n, e).steps) == c.largest_index, n
    if group.startswith("deep"):
        for n in names:                                      # every deep case shows all three by itself, beyond the register part
            c = bc.CASES[n]
            assert set(bc.SCAN_SITUATIONS) <= set(c.pins), n
            assert c.largest_index >= c.part
            if not c.opts.get("sort_reducers", True):        # (and the unsorted ones rounds at exactly 64 SR - 1 and 64 SR)
                assert set(c.index_pins) == {c.part - 1, c.part}, n
        return
    for n in names:
        assert bc.CASES[n].largest_index < bc.CASES[n].part - 64, n
    if group.startswith("edges"):                            # (the four groups of eight or sixteen pairs)
        assert sum(len(bc.CASES[n].seeds) for n in names) in (8, 16)
        for n in names:                                      # an episode ends inside every run: resets install new ideals
            c = bc.CASES[n]
            assert c.steps == 128
            for e in range(len(c.seeds)):
                assert bc.case_walk(n, e).dones.sum() >= 1, (n, c.seeds[e])


def test_every_class_and_option_has_its_case():
    """(distribution, options, caps) of the classes the cases are about: 8-byte HBM-resident and staged, 16-byte, 32-byte"""
    by = {(c.dist, tuple(sorted(c.opts.items())), None if c.caps is None else tuple(sorted(c.caps.items()))) for c in bc.CASES.values()}
    U, H = (("sort_reducers", False),), (("lds_max_basis", -1),)
    for key in (("8-3-200-uniform", U, None), ("4-8-400-uniform", U, None), ("3-20-510-weighted", U, H), ("3-20-510-weighted", U, None),
                ("3-20-10-weighted", (), H), ("3-20-10-weighted", U, None), ("4-5-4-uniform", (), None), ("5-10-5-uniform", (), None),
                ("8-3-4-weighted", (), None)):
        assert key in by, key
    assert any(1000 in [s for s, _ in c.seeds] for c in bc.CASES.values() if c.dist == "3-20-510-weighted" and c.caps == bc.HBM)
