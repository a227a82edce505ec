"""The cases of tests/host_step_cases.py on the oracle alone: each has the property it exists for.  A later change of a seed, a
step count or the action rule that empties a case of tests/test_host_step_large_gpu.py fails here, without a GPU."""
import numpy as np
import pytest

from tests import host_step_cases as hc


def _run(bo, c, steps=None):
    """-> (OracleBatch after the run, row counts [steps + 1, B]: at reset, then after every step)"""
    ob = hc.OracleBatch(bo, c)
    rows = [ob.rows()]
    for t in range(c.steps if steps is None else steps):
        ob.step(ob.actions(t))
        rows.append(ob.rows())
    return ob, np.array(rows)


def _neighbours_differ(rows):
    """every block of the run has neighbouring environments with different row counts: offsets are no multiples of one number"""
    return bool((np.diff(rows, axis=1) != 0).any(axis=1).all())


@pytest.mark.parametrize("name", sorted(hc.SCAN))
def test_scan_cases_end_episodes_and_have_ragged_rows(bo, name):
    c = hc.SCAN[name]
    ob, rows = _run(bo, c)
    assert c.batch > 64 and c.auto_reset
    assert ob.episodes >= (50 if c.batch == 65 else 150), ob.episodes     # (measured: 54 / 197 / 197 / 217)
    assert _neighbours_differ(rows)
    assert (rows > 0).all() and rows.max() < hc.BLOCK_ROWS               # auto-reset: no empty slice; the block never grows here
    # more than one row count inside the share of one scan thread, and across the last thread that owns any environment
    per = hc.per_thread(c.batch)
    if per > 1:
        owned = rows[-1][:c.batch - c.batch % per].reshape(-1, per)
        assert (owned.min(axis=1) != owned.max(axis=1)).sum() > owned.shape[0] // 2


def test_scan_batches_sit_on_the_partition_boundaries():
    per = {c.batch: hc.per_thread(c.batch) for c in hc.SCAN.values()}
    assert per == {65: 1, 1024: 1, 1025: 2, 2050: 3}
    assert 1025 % 2 == 1 and 2050 % 3 == 1                                # the last owning thread holds ONE environment
    assert sorted({c.k for c in hc.SCAN.values()}) == [1, 2]
    assert all(n in hc.SCAN for n in hc.SCAN_LEAN) and {hc.per_thread(hc.SCAN[n].batch) for n in hc.SCAN_LEAN} == {1, 2}


def test_wide_case_diverges_from_one_ideal(bo):
    c = hc.WIDE
    ob, rows = _run(bo, c)
    assert c.dist.startswith("cyclic") and c.batch > 256 and hc.per_thread(c.batch) == 1   # more workgroups than an MI355X has CUs
    assert len(set(rows[0].tolist())) == 1 and _neighbours_differ(rows[6:])
    assert len(set(rows[-1].tolist())) >= 10 and rows.min() > 0


@pytest.mark.parametrize("name", sorted(hc.PLAIN))
def test_plain_step_cases(bo, name):
    c = hc.PLAIN[name]
    ob, rows = _run(bo, c)
    assert ob.episodes > 0 and _neighbours_differ(rows)
    assert c.steps >= 4 * hc.PLAIN_OBS_EVERY
    if not c.auto_reset:                                                  # finished and live environments side by side
        seen = rows[hc.PLAIN_OBS_EVERY::hc.PLAIN_OBS_EVERY]                # (the blocks that are observed)
        assert ((seen == 0).any(axis=1) & (seen > 0).any(axis=1)).sum() >= 5


@pytest.mark.parametrize("name", sorted(hc.SPILL))
def test_spill_cases_outgrow_the_small_working_copy(bo, name):
    c = hc.SPILL[name]
    ob = hc.OracleBatch(bo, c)
    cap = hc.SPILL_CAPS["lds_max_basis"]
    mixed = big_finished = 0
    for t in range(c.steps):
        ob.step(ob.actions(t))
        nG, rows = np.array([o.nG for o in ob.o]), ob.rows()
        mixed += bool(((nG > cap) & (rows > 0)).any() and ((nG <= cap) & (rows > 0)).any())   # both kinds live in one block
        big_finished += int(((nG > cap) & (rows == 0)).sum())
    assert c.batch > 64 and ob.episodes >= 50 and mixed >= (20 if c.auto_reset else 10), (ob.episodes, mixed)   # (measured: 63 / 57 episodes)
    assert (big_finished > 100) == (not c.auto_reset)


def test_finish_case_empties_the_block_with_finished_environments_between_live_ones(bo):
    c = hc.FINISH
    assert not c.auto_reset and c.batch == 65
    ob, rows = _run(bo, c, hc.FINISH_ALL_DONE_AT + 1)
    total = rows.sum(axis=1)
    assert total[-1] == 0 and (total[:-1] > 0).all()                      # after step FINISH_ALL_DONE_AT, not before
    assert ob.episodes == c.batch
    # finished environments between live ones: a block with (live, finished, live) somewhere in it, for most of the run
    between = [bool(((r[:-2] > 0) & (r[1:-1] == 0) & (r[2:] > 0)).any()) for r in rows]
    assert sum(between) >= 60, sum(between)
    assert _neighbours_differ(rows[:-1])
    # the run of the GPU test, with its masked resets: resets happen, of finished environments only, and it still ends
    ob = hc.OracleBatch(bo, c)
    resets, t = 0, 0
    while ob.rows().sum() > 0:
        ob.step(ob.actions(t))
        mask = hc.finish_reset_mask(t, ob.rows())
        assert not (mask.astype(bool) & (ob.rows() > 0)).any()
        resets += int(mask.sum())
        ob.reset(mask)
        t += 1
        assert t <= c.steps
    assert (resets, t) == hc.FINISH_WITH_RESETS, (resets, t)


def test_grow_step_case_passes_128_and_256_rows_in_one_environment(bo):
    c = hc.GROW_STEP
    ob, rows = _run(bo, c)
    assert c.batch > 64 and rows[0].max() <= 10
    for threshold, at in hc.GROW_STEP_AT.items():
        over = rows[1:].max(axis=1) > threshold
        assert int(np.flatnonzero(over)[0]) == at, (threshold, np.flatnonzero(over)[:1])
        assert (rows[at + 1] > threshold).sum() == 1                      # one environment triggers it ...
        assert np.sort(rows[at + 1])[-2] < threshold                      # ... all others are below at that step
    assert rows.max() <= 4 * hc.BLOCK_ROWS                                # two enlargements: 128 -> 256 -> 512
    assert _neighbours_differ(rows)


@pytest.mark.parametrize("c", [hc.GROW_RESET, hc.COPY], ids=["grow_reset", "copy"])
def test_grow_reset_case_starts_above_the_first_block(bo, c):
    ob, rows = _run(bo, c)
    assert c.batch > 64
    assert rows[0].min() > hc.BLOCK_ROWS and rows.max() <= 2 * hc.BLOCK_ROWS   # (measured at reset: 137 to 150)
    assert _neighbours_differ(rows)


@pytest.mark.parametrize("name", sorted(hc.SHARED))
def test_shared_block_case_doubles_from_an_odd_capacity(bo, name):
    c = hc.SHARED[name]
    ob, rows = _run(bo, c)
    cap0 = int(rows[0].max()) + 1
    caps = hc.shared_capacities(rows)
    assert cap0 == 20 and cap0 & (cap0 - 1)                               # small and no power of two
    assert caps[0] == cap0 and caps[-1] >= 4 * cap0                       # enlarged at least twice, by doubling
    probes = [t for t in range(c.steps) if hc.shared_probe_rows(t, rows[t + 1], caps[t + 1])]
    assert len(probes) >= 3 and len({int(caps[t + 1]) for t in probes}) >= 2   # bbx_obs in between, at different capacities
    assert ob.episodes > 0 and _neighbours_differ(rows)


def test_grow_both_case_reaches_both_growth_conditions_in_the_same_step(bo):
    c = hc.GROW_BOTH
    ob, drv = hc.OracleBatch(bo, c), hc.GrowBothDriver()
    bo.fn("stat_max_terms")(1)
    both = []
    for t in range(c.steps):
        acts = drv.actions(ob)
        live = ob.rows() > 0
        before = int(ob.rows().max())
        ob.step(acts)
        longest = bo.fn("stat_max_terms")(1)
        after = int(ob.rows().max())
        # the call's observation needs a larger block (256 -> 512) and its step a longer polynomial than the records hold
        both.append(before <= 2 * hc.BLOCK_ROWS < after and longest > hc.MAX_POLY_TERMS)
        mask = drv.reset_mask(ob, live)
        ob.reset(mask)
    assert sum(both) == 1 and both[24]
    assert ob.rows().max() > 256
    rows = ob.rows()
    assert (rows == 0).any() and (rows > 0).any()                         # finished environments stay in the batch


def test_error_case_has_room_for_a_bad_action(bo):
    c = hc.ERROR
    ob, rows = _run(bo, c)
    assert c.batch == 65 and (rows > 0).all()
