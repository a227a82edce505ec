"""The host-stepped interface above 64 environments against the oracle: bbx_step_obs (step(), step_ragged(), reset()), bbx_reset
with a mask and bbx_obs on the device-buffer side of bbx_create's `zero_copy = batch <= 64` — actions uploaded, outputs copied
back from the device arrays, the padded observation in a device block that bbx_obs shares and that is enlarged inside a call,
the ragged block built by bbx_obs_offsets_kernel / bbx_obs_pack_kernel.  (test_gpu_parity.py and test_sessions.py hold the
pinned side, batches of 1 to 16.)  One oracle environment per environment; every comparison is exact and covers ALL
environments: rewards, dones, row counts, offsets, every observation matrix, after every call.  The cases and what the oracle
alone says about them: tests/host_step_cases.py, tests/test_host_step_cases_cpu.py."""
import numpy as np
import pytest

from oracle import ffi
from oracle.trace import poly_words
from tests import host_step_cases as hc

pytestmark = pytest.mark.gpu


def _make(c, **kw):
    from deepgroebner_amd import VecLeadMonomialsEnv
    env = VecLeadMonomialsEnv(c.dist, batch=c.batch, k=c.k, elimination=c.elimination, rewards=c.rewards, **kw)
    env.seed(np.arange(c.batch) + c.seed0)
    return env, hc.OracleBatch(ffi.load("bo"), c)


def _check_block(env, ob, flat, off, label):
    """the ragged block (flat [sum rows, cols], offsets [B + 1]) and env.rows against the oracle, every environment"""
    rows = ob.rows()
    assert env.rows.dtype == np.int32 and np.array_equal(env.rows, rows), (label, np.flatnonzero(env.rows != rows)[:8])
    assert off.dtype == np.int32 and off.shape == (ob.B + 1,) and off[0] == 0 and off[-1] == flat.shape[0], label
    assert np.array_equal(off, ob.offsets()), (label, np.flatnonzero(off != ob.offsets())[:8])
    assert flat.dtype == np.int32 and flat.ndim == 2 and flat.shape[1] == env.cols == 2 * env.nvars * ob.c.k, label
    want = [ob.obs(e) for e in range(ob.B)]
    if not np.array_equal(flat, np.concatenate(want)):
        for e in range(ob.B):
            assert np.array_equal(flat[off[e]:off[e + 1]], want[e]), (label, "environment", e)
        raise AssertionError(label)


def _check_list(env, ob, obs, label):
    """the list view (reset(), step()): one [rows_e, cols] matrix per environment"""
    assert len(obs) == ob.B and all(m.ndim == 2 and m.shape[1] == env.cols for m in obs), label
    off = np.concatenate([[0], np.cumsum([len(m) for m in obs])]).astype(np.int32)
    _check_block(env, ob, np.concatenate(obs), off, label)


def _step(env, ob, t, actions, auto_reset):
    """one step of both sides, step() and step_ragged() in turn; rewards, dones and the block of all environments compared"""
    want_r, want_d = ob.step(actions, auto_reset)
    if t % 2:
        flat, off, r, d = env.step_ragged(actions, auto_reset=auto_reset)
        check = lambda: _check_block(env, ob, flat, off, ("step_ragged", t))
    else:
        obs, r, d, infos = env.step(actions, auto_reset=auto_reset)
        assert infos == [{}] * ob.B
        check = lambda: _check_list(env, ob, obs, ("step", t))
    assert r.dtype == np.float64 and r.shape == (ob.B,) and (r == want_r).all(), (t, np.flatnonzero(r != want_r)[:8])
    assert d.dtype == bool and np.array_equal(d, want_d), (t, np.flatnonzero(d != want_d)[:8])
    check()


@pytest.mark.parametrize("name,lean", [(n, 0) for n in sorted(hc.SCAN)] + [(n, 1) for n in hc.SCAN_LEAN])
def test_steps_and_ragged_observations_across_the_scan_partition_boundaries(name, lean):
    """reset(), then steps with auto-reset at B = 65 (smallest batch of the device-buffer path; also with k = 1), 1024 (one
    environment per thread of the offsets kernel's scan), 1025 (two, the last owning thread holds one) and 2050 (three, the
    last one holds one); lean: accounting off.  Measured on the oracle: 54 / 54 / 197 / 197 / 217 episodes end inside the runs."""
    c = hc.SCAN[name]
    env, ob = _make(c)
    if lean:
        env.accounting(False)
    _check_list(env, ob, env.reset(), "reset")
    for t in range(c.steps):
        _step(env, ob, t, ob.actions(t), True)
    assert ob.episodes > 0
    print("%s lean %d: B %d, %d steps, %d episodes ended" % (name, lean, c.batch, c.steps, ob.episodes))


def test_wide_class_host_steps_with_more_workgroups_than_compute_units():
    """cyclic-6 at B = 300: the wide class, whose launches are two kernels above one workgroup per compute unit, stepped from
    the host; all environments start from the same ideal and diverge under the action rule."""
    c = hc.WIDE
    env, ob = _make(c)
    _check_list(env, ob, env.reset(), "reset")
    for t in range(c.steps):
        _step(env, ob, t, ob.actions(t), True)
    print("wide: B %d, %d steps, %d distinct row counts in the last block" % (c.batch, c.steps, len(set(ob.rows().tolist()))))


@pytest.mark.parametrize("name", sorted(hc.SPILL))
def test_environments_handed_to_the_hbm_resident_pass_inside_a_host_step(name):
    """3-8-6-uniform at B = 65 on the register/LDS class with a 16-element working copy: bases pass 16 elements from step 9
    on, those environments are continued by the HBM-resident pass inside the call, and its outputs and observation rows are the
    ones returned; without auto-reset, finished environments with such a basis sit next to live ones."""
    c = hc.SPILL[name]
    env, ob = _make(c, caps=hc.SPILL_CAPS)
    _check_list(env, ob, env.reset(), "reset")
    for t in range(c.steps):
        _step(env, ob, t, ob.actions(t), c.auto_reset)
    print("spill %s: B %d, %d steps, %d episodes ended, largest basis %d" % (name, c.batch, c.steps, ob.episodes, max(o.nG for o in ob.o)))


@pytest.mark.parametrize("name", sorted(hc.PLAIN))
def test_plain_steps_and_observations_of_the_current_state(name):
    """bbx_step (B = 65, no auto-reset: finished environments report 0.0 / done / 0 rows) and bbx_step_autoreset (B = 1025)
    through the C entries — no observation in the call —, outputs written over poisoned arrays; every fifth step
    observations() (bbx_obs, rows.max() rows per environment: the shared device block at whatever size that is)."""
    from deepgroebner_amd import _ffi
    c = hc.PLAIN[name]
    env, ob = _make(c)
    _check_list(env, ob, env.reset(), "reset")
    fn = _ffi.lib().bbx_step_autoreset if c.auto_reset else _ffi.lib().bbx_step
    for t in range(c.steps):
        acts = ob.actions(t)
        want_r, want_d = ob.step(acts)
        r = np.full(ob.B, 7.0); d = np.full(ob.B, 9, dtype=np.uint8); env.rows[:] = -5
        _ffi.check(fn(env._h, _ffi.ptr(acts), _ffi.ptr(r), _ffi.ptr(d), _ffi.ptr(env.rows)))
        assert (r == want_r).all() and np.array_equal(d, want_d.astype(np.uint8)) and np.array_equal(env.rows, ob.rows()), t
        if t % hc.PLAIN_OBS_EVERY == 0:
            _check_list(env, ob, env.observations(), ("observations", t))
    _step(env, ob, 0, np.zeros(ob.B, dtype=np.int32), c.auto_reset)       # (a step with its observation behind them)
    print("plain %s: B %d, %d steps, %d episodes ended" % (name, c.batch, c.steps, ob.episodes))


def test_no_auto_reset_masked_resets_empty_slices_and_the_empty_block():
    """B = 65 without auto-reset until every environment has finished (184 steps): finished environments own an empty slice
    between live neighbours and report (0.0, done, 0 rows); every twelfth step up to step 60 every other finished one is reset
    with reset(mask) (21 in all).  In the end the block is (0, cols) with all-equal offsets, and reset() starts everything again."""
    from deepgroebner_amd import _ffi
    c = hc.FINISH
    env, ob = _make(c)
    _check_list(env, ob, env.reset(), "reset")
    t = resets = between = events = 0
    while ob.rows().sum() > 0:
        assert t < c.steps
        _step(env, ob, t, ob.actions(t), False)
        rows = ob.rows()
        between += bool(((rows[:-2] > 0) & (rows[1:-1] == 0) & (rows[2:] > 0)).any())
        mask = hc.finish_reset_mask(t, rows)
        if mask.any():
            ob.reset(mask)
            resets += int(mask.sum())
            events += 1
            if events % 2:
                _check_list(env, ob, env.reset(mask), ("reset(mask)", t))
            else:                                                    # bbx_reset's own row counts, then the current state
                env.rows[:] = -5
                _ffi.check(_ffi.lib().bbx_reset(env._h, _ffi.ptr(mask), _ffi.ptr(env.rows)))
                assert np.array_equal(env.rows, ob.rows()), t
                _check_list(env, ob, env.observations(), ("observations after bbx_reset(mask)", t))
        t += 1
    assert (resets, t) == hc.FINISH_WITH_RESETS and between >= 60
    for i in range(2):                                               # everything finished: both views of the empty block
        want_r, want_d = ob.step(np.zeros(ob.B, dtype=np.int32), False)
        if i:
            flat, off, r, d = env.step_ragged(np.zeros(ob.B, dtype=np.int32))
        else:
            obs, r, d, _ = env.step(np.zeros(ob.B, dtype=np.int32))
            assert len(obs) == ob.B and all(m.shape == (0, env.cols) for m in obs)
            flat, off = np.concatenate(obs), np.zeros(ob.B + 1, dtype=np.int32)
        assert flat.shape == (0, env.cols) and flat.dtype == np.int32 and (off == 0).all() and off.shape == (ob.B + 1,)
        assert (r == 0.0).all() and d.all() and (env.rows == 0).all() and not want_r.any() and want_d.all()
    ob.reset()
    _check_list(env, ob, env.reset(), "reset after the empty block")
    for i in range(4):
        _step(env, ob, i, ob.actions(i), False)
    print("finish: B %d, %d steps, %d episodes ended, %d masked resets" % (c.batch, t, ob.episodes, resets))


def test_device_observation_block_enlarged_inside_a_step():
    """5-10-5-uniform at B = 66: one environment passes 128 rows at step 41 and 256 at step 102 while all others stay below, so
    the device block is enlarged (128 -> 256 -> 512 rows per environment) and rewritten by the second attempt of those calls."""
    c = hc.GROW_STEP
    env, ob = _make(c)
    _check_list(env, ob, env.reset(), "reset")
    cap, grown_at = hc.BLOCK_ROWS, []
    for t in range(c.steps):
        _step(env, ob, t, ob.actions(t), True)
        while cap < ob.rows().max():
            cap *= 2
            grown_at.append(t)
    assert grown_at == [hc.GROW_STEP_AT[128], hc.GROW_STEP_AT[256]]
    print("grow_step: B %d, %d steps, enlargements at steps %s" % (c.batch, c.steps, grown_at))


def test_device_observation_block_enlarged_inside_reset():
    """3-20-140-weighted at B = 66: 137 to 150 rows at reset, so the observation call inside the first reset() enlarges the block."""
    c = hc.GROW_RESET
    env, ob = _make(c)
    assert ob.rows().min() > hc.BLOCK_ROWS
    _check_list(env, ob, env.reset(), "reset")
    for t in range(c.steps):
        _step(env, ob, t, ob.actions(t), True)
    ob.reset()
    _check_list(env, ob, env.reset(), "second reset")


@pytest.mark.parametrize("name", sorted(hc.SHARED))
def test_padded_and_ragged_observations_share_the_device_block(name):
    """bbx_obs and bbx_step_obs write the same device block.  bbx_reset through the C entry (no ragged observation yet), then
    observations(max_rows = rows.max() + 1) leaves it 20 rows per environment; the steps that follow enlarge it by doubling
    from there (20 -> 40 -> 80); in between, padded observations with fewer rows than the block has: -1 fill behind the live
    rows, live rows equal to the oracle's; then more steps."""
    from deepgroebner_amd import _ffi
    c = hc.SHARED[name]
    env, ob = _make(c)
    _ffi.check(_ffi.lib().bbx_reset(env._h, None, _ffi.ptr(env.rows)))
    assert np.array_equal(env.rows, ob.rows())

    def padded(max_rows, label):
        block = env.observations(max_rows=max_rows, fill=True)
        assert block.shape == (ob.B, max_rows, env.cols) and block.dtype == np.int32
        rows = ob.rows()
        assert rows.max() <= max_rows
        for e in range(ob.B):
            assert np.array_equal(block[e, :rows[e]], ob.obs(e)) and (block[e, rows[e]:] == -1).all(), (label, e)

    cap = int(env.rows.max()) + 1
    padded(cap, "first")
    caps, probes = [cap], 0
    for t in range(c.steps):
        _step(env, ob, t, ob.actions(t), True)
        rows = ob.rows()
        while cap < rows.max():
            cap *= 2
        caps.append(cap)
        mr = hc.shared_probe_rows(t, rows, cap)
        if mr:
            padded(mr, t)
            probes += 1
    assert caps[-1] >= 4 * caps[0] and probes >= 3
    print("shared %s: B %d, %d steps, %d episodes ended, block rows %s, %d padded observations in between"
          % (name, c.batch, c.steps, ob.episodes, sorted(set(caps)), probes))


def test_records_and_device_observation_block_grow_in_the_same_call():
    """The trajectory of test_gpu_parity.py's test_step_with_observation_when_the_records_and_the_observation_block_grow_in_the_
    same_call (5-3-3-0.5-uniform, LCM elimination, the python flavour) in environments 0..4 of a batch of 65: at step 24 an
    intermediate polynomial of 5980 terms enlarges the records and a pair set of 279 rows the device block (256 -> 512)."""
    c = hc.GROW_BOTH
    env, ob = _make(c, mimic="python")
    drv = hc.GrowBothDriver()
    _check_list(env, ob, env.reset(), "reset")
    for t in range(c.steps):
        acts = drv.actions(ob)
        live = ob.rows() > 0
        _step(env, ob, t, acts, False)
        mask = drv.reset_mask(ob, live)
        if mask.any():
            ob.reset(mask)
            _check_list(env, ob, env.reset(mask), ("reset(mask)", t))
    assert env.capacities()["grown"] >= 1 and ob.rows().max() > 256
    print("grow_both: B %d, %d steps, records grown %d times, tallest pair set %d" % (c.batch, c.steps, env.capacities()["grown"], ob.rows().max()))


def _state_words(basis, pairs, order):
    words = [poly_words(co, x) for co, x in basis]
    return np.concatenate(words + [np.asarray(pairs, np.int32).ravel(), np.asarray(order, np.int32)])


def test_bad_action_in_one_environment_of_a_large_batch():
    """B = 65: an action equal to the row count in ONE environment raises BbxError (BBX_E_ACTION, as for one environment); the
    other environments have taken the step — their states are the oracle's — and a reset of that environment clears the error."""
    from deepgroebner_amd import _ffi
    c = hc.ERROR
    env, ob = _make(c)
    _check_list(env, ob, env.reset(), "reset")
    bad_env = 37
    for t in range(c.steps):
        acts = ob.actions(t)
        if t != 5:
            _step(env, ob, t, acts, True)
            continue
        acts[bad_env] = ob.rows()[bad_env]
        with pytest.raises(_ffi.BbxError) as ei:
            env.step(acts, auto_reset=True)
        assert ei.value.code == -6 and "environment %d" % bad_env in str(ei.value)
        ob.step(acts, True, skip=(bad_env,))                           # the others took their step
        mask = np.zeros(ob.B, dtype=np.uint8); mask[bad_env] = 1
        ob.reset(mask)
        _check_list(env, ob, env.reset(mask), "reset(mask) after the error")
        for e in range(ob.B):
            o = ob.o[e]
            assert np.array_equal(_state_words(*env.state(e)), _state_words(o.basis(), o.pairs(), o.reducer_order())), e


def test_copy_of_a_handle_with_an_enlarged_device_observation_block():
    """env.copy() after the observation block has been enlarged (3-20-140-weighted, B = 66): copy and original step
    independently — different actions — and both agree with their oracles."""
    c = hc.COPY
    env, ob = _make(c)
    _check_list(env, ob, env.reset(), "reset")
    for t in range(3):
        _step(env, ob, t, ob.actions(t), True)
    env2, ob2 = env.copy(), ob.copy()
    assert np.array_equal(env2.rows, ob2.rows())
    for t in range(3, c.steps):
        _step(env, ob, t, ob.actions(t), True)
        _step(env2, ob2, t + 1, ob2.actions(t + 7), True)
    ob2.reset()
    _check_list(env2, ob2, env2.reset(), "reset of the copy")
    _step(env, ob, 0, ob.actions(1), True)
