"""bbx_action_values on the device: Q[e][a] = r + gamma * value(strategy) of a copy of environment e stepped with action a,
== on doubles against the loop it replaces (copy, step, values: tests/action_value_cases.py twin_action_values) on every
kernel class, against the CPU oracle, from bases whose generator lead monomials tie, with padding, truncation, passes of
every size, growth of the records, and with the handle left exactly as it was."""
import time

import numpy as np
import pytest

import __graft_entry__ as graft
from oracle import ffi
from tests import action_value_cases as A
from tests import value_tie_cases as V
from tests.fast_harness import stream
from tests.test_values_device import CASES, _make          # the six cases (every kernel class bbx_values serves) and their batch

pytestmark = pytest.mark.gpu

OBS_ROWS = 512
STRATEGIES = ("degree", "normal", "sugar", "first", "env")      # 'env' selects First, as in bbx_values


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def _check_block(got, want, what):
    """(rc, q, rewards, dones, rows) of the call against (q, rewards, dones, rows) of a reference: == on doubles, no NaN where
    a < rows[e], nothing but NaN (dones: 0) beyond."""
    rc, q, r, d, rows = got
    wq, wr, wd, wrows = want
    assert rc == 0, what
    assert np.array_equal(rows, wrows), (what, rows, wrows)
    R = q.shape[1]
    live = np.arange(R)[None, :] < np.minimum(rows, R)[:, None]
    assert np.array_equal(np.isnan(q), ~live) and np.array_equal(np.isnan(r), ~live) and not d[~live].any(), what
    assert A.same_block(q, wq), (what, "q differs at", np.argwhere(~(q == wq) & live).tolist()[:8])
    assert A.same_block(r, wr), (what, "rewards")
    assert np.array_equal(d, wd), (what, "dones")


def _state_of(env):
    out = []
    for e in range(env.batch):
        basis, pairs, order = env.state(e)
        out.append(([(c.tolist(), x.tolist()) for c, x in basis], pairs.tolist(), order.tolist()))
    return out


def _assert_handles_equal(env, twin, steps=5):
    assert np.array_equal(env.stats(), twin.stats())
    assert np.array_equal(env.observations(OBS_ROWS), twin.observations(OBS_ROWS))
    for _ in range(steps):                                   # (auto-resets draw from the generator streams)
        a, b = env.rollout("random", 1, auto_reset=True), twin.rollout("random", 1, auto_reset=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert np.array_equal(env.observations(OBS_ROWS), twin.observations(OBS_ROWS))
    assert np.array_equal(env.stats(), twin.stats())


# ---- 1. every kernel class against the twin ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dist,caps,B", CASES)
def test_action_values_equal_copy_step_values(dist, caps, B):
    t0 = time.perf_counter()
    env = _make(dist, B, caps, k=1 if dist == "cyclic-5" else 2, walk=3 if dist == "cyclic-5" else 5)
    R = max(1, int(env.rows.max()))
    assert (env.rows > 0).all() and R > 1
    for gamma in (0.99, 0.9):
        for strategy in STRATEGIES:
            want = A.twin_action_values(env, strategy, gamma, R)
            _check_block(A.call(env, strategy, gamma, R), want, (dist, caps, strategy, gamma))
    print(dist, caps, "rows", env.rows.tolist(), "wall time %.2f s" % (time.perf_counter() - t0))


# ---- 2. against the CPU oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist,caps", [(d, c) for d, c, _ in CASES])
def test_action_values_equal_the_oracle(dist, caps):
    """Four environments, the same seeds on both sides, three common steps, then the definition on oracle.ffi.Env (copy, step,
    value) — nothing of the library in the reference."""
    from deepgroebner_amd import VecLeadMonomialsEnv
    from deepgroebner_amd.ideals import FixedIdealGenerator, cyclic
    bo = ffi.load("bo")
    B = 4
    if dist == "cyclic-5":
        env = VecLeadMonomialsEnv(FixedIdealGenerator(cyclic(5)), batch=B, k=1, caps=caps)
        orc = [bo.env(fixed=bo.cyclic(5)) for _ in range(B)]
    else:
        env = VecLeadMonomialsEnv(dist, batch=B, k=2, caps=caps)
        orc = [bo.env(dist) for _ in range(B)]
    env.seed(np.arange(B) + 900); env.reset()
    for e, o in enumerate(orc):
        o.seed(900 + e); o.reset()
    for t in range(3):
        acts = [ffi.agent_action(e, t, o.nP) if o.nP else 0 for e, o in enumerate(orc)]
        for o, a in zip(orc, acts):
            if o.nP:
                o.step(a)
        env.step(np.asarray(acts, dtype=np.int32), auto_reset=False)
    assert env.rows.tolist() == [o.nP for o in orc] and max(env.rows) > 0
    R = max(1, int(env.rows.max()))
    for strategy, gamma in (("degree", 0.99), ("first", 0.99), ("normal", 0.9)):
        wq = np.full((B, R), np.nan); wr = np.full((B, R), np.nan); wd = np.zeros((B, R), dtype=np.uint8)
        for e, o in enumerate(orc):
            q, r, d = A.oracle_action_values(o, strategy, gamma)
            wq[e, :o.nP], wr[e, :o.nP], wd[e, :o.nP] = q, r, d
        _check_block(A.call(env, strategy, gamma, R), (wq, wr, wd, env.rows), (dist, caps, strategy, gamma))


# ---- 3. generator lead-monomial ties with more than 16 basis elements -------------------------------------------------------
@pytest.mark.parametrize("name", ["fast|3-3-20-uniform", "fast_spill|3-5-18-maximum", "general|3-3-20-0.5-uniform", "listed_16_plus_one_step"])
def test_action_values_from_tied_bases(name):
    """The states of tests/value_tie_cases.py: value() must start from std::sort's reducer order, which differs from the
    environment's own above 16 elements.  The twin re-sorts the STEPPED state (values() of the stepped copy), so a resort that
    is missing, or made before the forced step, gives other doubles here; the oracle's Env says the same independently."""
    grp = V.build()[name]
    from deepgroebner_amd import VecLeadMonomialsEnv
    B = grp.batch
    env = VecLeadMonomialsEnv(grp.ctor, batch=B, k=2, caps=grp.caps, sort_input=grp.sort_input)
    if not grp.listed:
        env.seed(np.asarray(grp.seeds, dtype=np.int64))
    env.seed_agent(np.arange(B)); env.reset()
    for acts in grp.actions:
        env.step(np.asarray(acts, dtype=np.int32))
    assert env.rows.tolist() == [o.nP for o in grp.envs], name
    R = 24                                                  # (the leading actions: enough to differ, quick on the twin)
    for strategy in ("degree", "first"):
        got = A.call(env, strategy, 0.99, R)
        _check_block(got, A.twin_action_values(env, strategy, 0.99, R), (name, strategy, "twin"))
        for e in (0, B - 1):
            q, r, d = A.oracle_action_values(grp.envs[e], strategy, 0.99, limit=R)
            n = len(q)
            assert np.array_equal(got[1][e, :n], q[:n]) and np.array_equal(got[2][e, :n], r[:n]), (name, strategy, e, "oracle")


# ---- 4. padding and truncation ----------------------------------------------------------------------------------------------
def test_padding_truncation_and_finished_environments():
    B = 9
    env = _make("3-20-10-weighted", B)
    tall = int(env.rows.max())
    full = A.call(env, "degree", 0.99, tall)
    want = A.twin_action_values(env, "degree", 0.99, tall)
    _check_block(full, want, "untruncated")
    low = max(2, int(np.sort(env.rows)[B // 2]) - 1)             # below the tallest pair set, inside some environments
    assert low < tall
    for R in (low, 1):
        rc, q, r, d, rows = A.call(env, "degree", 0.99, R)
        assert rc == 0 and np.array_equal(rows, env.rows)      # the FULL counts: the cut shows
        assert A.same_block(q, full[1][:, :R]) and A.same_block(r, full[2][:, :R]) and np.array_equal(d, full[3][:, :R]), R
    rc, q, r, d, rows = A.call(env, "degree", 0.99, tall + 5)
    assert rc == 0 and np.array_equal(rows, env.rows)
    assert A.same_block(q[:, :tall], full[1]) and np.isnan(q[:, tall:]).all() and np.isnan(r[:, tall:]).all() and not d[:, tall:].any()
    # without the optional blocks
    rc, q, r, d, rows = A.call(env, "degree", 0.99, tall, rewards=False, dones=False)
    assert rc == 0 and r is None and d is None and A.same_block(q, full[1])
    # stepped without auto-reset until some environments are finished: their rows are 0 and all NaN
    for _ in range(400):
        if (env.rows == 0).any():
            break
        env.step(np.zeros(B, dtype=np.int32), auto_reset=False)
    assert (env.rows == 0).any() and (env.rows > 0).any(), env.rows
    R = int(env.rows.max())
    got = A.call(env, "first", 0.99, R)
    _check_block(got, A.twin_action_values(env, "first", 0.99, R), "some finished")
    assert np.isnan(got[1][env.rows == 0]).all()
    # the whole batch finished: BBX_OK, nothing launched, all NaN
    for _ in range(2000):
        if not env.rows.any():
            break
        env.step(np.zeros(B, dtype=np.int32), auto_reset=False)
    assert not env.rows.any()
    launched = env.kernels_launched()
    rc, q, r, d, rows = A.call(env, "degree", 0.99, 3)
    assert rc == 0 and not rows.any() and np.isnan(q).all() and np.isnan(r).all() and not d.any()
    assert env.kernels_launched() == launched


# ---- 5. passes --------------------------------------------------------------------------------------------------------------
def test_passes_of_every_size_give_the_same_block():
    from deepgroebner_amd import _ffi
    B = 7
    env = _make("3-20-10-weighted", B)
    R = int(env.rows.max())
    total = int(env.rows.sum())
    assert total > 7 and env.action_values_chunk(0) == 65536          # the default, and the setter returns the previous value
    ref = A.call(env, "degree", 0.99, R)
    assert ref[0] == 0
    for chunk in (1, 7, total, total + 100):
        before = env.action_values_chunk(chunk)
        got = A.call(env, "degree", 0.99, R)
        assert env.action_values_chunk(chunk) == chunk and before != chunk
        assert got[0] == 0 and all(np.array_equal(x, y, equal_nan=(x.dtype == np.float64)) for x, y in zip(got[1:], ref[1:])), chunk
    assert env.action_values_chunk(-1) == total + 100
    assert env.action_values_chunk(0) == 65536                        # <= 0 restored the default
    assert _ffi.lib().bbx_action_values_chunk(None, 3) == -1


# ---- 6. the handle is untouched ---------------------------------------------------------------------------------------------
def test_the_handle_is_left_as_it_was():
    B = 8
    env = _make("3-20-10-weighted", B)
    twin = env.copy()
    state0, rows0, stats0, caps0 = _state_of(env), env.rows.copy(), env.stats(), env.capacities()
    R = int(env.rows.max())
    alone = A.call(env, "degree", 0.99, R)
    assert alone[0] == 0
    assert _state_of(env) == state0 and np.array_equal(env.rows, rows0) and np.array_equal(env.stats(), stats0)
    assert env.capacities() == caps0                               # (no growth happened: default capacities)
    _assert_handles_equal(env, twin, steps=5)


def test_behind_a_queued_values_device_call_both_return_what_they_return_alone():
    import torch
    B = 8
    env = _make("3-20-10-weighted", B)
    twin = env.copy()
    R = int(env.rows.max())
    want_v = twin.values("normal", 0.99)
    want_q = A.call(twin, "degree", 0.99, R)
    out = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
    env.values_device(out, "normal", 0.99, None, stream())      # queued, not yet synced
    got = A.call(env, "degree", 0.99, R)
    env.sync()
    assert np.array_equal(out.cpu().numpy(), want_v)
    assert got[0] == 0 and all(np.array_equal(x, y, equal_nan=(x.dtype == np.float64)) for x, y in zip(got[1:], want_q[1:]))
    _assert_handles_equal(env, twin, steps=5)


def test_inside_a_host_stepped_loop_with_a_mailbox_session():
    """step x5 (a loop of host steps on a small lean batch: a mailbox session is active), action_values, step, reset — against
    a twin that made no action_values call."""
    B = 4
    env = _make("3-20-10-weighted", B, walk=0)
    env.accounting(False)
    twin = env.copy()

    def step(v, t):
        a = (t % np.maximum(v.rows, 1)).astype(np.int32)
        obs, r, d, _ = v.step(a, auto_reset=True)
        return obs, r, d, v.rows.copy()
    for t in range(5):
        x, y = step(env, t), step(twin, t)
        assert all(np.array_equal(p, q) for p, q in zip(x[0], y[0])) and all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:]))
    R = int(env.rows.max())
    got = A.call(env, "degree", 0.99, R)
    _check_block(got, A.twin_action_values(twin.copy(), "degree", 0.99, R), "in the loop")
    x, y = step(env, 5), step(twin, 5)
    assert all(np.array_equal(p, q) for p, q in zip(x[0], y[0])) and all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:]))
    a, b = env.reset(), twin.reset()
    assert np.array_equal(env.rows, twin.rows) and all(np.array_equal(p, q) for p, q in zip(a, b))
    assert np.array_equal(env.stats(), twin.stats())


# ---- 7. growth --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("caps", [{"max_basis": 12, "max_pairs": 16}, {"max_basis": 12, "max_pairs": 16, "lds_max_basis": -1}])
def test_clones_that_outgrow_the_records_enlarge_them(caps):
    """The capacities of tests/test_values_device.py's growth test: value rollouts from these states outgrow them."""
    B = 9
    env = _make("3-20-10-weighted", B, caps, seed=500, walk=0)
    ref = _make("3-20-10-weighted", B, dict(caps, max_basis=0, max_pairs=0), seed=500, walk=0)   # (0: the default capacities)
    twin = env.copy()
    before = env.capacities()
    assert ref.capacities()["max_basis"] > before["max_basis"] and np.array_equal(ref.rows, env.rows)
    R = int(env.rows.max())
    want = A.call(ref, "degree", 0.99, R)
    assert want[0] == 0 and ref.capacities()["grown"] == 0
    got = A.call(env, "degree", 0.99, R)
    after = env.capacities()
    print("capacities", before, "->", after)
    assert after["grown"] > before["grown"] and after["max_basis"] > before["max_basis"]
    assert got[0] == 0 and all(np.array_equal(x, y, equal_nan=(x.dtype == np.float64)) for x, y in zip(got[1:], want[1:]))
    again = A.call(env, "normal", 0.99, R)                      # (the clone arrays follow the new layout)
    _check_block(again, A.twin_action_values(ref, "normal", 0.99, R), "after growth")
    _assert_handles_equal(env, twin, steps=3)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    from deepgroebner_amd import _ffi
    env = _make("3-20-10-weighted", 3)
    for strategy in ("random", "sample"):
        rc = A.call(env, strategy, 0.99, 4)[0]
        assert rc == -5 and strategy in _ffi.lib().bbx_last_error().decode()
        with pytest.raises(_ffi.BbxError) as ei:
            env.action_values(strategy)
        assert ei.value.code == -5
    assert A.call(env, "degree", 0.99, 0)[0] == -1
    assert A.call(env, "degree", 0.99, -4)[0] == -1
    q = np.zeros((3, 4)); rows = np.zeros(3, dtype=np.int32)
    L = _ffi.lib()
    assert L.bbx_action_values(None, b"degree", 0.99, 4, _ffi.ptr(q), None, None, _ffi.ptr(rows)) == -1
    assert L.bbx_action_values(env._h, None, 0.99, 4, _ffi.ptr(q), None, None, _ffi.ptr(rows)) == -1
    assert L.bbx_action_values(env._h, b"degree", 0.99, 4, None, None, None, _ffi.ptr(rows)) == -1
    assert L.bbx_action_values(env._h, b"degree", 0.99, 4, _ffi.ptr(q), None, None, None) == -1


# ---- 9. the Python surface --------------------------------------------------------------------------------------------------
def test_python_surface_single_environment_and_vector():
    from deepgroebner_amd import BuchbergerEnv, CLeadMonomialsEnv, LeadMonomialsEnv, LookaheadAgent
    c = CLeadMonomialsEnv("3-20-10-weighted", k=2)
    c.seed(70); state = c.reset()
    for _ in range(3):
        state, _, done, _ = c.step(0)
        assert not done
    for strategy in ("degree", "first"):
        v = c.action_values(strategy, 0.99)
        rc, q, _, _, rows = A.call(c._vec, strategy, 0.99, len(state))
        assert rc == 0 and rows[0] == len(state) == len(v) and np.array_equal(v, q[0])
    assert LookaheadAgent("degree", 0.99).act(c) == int(np.argmax(c.action_values("degree", 0.99)))
    p = LeadMonomialsEnv("3-20-10-weighted", k=2)
    p.seed(70); n = len(p.reset())
    assert len(p.action_values(0.99)) == n and np.array_equal(p.action_values(0.99), p._vec.action_values("degree", 0.99)[0, :n])
    b = BuchbergerEnv("3-20-10-weighted")
    b.seed(70); _, P = b.reset()
    qb = b.action_values(0.99)
    assert len(qb) == len(P) and LookaheadAgent().act(b) == P[int(np.argmax(qb))]
    # the vector form: q alone, with_steps, a given max_rows, and self.rows untouched
    env = _make("3-20-10-weighted", 6)
    rows0 = env.rows.copy()
    R = int(rows0.max())
    want = A.twin_action_values(env, "degree", 0.99, R)
    q = env.action_values()
    q2, r2, d2 = env.action_values("degree", 0.99, with_steps=True)
    assert q.shape == (6, R) and q.dtype == np.float64 and A.same_block(q, want[0]) and A.same_block(q2, want[0])
    assert A.same_block(r2, want[1]) and d2.dtype == bool and np.array_equal(d2, want[2].astype(bool))
    assert env.action_values(max_rows=R + 3).shape == (6, R + 3) and env.action_values(max_rows=2).shape == (6, 2)
    assert np.array_equal(env.rows, rows0)
    # the agent: the first index of the maximum over the numbers of the twin block
    first_max = [int(np.flatnonzero(row == np.nanmax(row))[0]) for row in want[0]]
    act = LookaheadAgent("degree", 0.99).act(env)
    assert act.dtype == np.int32 and act.tolist() == first_max


def test_lookahead_agent_drives_a_batch_to_the_end():
    from deepgroebner_amd import LookaheadAgent
    from deepgroebner_amd.buchberger import best_actions
    B = 4
    env = _make("3-20-10-weighted", B, walk=0)
    agent = LookaheadAgent("degree", 0.99)
    ret, picked, steps = np.zeros(B), np.zeros(B), 0
    while env.rows.any():
        live = env.rows > 0
        q, rew, _ = env.action_values("degree", 0.99, with_steps=True)
        a = agent.act(env)
        assert np.array_equal(a, best_actions(q)) and not a[~live].any()
        picked[live] += rew[live, a[live]]
        _, r, d, _ = env.step(a, auto_reset=False)
        ret[live] += r[live]
        steps += 1
        assert steps < 2000                                  # (an episode of this distribution has a few hundred steps at the most)
    print("lookahead episodes:", steps, "steps, returns", ret.tolist())
    assert d.all() and np.array_equal(ret, picked) and (ret < 0).all()
