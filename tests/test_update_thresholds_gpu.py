"""The shared Gebauer-Moeller update (wave_update, csrc/bbx_device.h) and the write-through LDS copy in front of it (BEnvC,
csrc/bbx_binom.h) at the index thresholds inside them, and the update at the 16-bit degree limit.

A. Thresholds.  Binomial distributions with hundreds or thousands of generators put an environment next to a threshold at
   its reset and carry it across within a few dozen steps:
     480 lead / tail monomials and 512 pair words are what the copy of the 16-byte binomial class holds (BC_G, BC_P),
     2048 elements is the most its on-chip peel handles (one flag bit per 64 elements in a 32-bit mask),
     512 elements is where the other classes' peel leaves the per-wave LDS scratch for the record's arrays.
   Every case states its point as an assertion on the ORACLE's trajectory (tests/test_update_thresholds_cpu.py asserts the
   same without a device).  Each runs as one traced launch, as traced launches of 7 steps — the later ones then begin in
   the middle of an episode beyond the caps: the copy is loaded from a record larger than itself — and on the lean
   production kernels through device buffers.  Every comparison is exact: per step action, reward, |P|, |G| and the hashes
   of observation, pair set and new element; then the complete final state.

B. Degree limit.  Lead monomials within the limits whose lcm is not (tests/alg_cases.py: degree_limit_ideals): the pair
   set equals the reference's as long as no SELECTED pair passes the limit, on the wide and general classes; selecting a
   pair beyond it is BBX_ST_DEG_OVERFLOW and changes nothing."""
import functools

import numpy as np
import pytest

from oracle import ffi
from oracle.trace import run_trace
from tests import alg_cases as ac

BC_G, BC_P, PEEL_CACHED, PEEL_LDS = 480, 512, 2048, 512      # csrc/bbx_binom.h, csrc/bbx_device.h
SEEDS = (0, 1)
K = 2
KEYS = (("action", "action"), ("reward", "reward"), ("rows", "nP"), ("basis_size", "nG"), ("obs_hash", "obs_hash"),
        ("pairs_hash", "pairs_hash"), ("newpoly_hash", "newpoly_hash"))
HBM = {"lds_max_basis": -1}
GENERAL = {"general_class": 1, "lds_max_basis": -1}

# name -> (distribution, steps, caps, options, the point: a predicate of (|G| per state, |P| per state), reset state first)
CASES = {
    "copy-480-inside": ("4-8-470-uniform", 40, None, {}, lambda g, p: g[0] <= BC_G < g.max() and p[0] > BC_P > p.min()),
    "copy-480-at-reset": ("4-8-490-uniform", 30, None, {}, lambda g, p: g[0] > BC_G and p.min() > BC_P),
    "copy-512-pairs": ("4-8-459-uniform", 30, None, {}, lambda g, p: p[0] < BC_P < p.max() and p.min() < p[0] and g.max() <= BC_G),
    "copy-2048-peel": ("4-8-2044-uniform", 30, None, {}, lambda g, p: g[0] <= PEEL_CACHED < g[-1]),
    "hbm-8-byte-512": ("3-20-510-weighted", 30, HBM, {}, lambda g, p: g[0] <= PEEL_LDS < g.max()),
    "general-512": ("3-20-510-weighted", 30, GENERAL, {}, lambda g, p: g[0] <= PEEL_LDS < g.max()),
    "hbm-32-byte-512": ("8-3-505-uniform", 30, None, {}, lambda g, p: g[0] <= PEEL_LDS < g.max()),
    # sorted input: more than 16 generators come sorted from the host queue, the installs differ from the unsorted ones
    "copy-480-inside-sorted": ("4-8-478-uniform", 40, None, {"sort_input": True}, lambda g, p: g[0] <= BC_G < g.max() and p.max() > BC_P > p.min()),
    "copy-480-at-reset-sorted": ("4-8-490-uniform", 30, None, {"sort_input": True}, lambda g, p: g[0] > BC_G and p.max() > BC_P),
    # the copy where no peel runs (without Gebauer-Moeller 490 generators have some 115 000 pairs)
    "copy-480-at-reset-lcm": ("4-8-490-uniform", 12, None, {"elimination": "lcm"}, lambda g, p: g[0] > BC_G and p.min() > BC_P),
}
PLAIN = [n for n, c in CASES.items() if not c[3]]


@functools.lru_cache(maxsize=None)
def oracle_traces(name):
    """The oracle's trajectory of every environment of the case — computed once, shared by the three ways of running it."""
    dist, T, _, opts, _ = CASES[name]
    bo = ffi.load("bo")
    out = []
    for s in SEEDS:
        o = bo.env(dist, **opts)
        o.seed(s)
        out.append(run_trace(o, K, T, "hash", agent_seed=s))
    return out


def sizes(w):
    return np.concatenate([[w["init"][0]], w["nG"]]), np.concatenate([[w["init"][1]], w["nP"]])


def assert_point(name):
    for s, w in zip(SEEDS, oracle_traces(name)):
        g, p = sizes(w)
        assert not (w["nG"][1:] < w["nG"][:-1]).any(), (name, s, "an episode ended inside the rollout")
        assert CASES[name][4](g, p), (name, s, "the oracle no longer crosses the threshold: |G| %d..%d (reset %d, end %d), |P| %d..%d (reset %d)"
                                      % (g.min(), g.max(), g[0], g[-1], p.min(), p.max(), p[0]))


def final_words(w):
    return np.concatenate([w["final_basis"], w["final_pairs"].ravel(), w["final_order"]])


def make_env(name):
    from deepgroebner_amd import VecLeadMonomialsEnv
    dist, T, caps, opts, _ = CASES[name]
    env = VecLeadMonomialsEnv(dist, batch=len(SEEDS), k=K, caps=caps, **opts)
    env.seed(np.array(SEEDS)); env.seed_agent(np.array(SEEDS))
    return env, T


def check_traced(name, chunk):
    from tests.test_gpu_parity import _state_words
    assert_point(name)
    env, T = make_env(name)
    chunk = chunk or T
    env.trace_enable(chunk)
    env.reset()
    got = [[] for _ in SEEDS]
    for t0 in range(0, T, chunk):                            # (every launch writes its trace from slot 0)
        n = min(chunk, T - t0)
        env.rollout("random", n, auto_reset=True)
        for e in range(len(SEEDS)):
            got[e].append(env.trace_read(e, 0, n))
    for e, want in enumerate(oracle_traces(name)):
        g = np.concatenate(got[e])
        for key, wkey in KEYS:
            same = g[key] == want[wkey]
            assert same.all(), (name, chunk, "environment", e, key, "first difference at step", int(np.flatnonzero(~same)[0]))
        assert np.array_equal(_state_words(*env.state(e)), final_words(want)), (name, chunk, e, "final state")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_traced_launch(name):
    check_traced(name, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_traced_launches_of_7_steps_begin_beyond_the_caps(name):
    check_traced(name, 7)


@functools.lru_cache(maxsize=None)
def oracle_runs(name):
    dist, T, _, _, _ = CASES[name]
    return ffi.load("bo").run_random_many(dist, K, SEEDS, SEEDS, T, True, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PLAIN))
def test_lean_kernels_through_device_buffers(name):
    """The production variant (no accounting, no tracing) in launches of 10 steps on device buffers, the observation block
    written at every step: counters and complete final states of all environments, and the block the last step left."""
    import torch
    from tests.test_gpu_parity import _assert_equals_oracle_run
    assert_point(name)
    want = oracle_runs(name)
    for w, tr in zip(want, oracle_traces(name)):             # (the two oracle entry points describe the same run)
        assert (w["nG"], w["nP"]) == (int(tr["nG"][-1]), int(tr["nP"][-1]))
    env, T = make_env(name)
    env.reset()
    env.accounting(False)
    B, R = len(SEEDS), 2304
    assert R > max(int(sizes(tr)[1].max()) for tr in oracle_traces(name))
    d_obs = torch.empty((B, R, env.cols), dtype=torch.int32, device="cuda")
    d_rew = torch.empty(B, dtype=torch.float64, device="cuda"); d_done = torch.empty(B, dtype=torch.uint8, device="cuda")
    d_rows = torch.empty(B, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert T % 10 == 0
    for _ in range(T // 10):
        env.rollout_device("random", 10, True, stream, d_rew, d_done, d_rows, d_obs, R, False, True)
    env.sync(); torch.cuda.synchronize()
    _assert_equals_oracle_run(env, want)
    rows = d_rows.cpu().numpy()
    assert np.array_equal(rows, [w["nP"] for w in want])
    host = env.observations(max_rows=R, fill=False)
    got = d_obs.cpu().numpy()
    for e in range(B):
        assert np.array_equal(got[e, :rows[e]], host[e, :rows[e]]), e


# ---- B. the degree limit -----------------------------------------------------------------------------------------------------

CLASSES = {"wide": None, "wide-3-waves": {"wide_waves": 3}, "general": {"wide_waves": -1}}
ST_DEG_OVERFLOW = 5                                          # BBX_ST_DEG_OVERFLOW, csrc/bbx_common.h


def pairs_of(env, e):
    return [tuple(int(x) for x in p) for p in env.state(e)[1]]


@pytest.mark.gpu
@pytest.mark.parametrize("agent", ["first", "random"])
@pytest.mark.parametrize("cls", sorted(CLASSES))
@pytest.mark.parametrize("nv", [3, 4, 8])
def test_pair_sets_with_lcms_beyond_the_degree_limit(nv, cls, agent):
    """The pair list after reset() and after each of 6 steps equals the reference's: (0, 2), whose lcm has degree 70 000
    (66 100), leaves at the reset because lcm(1, 2) divides it, and later elements keep meeting lcms beyond the limit.  No
    selected pair's sugar passes the limit (asserted on the oracle), so no step may be refused.  At the end the complete
    state."""
    from deepgroebner_amd import VecLeadMonomialsEnv
    from deepgroebner_amd.ideals import FixedIdealGenerator
    from tests.test_gpu_parity import _state_words
    bo = ffi.load("bo")
    _, F = ac.degree_limit_ideals()[nv]
    B = 3
    env = VecLeadMonomialsEnv(FixedIdealGenerator(F), batch=B, k=K, caps=CLASSES[cls])
    env.seed_agent(np.arange(B) + 11); env.reset()
    oracles = []
    for e in range(B):
        o = bo.env(fixed=F); o.reset(); oracles.append(o)
        assert pairs_of(env, e) == [(0, 1), (1, 2)] == [tuple(p) for p in o.pairs().tolist()], ("reset", e, pairs_of(env, e))
    for t in range(6):
        rew, done, rows = env.rollout(agent, 1, auto_reset=False)
        for e, o in enumerate(oracles):
            assert o.nP > 0
            a = 0 if agent == "first" else ffi.agent_action(11 + e, t, o.nP)
            i, j = o.pairs()[a]
            assert ac.pair_sugar(o, i, j) <= 65535, (t, e)
            r = o.step(a)
            assert rew[e] == r and rows[e] == o.nP, (t, e, rew[e], r, rows[e], o.nP)
            assert pairs_of(env, e) == [tuple(p) for p in o.pairs().tolist()], (t, e, pairs_of(env, e))
    for e, o in enumerate(oracles):
        assert np.array_equal(_state_words(*env.state(e)), _state_words(o.basis(), o.pairs(), o.reducer_order())), e
    assert (env.stats()[:, 4] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_selecting_a_pair_beyond_the_degree_limit_is_refused_and_changes_nothing(cls):
    """[x^40000 z + 1, y^40000 z + 1]: the reset succeeds (one pair, lcm of degree 80 001); taking it is refused with
    BBX_ST_DEG_OVERFLOW — the environments' status, the error's text —, states and counters are what they were, and the
    handle goes on answering."""
    from deepgroebner_amd import VecLeadMonomialsEnv, _ffi
    from deepgroebner_amd.ideals import FixedIdealGenerator
    from tests.test_gpu_parity import _state_words
    bo = ffi.load("bo")
    F = ac.hard_limit_ideal()
    B = 3
    env = VecLeadMonomialsEnv(FixedIdealGenerator(F), batch=B, k=K, caps=CLASSES[cls])
    env.reset()
    o = bo.env(fixed=F); o.reset()
    want = _state_words(o.basis(), o.pairs(), o.reducer_order())
    before = env.stats()
    assert (before[:, 4] == 0).all() and (before[:, 0] == 0).all() and (before[:, 7] == 2).all()
    for e in range(B):
        assert pairs_of(env, e) == [(0, 1)] and np.array_equal(_state_words(*env.state(e)), want)
    with pytest.raises(_ffi.BbxError) as ei:
        env.rollout("first", 1, auto_reset=False)
    assert ei.value.code == -3 and "degree above 65535" in str(ei.value), str(ei.value)
    for _ in range(2):                                       # (and again: the handle still answers)
        after = env.stats()
        assert (after[:, 4] == ST_DEG_OVERFLOW).all(), after[:, 4]
        assert np.array_equal(np.delete(after, 4, axis=1), np.delete(before, 4, axis=1))
        for e in range(B):
            assert np.array_equal(_state_words(*env.state(e)), want), e
