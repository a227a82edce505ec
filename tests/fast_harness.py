"""What the GPU twins of the fast-class tests (tests/test_X_gpu.py) share: the batch they run, the comparison of a batch's
state with the oracle's, the device buffers of a rollout, and the test bodies every twin repeats on its own seeds — traced
rollout, lean rollout, value rollouts, one-layer policy rollout.  tests/test_X_cpu.py proves that the seeds reach the events
X is about (through tests/oracle_walk.py); a twin hands its seeds and its walk to the bodies here.  torch is imported inside
the functions, as in the tests: importing this module needs no device.

A `walk` below is the CPU twin's cached walk(seed, aseed): a tuple that begins (oracle environment after T steps, per-step
rewards, per-step done flags)."""
import ctypes as C

import numpy as np

from oracle import ffi
from oracle.trace import poly_words, run_trace
from tests import oracle_walk as ow

KEYS = (("action", "action"), ("reward", "reward"), ("rows", "nP"), ("basis_size", "nG"), ("done", "done"), ("obs_hash", "obs_hash"),
        ("pairs_hash", "pairs_hash"), ("newpoly_hash", "newpoly_hash"))
KERNELS = ("headline", "headline-session", "generic")       # the lean kernels of a rollout_device call, see check_lean_rollout


def make_env(dist, seeds, k, caps=None, trace=0, lean=False, agent=None, persistent=None, **kw):
    """A batch of `dist` over seeds = [(ideal seed, agent seed)] (or ideal seeds, with agent = their agent seeds): seed,
    seed_agent, trace_enable(trace) if trace, reset, accounting(False) if lean — lean="before reset" switches accounting off
    in front of trace_enable and reset, the order tests/test_episode_limit_gpu.py runs — and persistent(persistent) where it
    is given.  kw goes to the constructor (max_episode_length)."""
    from deepgroebner_amd import VecLeadMonomialsEnv
    if agent is None:
        seeds, agent = [s for s, _ in seeds], [a for _, a in seeds]
    env = VecLeadMonomialsEnv(dist, batch=len(seeds), k=k, caps=caps, **kw)
    env.seed(np.array(seeds))
    env.seed_agent(np.array(agent))
    if lean == "before reset":
        env.accounting(False)
    if trace:
        env.trace_enable(trace)
    env.reset()
    if lean is True:
        env.accounting(False)
    if persistent is not None:
        env.persistent(persistent)
    return env


# ---- comparisons ---------------------------------------------------------------------------------------------------------------
def assert_same_state(env, e, o, where):
    """Environment e of the batch against the oracle environment o (or an oracle_walk.Snapshot of one): basis length, basis
    term for term, pair list, reducer order."""
    want = o if isinstance(o, ow.Snapshot) else ow.snapshot(o)
    basis, pairs, order = env.state(e)
    assert len(basis) == want.nG, (where, e)
    got = np.concatenate([poly_words(c, x) for c, x in basis])
    assert np.array_equal(got, want.words), (where, e, "basis")
    assert np.array_equal(pairs, want.pairs), (where, e, "pairs")
    assert np.array_equal(order, want.order), (where, e, "reducer order")


def assert_same_states(env, seeds, walk, where):
    """environment e runs seeds[e]: each against the state walk(*seeds[e])[0]"""
    for e, sa in enumerate(seeds):
        assert_same_state(env, e, walk(*sa)[0], where)


def assert_trace_equal(got, want, keys, where, t0=0, n=None):
    """The fields `keys` of a trace_read block against steps t0 .. t0 + n of an oracle.trace.run_trace record."""
    where = where if isinstance(where, tuple) else (where,)
    for key, wkey in keys:
        w = np.asarray(want[wkey])[t0:None if n is None else t0 + n]
        g = got[key].astype(w.dtype)
        assert np.array_equal(g, w), where + (key, "first difference at step", t0 + int(np.flatnonzero(g != w)[0]))


def same_doubles(a, b):
    """== on doubles, NaN nowhere."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and not np.isnan(a).any() and bool(np.array_equal(a, b))


def assert_same_outputs(bufs, seeds, walk, k):
    """what the last launch left in rollout_buffers — reward, done flag, row count, observation rows — against the walks"""
    rew, done, rows, obs = (x.cpu().numpy() for x in bufs)
    for e, sa in enumerate(seeds):
        o, rewards, dones = walk(*sa)[:3]
        assert rew[e] == rewards[-1] and bool(done[e]) == bool(dones[-1]) and rows[e] == o.nP, e
        assert np.array_equal(obs[e, :o.nP], o.obs(k)), e


# ---- device plumbing -----------------------------------------------------------------------------------------------------------
def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def stream_ptr():
    return C.c_void_p(stream())


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def to_cuda(*arrays):
    """device copies of numpy arrays (None stays None)"""
    import torch
    return [None if a is None else torch.from_numpy(np.array(a, order="C")).cuda() for a in arrays]


def rollout_buffers(n, rows, cols, fill=-1, blocks=None):
    """(rewards, dones, row counts, observation blocks) of a rollout_device call over n environments: `blocks` (n unless
    given) blocks of rows x cols words holding `fill`."""
    import torch
    return (torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"),
            torch.zeros(n, dtype=torch.int32, device="cuda"),
            torch.full((n if blocks is None else blocks, rows, cols), fill, dtype=torch.int32, device="cuda"))


def policy_rollout(env, hidden, wseed, nT, useed, rows, fill=-1):
    """bbx_policy_rollout_device over nT steps with a one-layer policy of `hidden` units made from wseed (policy_cases) and
    uniforms drawn from useed: the weights, the policy, and a dict of the call's tensors — u, and per (step, environment)
    acts, logp, rews, dones, rows and the observation block (`rows` rows holding `fill` where nothing was written)."""
    import torch
    from tests import policy_cases as pc
    B = env.batch
    w = pc.make_weights(env.cols, (hidden,), wseed)
    pol = pc.to_policy(w, "cuda")
    p = pol._fused_weights()
    u = torch.rand((nT, B), device="cuda", generator=torch.Generator(device="cuda").manual_seed(useed))
    A = torch.zeros((nT, B), dtype=torch.int32, device="cuda"); L = torch.zeros((nT, B), dtype=torch.float32, device="cuda")
    Rw = torch.zeros((nT, B), dtype=torch.float64, device="cuda"); D = torch.zeros((nT, B), dtype=torch.uint8, device="cuda")
    N = torch.zeros((nT, B), dtype=torch.int32, device="cuda")
    O = torch.full((nT, B, rows, env.cols), fill, dtype=torch.int32, device="cuda")
    env.policy_rollout_device(p["prepared"], p["hidden"], nT, u, A, L, Rw, D, N, O, rows, B * rows * env.cols, stream())
    env.sync(); torch.cuda.synchronize()
    assert env.stats()[:, 4].max() == 0
    return w, pol, {"u": u, "acts": A, "logp": L, "rews": Rw, "dones": D, "rows": N, "obs": O}


def replay_policy_rollout(dist, seeds, k, acts, rews, dones, obs, rows, start=None):
    """The actions a policy rollout drew (numpy arrays per (step, environment), as policy_rollout names them) replayed on
    the oracle with auto-reset, from start[e] (an oracle environment; the reset state of seeds[e]'s ideal seed without):
    row count, observation rows, action range, reward and done flag of every (e, t).  Returns the oracle environments as
    they stand afterwards and the number of steps that inserted an element."""
    finals, inserted = [], 0
    for e, (seed, _) in enumerate(seeds):
        o = ow.fresh(dist, seed) if start is None else start[e]
        for t in range(len(acts)):
            assert rows[t, e] == o.nP and np.array_equal(obs[t, e, :o.nP], o.obs(k)), (e, t)
            assert 0 <= acts[t, e] < o.nP, (e, t)
            nG = o.nG
            r = o.step(int(acts[t, e]))
            inserted += int(o.nG == nG + 1)
            assert rews[t, e] == r and bool(dones[t, e]) == (o.nP == 0), (e, t)
            if o.nP == 0:
                o.reset()
        finals.append(o)
    return finals, inserted


# ---- the bodies the twins share ------------------------------------------------------------------------------------------------
def check_traced_rollout(dist, seeds, k, T, walk, caps=None):
    """T steps as ONE launch of the traced kernel: every trace field of every step against oracle.trace.run_trace, what the
    launch returns, the state (basis, pairs, reducer order) and the observation afterwards."""
    env = make_env(dist, seeds, k, caps=caps, trace=T)
    rew, done, rows = env.rollout("random", T, auto_reset=True)
    bo = ffi.load("bo")
    for e, (s, a) in enumerate(seeds):
        o = bo.env(dist)
        o.seed(s)
        want = run_trace(o, k, T, "hash", agent_seed=a)
        assert_trace_equal(env.trace_read(e, 0, T), want, KEYS, e)
        assert rew[e] == want["reward"][-1] and bool(done[e]) == bool(want["done"][-1]) and rows[e] == walk(s, a)[0].nP, e
    assert_same_states(env, seeds, walk, "traced")
    obs = env.observations()
    for e, sa in enumerate(seeds):
        assert np.array_equal(obs[e], walk(*sa)[0].obs(k)), e
    return env


def check_lean_rollout(kernel, launches, dist, seeds, k, walk, caps=None, rows=256):
    """The lean headline shape (hash agent, the observation written after every step, no fill) as the launches given —
    kernel "headline": one kernel per call; "headline-session": one persistent session; "generic": with obs_fill on, where
    the launcher takes the generic lean kernel.  Counters, state, outputs and (generic) the -1 fill behind the live rows."""
    B, T = len(seeds), sum(launches)
    env = make_env(dist, seeds, k, caps=caps, lean=True, persistent=kernel == "headline-session")
    bufs = rollout_buffers(B, rows, env.cols)
    for n in launches:
        env.rollout_device("random", n, True, stream(), *bufs, rows, kernel == "generic", True)
    env.sync()
    if kernel == "headline-session":
        assert env.session_stats()["sessions"] >= 1, env.session_stats()
    st = env.stats()
    assert (st[:, 0] == T).all() and (st[:, 4] == 0).all(), st
    assert_same_states(env, seeds, walk, (kernel, caps))
    assert_same_outputs(bufs, seeds, walk, k)
    for e, sa in enumerate(seeds):
        rewards, dones = walk(*sa)[1:3]
        # additions (1 + reductions per step) and episodes over the whole run
        assert st[e, 1] == int(np.sum(-rewards)) and st[e, 2] == int(dones.sum()), (e, st[e])
    if kernel == "generic":                                  # (the fill: -1 behind the live rows)
        got, nrows = bufs[3].cpu().numpy(), bufs[2].cpu().numpy()
        assert all((got[e, nrows[e]:] == -1).all() for e in range(B))
    return env


def check_state_after_every_launch(kernel, launch, dist, seeds, k, T, states, final, rows=256):
    """The lean run of check_lean_rollout cut into launches of `launch` steps: after EVERY launch the state of every
    environment against states(seed, aseed)[i], the oracle's after launch i; at the end the counters, and row count and
    observation against final(seed, aseed), the oracle environment after T steps."""
    B = len(seeds)
    env = make_env(dist, seeds, k, lean=True, persistent=kernel == "headline-session")
    bufs = rollout_buffers(B, rows, env.cols)
    for i in range(T // launch):
        env.rollout_device("random", launch, True, stream(), *bufs, rows, kernel == "generic", True)
        env.sync()
        for e, sa in enumerate(seeds):
            assert_same_state(env, e, states(*sa)[i], (kernel, "after step", (i + 1) * launch))
    st = env.stats()
    assert (st[:, 0] == T).all() and (st[:, 4] == 0).all(), st
    got_rows, got_obs = bufs[2].cpu().numpy(), bufs[3].cpu().numpy()
    for e, sa in enumerate(seeds):
        o = final(*sa)
        assert got_rows[e] == o.nP and np.array_equal(got_obs[e, :o.nP], o.obs(k)), e
    return env


def check_values_after_rollout(dist, seeds, k, stops, oracle_at, caps=None, strategies=("degree", "first"), gamma=0.99):
    """value() rollouts (the class's value kernel: to the end of the episode under a fixed strategy, on clones) from the
    state after each of `stops` hash-agent steps, ascending — 0: the reset state — against the oracle's value() from
    oracle_at(seed, aseed, stop), the oracle environment `stop` > 0 steps in.  The batch itself is where the oracle is at
    the last stop: its state is compared at the end."""
    env = make_env(dist, seeds, k, caps=caps)
    at = 0
    for stop in stops:
        if stop > at:
            env.rollout("random", stop - at, auto_reset=True)
            at = stop
        for strategy in strategies:
            got = env.values(strategy, gamma)
            for e, (s, a) in enumerate(seeds):
                o = oracle_at(s, a, stop) if stop else ow.fresh(dist, s)
                assert got[e] == o.value(strategy, gamma), (stop, strategy, e)
    for e, (s, a) in enumerate(seeds):
        assert_same_state(env, e, oracle_at(s, a, at), ("valued", caps))
    return env


def check_policy_rollout_one_layer(dist, seeds, k, nT, wseed, useed, start=0, start_oracle=None, rows=256):
    """bbx_policy_rollout_device with a one-layer policy of 64 hidden units, nT steps from the state `start` hash-agent steps
    in (start_oracle(seed, aseed): the oracle there): the environments — replayed on the oracle with the actions the kernel
    drew — step for step (row count, observation, action range, reward, done flag), and the state afterwards: basis, pair
    list, reducer order.  Returns the number of replayed steps that inserted an element."""
    env = make_env(dist, seeds, k, lean=True)
    if start:
        env.rollout("random", start, auto_reset=True)
    out = {key: x.cpu().numpy() for key, x in policy_rollout(env, 64, wseed, nT, useed, rows)[2].items()}
    finals, inserted = replay_policy_rollout(dist, seeds, k, out["acts"], out["rews"], out["dones"], out["obs"], out["rows"],
                                             [start_oracle(*sa).copy() for sa in seeds] if start else None)
    for e, o in enumerate(finals):
        assert_same_state(env, e, o, ("policy rollout", start))
    return inserted
