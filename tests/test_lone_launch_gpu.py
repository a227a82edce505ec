"""A persistent session that is ONE launch (rollout_device, join, sync — what a plain bench.py run times), or a few: its
initial control value is written on the session stream in front of the first kernel, the closing kernels are ordered behind
the stop once, and a closing wave whose environment owes nothing leaves before it stages anything (fast_body).
None of it may be visible except in time: outputs, counters and every environment's state equal, bit for bit, those of the
same calls made one kernel per launch."""

import numpy as np
import pytest

from tests.fast_harness import make_env

pytestmark = pytest.mark.gpu
DIST = "3-20-10-weighted"
R = 256
BATCHES = (64, 256, 1100)                                    # 1100: no multiple of the grid's quarters of 1024 environments
STEPS = (1, 2, 20, 63, 64, 65, 130)                          # around the 64-step block of the loop's housekeeping


def _env(dist, B, persistent, caps=None):
    return make_env(dist, np.arange(B) + 1000, 2, caps=caps, lean=True, agent=np.arange(B), persistent=persistent)


def _bufs(env, B, fill=0):
    import torch
    return (torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda"),
            torch.zeros(B, dtype=torch.int32, device="cuda"), torch.full((B, R, env.cols), fill, dtype=torch.int32, device="cuda"))


def _everything(env, bufs, capped=False):
    """What a caller can see of the batch: the outputs (of the observation block the live rows), the counters and status of
    every environment, and every environment's basis, pair list and reducer order as bbx_state_get hands them out.  capped: a
    class that environments leave — without the algorithmic-byte column, which the HBM-resident pass counts for the steps it
    takes and which depends on where an environment left (tests/test_sessions.py leaves it out likewise)."""
    import torch
    from deepgroebner_amd import _ffi
    rew, done, rows, obs = bufs
    live = (torch.arange(R, device="cuda")[None, :] < rows[:, None]).cpu().numpy()
    status = np.zeros(env.batch, dtype=np.int32)
    _ffi.check(_ffi.lib().bbx_env_status(env._h, _ffi.ptr(status)))
    out = {"rewards": rew.cpu().numpy(), "dones": done.cpu().numpy(), "rows": rows.cpu().numpy(), "obs": obs.cpu().numpy()[live],
           "stats": np.delete(env.stats(), 6, axis=1) if capped else env.stats(), "status": status}
    words = []
    for e in range(env.batch):
        basis, pairs, order = env.state(e)
        words.append(np.concatenate([np.array([len(basis), len(pairs)], dtype=np.int32)] + [np.concatenate([c, x.ravel()]) for c, x in basis]
                                    + [pairs.ravel(), order]).astype(np.int32).tobytes())
    out["state"] = words
    return out


def _same(a, b, where):
    for key in a:
        if key == "state":
            diff = [e for e, (x, y) in enumerate(zip(a[key], b[key])) if x != y]
            assert not diff, where + ("state of environments", diff[:8])
        else:
            x, y = np.asarray(a[key]), np.asarray(b[key])
            assert x.shape == y.shape, where + (key, x.shape, y.shape)
            assert np.array_equal(x, y), where + (key, "first differences at", np.argwhere(x != y)[:4].tolist())


def _run(B, calls, persistent, settle_before_join=False):
    """The calls on one batch, then join and sync.  settle_before_join: a copy of the observation block to the host, waited for,
    stands between the last call and the join — milliseconds in which the session's waves take every step issued and sit
    polling when the stop arrives (the 20 ms they wait for news are far from over)."""
    import torch
    env = _env(DIST, B, persistent)
    bufs = _bufs(env, B)
    s = torch.cuda.current_stream().cuda_stream
    for n in calls:
        env.rollout_device("random", n, True, s, *bufs, R, False, True)
    if settle_before_join:
        bufs[3].cpu()
    env.join(s)
    env.sync()
    return env, _everything(env, bufs)


@pytest.fixture(scope="module")
def separate_launches():
    """One kernel per launch: the reference of every case below, computed once per (batch, calls)."""
    memo = {}

    def get(B, calls):
        if (B, calls) not in memo:
            memo[(B, calls)] = _run(B, calls, False)[1]
        return memo[(B, calls)]
    return get


@pytest.mark.parametrize("K", STEPS)
@pytest.mark.parametrize("B", BATCHES)
def test_lone_launch_equals_one_kernel(B, K, separate_launches):
    env, got = _run(B, (K,), True)
    ss = env.session_stats()
    assert ss["sessions"] == 1 and ss["joined"] == 0, ss
    assert ss["later_kernel_steps"] == 0, ss                    # (the first kernel took every step: the closing ones found nothing owed)
    assert (got["stats"][:, 0] == K).all()
    _same(got, separate_launches(B, (K,)), (B, K))


@pytest.mark.parametrize("settle", [False, True])
@pytest.mark.parametrize("K", STEPS)
@pytest.mark.parametrize("B", BATCHES)
def test_three_calls_then_join(B, K, settle, separate_launches):
    env, got = _run(B, (K, 1, K), True, settle)
    ss = env.session_stats()
    assert ss["sessions"] + ss["joined"] == 3, ss
    assert (got["stats"][:, 0] == 2 * K + 1).all()
    _same(got, separate_launches(B, (K, 1, K)), (B, K, settle))


def test_lone_launch_of_a_class_that_environments_leave():
    """A register/LDS class capped at 16 basis elements: closing waves also find environments the HBM-resident pass served
    meanwhile, some of them too large to be staged — those are handed over as before, whatever they owe."""
    import torch
    outs = []
    for persistent in (True, False):
        env = _env(DIST, 96, persistent, caps={"lds_max_basis": 16})
        bufs = _bufs(env, 96)
        s = torch.cuda.current_stream().cuda_stream
        for n in (130, 1, 40):
            env.rollout_device("random", n, True, s, *bufs, R, False, True)
            env.join(s)                                         # (every call a session of its own)
        env.sync()
        outs.append(_everything(env, bufs, True))
        if persistent:
            assert env.session_stats()["sessions"] == 3 and env.session_stats()["spills"] > 0, env.session_stats()
    _same(outs[0], outs[1], ("capped class",))


def test_sessions_of_different_shapes_then_the_first_again():
    """Two sessions of one step each whose calls differ in shape (another agent, another observation block), back to back, then
    one of the first shape again: each initial control value travels on the session stream behind the closing kernels of the
    session before, which must never see it (what scripts/fuzz_sessions.py once found, tests/test_sessions.py)."""
    import torch
    B = 1000
    outs = []
    for persistent in (True, False):
        env = _env("3-10-10-uniform", B, persistent, caps={"lds_max_basis": 24})
        rew, done, rows, obs = _bufs(env, B, -1)
        obs2 = torch.full_like(obs, -1)
        s = torch.cuda.current_stream().cuda_stream
        env.rollout_device("random", 1, True, s, rew, done, rows, obs, R, False, False)
        env.rollout_device("first", 1, True, s, rew, done, rows, obs2, R, False, False)
        env.rollout_device("random", 1, True, s, rew, done, rows, obs, R, False, False)
        env.join(s)
        env.sync()
        if persistent:
            ss = env.session_stats()
            assert ss["sessions"] == 3 and ss["joined"] == 0, ss
        outs.append(_everything(env, (rew, done, rows, obs), True))
        outs[-1]["obs2"] = obs2.cpu().numpy()                   # (whole: written by the second call alone, -1 elsewhere)
        assert (outs[-1]["stats"][:, 0] == 3).all()
    _same(outs[0], outs[1], ("shapes",))


def test_policy_step_session_closes_like_separate_kernels():
    """Eight bbx_policy_step_device calls served by one session, joined: its closing kernels (the policy instantiation) leave
    early too.  Actions, log-probabilities and everything else against the same calls one kernel each."""
    import torch
    from deepgroebner_amd.rollout import PMLPPolicy
    torch.manual_seed(7)
    B, T = 64, 8
    envs = [_env(DIST, B, persistent) for persistent in (False, True)]
    policy = PMLPPolicy(envs[0].cols, [64]).cuda()
    w = policy._fused_weights()
    u = torch.rand((T, B), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    outs = []
    for env in envs:
        bufs = _bufs(env, B)
        rew, done, rows, obs = bufs
        act = torch.zeros(B, dtype=torch.int32, device="cuda"); logp = torch.zeros(B, dtype=torch.float32, device="cuda")
        env.rollout_device("first", 0, False, s, rew, done, rows, obs, R, True, False)   # the block the first call's policy reads
        env.sync()
        for t in range(T):
            env.policy_step_device(w["prepared"], w["hidden"], u[t], act, logp, rew, done, rows, obs, R, 2, s)
        env.join(s)
        env.sync()
        out = _everything(env, bufs)
        out["actions"] = act.cpu().numpy(); out["logprobs"] = logp.cpu().numpy()
        outs.append(out)
    ss = envs[1].session_stats()
    assert ss["sessions"] == 1 and ss["joined"] == T - 1 and ss["later_kernel_steps"] == 0, ss
    _same(outs[0], outs[1], ("policy steps",))
