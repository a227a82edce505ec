"""Truncated-horizon GAE on the device: bbx_gae_bootstrap_device behind DeviceTrajectoryBuffer.finish() against the torch loop
(bit for bit) and the exact reference of tests/gae_cases.py, and the rollouts that feed it — run_rollout_fused(critic=...,
bootstrap=True), run_rollout(value_strategy= / critic=, bootstrap=True): where the bootstrap comes from, that the rollout and the
environments are those of the plain call, a buffer of episodes that never end, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import gae_cases as gc
from tests.fast_harness import stream, stream_ptr

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 64), (7, 65), (33, 130)]              # one thread, a full wave, one past it, three blocks with a ragged last


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def _env(dist, B, seed=100):
    from deepgroebner_amd import VecLeadMonomialsEnv
    env = VecLeadMonomialsEnv(dist, batch=B, k=2)
    env.seed(np.arange(B) + seed)
    env.reset()
    return env


def _gen(seed):
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    return g


def _current_block(env, R):
    """What a zero-step launch writes: the padded observation block and the row counts of the states the environments are in."""
    import torch
    B = env.batch
    obs = torch.empty((B, R, env.cols), dtype=torch.int32, device="cuda")
    rew = torch.zeros(B, dtype=torch.float64, device="cuda"); done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(B, dtype=torch.int32, device="cuda")
    env.rollout_device("first", 0, False, stream(), rew, done, rows, obs, R, True, False)
    env.sync()
    return obs, rows


def _same_records(a, b, names=("actions", "rewards", "dones", "rows", "logprobs")):
    import torch
    assert a.t == b.t
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def _every_step_with_rows(buf):
    """The flat step numbers t * B + b of the steps whose state had more than one row, environment after environment."""
    import torch
    T, B = buf.t, buf.B
    step = torch.arange(T, dtype=torch.int32, device="cuda")[None, :] * B + torch.arange(B, dtype=torch.int32, device="cuda")[:, None]
    return step[buf.rows[:T].transpose(0, 1) != 1]


# ---- the kernel -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bootstrap", [True, False])
@pytest.mark.parametrize("T,B", SHAPES)
def test_the_kernel_equals_the_torch_loop_on_general_doubles(T, B, bootstrap):
    import torch
    case = gc.general_case(T, B, seed=40 + T)
    a, b = gc.new_buffer(case, "cuda", bootstrap=bootstrap), gc.new_buffer(case, "cuda", bootstrap=bootstrap)
    ret, adv, comp = a.finish()
    wret, wadv, wcomp = b._finish_torch()
    torch.cuda.synchronize()
    assert comp.dtype == wcomp.dtype and torch.equal(comp, wcomp)
    assert torch.equal(ret, wret) and torch.equal(adv, wadv) and torch.equal(a.lambda_returns, b.lambda_returns)
    assert a.returns is ret and a.advantages is adv and a.complete is comp
    assert bool(comp.all()) == (bootstrap or bool(case.dones[T - 1].all()))
    for targets in ("returns", "lambda"):
        got, want = a.get_index(None, targets=targets), b.get_index(None, targets=targets)
        same = lambda x, y: x.shape == y.shape and bool(((x == y) | (torch.isnan(x) & torch.isnan(y))).all())
        assert all(same(x, y) for x, y in zip(got, want))


@pytest.mark.parametrize("p_done", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("T,B", [(1, 1), (2, 64), (7, 65), (20, 130)])
def test_the_kernel_equals_the_fraction_reference_on_exact_cases(T, B, p_done):
    case = gc.exact_case(T, B, p_done, seed=100 * T + B)
    buf = gc.new_buffer(case, "cuda")
    ret, adv, comp = buf.finish()
    wret, wadv, wlret, _ = gc.reference(case)
    assert gc.equals_exactly(ret.cpu().numpy(), wret) and gc.equals_exactly(adv.cpu().numpy(), wadv)
    assert gc.equals_exactly(buf.lambda_returns.cpu().numpy(), wlret)
    assert bool(comp.all())


def test_a_nan_behind_a_done_last_step_reaches_no_output():
    import torch
    T, B = 33, 130
    case = gc.general_case(T, B, seed=21)
    closed = np.flatnonzero(case.dones[T - 1])
    never = np.flatnonzero(~case.dones.any(axis=0))
    assert closed.size >= 2 and never.size >= 2
    clean = gc.new_buffer(case, "cuda")
    clean.finish()
    other = case.last.copy(); other[closed] = float("nan")
    buf = gc.new_buffer(case._replace(last=other), "cuda")
    ret, adv, comp = buf.finish()
    for x, y in ((ret, clean.returns), (adv, clean.advantages), (buf.lambda_returns, clean.lambda_returns)):
        assert not torch.isnan(x).any() and torch.equal(x, y)
    assert bool(comp.all())
    want = case.rewards[T - 1, never] + case.gam * case.last[never]
    assert np.array_equal(ret[T - 1].cpu().numpy()[never], want)


@pytest.mark.parametrize("T,B", SHAPES)
def test_the_old_entry_is_the_new_one_with_two_nulls(T, B):
    import torch
    from deepgroebner_amd import _ffi
    case = gc.general_case(T, B, seed=60 + T)
    buf = gc.new_buffer(case, "cuda", bootstrap=False)
    p = lambda x: C.c_void_p(x.data_ptr())
    r, v, d = buf.rewards, buf.values, buf.dones
    outs = []
    for new in (False, True):
        ret = torch.full_like(r, 7.0); adv = torch.full_like(r, 7.0); comp = torch.full_like(d, True)
        if new:
            rc = _ffi.lib().bbx_gae_bootstrap_device(p(r), p(v), p(d), T, B, 0.99, 0.97, None, p(ret), p(adv), p(comp), None, stream_ptr())
        else:
            rc = _ffi.lib().bbx_gae_device(p(r), p(v), p(d), T, B, 0.99, 0.97, p(ret), p(adv), p(comp), stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        outs.append((ret, adv, comp))
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    wret, wadv, wcomp = buf._finish_torch()
    assert torch.equal(outs[0][0], wret) and torch.equal(outs[0][1], wadv) and torch.equal(outs[0][2], wcomp)


# ---- the fused rollout -----------------------------------------------------------------------------------------------------------

def test_run_rollout_fused_bootstraps_from_the_critic_and_leaves_the_rollout_alone():
    import torch
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, PMLPValue, run_rollout_fused
    B, T, R = 64, 32, 256
    env, twin = _env("3-20-10-weighted", B), _env("3-20-10-weighted", B)
    cols = env.cols
    torch.manual_seed(5)
    policy = PMLPPolicy(cols, (64,)).cuda()
    critic = PMLPValue(cols, (64,)).cuda()
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(R, cols))
    plain = DeviceTrajectoryBuffer(T, B, obs_shape=(R, cols))
    plain.last_values = torch.zeros(B, dtype=torch.float64, device="cuda")     # (a stale tail: the plain call clears it)
    run_rollout_fused(env, policy, T, buf, generator=_gen(11), critic=critic, bootstrap=True)
    run_rollout_fused(twin, policy, T, plain, generator=_gen(11), critic=critic)
    assert plain.last_values is None
    _same_records(buf, plain, ("actions", "rewards", "dones", "rows", "logprobs", "values", "states"))
    obs, rows = _current_block(twin, R)
    want = torch.empty(B, dtype=torch.float64, device="cuda")
    critic.values(obs, rows, out64=want)
    assert critic.last_path == "kernels"
    last = buf.last_values
    assert last.dtype == torch.float64 and tuple(last.shape) == (B,) and torch.equal(last, want) and float(last.abs().max()) > 0
    ret, adv, comp = buf.finish()
    assert bool(comp.all())
    assert torch.equal(buf.get_index(None)[0], _every_step_with_rows(buf))
    pcomp = plain.finish()[2]
    print("complete steps without the bootstrap: %d of %d; dones recorded: %d" % (int(pcomp.sum()), T * B, int(plain.dones.sum())))
    assert not bool(pcomp.all())                                               # the buffer's end did cut episodes
    assert torch.equal(ret[pcomp], plain.returns[pcomp]) and torch.equal(adv[pcomp], plain.advantages[pcomp])
    # both handles go on draw for draw
    assert np.array_equal(env.stats(), twin.stats())
    buf2 = DeviceTrajectoryBuffer(T, B, obs_shape=(R, cols)); plain2 = DeviceTrajectoryBuffer(T, B, obs_shape=(R, cols))
    run_rollout_fused(env, policy, T, buf2, generator=_gen(12))
    run_rollout_fused(twin, policy, T, plain2, generator=_gen(12))
    _same_records(buf2, plain2, ("actions", "rewards", "dones", "rows", "logprobs", "states"))
    assert buf2.last_values is None
    assert np.array_equal(env.stats(), twin.stats())


# ---- the per-step path -----------------------------------------------------------------------------------------------------------

def test_run_rollout_bootstraps_from_the_value_strategy():
    import torch
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, run_rollout
    B, T, R = 64, 8, 256
    env, twin = _env("3-20-10-weighted", B), _env("3-20-10-weighted", B)
    env.accounting(False); twin.accounting(False)
    torch.manual_seed(2)
    policy = PMLPPolicy(env.cols, (128,)).cuda()
    buf = DeviceTrajectoryBuffer(T, B, gam=0.97); plain = DeviceTrajectoryBuffer(T, B, gam=0.97)
    run_rollout(env, policy, T, buf, obs_rows=R, generator=_gen(5), value_strategy="degree", bootstrap=True)
    run_rollout(twin, policy, T, plain, obs_rows=R, generator=_gen(5), value_strategy="degree")
    _same_records(buf, plain, ("actions", "rewards", "dones", "rows", "logprobs", "values"))
    assert plain.last_values is None
    want = twin.values("degree", 0.97)
    got = buf.last_values.cpu().numpy()
    assert got.dtype == np.float64 and not np.isnan(got).any() and np.array_equal(got, want)
    assert bool(buf.finish()[2].all())
    assert np.array_equal(env.stats(), twin.stats())
    a, b = env.rollout("random", 3, auto_reset=True), twin.rollout("random", 3, auto_reset=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(env.stats(), twin.stats())


def test_run_rollout_fills_and_bootstraps_from_a_critic():
    import torch
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, PMLPValue, run_rollout
    B, T, R = 64, 8, 256
    env, twin = _env("3-20-10-weighted", B), _env("3-20-10-weighted", B)
    env.accounting(False); twin.accounting(False)
    cols = env.cols
    torch.manual_seed(2)
    policy = PMLPPolicy(cols, (128,)).cuda()
    critic = PMLPValue(cols, (64,)).cuda()
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(R, cols)); plain = DeviceTrajectoryBuffer(T, B, obs_shape=(R, cols))
    run_rollout(env, policy, T, buf, obs_rows=R, generator=_gen(5), critic=critic, bootstrap=True)
    run_rollout(twin, policy, T, plain, obs_rows=R, generator=_gen(5))
    assert not plain.values.any()
    plain.fill_values(critic)
    _same_records(buf, plain, ("actions", "rewards", "dones", "rows", "logprobs", "values", "states"))
    assert float(buf.values.abs().max()) > 0
    obs, rows = _current_block(twin, R)
    want = torch.empty(B, dtype=torch.float64, device="cuda")
    critic.values(obs, rows, out64=want)
    assert torch.equal(buf.last_values, want) and float(want.abs().max()) > 0
    assert bool(buf.finish()[2].all())
    # critic without bootstrap: the values, and no tail
    again = DeviceTrajectoryBuffer(T, B, obs_shape=(R, cols))
    again.last_values = want
    run_rollout(env, policy, T, again, obs_rows=R, generator=_gen(6), critic=critic)
    assert again.last_values is None and float(again.values.abs().max()) > 0


# ---- episodes that never end inside the buffer ---------------------------------------------------------------------------------------

def test_a_buffer_of_unfinished_episodes_trains_only_with_the_bootstrap():
    import torch
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, PMLPValue, ppo_update, run_rollout_fused, value_update
    B, T, R = 8, 16, 256
    torch.manual_seed(9)
    bufs = {}
    for bootstrap in (False, True):
        env = _env("5-10-5-uniform", B, seed=300)
        cols = env.cols
        if not bufs:
            policy = PMLPPolicy(cols, (64,)).cuda()
            critic = PMLPValue(cols, (64,)).cuda()
        buf = DeviceTrajectoryBuffer(T, B, obs_shape=(R, cols))
        run_rollout_fused(env, policy, T, buf, generator=_gen(4), critic=critic, bootstrap=bootstrap)
        bufs[bootstrap] = buf
    plain, buf = bufs[False], bufs[True]
    assert int(plain.dones.sum()) == 0 and int(buf.dones.sum()) == 0             # no episode ends within 16 steps (these seeds)
    assert int(plain.get_index(None)[0].numel()) == 0
    idx = buf.get_index(None)[0]
    want = _every_step_with_rows(buf)
    n = int(want.numel())
    assert torch.equal(idx, want) and n == int((buf.rows != 1).sum()) and n > T * B // 2
    popt = torch.optim.Adam(policy.parameters(), lr=1e-3); vopt = torch.optim.Adam(critic.parameters(), lr=1e-3)
    out = ppo_update(policy, buf, popt, 1, 32, generator=_gen(1))
    assert len(out) == 1 and out[0]["stats"][:, 0].sum() == n and (out[0]["stats"][:, 5] == 0).all()
    assert all(np.isfinite(out[0][k]) for k in ("loss", "entropy", "kl", "clip_frac")) and np.isfinite(out[0]["stats"]).all()
    vout = value_update(critic, buf, vopt, 1, 32, generator=_gen(2), targets="lambda")
    assert len(vout) == 1 and vout[0]["stats"][:, 0].sum() == n and (vout[0]["stats"][:, 5] == 0).all()
    assert np.isfinite(vout[0]["loss"]) and np.isfinite(vout[0]["stats"]).all()
    # the targets were the lambda-returns: sum of targets over the epoch, against the buffer's own (float32 targets, float64 sums)
    j = idx.to(torch.int64)
    t64 = buf.lambda_returns.reshape(-1)[j].to(torch.float32).to(torch.float64)
    assert abs(vout[0]["stats"][:, 3].sum() - float(t64.sum())) <= 1e-12 * float(t64.abs().sum())   # (n <= 128 double adds: n 2^-53)
    assert float((t64 - buf.returns.reshape(-1)[j]).abs().max()) > 0                                 # (and they are not the returns)
    with pytest.raises(ValueError):
        value_update(critic, buf, vopt, 1, 32, targets="td")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_anything_is_queued():
    import torch
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, PMLPValue, run_rollout, run_rollout_fused
    B, T, R = 16, 4, 64
    env = _env("3-20-10-weighted", B)
    cols = env.cols
    policy = PMLPPolicy(cols, (64,)).cuda()
    critic = PMLPValue(cols, (64,)).cuda()
    states = DeviceTrajectoryBuffer(T, B, obs_shape=(R, cols))
    bare = DeviceTrajectoryBuffer(T, B)
    launched, stats = env.kernels_launched(), env.stats()
    calls = [lambda: run_rollout_fused(env, policy, T, states, bootstrap=True),                               # no critic
             lambda: run_rollout_fused(env, policy, T, None, bootstrap=True),                                 # no buffer, no critic
             lambda: run_rollout_fused(env, policy, T, bare, critic=critic, bootstrap=True),                  # a buffer without states
             lambda: run_rollout(env, policy, T, states, obs_rows=R, bootstrap=True),                         # neither source
             lambda: run_rollout(env, policy, T, None, obs_rows=R, bootstrap=True),                           # no buffer
             lambda: run_rollout(env, policy, T, None, obs_rows=R, critic=critic, bootstrap=True),            # no buffer
             lambda: run_rollout(env, policy, T, bare, obs_rows=R, critic=critic),                            # a buffer without states
             lambda: run_rollout(env, policy, T, states, obs_rows=R, critic=critic, value_strategy="degree")]  # two baselines
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert env.kernels_launched() == launched and states.t == 0 and bare.t == 0, k
    assert np.array_equal(env.stats(), stats)
