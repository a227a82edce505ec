"""Device-side baseline values: bbx_values_device against the synchronous value calls (== on doubles: same clone, same
kernels, other plumbing), its ordering between asynchronous steps, the clone ring's slot reuse, growth of the records at the
wait, its refusals, run_rollout(value_strategy=...) and the GAE kernel behind DeviceTrajectoryBuffer.finish()."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as graft
from tests.fast_harness import same_doubles, stream

pytestmark = pytest.mark.gpu

OBS_ROWS = 512


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def _make(dist, B, caps=None, k=2, seed=70, walk=5):
    """A batch somewhere inside its episodes."""
    from deepgroebner_amd import VecLeadMonomialsEnv
    from deepgroebner_amd.ideals import FixedIdealGenerator, cyclic
    if dist == "cyclic-5":
        env = VecLeadMonomialsEnv(FixedIdealGenerator(cyclic(5)), batch=B, k=k, caps=caps)
    else:
        env = VecLeadMonomialsEnv(dist, batch=B, k=k, caps=caps)
    env.seed(np.arange(B) + seed); env.seed_agent(np.arange(B)); env.reset()
    if walk:
        env.rollout("random", walk, auto_reset=True)
    return env


def _values_device(env, strategy, gamma=0.99, seeds=None):
    import torch
    out = torch.full((env.batch,), -1.0, dtype=torch.float64, device="cuda")
    s = None if seeds is None else torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.int64)).cuda()
    env.values_device(out, strategy, gamma, s, stream())
    env.sync()
    return out.cpu().numpy()


CASES = [("3-20-10-weighted", None, 12), ("3-20-10-weighted", {"lds_max_basis": 16}, 12), ("3-20-10-weighted", {"lds_max_basis": -1}, 12),
         ("5-10-5-uniform", None, 12), ("3-5-4-0.5-uniform", None, 12), ("cyclic-5", None, 3)]


@pytest.mark.parametrize("dist,caps,B", CASES)
def test_values_device_equals_values_for_the_same_states(dist, caps, B):
    """Every kernel class bbx_values serves, every strategy, and "random" with seeds that exercise seed -> engine state (0,
    2^31 - 1 and -1: x = seed mod (2^31 - 1), 0 becomes 1) converted on the device."""
    env = _make(dist, B, caps, k=1 if dist == "cyclic-5" else 2, walk=3 if dist == "cyclic-5" else 5)
    for strategy in ("degree", "normal", "sugar", "first", "env"):
        want = env.values(strategy, 0.99)
        got = _values_device(env, strategy, 0.99)
        print(dist, caps, strategy, "max |diff|", np.abs(got - want).max())
        assert same_doubles(got, want), (dist, caps, strategy)
    assert same_doubles(_values_device(env, "degree", 0.9), env.values("degree", 0.9))
    rng = np.random.default_rng(11)
    seeds = rng.integers(-2 ** 31, 2 ** 31 - 1, size=B)
    seeds[:3] = (0, 2147483647, -1)
    want = env.values("random", 0.99, seeds=seeds)
    got = _values_device(env, "random", 0.99, seeds)
    assert same_doubles(got, want), (dist, caps, "random")


def _twin_walk(twin, T, strategy, gamma, rng):
    """values() then one step with a wait each: what the asynchronous calls must reproduce -> (values [T, B], actions [T, B])."""
    import torch
    B = twin.batch
    act = torch.zeros(B, dtype=torch.int32, device="cuda")
    rows = torch.from_numpy(twin.rows.astype(np.int32)).cuda()
    vals, actions = [], []
    for _ in range(T):
        vals.append(twin.values(strategy, gamma))
        r = rows.cpu().numpy()
        a = (rng.integers(0, 2 ** 31 - 1, size=B) % np.maximum(r, 1)).astype(np.int32)
        actions.append(a)
        act.copy_(torch.from_numpy(a))
        twin.step_device(act, rows=rows, stream=stream(), auto_reset=True)
        twin.sync()
    return np.stack(vals), np.stack(actions)


def _async_walk(env, actions, strategy, gamma):
    """values_device then step_device for every t, no wait inside, one sync."""
    import torch
    T, B = actions.shape
    acts = torch.from_numpy(actions).cuda()
    out = torch.full((T, B), -1.0, dtype=torch.float64, device="cuda")
    rows = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = stream()
    for t in range(T):
        env.values_device(out[t], strategy, gamma, None, s)
        env.step_device(acts[t], rows=rows, stream=s, auto_reset=True)
    env.sync()
    return out.cpu().numpy()


def _assert_handles_equal(env, twin, steps=5):
    assert np.array_equal(env.stats(), twin.stats())
    assert np.array_equal(env.observations(OBS_ROWS), twin.observations(OBS_ROWS))
    for _ in range(steps):                                   # (auto-resets draw from the generator streams)
        a, b = env.rollout("random", 1, auto_reset=True), twin.rollout("random", 1, auto_reset=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert np.array_equal(env.observations(OBS_ROWS), twin.observations(OBS_ROWS))
    assert np.array_equal(env.stats(), twin.stats())


def test_values_between_asynchronous_steps_are_those_of_their_place_in_the_stream():
    B, T = 64, 40
    env = _make("3-20-10-weighted", B)
    twin = env.copy()
    want, actions = _twin_walk(twin, T, "degree", 0.99, np.random.default_rng(3))
    got = _async_walk(env, actions, "degree", 0.99)
    bad = [t for t in range(T) if not np.array_equal(got[t], want[t])]
    assert not bad and not np.isnan(got).any(), bad
    _assert_handles_equal(env, twin)


@pytest.mark.parametrize("ring", ["2", None])
def test_more_calls_in_flight_than_the_ring_has_slots(ring):
    """The slot-reuse case: 16 calls queued behind each other on a ring of 2 (and of the default depth)."""
    B, T = 4096, 16
    old = os.environ.get("BBX_VALUE_RING")
    try:
        if ring is None:
            os.environ.pop("BBX_VALUE_RING", None)
        else:
            os.environ["BBX_VALUE_RING"] = ring
        env = _make("3-20-10-weighted", B)
        twin = env.copy()
    finally:
        if old is None:
            os.environ.pop("BBX_VALUE_RING", None)
        else:
            os.environ["BBX_VALUE_RING"] = old
    want, actions = _twin_walk(twin, T, "degree", 0.99, np.random.default_rng(4))
    got = _async_walk(env, actions, "degree", 0.99)
    bad = [t for t in range(T) if not np.array_equal(got[t], want[t])]
    assert not bad and not np.isnan(got).any(), bad
    assert np.array_equal(env.stats(), twin.stats())


GROWTH = [{"max_basis": 12, "max_pairs": 16}, {"max_basis": 12, "max_pairs": 16, "lds_max_basis": -1}]


@pytest.mark.parametrize("caps", GROWTH)
def test_value_rollouts_that_outgrow_the_records_are_finished_at_the_wait(caps):
    B = 9
    env = _make("3-20-10-weighted", B, caps, seed=500, walk=0)
    twin = env.copy()
    before = twin.capacities()
    want = twin.values("degree", 0.99)
    after = twin.capacities()
    assert after["grown"] > before["grown"], (before, after)       # the case covers growth
    assert env.capacities() == before
    got = _values_device(env, "degree", 0.99)
    print("twin", before, "->", after, "device", env.capacities())
    assert same_doubles(got, want)
    assert env.capacities()["grown"] > before["grown"] and env.capacities()["grown"] == after["grown"]   # the same rise
    assert all(env.capacities()[k] >= after[k] for k in ("max_basis", "max_pairs"))
    assert same_doubles(_values_device(env, "normal", 0.99), twin.values("normal", 0.99))   # the ring follows the new layout
    _assert_handles_equal(env, twin, steps=2)


def test_value_rollouts_that_outgrow_hard_limits_are_an_error_and_nan():
    from deepgroebner_amd import _ffi
    B = 64
    caps = {"max_basis": 48, "max_pairs": 128, "lds_max_basis": -1}
    ref = _make("3-20-10-weighted", B, caps, seed=500, walk=0)
    want = ref.values("degree", 0.99)
    assert ref.capacities()["grown"] > 0                           # some rollout outgrows these capacities
    env = _make("3-20-10-weighted", B, dict(caps, no_growth=1), seed=500, walk=0)
    twin = env.copy()
    with pytest.raises(_ffi.BbxError) as ei:
        twin.values("degree", 0.99)
    assert ei.value.code == -3
    import torch
    for _ in range(2):                                             # (the handle stays usable: the same answer again)
        out = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
        env.values_device(out, "degree", 0.99, None, stream())
        with pytest.raises(_ffi.BbxError) as ei:
            env.sync()
        assert ei.value.code == -3, ei.value
        named = int(re.search(r"environment (\d+)", str(ei.value)).group(1))
        got = out.cpu().numpy()
        assert np.isnan(got[named])
        ok = ~np.isnan(got)
        print("hard limits:", int((~ok).sum()), "of", B, "entries NaN, environment", named, "named")
        assert np.array_equal(got[ok], want[ok])                   # never a silently wrong value
    env.sync()
    assert np.array_equal(env.observations(OBS_ROWS), twin.observations(OBS_ROWS)) and np.array_equal(env.stats(), twin.stats())


def test_refusals_and_a_running_session():
    import torch
    from deepgroebner_amd import _ffi
    B = 256
    env = _make("3-20-10-weighted", B)
    out = torch.zeros(B, dtype=torch.float64, device="cuda")
    with pytest.raises(_ffi.BbxError) as ei:
        env.values_device(out, "sample", 0.99, None, stream())
    assert ei.value.code == -5
    with pytest.raises(_ffi.BbxError) as ei:
        env.values_device(out, "random", 0.99, None, stream())
    assert ei.value.code == -1
    codes = []
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out.add_(0.0)
        try:
            env.values_device(out, "degree", 0.99, None, torch.cuda.current_stream().cuda_stream)
        except _ffi.BbxError as e:
            codes.append(e.code)
    assert codes == [-5]
    # a persistent session in progress is closed first; the values are those behind its steps
    env.accounting(False)
    twin = env.copy()
    env.persistent(True)
    s = stream()
    for _ in range(3):
        env.rollout_device("degree", 20, True, s)
    env.values_device(out, "degree", 0.99, None, s)
    env.sync()
    assert env.session_stats()["sessions"] >= 1
    for _ in range(3):
        twin.rollout_device("degree", 20, True, s)
    twin.sync()
    assert same_doubles(out.cpu().numpy(), twin.values("degree", 0.99))
    assert np.array_equal(env.stats(), twin.stats())


def test_run_rollout_records_the_value_of_the_state_the_policy_is_about_to_see():
    import torch
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, run_rollout
    B, T, R = 256, 24, 256
    env = _make("3-20-10-weighted", B)
    env.accounting(False)
    plain, twin = env.copy(), env.copy()
    torch.manual_seed(2)
    policy = PMLPPolicy(env.cols, (128,)).cuda()
    gen = torch.Generator(device="cuda")
    buf = DeviceTrajectoryBuffer(T, B, gam=0.97)
    gen.manual_seed(5)
    run_rollout(env, policy, T, buf, obs_rows=R, generator=gen, value_strategy="degree")
    buf0 = DeviceTrajectoryBuffer(T, B, gam=0.97)
    gen.manual_seed(5)
    run_rollout(plain, policy, T, buf0, obs_rows=R, generator=gen)
    for name in ("actions", "rewards", "dones", "logprobs", "rows"):
        assert torch.equal(getattr(buf, name), getattr(buf0, name)), name
    assert not buf0.values.any()
    # the twin: values("degree", gam), then the same policy step, with a wait each
    s = stream()
    dev = "cuda"
    obs = torch.empty((B, R, env.cols), dtype=torch.int32, device=dev)
    rew = torch.zeros(B, dtype=torch.float64, device=dev); done = torch.zeros(B, dtype=torch.uint8, device=dev)
    rows = torch.zeros(B, dtype=torch.int32, device=dev); act = torch.zeros(B, dtype=torch.int32, device=dev)
    logp = torch.zeros(B, dtype=torch.float32, device=dev)
    twin.rollout_device("first", 0, False, s, rew, done, rows, obs, R, True, False)
    twin.sync()
    w = policy._fused_weights()
    gen.manual_seed(5)
    u_all = torch.rand((T, B), device=dev, generator=gen)
    want = np.zeros((T, B))
    for t in range(T):
        want[t] = twin.values("degree", 0.97)
        twin.policy_step_device(w["prepared"], w["hidden"], u_all[t], act, logp, rew, done, rows, obs, R, 2, s)
        twin.sync()
        assert torch.equal(act, buf.actions[t]), t
    got = buf.values.cpu().numpy()
    bad = [t for t in range(T) if not np.array_equal(got[t], want[t])]
    assert not bad and not np.isnan(got).any(), bad
    with pytest.raises(ValueError):
        run_rollout(env, policy, 4, DeviceTrajectoryBuffer(4, B), graph=True, value_strategy="degree")


def _filled_buffer(T, B, seed):
    import torch
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer
    rng = np.random.default_rng(seed)
    buf = DeviceTrajectoryBuffer(T, B, gam=0.99, lam=0.97)
    d = rng.random((T, B)) < 0.06
    d[0, 0] = True; d[T - 1, B - 1] = True                   # done flags at the first and the last step
    buf.rewards.copy_(torch.from_numpy(-rng.integers(0, 400, size=(T, B)) * rng.random((T, B))))
    buf.values.copy_(torch.from_numpy(-rng.random((T, B)) * 300.0))
    buf.dones.copy_(torch.from_numpy(d))
    buf.rows.copy_(torch.from_numpy(rng.integers(1, 9, size=(T, B)).astype(np.int32)))
    buf.actions.copy_(torch.from_numpy(rng.integers(0, 9, size=(T, B)).astype(np.int32)))
    buf.logprobs.copy_(torch.from_numpy(-rng.random((T, B)).astype(np.float32)))
    buf.t = T
    return buf


@pytest.mark.parametrize("T,B", [(256, 4096), (7, 3)])
def test_gae_kernel_equals_the_torch_loop(T, B):
    import torch
    a, b = _filled_buffer(T, B, 9), _filled_buffer(T, B, 9)
    ret, adv, comp = a.finish()
    wret, wadv, wcomp = b._finish_torch()
    torch.cuda.synchronize()
    print("T", T, "B", B, "max |ret diff|", (ret - wret).abs().max().item(), "max |adv diff|", (adv - wadv).abs().max().item())
    assert comp.dtype == wcomp.dtype and torch.equal(comp, wcomp)
    assert torch.equal(ret, wret) and torch.equal(adv, wadv)
    assert a.returns is ret and a.advantages is adv and a.complete is comp
    got, want = a.get(), b.get()                             # (b: the torch loop's results, as before the kernel)
    for x, y in zip(got, want):
        assert (x is None and y is None) or torch.equal(x, y)
    got, want = a.get(batch_size=512, sort=True), b.get(batch_size=512, sort=True)
    assert len(got) == len(want) and all(torch.equal(x, y) for g, w in zip(got, want) for x, y in zip(g, w) if x is not None)
