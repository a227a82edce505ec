"""A two-hidden-layer PMLP inside the step kernels (bbx_policy2_rollout_device; rollout.run_rollout_fused): the fused rollout
against the two-launch loop it replaces (bbx_pmlp2_act, then bbx_step_device_autoreset), against the torch module, on the
oracle, past 1024 rows, and its refusals — including the deeper policies run_rollout_fused used to run as a different network."""
import numpy as np
import pytest


def _policy(cols, hidden, seed):
    import torch
    from deepgroebner_amd.rollout import PMLPPolicy
    torch.manual_seed(seed)
    policy = PMLPPolicy(cols, list(hidden)).cuda()
    with torch.no_grad():
        for lin in list(policy.embedding) + [policy.deciding]:
            lin.weight.mul_(0.3)
    return policy


def _two_launch_reference(env, policy, u, R, obs_rows_check=True):
    """One vector step at a time: policy.act (bbx_pmlp2_act) on the padded block, then bbx_step_device_autoreset."""
    import torch
    T, B = u.shape
    s = torch.cuda.current_stream().cuda_stream
    obs = torch.full((B, R, env.cols), -1, dtype=torch.int32, device="cuda")
    rew = torch.zeros(B, dtype=torch.float64, device="cuda"); done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(B, dtype=torch.int32, device="cuda"); act = torch.zeros(B, dtype=torch.int32, device="cuda")
    logp = torch.zeros(B, dtype=torch.float32, device="cuda")
    env.rollout_device("first", 0, False, s, rew, done, rows, obs, R, True, False); env.sync()
    want = {k: [] for k in ("obs", "rows", "act", "logp", "rew", "done")}
    for t in range(T):
        want["obs"].append(obs.clone()); want["rows"].append(rows.clone())
        policy.act(obs, rows, u[t], act, logp)
        env.step_device(act, rew, done, rows, obs, R, 1, s, auto_reset=True)
        env.sync()
        for k, v in (("act", act), ("logp", logp), ("rew", rew), ("done", done)):
            want[k].append(v.clone())
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("dist,k,hidden,caps", [("3-20-10-weighted", 2, (128, 128), None), ("3-20-10-weighted", 2, (64, 64), None),
                                                ("3-20-10-weighted", 2, (100, 48), None),
                                                ("3-20-10-weighted", 2, (128, 128), {"lds_max_basis": 16}),
                                                ("3-20-10-weighted", 2, (64, 64), {"lds_max_basis": 16}),
                                                ("3-20-10-weighted", 2, (100, 48), {"lds_max_basis": 16}),
                                                ("5-10-5-uniform", 2, (128, 128), None), ("5-10-5-uniform", 1, (64, 64), None),
                                                ("4-5-4-uniform", 2, (128, 128), None)])
def test_two_layer_rollout_in_one_launch_equals_the_two_launch_loop(dist, k, hidden, caps):
    """bbx_policy2_rollout_device (T steps in two launches that cross a cut) against bbx_pmlp2_act + bbx_step_device_autoreset per
    step on a copy of the batch with the same uniforms: actions, log-probabilities, rewards, dones, row counts and observations
    identical (the logits come from the same tile code: pmlp2_tile), and so are the counters afterwards.  With the register/LDS
    class capped at 16 basis elements most environments move to the HBM-resident continuation mid-launch; the other rings run
    in the HBM-resident kernel from the start.  A few steps of the first case also against the torch module."""
    import torch
    B, T, R = (500, 70, 256) if dist.startswith("3-") else (200, 60, 1024)
    from deepgroebner_amd import VecLeadMonomialsEnv
    env = VecLeadMonomialsEnv(dist, batch=B, k=k, caps=caps)
    env.seed(np.arange(B) + 77); env.reset(); env.accounting(False)
    twin = env.copy(); twin.accounting(False)
    policy = _policy(env.cols, hidden, 3)
    w = policy._deep_weights()
    s = torch.cuda.current_stream().cuda_stream
    u = torch.rand((T, B), device="cuda")
    want = _two_launch_reference(env, policy, u, R)
    A = torch.zeros((T, B), dtype=torch.int32, device="cuda"); L = torch.zeros((T, B), dtype=torch.float32, device="cuda")
    Rw = torch.zeros((T, B), dtype=torch.float64, device="cuda"); D = torch.zeros((T, B), dtype=torch.uint8, device="cuda")
    N = torch.zeros((T, B), dtype=torch.int32, device="cuda")
    O = torch.full((T, B, R, env.cols), -1, dtype=torch.int32, device="cuda")
    cut = 29
    h1, h2 = w["hidden"]
    twin.policy2_rollout_device(w["prepared"], h1, h2, cut, u[:cut], A[:cut], L[:cut], Rw[:cut], D[:cut], N[:cut], O[:cut], R, B * R * env.cols, s)
    twin.sync()
    twin.policy2_rollout_device(w["prepared"], h1, h2, T - cut, u[cut:], A[cut:], L[cut:], Rw[cut:], D[cut:], N[cut:], O[cut:], R, B * R * env.cols, s)
    twin.sync()
    for t in range(T):
        assert torch.equal(N[t], want["rows"][t]), t
        assert torch.equal(A[t], want["act"][t]), t
        assert torch.equal(L[t], want["logp"][t]), t
        assert torch.equal(Rw[t], want["rew"][t]) and torch.equal(D[t], want["done"][t]), t
        live = torch.arange(R, device="cuda")[None, :] < N[t][:, None]
        assert torch.equal(O[t][live], want["obs"][t][live]), t
        assert (O[t][~live] == -1).all()
    assert np.array_equal(env.stats()[:, :5], twin.stats()[:, :5])
    if dist.startswith("3-"):
        assert D.sum() > 0
    if dist == "3-20-10-weighted" and hidden == (128, 128) and caps is None:
        for t in (0, 10, 40):                                     # the torch module on the blocks the fused rollout wrote
            a_t, l_t = policy.act_torch(O[t], N[t], u[t])
            same = A[t] == a_t
            assert int((~same).sum()) <= 1 and torch.allclose(L[t][same], l_t[same], atol=3e-4, rtol=1e-4), t


@pytest.mark.gpu
def test_fused_two_layer_rollout_fills_the_trajectory_buffer_like_run_rollout():
    """run_rollout_fused with a PMLP(128, 128) and a buffer that keeps the states against run_rollout of a twin with the same
    generator seed: actions, log-probabilities, rewards, dones, rows, states, returns and advantages equal."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, run_rollout, run_rollout_fused
    B, T, R = 256, 96, 128
    env = VecLeadMonomialsEnv("3-20-10-weighted", batch=B, k=2)
    env.seed(np.arange(B) + 31); env.reset(); env.accounting(False)
    twin = env.copy(); twin.accounting(False)
    policy = _policy(env.cols, (128, 128), 4)
    b1 = DeviceTrajectoryBuffer(T, B, 0.99, 0.97, obs_shape=(R, env.cols))
    b2 = DeviceTrajectoryBuffer(T, B, 0.99, 0.97, obs_shape=(R, env.cols))
    tot1, ep1 = run_rollout_fused(env, policy, T, buffer=b1, generator=torch.Generator(device="cuda").manual_seed(11), chunk=32)
    tot2, ep2 = run_rollout(twin, policy, T, buffer=b2, obs_rows=R, generator=torch.Generator(device="cuda").manual_seed(11), sync_every=32)
    torch.cuda.synchronize()
    for name in ("actions", "logprobs", "rewards", "dones", "rows", "states"):
        assert torch.equal(getattr(b1, name), getattr(b2, name)), name
    assert torch.equal(tot1, tot2) and torch.equal(ep1, ep2)
    r1, a1, c1 = b1.finish(); r2, a2, c2 = b2.finish()
    assert torch.equal(r1, r2) and torch.equal(a1, a2) and torch.equal(c1, c2)


@pytest.mark.gpu
def test_fused_two_layer_rollout_replays_on_the_oracle():
    """The actions a fused two-layer rollout drew, replayed environment by environment on the CPU oracle: the same
    observations, rewards and dones."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, run_rollout_fused
    from oracle import ffi
    bo = ffi.load("bo")
    B, T, k, R = 48, 150, 2, 128
    env = VecLeadMonomialsEnv("3-20-10-weighted", batch=B, k=k)
    env.seed(np.arange(B) + 700); env.reset()
    policy = _policy(env.cols, (128, 128), 2)
    buf = DeviceTrajectoryBuffer(T, B, 0.99, 0.97, obs_shape=(R, env.cols))
    total, episodes = run_rollout_fused(env, policy, T, buffer=buf, chunk=64)
    torch.cuda.synchronize()
    states = buf.states.cpu().numpy(); acts = buf.actions.cpu().numpy(); rews = buf.rewards.cpu().numpy()
    dones = buf.dones.cpu().numpy(); rows = buf.rows.cpu().numpy()
    for e in range(B):
        o = bo.env("3-20-10-weighted"); o.seed(700 + e); o.reset()
        tot, eps = 0.0, 0
        for t in range(T):
            want = o.obs(k)
            assert rows[t, e] == o.nP and np.array_equal(states[t, e, :o.nP], want) and (states[t, e, o.nP:] == -1).all(), (e, t)
            assert 0 <= acts[t, e] < o.nP
            r = o.step(int(acts[t, e]))
            tot += r
            assert rews[t, e] == r and bool(dones[t, e]) == (o.nP == 0), (e, t)
            if o.nP == 0:
                eps += 1
                o.reset()
        assert float(total[e]) == tot and int(episodes[e]) == eps


@pytest.mark.gpu
def test_two_layer_rollout_on_pair_sets_of_more_than_1024_rows():
    """5-15-5-uniform pre-rolled until a pair set passes 1100 rows: the fused two-layer rollout against the two-launch loop."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    B, T, R, k = 256, 8, 2048, 1
    env = VecLeadMonomialsEnv("5-15-5-uniform", batch=B, k=k)
    env.seed(np.arange(B) + 300); env.seed_agent(np.arange(B)); env.reset(); env.accounting(False)
    for _ in range(30):
        env.rollout("random", 100, auto_reset=True)
        if int(env.rows.max()) > 1100:
            break
    assert 1100 < int(env.rows.max()) <= R
    twin = env.copy(); twin.accounting(False)
    policy = _policy(env.cols, (64, 64), 5)
    w = policy._deep_weights()
    s = torch.cuda.current_stream().cuda_stream
    u = torch.rand((T, B), device="cuda")
    want = _two_launch_reference(env, policy, u, R)
    assert max(int(r.max()) for r in want["rows"]) > 1024
    A = torch.zeros((T, B), dtype=torch.int32, device="cuda"); L = torch.zeros((T, B), dtype=torch.float32, device="cuda")
    Rw = torch.zeros((T, B), dtype=torch.float64, device="cuda"); D = torch.zeros((T, B), dtype=torch.uint8, device="cuda")
    N = torch.zeros((T, B), dtype=torch.int32, device="cuda")
    twin.policy2_rollout_device(w["prepared"], *w["hidden"], T, u, A, L, Rw, D, N, None, R, 0, s)
    twin.sync()
    for t in range(T):
        assert torch.equal(N[t], want["rows"][t]), t
        assert torch.equal(A[t], want["act"][t]) and torch.equal(L[t], want["logp"][t]), t
        assert torch.equal(Rw[t], want["rew"][t]) and torch.equal(D[t], want["done"][t]), t
    assert np.array_equal(env.stats()[:, :5], twin.stats()[:, :5])


@pytest.mark.gpu
def test_two_layer_rollout_refusals():
    """BBX_E_UNSUPPORTED, before anything runs, for a non-binomial class, a layer wider than 128 units, accounting on and a
    block taller than 2048 rows; run_rollout_fused refuses three hidden layers and _fused_weights() a two-layer policy (both
    used to run a different network without a word)."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv, _ffi
    from deepgroebner_amd.rollout import run_rollout_fused
    B, T = 8, 4
    s = torch.cuda.current_stream().cuda_stream

    def outs(R, cols):
        return (torch.rand((T, B), device="cuda"), torch.zeros((T, B), dtype=torch.int32, device="cuda"), torch.zeros((T, B), device="cuda"),
                torch.zeros((T, B, R, cols), dtype=torch.int32, device="cuda"))

    def refused(env, w, h1, h2, R, text=None):
        u, A, L, O = outs(R, env.cols)
        with pytest.raises(_ffi.BbxError) as ex:
            env.policy2_rollout_device(w["prepared"], h1, h2, T, u, A, L, None, None, None, O, R, 0, s)
        assert ex.value.code == -5, str(ex.value)
        assert text is None or str(ex.value).endswith(text), str(ex.value)

    cyc = VecLeadMonomialsEnv("cyclic-4", batch=B, k=2); cyc.reset(); cyc.accounting(False)
    w = _policy(cyc.cols, (64, 64), 1)._deep_weights()
    refused(cyc, w, 64, 64, 64)
    env = VecLeadMonomialsEnv("3-20-10-weighted", batch=B, k=2); env.seed(np.arange(B)); env.reset(); env.accounting(False)
    w = _policy(env.cols, (128, 128), 1)._deep_weights()
    refused(env, w, 256, 128, 64)
    refused(env, w, 128, 256, 64)
    refused(env, w, 128, 128, 2049, "the policy kernels score at most 2048 rows per environment (obs_rows = 2049)")
    env.accounting(True)
    refused(env, w, 128, 128, 64)
    env.accounting(False)
    st0, k0 = env.stats(), env.kernels_launched()
    with pytest.raises(_ffi.BbxError) as ex:
        run_rollout_fused(env, _policy(env.cols, (64, 64, 64), 1), T)
    assert ex.value.code == -5
    with pytest.raises(_ffi.BbxError):
        run_rollout_fused(env, _policy(env.cols, (256, 64), 1), T)
    with pytest.raises(ValueError):
        _policy(env.cols, (128, 128), 1)._fused_weights()
    assert env.kernels_launched() == k0 and np.array_equal(env.stats(), st0)
