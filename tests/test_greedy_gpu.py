"""Greedy policy actions in every policy kernel and per-episode returns on the device: bbx_pmlp_act_greedy / bbx_pmlp2_act_greedy /
bbx_pmlp3_act_greedy against the float64 reference of tests/policy_cases.py and, bit for bit, against the training kernels'
log-probabilities; ties, no rows; bbx_policy_greedy on the rollouts inside the step kernels against the per-step composition
they stand for; a zero-weight greedy policy against the First strategy; bbx_episodes_device against the CPU loop; and
evaluate_policy on a list of ideals against strategy_stats."""
import ctypes as C

import numpy as np
import pytest

from tests import greedy_cases as gc
from tests import policy_cases as pc

pytestmark = pytest.mark.gpu
_ids = lambda v: str(v).replace(" ", "")


def _greedy(pol, obs, rows):
    """PMLPPolicy.act(greedy=True) through the HIP kernel of the policy's depth (never the torch path); sentinels in the outputs."""
    import torch
    cols, R = obs.shape[2], obs.shape[1]
    hidden = [l.out_features for l in pol.embedding]
    assert (len(hidden) == 1 and pol.fused_ok(cols, hidden[0]) and R <= 2048) or (pol.deep_ok(cols) and R <= pol.deep_max_rows()), "no kernel for this case"
    a = torch.full((obs.shape[0],), -7, dtype=torch.int32, device="cuda"); l = torch.full((obs.shape[0],), float("nan"), device="cuda")
    pol.act(obs, rows, None, a, l, greedy=True)
    torch.cuda.synchronize()
    return a, l


def _logprob_kernel(pol, obs, rows, actions):
    """bbx_pmlp_logprob / bbx_pmlp2_logprob of `actions` on the same prepared weights the act kernels read."""
    import torch
    from deepgroebner_amd import _ffi
    n, R, cols = obs.shape
    out = torch.full((n,), float("nan"), device="cuda"); ent = torch.zeros(n, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if len(pol.embedding) == 1:
        w = pol._fused_weights()
        _ffi.check(_ffi.lib().bbx_pmlp_logprob(p(obs), p(rows), p(actions), n, R, cols, w["prepared"], w["hidden"], p(out), p(ent), s))
    else:
        w = pol._deep_weights()
        _ffi.check(_ffi.lib().bbx_pmlp2_logprob(p(obs), p(rows), p(actions), n, R, cols, w["prepared"], w["hidden"][0], w["hidden"][1], p(out), p(ent), s))
    return out


# ---- 1. parity with float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", gc.SEEDS)
@pytest.mark.parametrize("cols,hidden", gc.SHAPES, ids=_ids)
def test_greedy_pick_against_the_float64_reference(cols, hidden, seed):
    """Every state of the case: the pick's reference logit is within 2 tol of the reference maximum (tol: the project's C_L
    bound), its log-probability within tol of the reference's; where exactly one row passes, the pick is the reference argmax.
    The share of such states is asserted too (and, on the reference alone, in tests/test_greedy_cpu.py)."""
    import torch
    case = gc.parity_case(cols, hidden, seed)
    pol = pc.to_policy(case.weights, "cuda")
    a, l = _greedy(pol, torch.from_numpy(case.obs).cuda(), torch.from_numpy(case.rows).cuda())
    a = a.cpu().numpy().astype(np.int64); l = l.cpu().numpy().astype(np.float64)
    e = np.arange(gc.B)
    assert ((a >= 0) & (a < case.ref.n)).all(), a[(a < 0) | (a >= case.ref.n)][:5]
    lg = np.where(np.isnan(case.ref.logits), -np.inf, case.ref.logits)
    gap = lg.max(axis=1) - lg[e, a]
    lerr = np.abs(l - case.ref.logsm[e, a])
    print("greedy %s seed %d: decided %.3f, largest gap / tol %.3f, largest |logprob error| / tol %.3f, picks off the argmax %d" %
          (pc.label(cols, hidden), seed, case.share, float((gap / case.ref.tol()).max()), float((lerr / case.ref.tol()).max()), int((a != case.argmax).sum())))
    assert case.share >= gc.SHARE_MIN[len(hidden)], case.share
    assert case.passing[e, a].all(), ("pick more than 2 tol behind the maximum", np.flatnonzero(~case.passing[e, a])[:5].tolist())
    assert (a[case.decided] == case.argmax[case.decided]).all()
    assert (lerr <= case.ref.tol()).all(), float((lerr / case.ref.tol()).max())


# ---- 2. consistent with the training kernels, no tolerance ------------------------------------------------------------------
@pytest.mark.parametrize("cols,hidden", gc.LOGPROB_SHAPES, ids=_ids)
def test_greedy_logprob_is_the_logprob_kernels_maximum_bit_for_bit(cols, hidden):
    """d_logprobs of *_act_greedy == bbx_pmlp[2]_logprob of the picked action, bit for bit; and the log-probability kernel's
    values for EVERY action a < n have the greedy one as their maximum (the pick is the kernels' own argmax), the pick the
    first action that reaches it."""
    import torch
    case = gc.parity_case(cols, hidden, gc.SEEDS[0])
    pol = pc.to_policy(case.weights, "cuda")
    obs = torch.from_numpy(case.obs).cuda(); rows = torch.from_numpy(case.rows).cuda()
    a, l = _greedy(pol, obs, rows)
    assert torch.equal(_logprob_kernel(pol, obs, rows, a), l)
    n = rows.to(torch.int64)
    every = torch.stack([_logprob_kernel(pol, obs, rows, torch.minimum(torch.full_like(rows, j), rows - 1)) for j in range(gc.R)])   # [R, B]
    live = torch.arange(gc.R, device="cuda")[:, None] < n[None, :]
    every = torch.where(live, every, torch.full_like(every, float("-inf")))
    assert torch.equal(every.max(dim=0).values, l)
    first = (every == l[None, :]).to(torch.int64).argmax(dim=0)
    assert torch.equal(first.to(torch.int32), a)


# ---- 3. ties go to the first row; 4. no rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,hidden", gc.SHAPES, ids=_ids)
def test_ties_go_to_the_first_row_and_no_rows_give_action_zero(cols, hidden):
    import torch
    w = pc.make_weights(cols, hidden, 11)
    pol = pc.to_policy(w, "cuda")
    counts = (1, 2, 64, 65, 129)
    R = 130
    row = pc.random_blocks(1, 1, cols, 12)[0, 0]
    obs = np.full((len(counts) + 3, R, cols), -1, dtype=np.int32)
    rows = np.zeros(len(counts) + 3, dtype=np.int32)
    for i, n in enumerate(counts):                          # every live row the same
        obs[i, :n] = row; rows[i] = n
    # the best row of a random block duplicated at rows 3 and 67 (and nowhere else at that logit)
    blk = pc.random_blocks(1, R, cols, 13)
    lg = pc.reference(w, blk, [R]).logits[0]
    best = int(np.argmax(lg))
    assert (lg == lg[best]).sum() == 1
    k = len(counts)
    top = blk[0, best].copy()
    obs[k] = blk[0]
    if best not in (3, 67):
        obs[k, best] = blk[0, (best + 1) % R]                # (a lower-scoring row in its place)
    obs[k, 3] = top; obs[k, 67] = top; rows[k] = R
    lg2 = pc.reference(w, obs[k:k + 1], [R]).logits[0]
    ref2 = pc.reference(w, obs[k:k + 1], [R])
    assert sorted(np.flatnonzero(lg2 == lg2.max()).tolist()) == [3, 67]
    assert lg2.max() - np.delete(lg2, [3, 67]).max() > 2.0 * ref2.tol()[0]   # (no third row within the kernels' error of the two)
    obs[k + 1] = blk[0]; rows[k + 1] = 0                     # no rows: action 0, log-probability 0.0f
    obs[k + 2] = blk[0]; rows[k + 2] = -3
    a, l = _greedy(pol, torch.from_numpy(obs).cuda(), torch.from_numpy(rows).cuda())
    a = a.cpu().numpy(); l = l.cpu().numpy()
    assert a[:k].tolist() == [0] * k, a[:k]
    ref = pc.reference(w, obs, rows)
    assert (np.abs(l[:k] - (-np.log(counts))) <= ref.tol()[:k]).all()   # (n equal terms: log-probability -log n, within the project's bound)
    assert a[k] == 3
    assert a[k + 1] == 0 and l[k + 1] == 0.0 and a[k + 2] == 0 and l[k + 2] == 0.0
    # all weights zero: every logit equal, action 0 everywhere
    wz = [(np.zeros_like(W), np.zeros_like(b)) for W, b in w]
    zero = pc.to_policy(wz, "cuda")
    rows2 = np.resize(np.array(gc.LIVE, dtype=np.int32), 24)
    blocks = pc.random_blocks(24, gc.R, cols, 14)
    a0, l0 = _greedy(zero, torch.from_numpy(blocks).cuda(), torch.from_numpy(rows2).cuda())
    assert (a0 == 0).all()
    assert (np.abs(l0.cpu().numpy() - (-np.log(rows2))) <= pc.reference(wz, blocks, rows2).tol()).all()


# ---- 5. rollouts with the switch on equal the per-step composition ------------------------------------------------------------
def _policy(cols, hidden, seed):
    import torch
    from deepgroebner_amd.rollout import PMLPPolicy
    torch.manual_seed(seed)
    policy = PMLPPolicy(cols, list(hidden)).cuda()
    with torch.no_grad():
        for lin in list(policy.embedding) + [policy.deciding]:
            lin.weight.mul_(0.3)
    return policy


def _outs(T, B):
    import torch
    return {"act": torch.full((T, B), -7, dtype=torch.int32, device="cuda"), "logp": torch.full((T, B), float("nan"), device="cuda"),
            "rew": torch.zeros((T, B), dtype=torch.float64, device="cuda"), "done": torch.zeros((T, B), dtype=torch.uint8, device="cuda"),
            "rows": torch.zeros((T, B), dtype=torch.int32, device="cuda")}


def _fused(env, policy, T, R, u):
    """T steps inside the step kernels (one or two hidden layers), every per-step output kept."""
    import torch
    o = _outs(T, env.batch)
    obs = torch.empty((env.batch, R, env.cols), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if len(policy.embedding) == 1:
        w = policy._fused_weights()
        env.policy_rollout_device(w["prepared"], w["hidden"], T, u, o["act"], o["logp"], o["rew"], o["done"], o["rows"], obs, R, 0, s)
    else:
        w = policy._deep_weights()
        env.policy2_rollout_device(w["prepared"], w["hidden"][0], w["hidden"][1], T, u, o["act"], o["logp"], o["rew"], o["done"], o["rows"], obs, R, 0, s)
    env.sync()
    return o


def _per_step(env, policy, T, R, greedy, u=None, one_call=False):
    """The composition a rollout stands for: *_act[_greedy] on the padded block, then bbx_step_device_autoreset, step by step — or
    (one_call) bbx_policy_step_device, whose mode is the handle's switch."""
    import torch
    B = env.batch
    o = _outs(T, B)
    s = torch.cuda.current_stream().cuda_stream
    obs = torch.full((B, R, env.cols), -1, dtype=torch.int32, device="cuda")
    rew = torch.zeros(B, dtype=torch.float64, device="cuda"); done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(B, dtype=torch.int32, device="cuda"); act = torch.zeros(B, dtype=torch.int32, device="cuda")
    logp = torch.zeros(B, dtype=torch.float32, device="cuda")
    env.rollout_device("first", 0, False, s, rew, done, rows, obs, R, True, False); env.sync()
    w = policy._fused_weights() if one_call else None
    for t in range(T):
        o["rows"][t].copy_(rows)
        if one_call:
            env.policy_step_device(w["prepared"], w["hidden"], None if u is None else u[t], act, logp, rew, done, rows, obs, R, 2, s)
        else:
            policy.act(obs, rows, None if u is None else u[t], act, logp, greedy=greedy)
            env.step_device(act, rew, done, rows, obs, R, 1, s, auto_reset=True)
        env.sync()
        for k, v in (("act", act), ("logp", logp), ("rew", rew), ("done", done)):
            o[k][t].copy_(v)
    return o


def _same(x, y, what):
    import torch
    for k in ("rows", "act", "logp", "rew", "done"):
        assert torch.equal(x[k], y[k]), (what, k, int((x[k] != y[k]).sum()))


@pytest.mark.parametrize("dist,hidden", [("3-20-10-weighted", (128,)), ("3-20-10-weighted", (64, 64)), ("5-10-5-uniform", (128,)),
                                         ("5-10-5-uniform", (64, 64))], ids=_ids)
def test_greedy_rollout_equals_greedy_act_then_step(dist, hidden):
    """bbx_policy_rollout_device / bbx_policy2_rollout_device with bbx_policy_greedy on (register/LDS class and HBM-resident binomial
    class) against *_act_greedy + bbx_step_device_autoreset on a same-seeded handle, step by step: actions, log-probabilities,
    rewards, dones and rows identical; the same through bbx_policy_step_device with the switch on (one layer); d_u is ignored
    (random, or NULL); and with the switch off again a sampled rollout equals one on a handle that never had it on."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    B, T, T2, k = 70, 40, 12, 2
    R = 256 if dist.startswith("3-") else 1024
    env = VecLeadMonomialsEnv(dist, batch=B, k=k)
    env.seed(np.arange(B) + 500); env.reset(); env.accounting(False)
    plain = env.copy(); other_u = env.copy(); stepper = env.copy()
    policy = _policy(env.cols, hidden, 6)
    want = _per_step(plain, policy, T, R, greedy=True)       # (`plain` never has the switch on)
    assert env.policy_greedy(True) is False
    got = _fused(env, policy, T, R, None)                    # d_u == NULL
    _same(got, want, "fused greedy rollout against act_greedy + step")
    assert int((got["act"] > 0).sum()) > 0
    if dist.startswith("3-"):                                # (episodes of 5-10-5-uniform outlast the 40 steps)
        assert int(got["done"].sum()) > 0
    assert np.array_equal(env.stats()[:, :5], plain.stats()[:, :5])
    other_u.policy_greedy(True)
    _same(_fused(other_u, policy, T, R, torch.rand((T, B), device="cuda")), got, "greedy rollouts with different d_u")
    if len(hidden) == 1:
        stepper.policy_greedy(True)
        _same(_per_step(stepper, policy, T, R, greedy=True, one_call=True), want, "bbx_policy_step_device with the switch on")
    # the switch off again: the draws of a handle that never had it on
    assert env.policy_greedy(False) is True
    u = torch.rand((T2, B), device="cuda")
    _same(_fused(env, policy, T2, R, u), _fused(plain, policy, T2, R, u), "sampled rollout after the switch went off")
    assert np.array_equal(env.stats()[:, :5], plain.stats()[:, :5])


# ---- 6. zero-weight greedy is the First strategy -------------------------------------------------------------------------------
def test_zero_weight_greedy_rollout_is_the_first_strategy():
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, episode_returns, run_rollout_fused
    B, T = 70, 64
    env = VecLeadMonomialsEnv("3-20-10-weighted", batch=B, k=2)
    env.seed(np.arange(B) + 900); env.reset(); env.accounting(False)
    twin = env.copy()
    policy = PMLPPolicy(env.cols, [64]).cuda()
    with torch.no_grad():
        for prm in policy.parameters():
            prm.zero_()
    st0 = env.stats()
    buf = DeviceTrajectoryBuffer(T, B)
    run_rollout_fused(env, policy, T, buffer=buf, chunk=T, greedy=True)
    assert env.policy_greedy(False) is False                 # (restored by the call)
    twin.rollout_device("first", T, True, torch.cuda.current_stream().cuda_stream); twin.sync()
    d, dt = env.stats() - st0, twin.stats() - st0
    assert np.array_equal(d[:, :3], dt[:, :3]) and (d[:, 0] == T).all() and d[:, 2].sum() > 0
    assert int((buf.actions != 0).sum()) == 0
    cret = torch.zeros(B, dtype=torch.float64, device="cuda"); clen = torch.zeros(B, dtype=torch.int32, device="cuda")
    count = torch.zeros(B, dtype=torch.int32, device="cuda")
    ep_ret, ep_len = episode_returns(buf.rewards, buf.dones, (cret, clen, count))
    assert np.array_equal(-(ep_ret.sum(dim=0) + cret).cpu().numpy(), d[:, 1].astype(np.float64))
    assert np.array_equal(count.cpu().numpy(), d[:, 2]) and np.array_equal((ep_len.sum(dim=0) + clen).cpu().numpy(), d[:, 0])


# ---- 7. bbx_episodes_device against the CPU loop -------------------------------------------------------------------------------
def test_episodes_kernel_equals_the_cpu_loop_in_one_call_and_in_chunks():
    import torch
    from deepgroebner_amd.rollout import episode_returns
    T, B = 33, 70
    r, d = gc.random_episode_block(T, B, 21)
    d[:, 5] = False                                          # an environment that finishes nothing
    rt, dt = torch.from_numpy(r), torch.from_numpy(d)
    want_ret, want_len = episode_returns(rt, dt)             # the torch loop on CPU tensors
    sc = gc.episodes_scalar(r, d)
    assert np.array_equal(want_ret.numpy(), sc[0]) and np.array_equal(want_len.numpy(), sc[1])
    rg, dg = rt.cuda(), dt.cuda()
    got_ret, got_len = episode_returns(rg, dg)               # NULL carries
    assert torch.equal(got_ret.cpu(), want_ret) and torch.equal(got_len.cpu(), want_len)
    got_ret8, _ = episode_returns(rg, dg.to(torch.uint8))
    assert torch.equal(got_ret8, got_ret)
    carry = (torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"),
             torch.zeros(B, dtype=torch.int32, device="cuda"))
    parts = [episode_returns(rg[a:b].contiguous(), dg[a:b].contiguous(), carry) for a, b in ((0, 7), (7, 20), (20, 33))]
    assert torch.equal(torch.cat([p[0] for p in parts]).cpu(), want_ret) and torch.equal(torch.cat([p[1] for p in parts]).cpu(), want_len)
    assert np.array_equal(carry[0].cpu().numpy(), sc[2]) and np.array_equal(carry[1].cpu().numpy(), sc[3]) and np.array_equal(carry[2].cpu().numpy(), sc[4])
    only = (carry[0], carry[1], None)                        # a NULL d_ep_count is allowed
    episode_returns(rg[:0], dg[:0], only)                    # nsteps == 0: legal, nothing changes
    assert np.array_equal(carry[0].cpu().numpy(), sc[2]) and np.array_equal(carry[1].cpu().numpy(), sc[3])


# ---- 8. evaluate_policy ----------------------------------------------------------------------------------------------------------
def test_evaluate_policy_on_a_list_of_ideals_equals_strategy_stats():
    """140 ideals of 3-20-10-weighted on a list handle of 70 environments, two episodes each, a zero-weight policy (greedy = the
    First strategy): returns[e, j] = -PolynomialAdditions of ideal e + j * B; max_steps = 3 leaves NaN / -1 where nothing finished."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv, parse_ideal_dist, strategy_stats
    from deepgroebner_amd.rollout import PMLPPolicy, evaluate_policy
    B, K = 70, 2
    g = parse_ideal_dist("3-20-10-weighted"); g.seed(4242)
    ideals = [next(g) for _ in range(B * K)]
    want = strategy_stats(ideals, "first")[:, 2].astype(np.float64)
    assert (want > 0).all()
    env = VecLeadMonomialsEnv(ideals, batch=B, k=2, caps={"queue_slots": 16})
    policy = PMLPPolicy(env.cols, [64]).cuda()
    with torch.no_grad():
        for prm in policy.parameters():
            prm.zero_()
    ev = evaluate_policy(env, policy, K, greedy=True, chunk=16)
    assert ev.complete is True and ev.steps % 16 == 0
    assert ev.returns.shape == (B, K) and ev.returns.dtype == torch.float64 and ev.lengths.shape == (B, K) and ev.lengths.dtype == torch.int32
    assert bool((ev.lengths > 0).all())
    e, j = np.meshgrid(np.arange(B), np.arange(K), indexing="ij")
    assert np.array_equal(ev.returns.cpu().numpy(), -want[e + j * B])
    env = VecLeadMonomialsEnv(ideals, batch=B, k=2, caps={"queue_slots": 16})   # (a fresh handle: the list starts over)
    short = evaluate_policy(env, policy, K, greedy=True, chunk=16, max_steps=3)
    assert short.complete is False and short.steps == 3
    ret, ln = short.returns.cpu().numpy(), short.lengths.cpu().numpy()
    missing = ln == -1
    assert missing.any() and np.isnan(ret[missing]).all() and not np.isnan(ret[~missing]).any()
    assert np.array_equal(ret[~missing], (-want[e + j * B])[~missing]) and (ln[~missing] <= 3).all()
