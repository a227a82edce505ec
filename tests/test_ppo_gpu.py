"""The PPO call on the device: bbx_pmlp_ppo_grad[_at] / bbx_pmlp2_ppo_grad[_at], PMLPPolicy.ppo_step_at and ppo_update.
The contract (include/bbx.h): log-probabilities and entropies are those of bbx_pmlp[2]_logprob[_at], the gradients those of
bbx_pmlp[2]_grad[_at] fed with the coefficients the call wrote, bit for bit; the coefficients, the per-position terms and the
statistics are held to the float64 reference of tests/ppo_cases.py, the clip decisions and the counts exactly."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_cases as pc
from tests import ppo_cases as pp
from tests.test_policy_indexed_gpu import GUARD, SENTINEL, _banded, _bits, _grad, _hidden, _logprob, _policy, _prepared, _same_bits
from tests.fast_harness import ptr, stream_ptr, to_cuda

pytestmark = pytest.mark.gpu
_ids = lambda v: str(v).replace(" ", "")
S = pp.S
BAD = (-1, S, 2 ** 31 - 1)
STAT_THREADS = pp.header_constants()
MODES = (0, 1, 2)


def _ppo(weights, obs, rows, actions, old, adv, loss, index=None, outputs=True):
    """bbx_pmlp[2]_ppo_grad (index None) or ..._at through the C ABI: logprobs, entropy and coef between sentinel bands, the
    gradients between NaN bands, NaN behind the workspace and around the statistics.  A dict of numpy arrays; tail: the
    workspace's u | H | old - new | flags."""
    import torch
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    prep, keep = _prepared(weights)
    n_src, Rr, cols = obs.shape
    n = n_src if index is None else index.numel()
    h = _hidden(weights)
    (lp, ent, coef), check_out = _banded((n, n, 2 * n), SENTINEL)
    sizes = (cols * h[0], h[0], h[0], 1) if len(h) == 1 else (cols * h[0], h[0], h[0] * h[1], h[1], h[1], 1)
    grads, check_grads = _banded(sizes, float("nan"))
    name = "bbx_pmlp_ppo" if len(h) == 1 else "bbx_pmlp2_ppo"
    nfl = getattr(lib, name + "_workspace_floats")(n, Rr, cols, *h)
    gfl = getattr(lib, name.replace("_ppo", "_grad") + "_workspace_floats")(n, Rr, cols, *h)
    assert nfl == gfl + 4 * n and gfl > 0
    ws = torch.full((nfl + GUARD,), float("nan"), device="cuda")
    stats = torch.full((6 + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    mode, scale, eps, ent_coef, c_kl = loss.args()
    src = (ptr(obs), ptr(rows), ptr(actions)) + ((n,) if index is None else (n_src, ptr(index), n)) + (Rr, cols, prep) + tuple(h)
    fn = getattr(lib, name + "_grad" + ("" if index is None else "_at"))
    _ffi.check(fn(*src, ptr(old), ptr(adv), mode, C.c_float(scale), C.c_float(eps), C.c_float(ent_coef), C.c_float(c_kl),
                  ptr(lp) if outputs else None, ptr(ent) if outputs else None, ptr(coef), C.c_void_p(stats.data_ptr() + 8 * GUARD), ptr(ws),
                  *[ptr(g) for g in grads], stream_ptr()))
    torch.cuda.synchronize()
    host = ws.cpu().numpy()
    assert np.isnan(host[nfl:]).all(), "the workspace was overrun"
    st = stats.cpu().numpy()
    assert np.isnan(st[:GUARD]).all() and np.isnan(st[GUARD + 6:]).all(), "written around the statistics"
    lp, ent, coef = check_out()
    if not outputs:
        assert (lp == SENTINEL).all() and (ent == SENTINEL).all()
    tail = host[gfl:nfl]
    return {"logprobs": lp, "entropy": ent, "coef": coef, "grads": check_grads(), "stats": st[GUARD:GUARD + 6].copy(),
            "u": tail[:n].copy(), "H": tail[n:2 * n].copy(), "d": tail[2 * n:3 * n].copy(), "flags": tail[3 * n:].copy().view(np.int32)}


def _stat_bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _index(n, bad=True):
    """n positions over the S recorded states: every state, repeats, and (bad) entries out of range."""
    rng = np.random.default_rng(n + 40)
    index = np.resize(rng.permutation(S), n).astype(np.int64)
    if n > S:
        index[S:] = rng.integers(0, S, size=n - S)
    if bad and n > 8:
        index[[3, n // 2, n - 1]] = BAD
    return index.astype(np.int32)


def _inputs(cols, hidden, index, far=False):
    """(old, adv, float64 logprob / entropy / their bounds) for the positions of `index`: the ratios placed (or far)."""
    new64, H64, tol, etol = pp.reference_at(cols, hidden, index)
    old = pp.far_old(new64, cols) if far else pp.placed_old(new64, cols)[0]
    assert pp.distance_from_bounds(new64, old) >= pp.MARGIN
    return old, pp.advantages(len(index), cols), new64, H64, tol, etol


# ---- 1. the call is its parts, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cols,hidden", pp.ONE + pp.TWO, ids=_ids)
def test_call_equals_its_parts_bit_for_bit(cols, hidden, mode):
    w, obs, rows, actions = pp.source(cols, hidden)
    index = _index(3 * S + 1)
    old, adv, *_ = _inputs(cols, hidden, index)
    loss = pp.Loss(mode, len(index), c_kl=0.3)
    d_obs, d_rows, d_act, d_idx, d_old, d_adv = to_cuda(obs, rows, actions, index, old, adv)
    got = _ppo(w, d_obs, d_rows, d_act, d_old, d_adv, loss, d_idx)
    # logprobs / entropy: bbx_pmlp[2]_logprob_at's
    lp, ent = _logprob(w, d_obs, d_rows, d_act, d_idx)
    _same_bits((got["logprobs"], got["entropy"]), (lp, ent), "logprob_at")
    assert np.isnan(lp).sum() > 3 and (lp == 0).any()                 # bad indices, bad actions, a state without rows
    # gradients: bbx_pmlp[2]_grad_at's on the coefficients the call wrote
    n = len(index)
    d_gl, d_ge = to_cuda(got["coef"][:n], got["coef"][n:])
    _same_bits(got["grads"], _grad(w, d_obs, d_rows, d_act, d_gl, d_ge, d_idx), "grad_at on coef")
    if cols >= 12:
        assert any((g != 0).any() for g in got["grads"]) and all(np.isfinite(g).all() for g in got["grads"])
    # a second call: the same bits, statistics included; without the two optional outputs: the same everything else
    again = _ppo(w, d_obs, d_rows, d_act, d_old, d_adv, loss, d_idx, outputs=False)
    _same_bits([got["coef"], got["u"], got["H"], got["d"], got["flags"].view(np.float32)] + got["grads"],
               [again["coef"], again["u"], again["H"], again["d"], again["flags"].view(np.float32)] + again["grads"], "second call")
    assert np.array_equal(_stat_bits(got["stats"]), _stat_bits(again["stats"]))
    # the plain call on the gathered arrays (indices in range: an index out of range has no gathered counterpart)
    index = _index(3 * S + 1, bad=False)
    old, adv, *_ = _inputs(cols, hidden, index)
    d_idx, d_old, d_adv = to_cuda(index, old, adv)
    at = _ppo(w, d_obs, d_rows, d_act, d_old, d_adv, loss, d_idx)
    plain = _ppo(w, *to_cuda(obs[index], rows[index], actions[index]), d_old, d_adv, loss)
    for k in ("logprobs", "entropy", "coef", "u", "H", "d"):
        _same_bits((at[k],), (plain[k],), "gathered: " + k)
    assert np.array_equal(at["flags"], plain["flags"]) and np.array_equal(_stat_bits(at["stats"]), _stat_bits(plain["stats"]))
    _same_bits(at["grads"], plain["grads"], "gathered: gradients")
    lp0, ent0 = _logprob(w, *to_cuda(obs[index], rows[index], actions[index]))
    _same_bits((plain["logprobs"], plain["entropy"]), (lp0, ent0), "logprob")
    d_gl, d_ge = to_cuda(plain["coef"][:n], plain["coef"][n:])
    _same_bits(plain["grads"], _grad(w, *to_cuda(obs[index], rows[index], actions[index]), d_gl, d_ge), "grad on coef")


# ---- 2. coefficients, terms and statistics against float64 -------------------------------------------------------------------
def _check_against_float64(cols, hidden, mode, index, far, what):
    w, obs, rows, actions = pp.source(cols, hidden)
    old, adv, new64, H64, tol, etol = _inputs(cols, hidden, index, far)
    n = len(index)
    loss = pp.Loss(mode, n, c_kl=0.3)
    got = _ppo(w, *to_cuda(obs, rows, actions, old, adv), loss, to_cuda(index)[0])
    u64, gl64, ge64, clipped, counted, r64, d64 = pp.reference_loss(loss, new64, H64, old, adv)
    st64 = pp.reference_stats(loss, new64, H64, old, adv)
    gl, ge = got["coef"][:n].astype(np.float64), got["coef"][n:].astype(np.float64)
    ratio = pp.needed_ratio(loss, got["coef"][:n], got["u"], got["logprobs"], old, adv)
    print("ratios ppo %s mode=%d %s n=%d r_r=%.3f" % (pc.label(cols, hidden), mode, what, n, ratio))
    # exact: who counts, the clip decision, the three counts
    assert np.array_equal(got["flags"] & 1, counted.astype(np.int32)), "counted"
    assert np.array_equal((got["flags"] >> 1) & 1, clipped.astype(np.int32)), "clipped"
    assert np.array_equal(np.isnan(got["logprobs"]), ~counted)
    live = counted & (adv != 0)
    if mode == 1:
        assert np.array_equal(gl[live] == 0, clipped[live]), "gl == 0 exactly where the position is clipped"
    else:
        assert (gl[live] != 0).all() and not clipped.any()
    assert (gl[~counted] == 0).all() and (ge[~counted] == 0).all() and (got["u"][~counted] == 0).all()
    assert got["stats"][0] == st64[0] == counted.sum() and got["stats"][4] == st64[4] and got["stats"][5] == st64[5] == (~counted).sum()
    # within the bounds
    bg, bu, bd = pp.bounds(loss, new64, old, adv, tol)
    assert (np.abs(gl - gl64) <= bg).all(), ("gl", float((np.abs(gl - gl64) - bg).max()))
    assert (np.abs(got["u"] - u64) <= bu).all(), ("u", float((np.abs(got["u"] - u64) - bu).max()))
    assert (np.abs(ge - ge64) <= pp.EPS * np.abs(ge64)).all()
    Hc = np.where(counted, H64, 0.0)
    assert (np.abs(got["H"] - Hc) <= np.where(counted, etol, 0.0)).all()
    assert (np.abs(got["d"] - np.where(counted, -d64, 0.0)) <= bd).all()
    for i, bound in ((1, bu.sum()), (2, np.where(counted, etol, 0.0).sum()), (3, bd.sum())):
        assert abs(got["stats"][i] - st64[i]) <= bound, (i, got["stats"][i], st64[i], bound)
    # the statistics ARE the double sums of the float32 terms the call wrote (any order of adding n <= 2^12 doubles: 2^-40 relative)
    for i, term in ((1, got["u"]), (2, got["H"]), (3, got["d"])):
        t = term[counted].astype(np.float64)
        assert abs(got["stats"][i] - t.sum()) <= 2.0 ** -40 * np.abs(t).sum()
    return got, ratio


@pytest.mark.parametrize("far", [False, True], ids=["placed", "far"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cols,hidden", pp.ONE + pp.TWO, ids=_ids)
def test_coefficients_terms_and_statistics_against_float64(cols, hidden, mode, far):
    got, ratio = _check_against_float64(cols, hidden, mode, _index(3 * S + 1), far, "far" if far else "placed")
    assert ratio <= pp.C_R, ratio                                      # (the epilogue's own arithmetic, inside its share of the bounds)
    if mode == 1 and not far:
        assert got["stats"][4] > 0 and got["stats"][4] < got["stats"][0]


@pytest.mark.parametrize("n", pp.STAT_THREADS_NS(STAT_THREADS))
@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (12, (128, 128))], ids=_ids)
def test_statistics_around_the_partition_boundaries(cols, hidden, n):
    """n = 0, 1 and just below, at and above what one pass of the statistics kernel's threads covers."""
    import torch
    w, obs, rows, actions = pp.source(cols, hidden)
    if n == 0:
        empty = torch.zeros(0, dtype=torch.int32, device="cuda"); none = torch.zeros(0, device="cuda")
        for index in (empty, None):
            src = to_cuda(obs, rows, actions) if index is not None else (torch.zeros((0,) + obs.shape[1:], dtype=torch.int32, device="cuda"), empty, empty)
            got = _ppo(w, *src, none, none, pp.Loss(1, 0), index)
            assert (got["stats"] == 0).all() and all((g == 0).all() for g in got["grads"])
        return
    got, ratio = _check_against_float64(cols, hidden, 1, _index(n), False, "partition")
    assert got["stats"][0] + got["stats"][5] == n


# ---- 3. the first epoch, exactly -------------------------------------------------------------------------------------------------
N1, SCALE1, ENT1 = 64, 2.0 ** -6, 2.0 ** -7


def _first_epoch_index():
    """64 positions over the recorded states whose action lies inside the live rows (or that have no row at all)."""
    w, obs, rows, actions = pp.source(12, (128,))
    live = np.clip(rows, 0, pp.R)
    fine = np.flatnonzero((live == 0) | ((actions >= 0) & (actions < live)))
    return np.resize(np.random.default_rng(50).permutation(fine), N1).astype(np.int32)


@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (64, (256,)), (12, (128, 128)), (33, (65, 64))], ids=_ids)
def test_first_epoch_coefficients_are_exact(cols, hidden):
    """old_logprobs are what bbx_pmlp[2]_logprob_at just returned: r = 1, and every counted gl is -(scale A), bit for bit."""
    w, obs, rows, actions = pp.source(cols, hidden)
    index = _index(N1)
    d_obs, d_rows, d_act, d_idx = to_cuda(obs, rows, actions, index)
    lp, ent = _logprob(w, d_obs, d_rows, d_act, d_idx)
    old = np.nan_to_num(lp, nan=0.0).astype(np.float32)
    adv = pp.advantages(N1, cols)
    for mode in (1, 2):
        loss = pp.Loss(mode, N1, ent_coef=ENT1, c_kl=0.0, scale=SCALE1)
        got = _ppo(w, d_obs, d_rows, d_act, *to_cuda(old, adv), loss, d_idx)
        counted = ~np.isnan(lp)
        want = -(np.float32(SCALE1) * adv)
        assert counted.sum() >= N1 - 8 and (~counted).any()
        assert np.array_equal(_bits(got["coef"][:N1][counted]), _bits(want[counted]))
        assert (got["coef"][N1:][counted] == np.float32(-(SCALE1 * ENT1))).all()
        assert (got["coef"][:N1][~counted] == 0).all() and (got["coef"][N1:][~counted] == 0).all()
        assert np.array_equal(_bits(got["u"][counted]), _bits(adv[counted])) and (got["d"] == 0).all()
        assert got["stats"][3] == 0 and got["stats"][4] == 0
        assert abs(got["stats"][1] - adv[counted].astype(np.float64).sum()) <= 2.0 ** -40 * np.abs(adv).sum()


def _clipped_loss(logp, ent, old, adv, ent_coef):
    import torch
    ratio = torch.exp(logp - old)
    return -torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean() - ent_coef * ent.mean()


@pytest.mark.parametrize("hidden", [(128,), (128, 128)], ids=_ids)
def test_first_epoch_ppo_step_at_leaves_the_gradients_of_the_autograd_loss(hidden):
    import torch
    w, obs, rows, actions = pp.source(12, hidden)
    index = _first_epoch_index()
    st, rw, act, idx = to_cuda(obs, rows, actions, index)
    adv = to_cuda(pp.advantages(N1, 3))[0]
    pol, ref = _policy(w), _policy(w)
    with torch.no_grad():
        old, _ = ref.evaluate_at(st, act, rw, idx)
    assert torch.isfinite(old).all()
    logp, ent = ref.evaluate_at(st, act, rw, idx)
    assert type(logp.grad_fn).__name__.startswith("_PMLPEvaluate" if len(hidden) == 1 else "_PMLP2Evaluate")
    _clipped_loss(logp, ent, old, adv, ENT1).backward()
    stats, lp, en = pol.ppo_step_at(st, act, rw, idx, old, adv, clip=0.2, ent_coef=ENT1)
    assert torch.equal(lp.view(torch.int32), logp.detach().view(torch.int32)) and torch.equal(en.view(torch.int32), ent.detach().view(torch.int32))
    for (name, a), b in zip(pol.named_parameters(), ref.parameters()):
        assert a.grad is not None and a.grad.shape == a.shape and a.grad.is_contiguous(), name
        assert torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32)), name
    assert any(float(q.grad.abs().max()) > 0 for q in pol.parameters())
    s = stats.cpu().numpy()
    assert s[0] == N1 and s[3] == 0 and s[4] == 0 and s[5] == 0
    assert abs(s[2] - float(ent.detach().double().sum())) <= 2.0 ** -40 * float(ent.detach().double().abs().sum())
    # a second call adds, as backward() would; the gathered form leaves the same bits
    pol.ppo_step_at(st, act, rw, idx, old, adv, clip=0.2, ent_coef=ENT1)
    assert all(torch.equal(a.grad, 2 * b.grad) for a, b in zip(pol.parameters(), ref.parameters()))
    pol.zero_grad(set_to_none=True)
    j = idx.long()
    pol.ppo_step(st[j], act[j], rw[j], old, adv, clip=0.2, ent_coef=ENT1)
    assert all(torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32)) for a, b in zip(pol.parameters(), ref.parameters()))


# ---- 4. ppo_update -------------------------------------------------------------------------------------------------------------
def _buffer_of_64(pol):
    """8 steps of 8 environments, every episode complete, every state with 2 .. 33 rows and an action inside them; the recorded
    log-probabilities are the policy's own (the first epoch: r = 1)."""
    import torch
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer
    T = B = 8
    rng = np.random.default_rng(61)
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(33, 12))
    rows = np.resize(np.array((33, 2, 17, 32, 5, 31, 9, 20, 3), dtype=np.int32), T * B).reshape(T, B)
    st = pc.fill_padding(pc.random_blocks(T * B, 33, 12, 62), rows.reshape(-1), False).reshape(T, B, 33, 12)
    done = np.zeros((T, B), dtype=bool); done[T - 1] = True; done[3, ::2] = True
    buf.states.copy_(torch.from_numpy(st)); buf.rows.copy_(torch.from_numpy(rows)); buf.dones.copy_(torch.from_numpy(done))
    buf.actions.copy_(torch.from_numpy((rng.integers(0, 1 << 30, size=(T, B)) % rows).astype(np.int32)))
    buf.rewards.copy_(torch.from_numpy(-rng.integers(1, 30, size=(T, B)).astype(np.float64)))
    buf.values.copy_(torch.from_numpy(rng.normal(size=(T, B))))
    buf.t = T
    with torch.no_grad():
        lp, _ = pol.evaluate_at(buf.states, buf.actions, buf.rows, torch.arange(T * B, dtype=torch.int32, device="cuda"))
    buf.logprobs.copy_(lp.view(T, B))
    return buf


@pytest.mark.parametrize("hidden", [(128,), (128, 128)], ids=_ids)
def test_ppo_update_equals_the_hand_written_loop_bit_for_bit(hidden):
    import torch
    from deepgroebner_amd.rollout import ppo_update
    w = pc.make_weights(12, hidden, 63)
    pol, ref = _policy(w), _policy(w)
    buf = _buffer_of_64(ref)
    idx, act, old, adv, _ = buf.get_index()
    assert idx.numel() == N1
    opt_ref = torch.optim.SGD(ref.parameters(), lr=0.05)
    opt_ref.zero_grad()
    logp, ent = ref.evaluate_at(buf.states, buf.actions, buf.rows, idx)
    _clipped_loss(logp, ent, old, adv, ENT1).backward()
    opt_ref.step()
    out = ppo_update(pol, buf, torch.optim.SGD(pol.parameters(), lr=0.05), epochs=1, batch_size=N1, clip=0.2, ent_coef=ENT1, shuffle=False)
    for (name, a), b in zip(pol.named_parameters(), ref.parameters()):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), name
    assert not torch.equal(pol.embedding[0].bias.detach().cpu(), torch.from_numpy(w[0][1]))      # (the step moved the weights)
    assert len(out) == 1 and out[0]["stats"].shape == (1, 6) and out[0]["stats"][0, 0] == N1 and out[0]["kl"] == 0 and out[0]["clip_frac"] == 0


def test_ppo_update_on_a_real_rollout_with_adam():
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, ppo_update, run_rollout_fused
    torch.manual_seed(5)
    B, T = 8, 40
    env = VecLeadMonomialsEnv("3-20-10-weighted", batch=B, k=2)
    env.seed(np.arange(B) + 11); env.reset()
    policy = PMLPPolicy(env.cols, [128]).cuda()
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(256, env.cols))
    run_rollout_fused(env, policy, T, buffer=buf)
    n = int(buf.get_index()[0].numel())
    assert n > B
    before = [q.detach().clone() for q in policy.parameters()]
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    out = ppo_update(policy, buf, torch.optim.Adam(policy.parameters(), lr=1e-3), epochs=2, batch_size=64, ent_coef=0.01, generator=gen)
    assert len(out) == 2
    for o in out:
        assert o["stats"].shape == ((n + 63) // 64, 6) and np.isfinite(o["stats"]).all() and o["stats"][:, 0].sum() == n and o["stats"][:, 5].sum() == 0
        assert np.isfinite([o["loss"], o["entropy"], o["kl"], o["clip_frac"]]).all() and o["entropy"] > 0
    assert abs(out[0]["stats"][0, 3]) < 1e-6 * 64                     # the first minibatch of the first epoch: the rollout's own weights
    assert all(torch.isfinite(q).all() for q in policy.parameters()) and any(not torch.equal(a, b) for a, b in zip(before, policy.parameters()))
