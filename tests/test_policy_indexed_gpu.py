"""The indexed training kernels (bbx_pmlp_logprob_at / bbx_pmlp_grad_at and the two-layer pair), DeviceTrajectoryBuffer.get_index
and PMLPPolicy.evaluate_at on the device.  The contract is bit-equality with the calls without _at on the gathered contiguous
arrays obs[index], rows[index], actions[index]; one float64 check per depth holds the new entries to the reference itself."""
import functools

import numpy as np
import pytest

from tests import policy_cases as pc
from tests import policy_grad_cases as gc
from tests import policy2_grad_cases as g2
from tests.fast_harness import ptr, stream_ptr, to_cuda

pytestmark = pytest.mark.gpu
_ids = lambda v: str(v).replace(" ", "")
GUARD = 64
SENTINEL = 7.0

ONE = [(1, (1,)), (12, (128,)), (33, (65,)), (64, (256,))]
TWO = [(12, (128, 128)), (33, (65, 64)), (1, (1, 1))]
S, R = 37, 40
ROWS = (33, 0, 40, 1, 2, 45, -3, 17, 31, 32)      # the tile of 32 and around it, none, one, more than obs_rows


def _hidden(weights):
    return [W.shape[1] for W, _ in weights[:-1]]


def _policy(weights):
    pol = pc.to_policy(weights, "cuda")
    pol.deep_kernels = True
    return pol


def _prepared(weights):
    pol = _policy(weights)
    return (pol._fused_weights() if len(weights) == 2 else pol._deep_weights())["prepared"], pol


def _banded(sizes, fill):
    """Buffers of `sizes` floats inside one allocation with guard bands of `fill` around each; (views, check): check() returns the
    buffers as numpy after asserting that the bands still hold `fill`."""
    import torch
    buf = torch.full((sum(sizes) + (len(sizes) + 1) * GUARD,), fill, device="cuda")
    offs = np.cumsum([GUARD] + [s + GUARD for s in sizes[:-1]])
    views = [buf[int(o):int(o) + s] for o, s in zip(offs, sizes)]

    def check():
        host = buf.cpu().numpy()
        inside = np.zeros(len(host), dtype=bool)
        for o, s in zip(offs, sizes):
            inside[int(o):int(o) + s] = True
        band = host[~inside]
        assert (np.isnan(band).all() if np.isnan(fill) else (band == fill).all()), "a guard band was written"
        return [host[int(o):int(o) + s].copy() for o, s in zip(offs, sizes)]
    return views, check


def _logprob(weights, obs, rows, actions, index=None, entropy=True):
    """bbx_pmlp[2]_logprob (index None) or bbx_pmlp[2]_logprob_at through the C ABI; the outputs between sentinel bands;
    (logprobs, entropy or None) as numpy."""
    import torch
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    prep, keep = _prepared(weights)
    n_src, Rr, cols = obs.shape
    n = n_src if index is None else index.numel()
    (lp, ent), check = _banded((n, n), SENTINEL)
    name = "bbx_pmlp_logprob" if len(weights) == 2 else "bbx_pmlp2_logprob"
    if index is None:
        _ffi.check(getattr(lib, name)(ptr(obs), ptr(rows), ptr(actions), n, Rr, cols, prep, *_hidden(weights), ptr(lp), ptr(ent) if entropy else None, stream_ptr()))
    else:
        _ffi.check(getattr(lib, name + "_at")(ptr(obs), ptr(rows), ptr(actions), n_src, ptr(index), n, Rr, cols, prep, *_hidden(weights), ptr(lp),
                                              ptr(ent) if entropy else None, stream_ptr()))
    torch.cuda.synchronize()
    lp, ent = check()
    if not entropy:
        assert (ent == SENTINEL).all()
    return lp, (ent if entropy else None)


def _grad(weights, obs, rows, actions, glogp, gent, index=None):
    """bbx_pmlp[2]_grad or ..._grad_at through the C ABI, the outputs inside one buffer with NaN guard bands between them and
    behind the workspace; the gradients as numpy (flat)."""
    import torch
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    prep, keep = _prepared(weights)
    n_src, Rr, cols = obs.shape
    n = n_src if index is None else index.numel()
    h = _hidden(weights)
    sizes = (cols * h[0], h[0], h[0], 1) if len(h) == 1 else (cols * h[0], h[0], h[0] * h[1], h[1], h[1], 1)
    outs, check = _banded(sizes, float("nan"))
    name = "bbx_pmlp_grad" if len(h) == 1 else "bbx_pmlp2_grad"
    nfl = getattr(lib, name + "_workspace_floats")(n, Rr, cols, *h)
    assert nfl > 0
    ws = torch.full((nfl + GUARD,), float("nan"), device="cuda")
    if index is None:
        _ffi.check(getattr(lib, name)(ptr(obs), ptr(rows), ptr(actions), n, Rr, cols, prep, *h, ptr(glogp), ptr(gent), ptr(ws), *[ptr(o) for o in outs], stream_ptr()))
    else:
        _ffi.check(getattr(lib, name + "_at")(ptr(obs), ptr(rows), ptr(actions), n_src, ptr(index), n, Rr, cols, prep, *h, ptr(glogp), ptr(gent), ptr(ws),
                                              *[ptr(o) for o in outs], stream_ptr()))
    torch.cuda.synchronize()
    assert np.isnan(ws[nfl:].cpu().numpy()).all(), "the workspace was overrun"
    return check()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same_bits(got, want, what):
    for i, (x, y) in enumerate(zip(got, want)):
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (what, i, int((_bits(x) != _bits(y)).sum()), "of", x.size)


@functools.lru_cache(maxsize=None)
def _source(cols, hidden, n_src=S, rr=R, seed=600):
    """Recorded states: row counts cycling through ROWS, garbage beyond the live rows, a few actions out of range."""
    w = pc.make_weights(cols, hidden, seed)
    rows = np.resize(np.array(ROWS, dtype=np.int32), n_src)
    obs = pc.fill_padding(pc.random_blocks(n_src, rr, cols, seed + 1), rows, True, seed + 2)
    rng = np.random.default_rng(seed + 3)
    live = np.clip(rows, 0, rr)
    actions = (rng.integers(0, 1 << 30, size=n_src) % np.maximum(live, 1)).astype(np.int32)
    if n_src > 4:
        actions[4] = -1
    if n_src > 7:
        actions[7] = rr
    for a in (obs, rows, actions):
        a.setflags(write=False)
    return w, obs, rows, actions


def _index_lists():
    rng = np.random.default_rng(9)
    yield "identity", np.arange(S)
    yield "reversed", np.arange(S)[::-1]
    yield "permutation", rng.permutation(S)
    yield "repeats", rng.integers(0, S, size=3 * S + 1)
    yield "first", np.array([0])
    yield "last", np.array([S - 1])


# ---- log-probability and entropy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,hidden", ONE + TWO, ids=_ids)
def test_logprob_and_entropy_equal_the_gathered_call_bit_for_bit(cols, hidden):
    w, obs, rows, actions = _source(cols, hidden)
    d_obs, d_rows, d_act = to_cuda(obs, rows, actions)
    for name, index in _index_lists():
        index = index.astype(np.int32)
        d_idx, = to_cuda(index)
        lp, ent = _logprob(w, d_obs, d_rows, d_act, d_idx)
        lp0, ent0 = _logprob(w, *to_cuda(obs[index], rows[index], actions[index]))
        _same_bits((lp, ent), (lp0, ent0), name)
        assert lp.shape == (len(index),)
        if name == "identity":
            assert np.isnan(lp).any() and np.isfinite(lp).any() and (lp == 0.0).any()      # a bad action, live states, no row
        if name == "repeats":
            lp2, none = _logprob(w, d_obs, d_rows, d_act, d_idx, entropy=False)
            assert none is None
            _same_bits((lp2,), (lp0,), "NULL entropy")


BAD = (-1, S, 2 ** 31 - 1)


def _with_bad_indices():
    """A valid list with entries out of range mixed in; (index, keep): keep marks the valid positions."""
    rng = np.random.default_rng(10)
    index = rng.integers(0, S, size=23).astype(np.int64)
    at = np.array([0, 5, 6, 13, 22])
    index[at] = np.array([BAD[0], BAD[1], BAD[2], BAD[0], BAD[2]])
    keep = np.ones(len(index), dtype=bool); keep[at] = False
    return index.astype(np.int32), keep


@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (64, (256,)), (12, (128, 128)), (33, (65, 64))], ids=_ids)
def test_indices_out_of_range(cols, hidden):
    """-1, S and 2^31 - 1 among valid indices: NaN and NaN there, the other positions as without them; the gradients those of the
    list without them, whatever upstream gradients their positions carry.  The sources are exact-size allocations."""
    w, obs, rows, actions = _source(cols, hidden)
    d_obs, d_rows, d_act = to_cuda(obs, rows, actions)
    index, keep = _with_bad_indices()
    lp, ent = _logprob(w, d_obs, d_rows, d_act, to_cuda(index)[0])
    assert np.isnan(lp[~keep]).all() and np.isnan(ent[~keep]).all()
    lp0, ent0 = _logprob(w, d_obs, d_rows, d_act, to_cuda(index[keep])[0])
    _same_bits((lp[keep], ent[keep]), (lp0, ent0), "valid positions")
    rng = np.random.default_rng(11)
    glogp = rng.normal(size=len(index)).astype(np.float32); gent = rng.normal(size=len(index)).astype(np.float32)
    glogp[~keep] = np.array([np.nan, np.inf, -np.inf, 1e30, np.nan], dtype=np.float32)
    gent[~keep] = np.array([np.inf, np.nan, 1e30, np.nan, -np.inf], dtype=np.float32)
    for with_gent in (True, False):
        got = _grad(w, d_obs, d_rows, d_act, *to_cuda(glogp, gent if with_gent else None, index))
        want = _grad(w, d_obs, d_rows, d_act, *to_cuda(glogp[keep], gent[keep] if with_gent else None, index[keep]))
        assert all(np.isfinite(x).all() for x in got) and any((x != 0).any() for x in got)
        # the same positions holding a recorded state without rows (which contributes nothing: tests/test_policy_grad_gpu.py) in
        # their place: the same n, the same partition — the same bits
        blank = index.copy(); blank[~keep] = 1
        assert rows[1] == 0
        _same_bits(got, _grad(w, d_obs, d_rows, d_act, *to_cuda(glogp, gent if with_gent else None, blank)), "a state without rows in their place")
        # removed: the partition of the positions over waves follows n, which now differs — the same numbers added in another order,
        # so both are held to the float64 reference of the shorter list (and bit for bit below, where either list is one wave's)
        sel = index[keep]
        ref = pc.reference(w, obs[sel], rows[sel])
        f = gc.reference_grad if len(hidden) == 1 else g2.reference_grad2
        want64, A = f(w, obs[sel], rows[sel], actions[sel], glogp[keep], gent[keep] if with_gent else None, ref=ref)
        chk = gc.check_grads if len(hidden) == 1 else g2.check_grads
        chk(got, want64, A, ref, what="with bad indices")
        chk(want, want64, A, ref, what="without them")
    # a list short enough for one wave / one workgroup either way: the same partition, the same bits
    short, skeep = index[:4], keep[:4]
    got = _grad(w, d_obs, d_rows, d_act, *to_cuda(glogp[:4], gent[:4], short))
    want = _grad(w, d_obs, d_rows, d_act, *to_cuda(glogp[:4][skeep], gent[:4][skeep], short[skeep]))
    _same_bits(got, want, "one wave")
    # nothing but indices out of range: zeros
    none = np.array(BAD, dtype=np.int32)
    z = _grad(w, d_obs, d_rows, d_act, *to_cuda(glogp[~keep][:3], gent[~keep][:3], none))
    assert all((x == 0).all() for x in z)


# ---- gradients ---------------------------------------------------------------------------------------------------------------
SPW, _ = gc.header_constants()
SPG, _ = g2.header_constants()
GRAD_BATCHES_1 = sorted({1, 5, SPW + 1, 2 * SPW + 1})        # GRAD_BATCHES of tests/test_policy_grad_gpu.py
GRAD_BATCHES_2 = sorted({1, 5, SPG + 1, 2 * SPG + 1})        # ... and of tests/test_policy2_grad_gpu.py


def _grad_index(n, n_src):
    """A permutation of n of the n_src states with two repeats; state 0 (33 rows, a valid action: it has a gradient) comes first."""
    index = np.random.default_rng(n + 2).permutation(n_src)           # (a draw that mixes states with and without a gradient)
    at = int(np.flatnonzero(index == 0)[0])
    index[0], index[at] = index[at], index[0]
    index = index[:n]
    if n > 2:
        index[n // 2] = index[0]; index[n - 1] = index[1]
    return index.astype(np.int32)


GRAD_CASES = [(c, h, n) for c, h in ONE for n in GRAD_BATCHES_1] + [(c, h, n) for c, h in TWO for n in GRAD_BATCHES_2]


@pytest.mark.parametrize("cols,hidden,n", GRAD_CASES, ids=_ids)
def test_gradients_equal_the_gathered_call_bit_for_bit(cols, hidden, n):
    w, obs, rows, actions = _source(cols, hidden, n + 3, 136, 700 + n)
    index = _grad_index(n, n + 3)
    rng = np.random.default_rng(n + 1)
    glogp = rng.normal(size=n).astype(np.float32); gent = rng.normal(size=n).astype(np.float32)
    d_obs, d_rows, d_act = to_cuda(obs, rows, actions)
    gathered = to_cuda(obs[index], rows[index], actions[index])
    for ge in (gent, None):
        got = _grad(w, d_obs, d_rows, d_act, *to_cuda(glogp, ge, index))
        want = _grad(w, *gathered, *to_cuda(glogp, ge))
        _same_bits(got, want, "gent" if ge is not None else "NULL gent")
        again = _grad(w, d_obs, d_rows, d_act, *to_cuda(glogp, ge, index))
        _same_bits(again, got, "second call")
    assert rows[0] == 33 and 0 <= actions[0] < 33 and index[0] == 0
    live = np.clip(rows, 0, 136)[index]
    has = (live > 1) & (actions[index] >= 0) & (actions[index] < live)
    assert n == 1 or (len(set(index[has])) >= 2 and (~has).any()), "the case should mix states with and without a gradient"
    if cols >= 12:                                                     # (a single unit may well be dead on every row)
        assert any((x != 0).any() for x in got)


@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (12, (128, 128))], ids=_ids)
def test_no_positions_zero_the_gradients(cols, hidden):
    import torch
    w, obs, rows, actions = _source(cols, hidden)
    d_obs, d_rows, d_act = to_cuda(obs, rows, actions)
    empty = torch.zeros(0, dtype=torch.int32, device="cuda"); none = torch.zeros(0, device="cuda")
    z = _grad(w, d_obs, d_rows, d_act, none, none, empty)
    assert len(z) == (4 if len(hidden) == 1 else 6) and all((x == 0).all() for x in z)


@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (12, (128, 128))], ids=_ids)
def test_gradients_against_float64(cols, hidden):
    """The indexed entries against the float64 reference on the gathered arrays, with the bounds of the entries without _at."""
    w, obs, rows, actions = _source(cols, hidden)
    index = np.array([0, 9, 2, 30, 9], dtype=np.int32)               # rows 33, 32, 40, 33, 32; one state twice
    rng = np.random.default_rng(12)
    glogp = rng.normal(size=5).astype(np.float32); gent = rng.normal(size=5).astype(np.float32)
    got = _grad(w, *to_cuda(obs, rows, actions, glogp, gent, index))
    ref = pc.reference(w, obs[index], rows[index])
    if len(hidden) == 1:
        want, A = gc.reference_grad(w, obs[index], rows[index], actions[index], glogp, gent, ref=ref)
        print("ratios indexed %s r_g=%.3f" % (pc.label(cols, hidden), gc.grad_ratio(got, want, A, ref)))
        gc.check_grads(got, want, A, ref, what="indexed")
    else:
        want, A = g2.reference_grad2(w, obs[index], rows[index], actions[index], glogp, gent, ref=ref)
        print("ratios indexed %s r_g=%.3f" % (pc.label(cols, hidden), g2.grad_ratio(got, want, A, ref)))
        g2.check_grads(got, want, A, ref, what="indexed")
    assert any(np.abs(x).max() > 0 for x in want)
    lp, ent = _logprob(w, *to_cuda(obs, rows, actions, index))
    rl, rh, _ = gc.reference_eval(w, obs[index], rows[index], actions[index], ref=ref)
    assert (np.abs(lp - rl) <= ref.tol()).all()
    assert (np.abs(ent - rh) <= (gc.entropy_tol(ref) if len(hidden) == 1 else g2.entropy_tol(ref))).all()


# ---- autograd ----------------------------------------------------------------------------------------------------------------
def _hand_filled_buffer(T=6, B=4, rr=33, cols=12):
    import torch
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer
    rng = np.random.default_rng(31)
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(rr, cols))
    rows = np.resize(np.array((33, 2, 17, 1, 32, 5, 31, 9, 20, 1, 3), dtype=np.int32), T * B).reshape(T, B)
    st = pc.fill_padding(pc.random_blocks(T * B, rr, cols, 32), rows.reshape(-1), False).reshape(T, B, rr, cols)
    done = np.zeros((T, B), dtype=bool)
    done[T - 1, 0] = True; done[[1, 4], 1] = True; done[:, 2] = True           # environment 3 never finishes
    buf.states.copy_(torch.from_numpy(st)); buf.rows.copy_(torch.from_numpy(rows)); buf.dones.copy_(torch.from_numpy(done))
    buf.actions.copy_(torch.from_numpy((rng.integers(0, 1 << 30, size=(T, B)) % np.maximum(rows, 1)).astype(np.int32)))
    buf.rewards.copy_(torch.from_numpy(-rng.integers(1, 30, size=(T, B)).astype(np.float64)))
    buf.values.copy_(torch.from_numpy(rng.normal(size=(T, B))))
    buf.logprobs.copy_(torch.from_numpy((-rng.uniform(0.1, 3.0, size=(T, B))).astype(np.float32)))
    buf.t = T
    return buf


def _ppo_pass(pol, opt, batches, evaluate):
    """One PPO pass (clipped surrogate and an entropy bonus), the gradients of all minibatches accumulated; the .grad of every
    parameter, cloned."""
    import torch
    opt.zero_grad()
    for batch in batches:
        logp, ent = evaluate(batch)
        old, adv = batch[2], batch[3]
        ratio = torch.exp(logp - old)
        loss = -torch.minimum(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean() - 0.01 * ent.mean()
        loss.backward()
    return [q.grad.clone() for q in pol.parameters()]


@pytest.mark.parametrize("hidden", [(128,), (128, 128)], ids=_ids)
def test_evaluate_at_trains_like_evaluate_on_the_gathered_batches(hidden):
    import torch
    buf = _hand_filled_buffer()
    pol = _policy(pc.make_weights(12, hidden, 33))
    opt = torch.optim.SGD(pol.parameters(), lr=0.05)
    kind = "_PMLPEvaluate" if len(hidden) == 1 else "_PMLP2Evaluate"
    seen = []

    def at(batch):
        out = pol.evaluate_at(buf.states, buf.actions, buf.rows, batch[0])
        seen.append(type(out[0].grad_fn).__name__)
        return out
    for step in range(2):                                              # (the second pass: after an optimizer step)
        gathered = buf.get(batch_size=8, sort=True, with_rows=True)
        indexed = buf.get_index(batch_size=8, sort=True)
        assert len(gathered) == len(indexed) >= 2 and all(b[0].dtype == torch.int32 for b in indexed)
        want = _ppo_pass(pol, opt, gathered, lambda b: pol.evaluate(b[0], b[1], b[5]))
        got = _ppo_pass(pol, opt, indexed, at)
        assert all(name.startswith(kind) for name in seen)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), step
        assert all(torch.isfinite(g).all() for g in got) and any(float(g.abs().max()) > 0 for g in got)
        before = [q.detach().clone() for q in pol.parameters()]
        opt.step()
        assert any(not torch.equal(a, b) for a, b in zip(before, pol.parameters()))


@pytest.mark.parametrize("hidden", [(128,), (128, 128)], ids=_ids)
@pytest.mark.parametrize("how", ["non-contiguous", "int64"])
def test_evaluate_at_gathers_what_the_kernels_cannot_read_in_place(how, hidden):
    """A transposed view of the buffer, or int64 states: the gather path (no copy of the whole buffer), within the float64 bounds."""
    import torch
    buf = _hand_filled_buffer()
    w = pc.make_weights(12, hidden, 34)
    pol = _policy(w)
    index = buf.get_index(sort=True)[0]
    flat = lambda x: x.reshape((-1,) + tuple(x.shape[2:]))
    if how == "int64":
        st, act, rows = buf.states.to(torch.int64), buf.actions, buf.rows
        idx = index
    else:                                                              # [B, T, ...] views of the [T, B, ...] arrays: step t * B + b sits at b * T + t
        st, act, rows = buf.states.transpose(0, 1), buf.actions.transpose(0, 1), buf.rows.transpose(0, 1)
        assert not st.is_contiguous()
        idx = (index % buf.B) * buf.T + index // buf.B
    logp, ent = pol.evaluate_at(st, act, rows, idx)
    j = index.long().cpu().numpy()
    obs_h, rows_h, act_h = flat(buf.states).cpu().numpy()[j], flat(buf.rows).cpu().numpy()[j], flat(buf.actions).cpu().numpy()[j]
    rl, rh, ref = gc.reference_eval(w, obs_h, rows_h, act_h)
    assert (np.abs(logp.detach().cpu().numpy() - rl) <= ref.tol()).all()
    assert (np.abs(ent.detach().cpu().numpy() - rh) <= (gc.entropy_tol(ref) if len(hidden) == 1 else g2.entropy_tol(ref))).all()
    wt = np.random.default_rng(35).normal(size=len(j)).astype(np.float32)
    ((torch.from_numpy(wt).cuda() * logp).sum() - 0.01 * ent.sum()).backward()
    gent = np.full(len(j), -0.01)
    if len(hidden) == 1:
        lin = pol.embedding[0]
        got = [t.cpu().numpy() for t in (lin.weight.grad.t(), lin.bias.grad, pol.deciding.weight.grad.reshape(-1), pol.deciding.bias.grad.reshape(-1))]
        want, A = gc.reference_grad(w, obs_h, rows_h, act_h, wt, gent, ref=ref)
        gc.check_grads(got, want, A, ref, what=how)
    else:
        l1, l2 = pol.embedding
        got = [t.cpu().numpy() for t in (l1.weight.grad.t(), l1.bias.grad, l2.weight.grad.t(), l2.bias.grad, pol.deciding.weight.grad.reshape(-1),
                                         pol.deciding.bias.grad.reshape(-1))]
        want, A = g2.reference_grad2(w, obs_h, rows_h, act_h, wt, gent, ref=ref)
        g2.check_grads(got, want, A, ref, what=how)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_evaluate_at_reproduces_the_log_probabilities_of_a_real_rollout():
    """run_rollout_fused into a buffer with states; for every step get_index() selects, evaluate_at's log-probability is the one
    the rollout kernel recorded, bit for bit."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, run_rollout_fused
    torch.manual_seed(5)
    B, T = 8, 40
    env = VecLeadMonomialsEnv("3-20-10-weighted", batch=B, k=2)
    env.seed(np.arange(B) + 11); env.reset()
    policy = PMLPPolicy(env.cols, [128]).cuda()
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(256, env.cols))
    run_rollout_fused(env, policy, T, buffer=buf)
    index = buf.get_index()[0]
    assert index.numel() > B and index.dtype == torch.int32
    with torch.no_grad():
        logp, ent = policy.evaluate_at(buf.states, buf.actions, buf.rows, index)
    recorded = buf.logprobs.view(-1)[index.long()]
    assert torch.equal(logp.view(torch.int32), recorded.view(torch.int32))
    assert torch.isfinite(ent).all() and float(ent.max()) > 0
