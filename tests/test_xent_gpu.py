"""Cross-entropy training on the device: bbx_pmlp[2]_xent[_at], bbx_pmlp[2]_xent_grad[_at], PMLPPolicy.xent_step[_at] and
imitation_update.  Losses, entropies, statistics and gradients are held to the float64 reference of tests/xent_cases.py; one-hot
targets reproduce the policy gradient bit for bit; the call equals its parts and repeats itself bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_cases as pc
from tests import policy_grad_cases as gc
from tests import policy2_grad_cases as g2
from tests import xent_cases as xc
from tests.test_policy_indexed_gpu import GUARD, SENTINEL, _banded, _bits, _grad, _hidden, _policy, _prepared, _same_bits
from tests.fast_harness import ptr, stream_ptr, to_cuda

pytestmark = pytest.mark.gpu
_ids = lambda v: str(v).replace(" ", "")
STAT_THREADS = 1024
STATES_PER_WAVE, MAX_WAVES = gc.header_constants()
STATES_PER_GROUP, MAX_GROUPS = g2.header_constants()


def _stem(h):
    return "bbx_pmlp_xent" if len(h) == 1 else "bbx_pmlp2_xent"


def _xent(weights, obs, rows, targets, index=None, w=None, scale=1.0, entropy=True):
    """bbx_pmlp[2]_xent (index None) or ..._at through the C ABI, the outputs between sentinel bands: (losses, entropy or None)."""
    import torch
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    prep, keep = _prepared(weights)
    n_src, Rr, cols = obs.shape
    n = n_src if index is None else index.numel()
    h = _hidden(weights)
    (ls, ent), check = _banded((n, n), SENTINEL)
    src = (ptr(obs), ptr(rows), ptr(targets)) + ((n,) if index is None else (n_src, ptr(index), n)) + (Rr, cols, prep) + tuple(h)
    fn = getattr(lib, _stem(h) + ("" if index is None else "_at"))
    _ffi.check(fn(*src, ptr(w), C.c_float(scale), ptr(ls), ptr(ent) if entropy else None, stream_ptr()))
    torch.cuda.synchronize()
    ls, ent = check()
    return ls, (ent if entropy else None)


def _xent_grad(weights, obs, rows, targets, index=None, w=None, scale=1.0, outputs=True):
    """bbx_pmlp[2]_xent_grad (index None) or ..._at through the C ABI: losses, entropy and coef between sentinel bands, the gradients
    between NaN bands, NaN behind the workspace and around the statistics.  A dict of numpy arrays; the tail's parts by name."""
    import torch
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    prep, keep = _prepared(weights)
    n_src, Rr, cols = obs.shape
    n = n_src if index is None else index.numel()
    h = _hidden(weights)
    (ls, ent, coef), check_out = _banded((n, n, 2 * n), SENTINEL)
    sizes = (cols * h[0], h[0], h[0], 1) if len(h) == 1 else (cols * h[0], h[0], h[0] * h[1], h[1], h[1], 1)
    grads, check_grads = _banded(sizes, float("nan"))
    name = _stem(h)
    nfl = getattr(lib, name + "_workspace_floats")(n, Rr, cols, *h)
    gfl = getattr(lib, name.replace("_xent", "_grad") + "_workspace_floats")(n, Rr, cols, *h)
    assert nfl == gfl + 5 * n and gfl > 0
    ws = torch.full((nfl + GUARD,), float("nan"), device="cuda")
    stats = torch.full((6 + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    src = (ptr(obs), ptr(rows), ptr(targets)) + ((n,) if index is None else (n_src, ptr(index), n)) + (Rr, cols, prep) + tuple(h)
    fn = getattr(lib, name + "_grad" + ("" if index is None else "_at"))
    _ffi.check(fn(*src, ptr(w), C.c_float(scale), ptr(ls) if outputs else None, ptr(ent) if outputs else None, ptr(coef),
                  C.c_void_p(stats.data_ptr() + 8 * GUARD), ptr(ws), *[ptr(g) for g in grads], stream_ptr()))
    torch.cuda.synchronize()
    host = ws.cpu().numpy()
    assert np.isnan(host[nfl:]).all(), "the workspace was overrun"
    st = stats.cpu().numpy()
    assert np.isnan(st[:GUARD]).all() and np.isnan(st[GUARD + 6:]).all(), "written around the statistics"
    ls, ent, coef = check_out()
    if not outputs:
        assert (ls == SENTINEL).all() and (ent == SENTINEL).all()
    tail = host[gfl:nfl]
    return {"losses": ls, "entropy": ent, "coef": coef, "grads": check_grads(), "stats": st[GUARD:GUARD + 6].copy(),
            "wl": tail[:n].copy(), "wT": tail[n:2 * n].copy(), "H": tail[2 * n:3 * n].copy(), "w": tail[3 * n:4 * n].copy(),
            "flags": tail[4 * n:].copy().view(np.int32)}


def _stat_bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _check_against_float64(weights, obs, rows, targets, index, w, scale, what):
    """One call (index None: the plain form) against the reference; prints the ratios it needed."""
    depth = len(weights) - 1
    got = _xent_grad(weights, *to_cuda(obs, rows, targets), None if index is None else to_cuda(index)[0], to_cuda(w)[0], scale)
    xr = xc.reference(weights, obs, rows, targets, index, w, scale)
    n = len(xr.n)
    r_x, r_g = xc.loss_ratio(xr, got["losses"]), xc.grad_ratio(xr, got["grads"])
    print("ratios xent %s %s n=%d r_x=%.3f r_g=%.3f" % (pc.label(weights[0][0].shape[0], _hidden(weights)), what, n, r_x, r_g))
    cn = xr.counted
    # exact: who counts, the NaN of the others, the two counts, the coefficients of the positions that are not counted
    assert np.array_equal(got["flags"] & 1, cn.astype(np.int32)), "counted"
    assert np.array_equal(np.isnan(got["losses"]), ~cn) and np.array_equal(np.isnan(got["entropy"]), np.isnan(xr.H))
    assert got["stats"][0] == cn.sum() and got["stats"][5] == (~cn).sum()
    c, T = got["coef"][:n], got["coef"][n:]
    assert (c[~cn] == 0).all() and (T[~cn] == 0).all()
    for k in ("wl", "wT", "H", "w"):
        assert (got[k][~cn] == 0).all(), k
    wk = np.ones(n, dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    assert np.array_equal(_bits(c[cn]), _bits((np.float32(scale) * wk)[cn])), "c = scale * w, one float32 product"
    # one live row, no live row, T = 0: exactly nothing
    lone = cn & (xr.n <= 1)
    assert (got["losses"][lone] == 0).all() and (got["entropy"][cn & (xr.n == 0)] == 0).all()
    assert (got["losses"][cn & (xr.T == 0)] == 0).all()
    # within the bounds
    lt, et = xc.loss_tol(xr), xc.entropy_tol(xr, depth)
    l64 = np.where(cn, xr.l, 0.0)
    err = np.abs(np.where(cn, got["losses"], 0.0) - l64)
    assert (err <= lt).all(), ("losses", float((err - lt).max()))
    inside = ~np.isnan(xr.H)
    assert (np.abs(got["entropy"][inside] - xr.H[inside]) <= et[inside]).all(), "entropy"
    assert (np.abs(T - xr.T) <= xc.total_tol(xr)).all(), "T"
    xc.check_grads(xr, got["grads"], depth, what)
    for i, bound in zip((1, 2, 3, 4), xc.stats_tol(xr, depth)):
        assert abs(got["stats"][i] - xr.stats[i]) <= bound, (i, got["stats"][i], xr.stats[i], bound)
    # the statistics ARE the double sums of the float32 terms the call wrote
    for i, term in ((1, got["wl"]), (2, got["wT"]), (3, got["H"]), (4, got["w"])):
        t = term[cn].astype(np.float64)
        assert abs(got["stats"][i] - t.sum()) <= 2.0 ** -40 * np.abs(t).sum()
    assert r_x <= xc.C_X and r_g <= (gc.C_G if depth == 1 else g2.C_G2), (r_x, r_g)
    return got, xr


# ---- 1. against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("null_weights", [False, True], ids=["weights", "null"])
@pytest.mark.parametrize("cols,hidden", xc.SHAPES_ONE + xc.SHAPES_TWO, ids=_ids)
def test_losses_statistics_and_gradients_against_float64(cols, hidden, null_weights):
    w, obs, rows, targets = xc.source(cols, hidden)
    index = xc.index_of()
    wk = None if null_weights else xc.weights_for(index)
    got, xr = _check_against_float64(w, obs, rows, targets, index, wk, 1.0 / len(index), "at")
    assert xc.healthy_fraction(xr) >= 0.8 and (~xr.counted).sum() >= 4
    assert any((g != 0).any() for g in got["grads"])
    # the plain form on the gathered states (indices in range: an index out of range has no gathered counterpart)
    index = xc.index_of(bad=False)
    j = index.astype(np.int64)
    wk = None if null_weights else xc.weights_for(index)
    got, xr = _check_against_float64(w, obs[j], rows[j], targets[j], None, wk, 0.25, "plain")
    assert xc.healthy_fraction(xr) >= 0.8


# ---- 2. one-hot targets reproduce the policy gradient bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (12, (128, 128))], ids=_ids)
def test_one_hot_targets_reproduce_the_policy_gradient_bit_for_bit(cols, hidden):
    n, R, scale = 37, 40, 2.0 ** -5
    w = pc.make_weights(cols, hidden, 940)
    rows = (2 + (np.arange(n) * 7) % (R + 3)).astype(np.int32)        # 2 .. 44: more than obs_rows among them
    obs = pc.fill_padding(pc.random_blocks(n, R, cols, 941), rows, True, 942)
    live = np.clip(rows, 0, R)
    actions = (np.random.default_rng(943).integers(0, 1 << 30, size=n) % live).astype(np.int32)
    targets = np.full((n, R), np.nan, dtype=np.float32)
    for s in range(n):
        targets[s, :live[s]] = 0.0
        targets[s, actions[s]] = 1.0
    d_obs, d_rows, d_act, d_t = to_cuda(obs, rows, actions, targets)
    got = _xent_grad(w, d_obs, d_rows, d_t, None, None, scale)
    assert (got["coef"][n:] == 1.0).all() and (got["coef"][:n] == np.float32(scale)).all() and got["stats"][0] == n
    want = _grad(w, d_obs, d_rows, d_act, to_cuda(np.full(n, -scale, dtype=np.float32))[0], None)
    _same_bits(got["grads"], want, "policy gradient with glogp = -scale")
    assert all((g != 0).any() for g in got["grads"])


# ---- 3. the call equals its parts, and is deterministic ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (40, (256,)), (12, (128, 128)), (33, (40, 100))], ids=_ids)
def test_call_equals_its_parts_and_repeats_itself(cols, hidden):
    w, obs, rows, targets = xc.source(cols, hidden)
    index = xc.index_of()
    wk = xc.weights_for(index)
    scale = 1.0 / len(index)
    d_obs, d_rows, d_t, d_idx, d_w = to_cuda(obs, rows, targets, index, wk)
    got = _xent_grad(w, d_obs, d_rows, d_t, d_idx, d_w, scale)
    # losses / entropy: bbx_pmlp[2]_xent_at's
    ls, ent = _xent(w, d_obs, d_rows, d_t, d_idx, d_w, scale)
    _same_bits((got["losses"], got["entropy"]), (ls, ent), "xent_at")
    ls2, none = _xent(w, d_obs, d_rows, d_t, d_idx, d_w, scale, entropy=False)
    _same_bits((ls2,), (ls,), "xent_at without entropy")
    # a second call: the same bits, statistics included; without the two optional outputs: the same everything else
    again = _xent_grad(w, d_obs, d_rows, d_t, d_idx, d_w, scale, outputs=False)
    names = ("coef", "wl", "wT", "H", "w")
    _same_bits([got[k] for k in names] + got["grads"], [again[k] for k in names] + again["grads"], "second call")
    assert np.array_equal(got["flags"], again["flags"]) and np.array_equal(_stat_bits(got["stats"]), _stat_bits(again["stats"]))
    # the plain call on the gathered arrays (indices in range: an index out of range has no gathered counterpart)
    index = xc.index_of(bad=False)
    j = index.astype(np.int64)
    wk = xc.weights_for(index)
    d_idx, d_w = to_cuda(index, wk)
    at = _xent_grad(w, d_obs, d_rows, d_t, d_idx, d_w, scale)
    plain = _xent_grad(w, *to_cuda(obs[j], rows[j], targets[j]), None, d_w, scale)
    for k in ("losses", "entropy") + names:
        _same_bits((at[k],), (plain[k],), "gathered: " + k)
    assert np.array_equal(at["flags"], plain["flags"]) and np.array_equal(_stat_bits(at["stats"]), _stat_bits(plain["stats"]))
    _same_bits(at["grads"], plain["grads"], "gathered: gradients")


# ---- 4. partition boundaries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, STATES_PER_WAVE, STATES_PER_WAVE + 1, STATES_PER_WAVE * MAX_WAVES + 4])
def test_one_layer_partition_boundaries(n):
    assert (STATES_PER_WAVE, MAX_WAVES) == (4, 1024)                   # n = 1, 4, 5 and 4100: past MAX_WAVES x 4, waves take several states
    w, obs, rows, targets = xc.partition_case(12, (128,), 8, n)
    _check_against_float64(w, obs, rows, targets, None, None, 1.0 / n, "partition")


@pytest.mark.parametrize("n", [STATES_PER_GROUP, STATES_PER_GROUP + 1, STATES_PER_GROUP * MAX_GROUPS + 1])
def test_two_layer_partition_boundaries(n):
    assert (STATES_PER_GROUP, MAX_GROUPS) == (4, 512)
    w, obs, rows, targets = xc.partition_case(12, (64, 64), 4, n)
    _check_against_float64(w, obs, rows, targets, None, None, 1.0 / n, "partition")


@pytest.mark.parametrize("n", [STAT_THREADS - 1, STAT_THREADS, STAT_THREADS + 1])
@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (12, (64, 64))], ids=_ids)
def test_statistics_around_the_partition_boundaries(cols, hidden, n):
    from tests import ppo_cases as pp
    assert pp.header_constants() == STAT_THREADS
    w, obs, rows, targets = xc.source(cols, hidden, obs_rows=8, rows=(2, 5, 8, 3, 0, 7), kinds=("soft", "unnormalised", "onehot", "soft", "soft", "negative"))
    rng = np.random.default_rng(n)
    index = rng.integers(0, 6, size=n).astype(np.int32)
    index[[3, n - 1]] = (-1, 6)
    wk = rng.uniform(0.5, 1.5, size=n).astype(np.float32)
    got, xr = _check_against_float64(w, obs, rows, targets, index, wk, 1.0 / n, "statistics")
    assert got["stats"][0] + got["stats"][5] == n and got["stats"][5] > 2


@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (12, (64, 64))], ids=_ids)
def test_no_position_at_all(cols, hidden):
    import torch
    w, obs, rows, targets = xc.source(cols, hidden)
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    for index in (empty, None):
        if index is None:
            src = (torch.zeros((0,) + obs.shape[1:], dtype=torch.int32, device="cuda"), empty, torch.zeros((0, obs.shape[1]), device="cuda"))
        else:
            src = to_cuda(obs, rows, targets)
        got = _xent_grad(w, *src, index, None, 0.0)
        assert (got["stats"] == 0).all() and all((g == 0).all() for g in got["grads"])
    # NULL per-position arrays are accepted
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    prep, keep = _prepared(w)
    h = _hidden(w)
    sizes = (cols * h[0], h[0], h[0], 1) if len(h) == 1 else (cols * h[0], h[0], h[0] * h[1], h[1], h[1], 1)
    grads = [torch.full((s,), float("nan"), device="cuda") for s in sizes]
    ws = torch.empty(getattr(lib, _stem(h) + "_workspace_floats")(0, obs.shape[1], cols, *h), device="cuda")
    stats = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    _ffi.check(getattr(lib, _stem(h) + "_grad")(None, None, None, 0, obs.shape[1], cols, prep, *h, None, C.c_float(1.0), None, None, None, ptr(stats), ptr(ws),
                                                *[ptr(g) for g in grads], stream_ptr()))
    _ffi.check(getattr(lib, _stem(h))(None, None, None, 0, obs.shape[1], cols, prep, *h, None, C.c_float(1.0), None, None, stream_ptr()))
    torch.cuda.synchronize()
    assert (stats == 0).all() and all((g == 0).all() for g in grads)


# ---- 5. Python ------------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    """The distance of two float32 arrays in units in the last place of the larger magnitude."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    m = np.maximum(np.abs(a), np.abs(b))
    ulp = np.where(m > 0, 2.0 ** (np.floor(np.log2(np.where(m > 0, m, 1.0))) - 23), 2.0 ** -149)
    return np.abs(a - b) / ulp


@pytest.mark.parametrize("hidden", [(128,), (128, 128)], ids=_ids)
def test_xent_step_at_adds_to_grad(hidden):
    import torch
    w, obs, rows, targets = xc.source(12, hidden)
    index = xc.index_of()
    st, rw, tg, idx, wk = to_cuda(obs, rows, targets, index, xc.weights_for(index))
    pol = _policy(w)
    assert all(q.grad is None for q in pol.parameters())
    stats, losses, ent = pol.xent_step_at(st, rw, idx, tg, wk)
    once = [q.grad.detach().clone() for q in pol.parameters()]
    assert all(g is not None and g.shape == q.shape and g.is_contiguous() for g, q in zip(once, pol.parameters()))
    xr = xc.reference(w, obs, rows, targets, index, xc.weights_for(index), 1.0 / len(index))
    depth = len(hidden)
    kernel_order = [g.t() if g.dim() == 2 and g.shape[0] != 1 else g for g in once]
    xc.check_grads(xr, [g.cpu().numpy().reshape(-1) for g in kernel_order], depth, "xent_step_at")
    assert stats.cpu().numpy()[0] == xr.counted.sum() and np.array_equal(np.isnan(losses.cpu().numpy()), ~xr.counted)
    pol.xent_step_at(st, rw, idx, tg, wk)
    for a, q in zip(once, pol.parameters()):
        assert (_ulps(q.grad.cpu().numpy(), 2 * a.cpu().numpy()) <= 1).all()
    # the gathered form leaves the same bits for indices in range; xent_at returns the step's losses
    index = xc.index_of(bad=False)
    idx, wk = to_cuda(index, xc.weights_for(index))
    pol.zero_grad(set_to_none=True)
    s1, l1, e1 = pol.xent_step_at(st, rw, idx, tg, wk)
    g1 = [q.grad.detach().clone() for q in pol.parameters()]
    pol.zero_grad(set_to_none=True)
    j = idx.long()
    s2, l2, e2 = pol.xent_step(st[j], rw[j], tg[j], wk)
    assert all(torch.equal(a.view(torch.int32), q.grad.view(torch.int32)) for a, q in zip(g1, pol.parameters()))
    assert torch.equal(s1, s2) and torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    l3, e3 = pol.xent_at(st, rw, idx, tg, wk)
    assert torch.equal(l1.view(torch.int32), l3.view(torch.int32)) and torch.equal(e1.view(torch.int32), e3.view(torch.int32))


def test_three_layers_take_the_torch_path_and_match_the_reference():
    import torch
    cols, hidden = 12, (32, 24, 16)
    w = pc.make_weights(cols, hidden, 950)
    obs_rows = 20
    rows = np.array((0, 1, 2, 9, 20, 33, 7, 12), dtype=np.int32)
    kinds = ("soft", "soft", "soft", "unnormalised", "onehot", "soft", "negative", "zero")
    obs = pc.fill_padding(pc.random_blocks(len(rows), obs_rows, cols, 951), rows, True, 952)
    targets = xc.targets_for(rows, obs_rows, kinds, 953)
    pol = pc.to_policy(w, "cuda", torch.float64)
    st, rw, tg = to_cuda(obs, rows, targets)
    assert pol._kernel_depth(st) == 0
    stats, losses, ent = pol.xent_step(st, rw, tg)
    xr = _reference3(w, obs, rows, targets)
    assert np.array_equal(np.isnan(losses.cpu().numpy()), ~xr["counted"])
    cn = xr["counted"]
    assert np.allclose(losses.cpu().numpy()[cn], xr["l"][cn], rtol=1e-10, atol=1e-12)
    assert np.allclose(stats.cpu().numpy(), xr["stats"], rtol=1e-10, atol=1e-12)
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in pol.parameters()) and float(pol.deciding.bias.grad.abs().sum()) >= 0


def _reference3(w, obs, rows, targets):
    """l, counted and stats of a three-layer policy in float64 (pc.reference scores any depth)."""
    ref = pc.reference(w, obs, rows)
    N = len(rows)
    l = np.full(N, np.nan); H = np.zeros(N); T = np.zeros(N); counted = np.zeros(N, dtype=bool)
    for k in range(N):
        n = int(ref.n[k])
        t = targets[k, :n].astype(np.float64)
        logp = ref.logsm[k, :n]
        H[k] = -(np.exp(logp) * logp).sum()
        if ((t < 0) | ~np.isfinite(t)).any():
            continue
        counted[k] = True; l[k] = -(t * logp).sum(); T[k] = t.sum()
    z = lambda x: np.where(counted, x, 0.0)
    return {"l": l, "counted": counted, "stats": np.array([counted.sum(), z(l).sum(), z(T).sum(), z(H).sum(), counted.sum(), (~counted).sum()], dtype=np.float64)}


@pytest.mark.parametrize("hidden", [(128,), (128, 128)], ids=_ids)
def test_imitation_update_equals_the_hand_written_loop_bit_for_bit(hidden):
    import torch
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, imitation_update
    T = B = 8
    w = pc.make_weights(12, hidden, 960)
    pol, ref = _policy(w), _policy(w)
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(33, 12), targets=True)
    rows = np.resize(np.array((33, 2, 17, 32, 5, 31, 9, 20, 3), dtype=np.int32), T * B)
    st = pc.fill_padding(pc.random_blocks(T * B, 33, 12, 961), rows, False)
    tg = xc.targets_for(rows, 33, np.resize(np.array(("soft", "onehot", "unnormalised")), T * B), 962)
    for t in range(T):
        sl = slice(t * B, (t + 1) * B)
        z = torch.zeros(B, device="cuda")
        buf.store(*to_cuda(st[sl], rows[sl]), z.int(), z.double(), z, None, z.bool(), target=to_cuda(tg[sl])[0])
    assert buf.t == T and buf.returns is None
    opt_ref = torch.optim.SGD(ref.parameters(), lr=0.05)
    opt_ref.zero_grad()
    half = T * B // 2
    hand = []
    for i in range(0, T * B, half):
        idx = torch.arange(i, i + half, dtype=torch.int32, device="cuda")
        hand.append(ref.xent_step_at(buf.states, buf.rows, idx, buf.targets)[0])
        opt_ref.step(); opt_ref.zero_grad()
    out = imitation_update(pol, buf, torch.optim.SGD(pol.parameters(), lr=0.05), epochs=1, batch_size=half, shuffle=False)
    for (name, a), b in zip(pol.named_parameters(), ref.parameters()):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), name
    assert not torch.equal(pol.embedding[0].bias.detach().cpu(), torch.from_numpy(w[0][1]))      # (the steps moved the weights)
    assert buf.returns is None                                                                   # (nothing was finished)
    hs = torch.stack(hand).cpu().numpy()
    assert len(out) == 1 and np.array_equal(out[0]["stats"], hs) and out[0]["stats"][:, 0].sum() == T * B
    assert out[0]["loss"] == hs[:, 1].sum() / hs[:, 4].sum() and out[0]["entropy"] > 0


def test_twenty_adam_steps_lower_the_loss_on_a_real_rollout():
    """One minibatch of 256 states from an 8-step rollout of 32 environments, targets from action_values("degree") at temperature 1."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, action_value_targets
    torch.manual_seed(11)
    B, T, R = 32, 8, 64
    env = VecLeadMonomialsEnv("3-20-10-weighted", batch=B, k=2)
    env.seed(np.arange(B) + 21); env.reset()
    policy = PMLPPolicy(env.cols, [128]).cuda()
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(R, env.cols), targets=True)
    _collect(env, policy, buf, T, R, 1.0)
    index = torch.arange(T * B, dtype=torch.int32, device="cuda")
    assert index.numel() == 256
    opt = torch.optim.Adam(policy.parameters(), lr=1e-3)
    opt.zero_grad()
    means = []
    for _ in range(21):
        stats, _, _ = policy.xent_step_at(buf.states, buf.rows, index, buf.targets)
        s = stats.cpu().numpy()
        means.append(s[1] / s[4])
        opt.step(); opt.zero_grad()
    print("xent descent: %.6f -> %.6f" % (means[0], means[-1]))
    assert s[0] == 256 and s[5] == 0 and np.isfinite(means).all()
    assert means[-1] < means[0]


def _collect(env, policy, buf, T, R, temperature):
    """T steps under the policy, the action-value targets of every state recorded beside it."""
    import torch
    from deepgroebner_amd.rollout import action_value_targets
    B = env.batch
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    stream = torch.cuda.current_stream().cuda_stream
    obs = torch.empty((B, R, env.cols), dtype=torch.int32, device="cuda")
    rew = torch.zeros(B, dtype=torch.float64, device="cuda"); done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(B, dtype=torch.int32, device="cuda")
    env.rollout_device("first", 0, False, stream, rew, done, rows, obs, R, True, False)   # (a zero-step launch: the block and the row counts)
    env.sync()
    for t in range(T):
        q = torch.from_numpy(env.action_values("degree")).cuda()
        target = action_value_targets(q, rows, R, temperature)
        assert torch.isfinite(target).all() and float(target.sum(dim=1).min()) > 0.999
        state, count = obs.clone(), rows.clone()
        actions, logp = policy.act(obs, rows, torch.rand(B, device="cuda", generator=gen))
        env.step_device(actions, rew, done, rows, obs, R, True, stream, auto_reset=True)
        env.sync()
        buf.store(state, count, actions, rew, logp, None, done, target=target)
