"""bbx_pmlp_logprob / bbx_pmlp_grad and PMLPPolicy.evaluate on the device against the float64 reference of
tests/policy_grad_cases.py (tests/test_policy_grad_cpu.py checks that reference against autograd in double precision): the
log-probability of every live row at every instantiation and tile boundary, the entropy, the three conventions, bit-equality
with the sampler, the gradients at the batch sizes where the partition of the states changes, the operand permutation of the
backward pass with exact integer data, determinism, and the autograd wrapper.  Each case prints the ratio of its bound it
needed before it asserts (pytest -s)."""

import numpy as np
import pytest

from tests import policy_cases as pc
from tests import policy_grad_cases as gc
from tests.fast_harness import ptr, stream_ptr, to_cuda

pytestmark = pytest.mark.gpu
_ids = lambda v: str(v).replace(" ", "")
GUARD = 64


def _prepared(weights):
    """(prepared weights on the device, the policy that keeps them alive)"""
    pol = pc.to_policy(weights, "cuda")
    return pol._fused_weights()["prepared"], pol


def _logprob(weights, obs, rows, actions, entropy=True):
    """bbx_pmlp_logprob through the C ABI on device copies; (logprobs, entropy or None) as numpy."""
    import torch
    from deepgroebner_amd import _ffi
    prep, keep = _prepared(weights)
    N, R, cols = obs.shape
    lp = torch.full((N,), 7.0, device="cuda"); ent = torch.full((N,), 7.0, device="cuda")
    _ffi.check(_ffi.lib().bbx_pmlp_logprob(ptr(obs), ptr(rows), ptr(actions), N, R, cols, prep, weights[0][0].shape[1], ptr(lp),
                                           ptr(ent) if entropy else None, stream_ptr()))
    torch.cuda.synchronize()
    return lp.cpu().numpy(), (ent.cpu().numpy() if entropy else None)


def _grad(weights, obs, rows, actions, glogp, gent, prep=None):
    """bbx_pmlp_grad through the C ABI, the four outputs inside one buffer with NaN guard bands between them: returns
    (gW1 [cols][hidden], gb1, gw2, gb2) as numpy after checking that the bands are untouched."""
    import torch
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    if prep is None:
        prep, keep = _prepared(weights)
    N, R, cols = obs.shape
    hidden = weights[0][0].shape[1]
    sizes = (cols * hidden, hidden, hidden, 1)
    buf = torch.full((sum(sizes) + 5 * GUARD,), float("nan"), device="cuda")
    offs = np.cumsum([GUARD] + [s + GUARD for s in sizes[:-1]])
    outs = [buf[int(o):int(o) + s] for o, s in zip(offs, sizes)]
    nfl = lib.bbx_pmlp_grad_workspace_floats(N, R, cols, hidden)
    assert nfl > 0
    ws = torch.full((nfl + GUARD,), float("nan"), device="cuda")
    _ffi.check(lib.bbx_pmlp_grad(ptr(obs), ptr(rows), ptr(actions), N, R, cols, prep, hidden, ptr(glogp), ptr(gent) if gent is not None else None,
                                 ptr(ws), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), stream_ptr()))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    inside = np.zeros(len(host), dtype=bool)
    for o, s in zip(offs, sizes):
        inside[int(o):int(o) + s] = True
    assert np.isnan(host[~inside]).all(), "the guard bands around the gradient outputs were written"
    assert np.isnan(ws[nfl:].cpu().numpy()).all(), "the workspace was overrun"
    got = [host[int(o):int(o) + s].copy() for o, s in zip(offs, sizes)]
    got[0] = got[0].reshape(cols, hidden)
    return tuple(got)


# ---- log-probability and entropy ---------------------------------------------------------------------------------------------
EVAL_SHAPES = pc.one_layer_shapes() + [(12, (128,))]


def _every_row(case):
    """Actions covering every live row of a sweep case: copy j of a block records row j."""
    return np.concatenate([np.arange(int(n)) for n in case.base_ref.n]).astype(np.int32)


def _eval_cases(cols, hidden, seed):
    sweep = pc.row_sweep(cols, hidden, pc.LIVE_ROWS, seed, R=129, garbage=False)
    yield sweep, _every_row(sweep)
    sweep = pc.row_sweep(cols, hidden, pc.LIVE_ROWS, seed + 10, R=136, garbage=True)
    yield sweep, _every_row(sweep)
    for B, R, rows, s, garbage in ((5, 15, (15, 0, 7, -3, 20), seed + 2, True), (9, 24, (40, 0, 24, -3, 1, 15, 16, 17, 40), seed + 3, False),
                                   (1, 1, (5,), seed + 4, True)):
        case = pc.edge_case(cols, hidden, B, R, rows, s, garbage)
        n = np.maximum(case.ref.n, 1)
        yield case, (np.random.default_rng(s).integers(0, 1 << 30, size=B) % n).astype(np.int32)


@pytest.mark.parametrize("cols,hidden", EVAL_SHAPES, ids=_ids)
def test_logprob_and_entropy_at_every_row_and_boundary(cols, hidden):
    """Per shape: every live row of every count around the tiles of 32 rows and the wave of 64 recorded once (blocks of 129 rows
    with -1 padding, of 136 with garbage), then the obs_rows / rows edges.  logprob within Ref.tol(), entropy within
    C_H 2^-24 K (1 + log n); a state without rows: 0.0 and 0.0."""
    worst_l = worst_h = 0.0
    for case, actions in _eval_cases(cols, hidden, 300):
        obs, rows, act = to_cuda(case.obs, case.rows.astype(np.int32), actions)
        lp, ent = _logprob(case.weights, obs, rows, act)
        rl, rh, ref = gc.reference_eval(case.weights, None, None, actions, ref=case.ref)
        dead = ref.n <= 0
        assert (lp[dead] == 0.0).all() and (ent[dead] == 0.0).all(), case.name
        assert np.isfinite(lp).all() and np.isfinite(ent).all(), case.name
        el, eh = np.abs(lp - rl), np.abs(ent - rh)
        r_l = float((el / ref.tol(1.0)).max()); r_h = float((eh / gc.entropy_tol(ref, 1.0)).max())
        print("ratios %-60s N=%-5d r_l=%.3f r_h=%.3f" % (case.name, len(actions), r_l, r_h))
        worst_l, worst_h = max(worst_l, r_l), max(worst_h, r_h)
        assert (el <= ref.tol()).all(), (case.name, "logprob", r_l)
        assert (eh <= gc.entropy_tol(ref)).all(), (case.name, "entropy", r_h)
        one = ref.n == 1
        assert (lp[one] == 0.0).all() and (ent[one] == 0.0).all(), case.name
    print("worst %s r_l=%.3f r_h=%.3f" % (pc.label(cols, hidden), worst_l, worst_h))


def test_conventions_are_exact():
    """n_s <= 0: 0.0 / 0.0; n_s == 1: 0 / 0; an action outside [0, n_s): NaN with the entropy still computed; a NULL entropy
    pointer leaves the log-probabilities as they are."""
    case = pc.edge_case(12, (128,), 8, 24, (0, -3, 1, 1, 24, 40, 7, 16), 5, True)
    actions = np.array([0, 5, 0, 1, 24, -1, 7, 15], dtype=np.int32)
    obs, rows, act = to_cuda(case.obs, case.rows.astype(np.int32), actions)
    lp, ent = _logprob(case.weights, obs, rows, act)
    rl, rh, ref = gc.reference_eval(case.weights, None, None, actions, ref=case.ref)
    assert lp[0] == 0.0 and ent[0] == 0.0 and lp[1] == 0.0 and ent[1] == 0.0
    assert lp[2] == 0.0 and ent[2] == 0.0
    assert np.isnan(lp[3]) and ent[3] == 0.0                       # one row, action 1: outside
    assert np.isnan(lp[4]) and np.isnan(lp[5]) and np.isnan(lp[6])
    assert (np.abs(ent - rh) <= gc.entropy_tol(ref)).all() and ent[4] > 0 and ent[5] > 0
    assert np.isfinite(lp[7]) and abs(lp[7] - rl[7]) <= ref.tol()[7]
    lp2, none = _logprob(case.weights, obs, rows, act, entropy=False)
    assert none is None and np.array_equal(lp, lp2, equal_nan=True)


@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (64, (256,))], ids=_ids)
def test_logprob_equals_the_samplers_bit_for_bit(cols, hidden):
    """bbx_pmlp_act, then bbx_pmlp_logprob with the sampled actions on the same block and weights: the same bits."""
    import torch
    live = pc.LIVE_ROWS + (2048,)
    case = pc.edge_case(cols, hidden, len(live), 2048, live, 41, True)
    pol = pc.to_policy(case.weights, "cuda")
    obs, rows, u = to_cuda(case.obs, case.rows.astype(np.int32), case.u)
    a, l = pol.act(obs, rows, u)
    torch.cuda.synchronize()
    lp, _ = _logprob(case.weights, obs, rows, a)
    assert np.array_equal(l.cpu().numpy().view(np.uint32), lp.view(np.uint32))
    pc.check_case(case, a.cpu().numpy(), l.cpu().numpy())


# ---- gradients ---------------------------------------------------------------------------------------------------------------
GRAD_SHAPES = [(1, (1,)), (12, (128,)), (13, (33,)), (33, (65,)), (64, (256,))]
SPW, MAXW = gc.header_constants()
# one state; five; one more than a wave takes before a second wave is added; three waves with uneven shares (every one of these
# beyond SPW has the second kernel add more than one partial per output)
GRAD_BATCHES = sorted({1, 5, SPW + 1, 2 * SPW + 1})
GRAD_ROWS = (33, 0, 129, 1, 2, 64, 17, 31, 65, 1, 128, 16, 32, 63, 15, 127)


def _grad_case(cols, hidden, N, seed, R=136, rows=GRAD_ROWS, with_gent=True):
    w = pc.make_weights(cols, hidden, seed)
    rows = np.resize(np.array(rows, dtype=np.int32), N)
    obs = pc.fill_padding(pc.random_blocks(N, R, cols, seed + 1), rows, True, seed + 2)
    rng = np.random.default_rng(seed + 3)
    n = np.clip(rows, 0, R)
    actions = (rng.integers(0, 1 << 30, size=N) % np.maximum(n, 1)).astype(np.int32)
    glogp = rng.normal(size=N).astype(np.float32)
    gent = rng.normal(size=N).astype(np.float32) if with_gent else None
    return w, obs, rows, actions, glogp, gent


def _run_grad(w, obs, rows, actions, glogp, gent, what, summed=False):
    ref = pc.reference(w, obs, rows)
    want, A = gc.reference_grad(w, obs, rows, actions, glogp, gent, scale=gc.state_scale(ref) if summed else None, ref=ref)
    got = _grad(w, *to_cuda(obs, rows, actions, glogp, gent))
    r = gc.grad_ratio(got, want, A, None if summed else ref)
    print("ratios %-60s r_g=%.3f" % (what, r))
    gc.check_grads(got, want, A, None if summed else ref, what=what)
    return r


@pytest.mark.parametrize("N", GRAD_BATCHES)
@pytest.mark.parametrize("cols,hidden", GRAD_SHAPES, ids=_ids)
def test_gradients_against_float64(cols, hidden, N):
    """Row counts mixed over the tile edges, 0 and 1, garbage beyond them, glogp and gent of both signs; once more without
    gent (NULL).  Every entry of dW1, db1, dw2, db2 within C_G 2^-24 sum_s K_s A_theta,s; the outputs have the unpadded shapes
    and nothing around them is written."""
    w, obs, rows, actions, glogp, gent = _grad_case(cols, hidden, N, 500 + N)
    _run_grad(w, obs, rows, actions, glogp, gent, "grad %s N=%d" % (pc.label(cols, hidden), N))
    if N == 5:
        _run_grad(w, obs, rows, actions, glogp, None, "grad %s N=%d gent=NULL" % (pc.label(cols, hidden), N))


def test_gradients_large_batch_and_determinism():
    """More states than PMLP_GRAD_STATES_PER_WAVE x PMLP_GRAD_MAX_WAVES: every wave loops over several states and the second
    kernel adds PMLP_GRAD_MAX_WAVES partials per output.  Two calls on the same inputs return the same bits."""
    N = SPW * MAXW + 5
    w, obs, rows, actions, glogp, gent = _grad_case(12, (128,), N, 77, R=33, rows=(33, 0, 2, 1, 17, 32, 31, 16, 15))
    actions[7] = 40; actions[11] = -1                              # bad actions contribute nothing
    _run_grad(w, obs, rows, actions, glogp, gent, "grad 12x128 N=%d" % N, summed=True)
    dev = to_cuda(obs, rows, actions, glogp, gent)
    a = _grad(w, *dev); b = _grad(w, *dev)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_gradients_are_deterministic_at_the_largest_shape():
    w, obs, rows, actions, glogp, gent = _grad_case(64, (256,), 2 * SPW + 1, 78)
    dev = to_cuda(obs, rows, actions, glogp, gent)
    a = _grad(w, *dev); b = _grad(w, *dev)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_states_without_a_gradient_contribute_exactly_nothing():
    """No row, one row, a bad action: whatever their glogp / gent (NaN included for the skipped ones), the outputs are those of
    the other states alone; n == 0 zeroes the outputs."""
    w, obs, rows, actions, glogp, gent = _grad_case(12, (128,), 6, 90, R=40, rows=(0, 17, 1, 33, -2, 20))
    actions[3] = 33
    dev = to_cuda(obs, rows, actions, glogp, gent)
    a = _grad(w, *dev)
    glogp2, gent2 = glogp.copy(), gent.copy()
    glogp2[[0, 3, 4]] = np.nan; gent2[[0, 3, 4]] = np.inf; glogp2[2] = 1e30; gent2[2] = -1e30
    b = _grad(w, *to_cuda(obs, rows, actions, glogp2, gent2))
    keep = [1, 5]
    c = _grad(w, *to_cuda(obs[keep], rows[keep], actions[keep], glogp[keep], gent[keep]))
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    import torch
    z = _grad(w, torch.zeros((0, 40, 12), dtype=torch.int32, device="cuda"), *to_cuda(rows[:0], actions[:0], glogp[:0], gent[:0]))
    assert all((x == 0).all() for x in z)


@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("cols,hidden", [(12, 128), (33, 70)], ids=_ids)
def test_operand_permutation_with_exact_integers(cols, hidden, n):
    """Small integer weights and entries; the units come in pairs with the same first-layer column and opposite deciding weights,
    so every logit is exactly b2 although the rows differ: p_r = 1 / n exactly (n a power of two), and with glogp a multiple of n
    every g_r is an integer.  Every product and sum of the backward pass is then exact in fp32, and dW1, db1, dw2, db2 equal the
    float64 reference exactly — a row or column of the permuted operands in the wrong place changes almost every entry."""
    rng = np.random.default_rng(cols * 1000 + n)
    half = hidden // 2
    W1h = rng.integers(-2, 3, size=(cols, half)); b1h = rng.integers(-40, 6, size=half); w2h = rng.integers(-3, 4, size=half)
    w = [(np.concatenate([W1h, W1h], axis=1).astype(np.float32), np.concatenate([b1h, b1h]).astype(np.float32)),
         (np.concatenate([w2h, -w2h]).astype(np.float32), np.array([1.0], dtype=np.float32))]
    N = SPW + 2
    rows = np.full(N, n, dtype=np.int32)
    obs = pc.fill_padding(pc.random_blocks(N, n + 3, cols, n), rows, True, 1)
    actions = rng.integers(0, n, size=N).astype(np.int32)
    glogp = (n * rng.choice(np.array([-3, -2, -1, 1, 2, 3]), size=N)).astype(np.float32)
    ref = pc.reference(w, obs, rows)
    assert (ref.logits[:, :n] == 1.0).all()
    want, A = gc.reference_grad(w, obs, rows, actions, glogp, None, ref=ref)
    got = _grad(w, *to_cuda(obs, rows, actions, glogp, None))
    assert sum(int((np.rint(x) != 0).sum()) for x in want[:3]) > (cols * hidden) // 4, "the case is degenerate"
    for name, x, y in zip(("dW1", "db1", "dw2", "db2"), got, want):
        assert np.abs(y - np.rint(y)).max() <= 1e-8
        assert np.array_equal(x.astype(np.float64).reshape(y.shape), np.rint(y)), (name, int((x.reshape(y.shape) != np.rint(y)).sum()))


# ---- autograd ----------------------------------------------------------------------------------------------------------------
def test_evaluate_backward_and_an_optimizer_step():
    """PMLPPolicy.evaluate on the GPU (rows derived from the -1 padding), loss = (w logp).sum() - 0.01 ent.mean(), backward: the
    .grad of all four parameters within the gradient bound; after optimizer.step() a second evaluate sees the new weights."""
    import torch
    N, R, cols, hidden = 37, 40, 12, (128,)
    w = pc.make_weights(cols, hidden, 21)
    rows = np.resize(np.array((33, 2, 40, 17, 5, 32, 31), dtype=np.int32), N)
    obs = pc.fill_padding(pc.random_blocks(N, R, cols, 22), rows, False)
    rng = np.random.default_rng(23)
    actions = (rng.integers(0, 1 << 30, size=N) % rows).astype(np.int32)
    wt = rng.normal(size=N).astype(np.float32)
    pol = pc.to_policy(w, "cuda")
    opt = torch.optim.SGD(pol.parameters(), lr=0.05)
    st, act, wtd = to_cuda(obs, actions, wt)
    logp, ent = pol.evaluate(st, act)
    assert logp.requires_grad and logp.grad_fn is not None and type(logp.grad_fn).__name__.startswith("_PMLPEvaluate")
    loss = (wtd * logp).sum() - 0.01 * ent.mean()
    opt.zero_grad(); loss.backward()
    ref = pc.reference(w, obs, rows)
    want, A = gc.reference_grad(w, obs, rows, actions, wt, np.full(N, -0.01 / N), ref=ref)
    lin = pol.embedding[0]
    got = (lin.weight.grad.t().cpu().numpy(), lin.bias.grad.cpu().numpy(), pol.deciding.weight.grad.reshape(-1).cpu().numpy(),
           pol.deciding.bias.grad.reshape(-1).cpu().numpy())
    print("ratios autograd r_g=%.3f" % gc.grad_ratio(got, want, A, ref))
    gc.check_grads(got, want, A, ref, what="autograd")
    rl, rh, _ = gc.reference_eval(w, obs, rows, actions, ref=ref)
    assert (np.abs(logp.detach().cpu().numpy() - rl) <= ref.tol()).all()
    opt.step()
    w2 = pc.weights_of(pol)
    assert not np.array_equal(w2[0][0], w[0][0])
    logp2, ent2 = pol.evaluate(st, act, torch.from_numpy(rows).cuda())
    rl2, rh2, ref2 = gc.reference_eval(w2, obs, rows, actions)
    assert (np.abs(logp2.detach().cpu().numpy() - rl2) <= ref2.tol()).all()
    assert (np.abs(ent2.detach().cpu().numpy() - rh2) <= gc.entropy_tol(ref2)).all()
    assert np.abs(rl2 - rl).max() > 10 * ref2.tol().max(), "the step did not move the policy: the check above proves nothing"


def test_two_layers_take_the_torch_path_and_still_train():
    import torch
    w = pc.make_weights(12, (64, 64), 31)
    rows = np.array((5, 17, 2, 24), dtype=np.int32)
    obs = pc.fill_padding(pc.random_blocks(4, 24, 12, 32), rows, False)
    pol = pc.to_policy(w, "cuda")
    st, act = to_cuda(obs, np.array((4, 0, 1, 23), dtype=np.int32))
    logp, ent = pol.evaluate(st, act)
    assert not type(logp.grad_fn).__name__.startswith("_PMLPEvaluate")
    (logp.sum() - 0.01 * ent.mean()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0 for p in pol.parameters())
    rl, rh, ref = gc.reference_eval(w, obs, rows, act.cpu().numpy())
    assert (np.abs(logp.detach().cpu().numpy() - rl) <= ref.tol()).all()
