"""bbx_pmlp_value / bbx_pmlp_value_grad / bbx_pmlp_value_fit (and their _at forms) and the Python surface around them — PMLPValue,
DeviceTrajectoryBuffer.fill_values, run_rollout_fused(critic=...), value_update — on the device, against the float64 reference
of tests/value_cases.py (tests/test_value_model_cpu.py checks that reference against autograd in double precision): the values
of all three pools at every instantiation and tile boundary, the gradients where the partition of the positions changes, the
bit-for-bit relations include/bbx.h promises, and the training loop's plumbing.  Each case prints the ratio of its bound it
needed before it asserts (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_cases as pc
from tests import policy_grad_cases as gc
from tests import value_cases as vc
from tests.fast_harness import ptr, stream_ptr, to_cuda

pytestmark = pytest.mark.gpu
_ids = lambda v: str(v).replace(" ", "")
GUARD = 64


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


class Weights:
    """Prepared weights on the device (and the policy object that keeps them alive)."""

    def __init__(self, weights):
        self.w = weights
        self.keep = pc.to_policy(weights, "cuda")                    # (the critic's prepared layout IS the one-layer policy's)
        self.prep = self.keep._fused_weights()["prepared"]
        self.cols, self.hidden = weights[0][0].shape


def _src(obs, rows, index, n):
    R, cols = obs.shape[-2:]
    return (ptr(obs), ptr(rows)) + ((n,) if index is None else (rows.numel(), ptr(index), n)) + (R, cols)


def _value(W, obs, rows, pool, index=None, want32=True, want64=True):
    """bbx_pmlp_value[_at] through the C ABI -> (float32 [n] or None, float64 [n] or None) as numpy; guard bands checked."""
    import torch
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    n = rows.numel() if index is None else index.numel()
    v32 = torch.full((n + GUARD,), 7.0, device="cuda") if want32 else None
    v64 = torch.full((n + GUARD,), 7.0, dtype=torch.float64, device="cuda") if want64 else None
    fn = lib.bbx_pmlp_value if index is None else lib.bbx_pmlp_value_at
    _ffi.check(fn(*_src(obs, rows, index, n), W.prep, W.hidden, vc.POOL_ID[pool], ptr(v32), ptr(v64), stream_ptr()))
    torch.cuda.synchronize()
    out = []
    for v in (v32, v64):
        if v is None:
            out.append(None)
        else:
            h = v.cpu().numpy()
            assert (h[n:] == 7.0).all(), "written beyond the n values"
            out.append(h[:n].copy())
    return tuple(out)


def _grad_outputs(W):
    import torch
    sizes = (W.cols * W.hidden, W.hidden, W.hidden, 1)
    buf = torch.full((sum(sizes) + 5 * GUARD,), float("nan"), device="cuda")
    offs = np.cumsum([GUARD] + [s + GUARD for s in sizes[:-1]])
    return buf, sizes, offs, [buf[int(o):int(o) + s] for o, s in zip(offs, sizes)]


def _read_grads(W, buf, sizes, offs):
    host = buf.cpu().numpy()
    inside = np.zeros(len(host), dtype=bool)
    for o, s in zip(offs, sizes):
        inside[int(o):int(o) + s] = True
    assert np.isnan(host[~inside]).all(), "the guard bands around the gradient outputs were written"
    got = [host[int(o):int(o) + s].copy() for o, s in zip(offs, sizes)]
    got[0] = got[0].reshape(W.cols, W.hidden)
    return tuple(got)


def _vgrad(W, obs, rows, pool, gvalue, index=None):
    """bbx_pmlp_value_grad[_at] through the C ABI -> (gW1 [cols][hidden], gb1, gw2, gb2) as numpy; guard bands checked."""
    import torch
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    n = rows.numel() if index is None else index.numel()
    R = obs.shape[-2]
    buf, sizes, offs, outs = _grad_outputs(W)
    nfl = lib.bbx_pmlp_value_grad_workspace_floats(n, R, W.cols, W.hidden)
    assert nfl > 0
    ws = torch.full((nfl + GUARD,), float("nan"), device="cuda")
    fn = lib.bbx_pmlp_value_grad if index is None else lib.bbx_pmlp_value_grad_at
    _ffi.check(fn(*_src(obs, rows, index, n), W.prep, W.hidden, vc.POOL_ID[pool], ptr(gvalue), ptr(ws), *[ptr(o) for o in outs], stream_ptr()))
    torch.cuda.synchronize()
    assert np.isnan(ws[nfl:].cpu().numpy()).all(), "the workspace was overrun"
    return _read_grads(W, buf, sizes, offs)


def _fit(W, obs, rows, pool, targets, scale, index=None):
    """bbx_pmlp_value_fit[_at] -> (values [n], coef [n], stats [6], the four gradients) as numpy; guard bands checked."""
    import torch
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    n = rows.numel() if index is None else index.numel()
    R = obs.shape[-2]
    buf, sizes, offs, outs = _grad_outputs(W)
    nfl = lib.bbx_pmlp_value_fit_workspace_floats(n, R, W.cols, W.hidden)
    assert nfl > 0
    ws = torch.full((nfl + GUARD,), float("nan"), device="cuda")
    values = torch.full((n + GUARD,), 7.0, device="cuda"); coef = torch.full((n + GUARD,), 7.0, device="cuda")
    stats = torch.full((6 + GUARD,), 7.0, dtype=torch.float64, device="cuda")
    fn = lib.bbx_pmlp_value_fit if index is None else lib.bbx_pmlp_value_fit_at
    _ffi.check(fn(*_src(obs, rows, index, n), W.prep, W.hidden, vc.POOL_ID[pool], ptr(targets), C.c_float(scale), ptr(values), ptr(coef), ptr(stats),
                  ptr(ws), *[ptr(o) for o in outs], stream_ptr()))
    torch.cuda.synchronize()
    assert np.isnan(ws[nfl:].cpu().numpy()).all(), "the workspace was overrun"
    v, c, s = values.cpu().numpy(), coef.cpu().numpy(), stats.cpu().numpy()
    assert (v[n:] == 7.0).all() and (c[n:] == 7.0).all() and (s[6:] == 7.0).all(), "written beyond the outputs"
    return v[:n].copy(), c[:n].copy(), s[:6].copy(), _read_grads(W, buf, sizes, offs)


# ---- values ------------------------------------------------------------------------------------------------------------------
def _check_values(W, w, obs, rows, what):
    """All three pools of one block against float64; returns the largest ratio of the sum / mean pools."""
    ref = pc.reference(w, obs, rows)
    dobs, drows = to_cuda(obs, rows)
    worst = 0.0
    got = {}
    for pool in vc.POOLS:
        want, _ = vc.reference_values(w, obs, rows, pool, ref=ref)
        v32, v64 = _value(W, dobs, drows, pool)
        got[pool] = v32
        r = vc.value_ratio(ref, pool, v32, want)
        print("ratios %-50s %-4s N=%-3d r_v=%.3f" % (what, pool, len(rows), r))
        assert np.isfinite(v32).all(), (what, pool)
        assert (v32[ref.n <= 0] == 0.0).all() and not np.signbit(v32[ref.n <= 0]).any(), (what, pool, "a state without rows is worth 0.0f")
        assert np.array_equal(_bits(v64), _bits(v32.astype(np.float64))), (what, pool, "d_values64 is d_values widened")
        bad = np.abs(v32 - want) > vc.value_tol(ref, pool, want)
        assert not bad.any(), (what, pool, np.flatnonzero(bad)[:5].tolist(), r)
        if pool != "lse":
            worst = max(worst, r)
    one = ref.n == 1
    assert np.array_equal(_bits(got["sum"][one]), _bits(got["mean"][one])), (what, "sum and mean agree bit for bit on one live row")
    return worst


@pytest.mark.parametrize("cols,hidden", pc.one_layer_shapes(), ids=_ids)
def test_values_against_float64(cols, hidden):
    """Per shape and pool: nine states with the live-row counts around the tiles of 32 rows and the wave of 64 (blocks of 136 rows,
    garbage beyond the live rows), five with row counts of 0, negative and above obs_rows (clamped), and a single one-row block:
    n = 9, 5, 1.  Each value within its bound; 0.0f without rows; d_values64 the float widened; only one of the two outputs."""
    w = pc.make_weights(cols, hidden, 700)
    W = Weights(w)
    worst = 0.0
    for rows, R, seed in ((vc.LIVE_ROWS, 136, 701), ((15, 0, 7, -3, 20), 15, 702), ((5,), 1, 703)):
        _, obs, rows = vc.value_case(cols, hidden, rows, R, seed)
        assert len(rows) in vc.BATCHES
        worst = max(worst, _check_values(W, w, obs, rows, "values %s R=%d" % (pc.label(cols, hidden), R)))
    print("worst %s r_v=%.3f" % (pc.label(cols, hidden), worst))
    _, obs, rows = vc.value_case(cols, hidden, (15, 0, 7, -3, 20), 15, 702)
    dobs, drows = to_cuda(obs, rows)
    both = _value(W, dobs, drows, "mean")
    only32, none = _value(W, dobs, drows, "mean", want64=False)
    none2, only64 = _value(W, dobs, drows, "mean", want32=False)
    assert none is None and none2 is None and np.array_equal(_bits(only32), _bits(both[0])) and np.array_equal(_bits(only64), _bits(both[1]))


def test_values_of_tall_blocks():
    """2047 and 2048 live rows of a 2048-row block at 12 x 128: every lane adds 32 scores before the tree."""
    w = pc.make_weights(12, (128,), 710)
    _, obs, rows = vc.value_case(12, (128,), vc.TALL_ROWS, 2048, 711)
    r = _check_values(Weights(w), w, obs, rows, "values 12x128 tall")
    print("worst tall r_v=%.3f" % r)


# ---- gradients ---------------------------------------------------------------------------------------------------------------
GRAD_SHAPES = [(1, (1,)), (12, (128,)), (33, (64,)), (64, (256,))]


def _run_grad(W, w, obs, rows, gvalue, pool, what):
    want, A = vc.reference_grad(w, obs, rows, gvalue, pool)
    got = _vgrad(W, *to_cuda(obs, rows), pool, to_cuda(gvalue)[0])
    r = gc.grad_ratio(got, want, A)
    print("ratios %-50s %-4s N=%-5d r_vg=%.3f" % (what, pool, len(rows), r))
    gc.check_grads(got, want, A, None, c_g=vc.C_VG, what=(what, pool))
    return got


@pytest.mark.parametrize("pool", vc.POOLS)
@pytest.mark.parametrize("cols,hidden", GRAD_SHAPES, ids=_ids)
def test_gradients_against_float64(cols, hidden, pool):
    """Five states with row counts over the tile edges, 0 and 1 (garbage beyond them; the gvalue of the state without rows is NaN
    and must not be read), then 1030 states of 4 rows: several states to every wave, hundreds of partials per output in the reduce."""
    w, obs, rows, gvalue = vc.grad_case(cols, hidden, (33, 0, 129, 1, 2), 136, 720)
    gvalue[1] = np.nan
    W = Weights(w)
    _run_grad(W, w, obs, rows, gvalue, pool, "vgrad %s" % pc.label(cols, hidden))
    N = 1030
    _, obs, rows, gvalue = vc.grad_case(cols, hidden, (4,) * N, 4, 721)
    _run_grad(W, w, obs, rows, gvalue, pool, "vgrad %s" % pc.label(cols, hidden))


@pytest.mark.parametrize("pool", vc.POOLS)
def test_one_row_states_contribute_and_rowless_states_do_not(pool):
    """A call made only of one-row states has the reference's (non-zero) gradient — the policy's gradient kernel would skip every
    one of them; states without rows among them, whatever their gvalue, leave the bits as they are."""
    w, obs, rows, gvalue = vc.grad_case(12, (128,), (1,) * 7, 5, 730)
    W = Weights(w)
    got = _run_grad(W, w, obs, rows, gvalue, pool, "vgrad one-row states")
    assert abs(got[3][0]) > 0 and np.abs(got[0]).max() > 0 and np.abs(got[2]).max() > 0
    assert abs(float(got[3][0]) - float(gvalue.astype(np.float64).sum())) <= 8 * vc.EPS * np.abs(gvalue).sum()
    # rowless states among them (a longer call: another partition of the positions, so held to the reference, which leaves them
    # out, not to the bits above): a gvalue of NaN, 1e30 or -inf there would show in every output if it were read
    rows2 = np.concatenate([rows[:3], np.array([0, -5], dtype=np.int32), rows[3:], np.array([0], dtype=np.int32)])
    obs2 = np.concatenate([obs[:3], obs[:2], obs[3:], obs[:1]])
    gv2 = np.concatenate([gvalue[:3], np.array([np.nan, 1e30], dtype=np.float32), gvalue[3:], np.array([-np.inf], dtype=np.float32)])
    got2 = _run_grad(W, w, obs2, rows2, gv2, pool, "vgrad one-row + rowless states")
    assert all(np.isfinite(x).all() for x in got2)


# ---- bit-for-bit relations -----------------------------------------------------------------------------------------------------
def _buffer_case(seed=740, S=23):
    rows = np.resize(np.array((33, 0, 17, 1, 2, 64, 40, 5, 31, 32), dtype=np.int32), S)
    w, obs, rows, _ = vc.grad_case(12, (128,), rows, 40, seed)
    return w, obs, rows


@pytest.mark.parametrize("pool", vc.POOLS)
def test_indexed_calls_equal_the_contiguous_calls_on_gathered_arrays(pool):
    """A permuted index with repeated entries: values, gradients and the whole fit call equal, bit for bit, the calls without _at
    on obs[index], rows[index]."""
    w, obs, rows = _buffer_case()
    W = Weights(w)
    rng = np.random.default_rng(741)
    index = np.concatenate([rng.permutation(len(rows)), rng.integers(0, len(rows), size=14)]).astype(np.int32)
    gvalue = rng.normal(size=len(index)).astype(np.float32); targets = rng.normal(size=len(index)).astype(np.float32)
    dobs, drows, dindex, dgv, dtg = to_cuda(obs, rows, index, gvalue, targets)
    gobs, grows = to_cuda(obs[index], rows[index])
    a = _value(W, dobs, drows, pool, dindex); b = _value(W, gobs, grows, pool)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    ga = _vgrad(W, dobs, drows, pool, dgv, dindex); gb = _vgrad(W, gobs, grows, pool, dgv)
    for x, y in zip(ga, gb):
        assert np.array_equal(_bits(x), _bits(y))
    fa = _fit(W, dobs, drows, pool, dtg, 0.25, dindex); fb = _fit(W, gobs, grows, pool, dtg, 0.25)
    assert np.array_equal(_bits(fa[0]), _bits(fb[0])) and np.array_equal(_bits(fa[1]), _bits(fb[1])) and np.array_equal(_bits(fa[2]), _bits(fb[2]))
    for x, y in zip(fa[3], fb[3]):
        assert np.array_equal(_bits(x), _bits(y))


@pytest.mark.parametrize("pool", vc.POOLS)
def test_an_index_out_of_range_gives_nan_and_contributes_nothing(pool):
    """Indices -1 and n_src: NaN values, coef 0, not counted, nothing read there (gvalue NaN at those positions).  The gradients
    equal, BIT FOR BIT, those of the call in which these positions point at a state without rows instead (the same partition of
    the positions over the waves); against the call with the positions REMOVED the partition differs — position k goes to wave
    k mod waves — so those are held within the float bound."""
    w, obs, rows = _buffer_case(750)
    rows[1] = 0                                                          # (a state without rows to stand in)
    W = Weights(w)
    S = len(rows)
    rng = np.random.default_rng(751)
    index = rng.integers(0, S, size=19).astype(np.int32)
    bad = np.array([3, 11])
    index[bad] = (-1, S)
    keep = np.setdiff1d(np.arange(len(index)), bad)
    gvalue = rng.normal(size=len(index)).astype(np.float32); gvalue[bad] = np.nan
    targets = rng.normal(size=len(index)).astype(np.float32)
    dobs, drows, dindex, dgv, dtg = to_cuda(obs, rows, index, gvalue, targets)
    v32, v64 = _value(W, dobs, drows, pool, dindex)
    assert np.isnan(v32[bad]).all() and np.isnan(v64[bad]).all() and np.isfinite(v32[keep]).all()
    got = _vgrad(W, dobs, drows, pool, dgv, dindex)
    standin = index.copy(); standin[bad] = 1
    same = _vgrad(W, dobs, drows, pool, dgv, to_cuda(standin)[0])
    for x, y in zip(got, same):
        assert np.array_equal(_bits(x), _bits(y))
    want, A = vc.reference_grad(w, obs[index[keep]], rows[index[keep]], gvalue[keep], pool)
    removed = _vgrad(W, dobs, drows, pool, to_cuda(gvalue[keep])[0], to_cuda(index[keep])[0])
    gc.check_grads(got, want, A, None, c_g=vc.C_VG, what="out of range")
    gc.check_grads(removed, want, A, None, c_g=vc.C_VG, what="removed")
    # the fit call: coef 0 and not counted there; an empty source: every index is out of range
    fv, fc, fs, fg = _fit(W, dobs, drows, pool, dtg, 0.5, dindex)
    assert np.isnan(fv[bad]).all() and (fc[bad] == 0.0).all() and fs[0] == len(keep) and fs[5] == len(bad)
    allbad = to_cuda(np.full(len(index), 7, dtype=np.int32))[0]           # a source of one state: every index is out of range
    fv, fc, fs, fg = _fit(W, dobs[:1].contiguous(), drows[:1].contiguous(), pool, dtg, 0.5, allbad)
    assert np.isnan(fv).all() and (fc == 0.0).all() and fs[0] == 0 and fs[5] == len(index) and all((g == 0).all() for g in fg)


@pytest.mark.parametrize("pool", vc.POOLS)
def test_the_fit_call_is_its_three_parts_bit_for_bit(pool):
    """Values = bbx_pmlp_value's; coef = the float32 recipe in numpy; gradients = bbx_pmlp_value_grad's with d_gvalue = d_coef;
    statistics = numpy's double sums of the float32 terms (1e-12 relative; the counts exactly); two calls give the same bits;
    n == 0 zeroes gradients and statistics."""
    w, obs, rows = _buffer_case(760, S=1030)
    W = Weights(w)
    targets = np.random.default_rng(761).normal(size=len(rows)).astype(np.float32) * 3
    scale = 1.0 / len(rows)
    dobs, drows, dtg = to_cuda(obs, rows, targets)
    v, coef, stats, grads = _fit(W, dobs, drows, pool, dtg, scale)
    v32, _ = _value(W, dobs, drows, pool)
    assert np.array_equal(_bits(v), _bits(v32))
    want_coef, _, counted = vc.fit_recipe(v, targets, np.float32(scale))
    assert counted.all() and np.array_equal(_bits(coef), _bits(want_coef))
    parts = _vgrad(W, dobs, drows, pool, to_cuda(coef)[0])
    for x, y in zip(grads, parts):
        assert np.array_equal(_bits(x), _bits(y))
    want = vc.fit_stats(v, targets, np.float32(scale))
    assert stats[0] == want[0] == len(rows) and stats[5] == want[5] == 0
    assert (np.abs(stats - want) <= 1e-12 * np.abs(want)).all(), (stats, want)
    again = _fit(W, dobs, drows, pool, dtg, scale)
    assert np.array_equal(_bits(again[0]), _bits(v)) and np.array_equal(_bits(again[1]), _bits(coef)) and np.array_equal(_bits(again[2]), _bits(stats))
    for x, y in zip(again[3], grads):
        assert np.array_equal(_bits(x), _bits(y))
    vg = _vgrad(W, dobs, drows, pool, dtg); vg2 = _vgrad(W, dobs, drows, pool, dtg)
    for x, y in zip(vg, vg2):
        assert np.array_equal(_bits(x), _bits(y))
    import torch
    z = _fit(W, torch.zeros((0, 40, 12), dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), pool, None, 1.0)
    assert (z[2] == 0).all() and all((g == 0).all() for g in z[3])


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def _param_grads(critic):
    lin = critic.embedding[0]
    return (lin.weight.grad.t().contiguous().cpu().numpy(), lin.bias.grad.cpu().numpy(), critic.head.weight.grad.reshape(-1).cpu().numpy(),
            critic.head.bias.grad.reshape(-1).cpu().numpy())


@pytest.mark.parametrize("pool", vc.POOLS)
def test_evaluate_backward_equals_the_abi(pool):
    """PMLPValue.evaluate(...).sum().backward(): the values are bbx_pmlp_value's and the .grad of the four parameters
    bbx_pmlp_value_grad's with gvalue = 1, bit for bit; evaluate_at on a buffer the same on the gathered states; two hidden
    layers take the torch path and say so."""
    import torch
    w, obs, rows = _buffer_case(770)
    W = Weights(w)
    critic = vc.to_critic(w, pool, "cuda")
    dobs, drows = to_cuda(obs, rows)
    v = critic.evaluate(dobs, drows)
    assert critic.last_path == "kernels" and v.requires_grad and type(v.grad_fn).__name__.startswith("_PMLPValueEvaluate")
    v.sum().backward()
    want_v, _ = _value(W, dobs, drows, pool)
    assert np.array_equal(_bits(v.detach().cpu().numpy()), _bits(want_v))
    want_g = _vgrad(W, dobs, drows, pool, torch.ones(len(rows), device="cuda"))
    for x, y in zip(_param_grads(critic), want_g):
        assert np.array_equal(_bits(x), _bits(y))
    index = np.array([5, 5, 0, 22, 7, 3], dtype=np.int32)
    critic.zero_grad()
    va = critic.evaluate_at(dobs, drows, torch.from_numpy(index).cuda())
    (2.0 * va).sum().backward()
    gobs, grows = to_cuda(obs[index], rows[index])
    want_g = _vgrad(W, gobs, grows, pool, torch.full((len(index),), 2.0, device="cuda"))
    for x, y in zip(_param_grads(critic), want_g):
        assert np.array_equal(_bits(x), _bits(y))
    deep = vc.to_critic(pc.make_weights(12, (64, 64), 771), pool, "cuda")
    vd = deep.evaluate(dobs, drows)
    assert deep.last_path == "torch" and not type(vd.grad_fn).__name__.startswith("_PMLPValueEvaluate")
    vd.sum().backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in deep.parameters())


def test_fit_step_at_in_place_equals_fit_step_on_the_gathered_copy():
    """fit_step_at over a [T, B, R, cols] buffer in place and fit_step on states[index]: the same statistics, values and .grad,
    bit for bit; a second call ADDS to .grad; after an optimiser step the prepared weights are refilled."""
    import torch
    w, obs, rows = _buffer_case(780, S=24)
    critic = vc.to_critic(w, "mean", "cuda"); other = vc.to_critic(w, "mean", "cuda")
    dobs, drows = to_cuda(obs.reshape(4, 6, 40, 12), rows.reshape(4, 6))
    index = torch.from_numpy(np.array([23, 1, 1, 8, 15, 0, 4], dtype=np.int64)).cuda()
    targets = torch.linspace(-2, 2, 7, device="cuda")
    st_a, v_a = critic.fit_step_at(dobs, drows, index, targets)
    flat_obs, flat_rows = dobs.view(-1, 40, 12), drows.view(-1)
    st_b, v_b = other.fit_step(flat_obs[index], flat_rows[index], targets)
    assert critic.last_path == "kernels" and other.last_path == "kernels"
    assert torch.equal(st_a, st_b) and torch.equal(v_a, v_b)
    first = _param_grads(critic)
    for x, y in zip(first, _param_grads(other)):
        assert np.array_equal(_bits(x), _bits(y))
    critic.fit_step_at(dobs, drows, index, targets)
    for x, y in zip(_param_grads(critic), first):
        assert np.array_equal(x, 2 * y)
    opt = torch.optim.SGD(critic.parameters(), lr=0.1)
    before = critic.values(flat_obs, flat_rows).clone()
    opt.step()
    after = critic.values(flat_obs, flat_rows)
    assert not torch.equal(before, after)
    want, ref = vc.reference_values(_weights_of(critic), obs, rows, "mean")
    assert (np.abs(after.cpu().numpy() - want) <= vc.value_tol(ref, "mean", want)).all()


def _weights_of(critic):
    f = lambda t: t.detach().cpu().numpy().astype(np.float32)
    return [(f(critic.embedding[0].weight).T.copy(), f(critic.embedding[0].bias)), (f(critic.head.weight).reshape(-1), f(critic.head.bias).reshape(-1))]


@pytest.fixture(scope="module")
def rollout_pair():
    """The same fused rollout twice, same seeds: with a critic and without (3-20-10-weighted, B = 64, 64-row blocks, 8 steps)."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, PMLPValue, run_rollout_fused
    B, R, T = 64, 64, 8
    torch.manual_seed(5)
    policy = PMLPPolicy(12, (128,)).cuda()
    critic = PMLPValue(12, (64,), pool="mean").cuda()
    out = []
    for cr in (critic, None):
        env = VecLeadMonomialsEnv("3-20-10-weighted", batch=B, k=2)
        env.seed(np.arange(B) + 100)
        env.reset()
        buf = DeviceTrajectoryBuffer(T, B, obs_shape=(R, 12))
        gen = torch.Generator(device="cuda"); gen.manual_seed(11)
        run_rollout_fused(env, policy, T, buf, generator=gen, critic=cr)
        torch.cuda.synchronize()
        out.append(buf)
    return critic, out[0], out[1]


def test_run_rollout_fused_fills_the_values_and_leaves_the_rollout_alone(rollout_pair):
    import torch
    critic, with_critic, without = rollout_pair
    R, cols = with_critic.states.shape[2:]
    assert with_critic.t == 8 and without.t == 8
    want = critic.values(with_critic.states.view(-1, R, cols), with_critic.rows.view(-1))
    assert critic.last_path == "kernels"
    assert torch.equal(with_critic.values.view(-1), want.to(torch.float64)) and float(with_critic.values.abs().max()) > 0
    assert (without.values == 0).all()
    for name in ("actions", "rewards", "logprobs", "dones", "rows", "states"):
        assert torch.equal(getattr(with_critic, name), getattr(without, name)), name
    with pytest.raises(ValueError):
        from deepgroebner_amd.rollout import DeviceTrajectoryBuffer
        DeviceTrajectoryBuffer(8, 64).fill_values(critic)


def test_value_update_reduces_the_loss(rollout_pair):
    """Three epochs with Adam (lr 1e-3), a fixed seed: the reported loss falls — a check of the signs.  value_update fits the
    steps of COMPLETE episodes (get_index), and no episode of 3-20-10-weighted ends within the 8 steps of the buffers above (the
    shortest of these seeds under a random agent takes 17): on that buffer an epoch has nothing to report, which is checked; the
    update itself runs on the same environments and critic stepped on for 48 steps into 256-row blocks."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, run_rollout_fused, value_update
    critic, short, _ = rollout_pair
    opt = torch.optim.Adam(critic.parameters(), lr=1e-3)
    if int(short.get_index(None)[0].numel()) == 0:
        none = value_update(critic, short, opt, 1, 64)
        assert none[0]["stats"].shape == (0, 6) and none[0]["loss"] == 0.0
    B, T = 64, 48
    torch.manual_seed(5)
    policy = PMLPPolicy(12, (128,)).cuda()
    env = VecLeadMonomialsEnv("3-20-10-weighted", batch=B, k=2)
    env.seed(np.arange(B) + 100)
    env.reset()
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(256, 12))
    gen = torch.Generator(device="cuda"); gen.manual_seed(11)
    run_rollout_fused(env, policy, T, buf, generator=gen, critic=critic)
    assert int(buf.get_index(None)[0].numel()) > 2 * 64
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    out = value_update(critic, buf, opt, 3, 64, generator=gen)
    print("value_update losses", [o["loss"] for o in out], "explained variance", [o["explained_variance"] for o in out])
    assert len(out) == 3 and all(o["stats"].shape[1] == 6 and (o["stats"][:, 5] == 0).all() for o in out)
    assert critic.last_path == "kernels"
    assert out[-1]["loss"] < out[0]["loss"]
