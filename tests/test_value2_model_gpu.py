"""bbx_pmlp2_value / bbx_pmlp2_value_grad / bbx_pmlp2_value_fit (and their _at forms) and the Python surface around them — PMLPValue with
deep_kernels, DeviceTrajectoryBuffer.fill_values, run_rollout_fused(critic=...), value_update — on the device, against the float64
reference of tests/value2_cases.py (tests/test_value2_model_cpu.py checks that reference against autograd in double precision): the
values of all three pools at every padded-size pair and k-step count, the gradients where the partition of the positions changes,
exact-integer cases, the bit-for-bit relations include/bbx.h promises, and the training loop's plumbing.  Each case prints the ratio of
its bound it needed before it asserts (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

from tests import policy2_grad_cases as g2
from tests import policy_cases as pc
from tests import policy_grad_cases as gc
from tests import value2_cases as v2
from tests import value_cases as vc
from tests.fast_harness import ptr, stream_ptr, to_cuda

pytestmark = pytest.mark.gpu
_ids = lambda v: str(v).replace(" ", "")
GUARD = 64


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _same(xs, ys):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


class Weights:
    """Prepared weights on the device (and the policy object that keeps them alive)."""

    def __init__(self, weights):
        self.w = weights
        self.keep = pc.to_policy(weights, "cuda")                    # (the critic's prepared layout IS the two-layer policy's)
        self.prep = self.keep._deep_weights()["prepared"]
        self.cols = weights[0][0].shape[0]
        self.hidden = (weights[0][0].shape[1], weights[1][0].shape[1])
        h1, h2 = self.hidden
        self.sizes = (self.cols * h1, h1, h1 * h2, h2, h2, 1)


def _src(obs, rows, index, n):
    R, cols = obs.shape[-2:]
    return (ptr(obs), ptr(rows)) + ((n,) if index is None else (rows.numel(), ptr(index), n)) + (R, cols)


def _value(W, obs, rows, pool, index=None, want32=True, want64=True):
    """bbx_pmlp2_value[_at] through the C ABI -> (float32 [n] or None, float64 [n] or None) as numpy; guard bands checked."""
    import torch
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    n = rows.numel() if index is None else index.numel()
    v32 = torch.full((n + GUARD,), 7.0, device="cuda") if want32 else None
    v64 = torch.full((n + GUARD,), 7.0, dtype=torch.float64, device="cuda") if want64 else None
    fn = lib.bbx_pmlp2_value if index is None else lib.bbx_pmlp2_value_at
    _ffi.check(fn(*_src(obs, rows, index, n), W.prep, *W.hidden, vc.POOL_ID[pool], ptr(v32), ptr(v64), stream_ptr()))
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
    buf = torch.full((sum(W.sizes) + 7 * GUARD,), float("nan"), device="cuda")
    offs = np.cumsum([GUARD] + [s + GUARD for s in W.sizes[:-1]])
    return buf, offs, [buf[int(o):int(o) + s] for o, s in zip(offs, W.sizes)]


def _read_grads(W, buf, offs):
    host = buf.cpu().numpy()
    inside = np.zeros(len(host), dtype=bool)
    for o, s in zip(offs, W.sizes):
        inside[int(o):int(o) + s] = True
    assert np.isnan(host[~inside]).all(), "the guard bands around the gradient outputs were written"
    got = [host[int(o):int(o) + s].copy() for o, s in zip(offs, W.sizes)]
    got[0] = got[0].reshape(W.cols, W.hidden[0]); got[2] = got[2].reshape(W.hidden)
    return tuple(got)


def _vgrad(W, obs, rows, pool, gvalue, index=None):
    """bbx_pmlp2_value_grad[_at] through the C ABI -> the six gradients as numpy; guard bands checked."""
    import torch
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    n = rows.numel() if index is None else index.numel()
    R = obs.shape[-2]
    buf, offs, outs = _grad_outputs(W)
    nfl = lib.bbx_pmlp2_value_grad_workspace_floats(n, R, W.cols, *W.hidden)
    assert nfl > 0
    ws = torch.full((nfl + GUARD,), float("nan"), device="cuda")
    fn = lib.bbx_pmlp2_value_grad if index is None else lib.bbx_pmlp2_value_grad_at
    _ffi.check(fn(*_src(obs, rows, index, n), W.prep, *W.hidden, vc.POOL_ID[pool], ptr(gvalue), ptr(ws), *[ptr(o) for o in outs], stream_ptr()))
    torch.cuda.synchronize()
    assert np.isnan(ws[nfl:].cpu().numpy()).all(), "the workspace was overrun"
    return _read_grads(W, buf, offs)


def _fit(W, obs, rows, pool, targets, scale, index=None, stats=True):
    """bbx_pmlp2_value_fit[_at] -> (values [n], coef [n], stats [6] or None, the six gradients) as numpy; guard bands checked."""
    import torch
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    n = rows.numel() if index is None else index.numel()
    R = obs.shape[-2]
    buf, offs, outs = _grad_outputs(W)
    nfl = lib.bbx_pmlp2_value_fit_workspace_floats(n, R, W.cols, *W.hidden)
    assert nfl > 0
    ws = torch.full((nfl + GUARD,), float("nan"), device="cuda")
    values = torch.full((n + GUARD,), 7.0, device="cuda"); coef = torch.full((n + GUARD,), 7.0, device="cuda")
    st = torch.full((6 + GUARD,), 7.0, dtype=torch.float64, device="cuda") if stats else None
    fn = lib.bbx_pmlp2_value_fit if index is None else lib.bbx_pmlp2_value_fit_at
    _ffi.check(fn(*_src(obs, rows, index, n), W.prep, *W.hidden, vc.POOL_ID[pool], ptr(targets), C.c_float(scale), ptr(values), ptr(coef), ptr(st),
                  ptr(ws), *[ptr(o) for o in outs], stream_ptr()))
    torch.cuda.synchronize()
    assert np.isnan(ws[nfl:].cpu().numpy()).all(), "the workspace was overrun"
    v, c = values.cpu().numpy(), coef.cpu().numpy()
    assert (v[n:] == 7.0).all() and (c[n:] == 7.0).all(), "written beyond the outputs"
    s = None
    if stats:
        s = st.cpu().numpy()
        assert (s[6:] == 7.0).all(), "written beyond the statistics"
        s = s[:6].copy()
    return v[:n].copy(), c[:n].copy(), s, _read_grads(W, buf, offs)


# ---- values ------------------------------------------------------------------------------------------------------------------
def _check_values(W, w, obs, rows, what):
    """All three pools of one block against float64; returns the largest ratio of the sum / mean pools."""
    ref = pc.reference(w, obs, rows)
    dobs, drows = to_cuda(obs, rows)
    worst = 0.0
    got = {}
    for pool in v2.POOLS:
        want, _ = vc.reference_values(w, obs, rows, pool, ref=ref)
        v32, v64 = _value(W, dobs, drows, pool)
        got[pool] = v32
        r = vc.value_ratio(ref, pool, v32, want)
        print("ratios %-50s %-4s N=%-3d r_v2=%.3f" % (what, pool, len(rows), r))
        assert np.isfinite(v32).all(), (what, pool)
        assert (v32[ref.n <= 0] == 0.0).all() and not np.signbit(v32[ref.n <= 0]).any(), (what, pool, "a state without rows is worth 0.0f")
        assert np.array_equal(_bits(v64), _bits(v32.astype(np.float64))), (what, pool, "d_values64 is d_values widened")
        bad = np.abs(v32 - want) > vc.value_tol(ref, pool, want, c_v=v2.C_V2)
        assert not bad.any(), (what, pool, np.flatnonzero(bad)[:5].tolist(), r)
        if pool != "lse":
            worst = max(worst, r)
    one = ref.n == 1
    assert np.array_equal(_bits(got["sum"][one]), _bits(got["mean"][one])), (what, "sum and mean agree bit for bit on one live row")
    return worst


@pytest.mark.parametrize("cols,hidden", v2.VALUE_SHAPES, ids=_ids)
def test_values_against_float64(cols, hidden):
    """Per shape and pool: fifteen states with 0, negative, more than obs_rows (clamped) and the live-row counts around the tiles of
    16 rows and the wave of 64, in blocks of 129 rows with garbage beyond the live rows; a single one-row block.  Each value within
    its bound; 0.0f without rows; d_values64 the float widened; only one of the two outputs."""
    w = pc.make_weights(cols, hidden, 800)
    W = Weights(w)
    worst = 0.0
    for rows, R, seed in ((v2.SWEEP_ROWS, v2.SWEEP_R, 801), ((5,), 1, 803)):
        _, obs, rows = v2.value_case(cols, hidden, rows, R, seed)
        worst = max(worst, _check_values(W, w, obs, rows, "values2 %s R=%d" % (pc.label(cols, hidden), R)))
    print("worst %s r_v2=%.3f" % (pc.label(cols, hidden), worst))
    _, obs, rows = v2.value_case(cols, hidden, (15, 0, 7, -3, 20), 15, 802)
    dobs, drows = to_cuda(obs, rows)
    both = _value(W, dobs, drows, "mean")
    only32, none = _value(W, dobs, drows, "mean", want64=False)
    none2, only64 = _value(W, dobs, drows, "mean", want32=False)
    assert none is None and none2 is None and np.array_equal(_bits(only32), _bits(both[0])) and np.array_equal(_bits(only64), _bits(both[1]))


def test_values_of_tall_blocks():
    """2047 and 2048 live rows of a 2048-row block at 12 x 128 x 128: 128 tiles per state, every lane adds 32 scores before the tree."""
    w = pc.make_weights(12, (128, 128), 810)
    _, obs, rows = v2.value_case(12, (128, 128), v2.TALL_ROWS, 2048, 811)
    r = _check_values(Weights(w), w, obs, rows, "values2 12x128x128 tall")
    print("worst tall r_v2=%.3f" % r)


@pytest.mark.parametrize("pool", v2.POOLS)
def test_values_beyond_one_round_of_the_grid(pool):
    """4200 two-row states at 12 x 64 x 64: more positions than 2 x CUs x waves, so the waves stride; the values equal, bit for bit,
    the same states evaluated in slices of 64 (one workgroup round each)."""
    import torch
    N = 4200
    assert N > 2 * torch.cuda.get_device_properties(0).multi_processor_count * 8
    w, obs, rows = v2.value_case(12, (64, 64), (2,) * N, 2, 820)
    W = Weights(w)
    dobs, drows = to_cuda(obs, rows)
    whole, _ = _value(W, dobs, drows, pool, want64=False)
    parts = np.concatenate([_value(W, dobs[i:i + 64], drows[i:i + 64], pool, want64=False)[0] for i in range(0, N, 64)])
    assert np.array_equal(_bits(whole), _bits(parts))
    want, ref = vc.reference_values(w, obs, rows, pool)
    assert (np.abs(whole - want) <= vc.value_tol(ref, pool, want, c_v=v2.C_V2)).all()


# ---- gradients ---------------------------------------------------------------------------------------------------------------
def _run_grad(W, w, obs, rows, gvalue, pool, what):
    want, A = v2.reference_grad2(w, obs, rows, gvalue, pool)
    got = _vgrad(W, *to_cuda(obs, rows), pool, to_cuda(gvalue)[0])
    r = gc.grad_ratio(got, want, A)
    print("ratios %-50s %-4s N=%-5d r_vg2=%.3f" % (what, pool, len(rows), r))
    v2.check_grads(got, want, A, what=(what, pool))
    return got


GRAD_ROWS = {1: (33,), 5: (33, 0, 129, 1, 2), 9: (15, 16, 17, 31, 32, 63, 64, 65, -3)}      # N -> rows of the sweep, in blocks of 134 rows


@pytest.mark.parametrize("pool", v2.POOLS)
@pytest.mark.parametrize("cols,hidden", v2.GRAD_SHAPES, ids=_ids)
def test_gradients_against_float64(cols, hidden, pool):
    """N = 1, 5 and 9 states with row counts over the tile edges, 0, negative and 1 (garbage beyond them; the gvalue of a state
    without rows is NaN and must not be read)."""
    w = pc.make_weights(cols, hidden, 830)
    W = Weights(w)
    for N in v2.BATCHES:
        _, obs, rows, gvalue = v2.grad_case(cols, hidden, GRAD_ROWS[N], 134, 830 + N)
        gvalue[rows <= 0] = np.nan
        _run_grad(W, w, obs, rows, gvalue, pool, "vgrad2 %s" % pc.label(cols, hidden))


@pytest.mark.parametrize("pool", v2.POOLS)
def test_gradients_with_more_positions_than_the_partition_has_slots(pool):
    """More four-row states than PMLP2_GRAD_STATES_PER_GROUP x PMLP2_GRAD_MAX_GROUPS at 12 x 64 x 64: every workgroup strides over
    more than its share, 512 partials per output in the reduce."""
    spg, maxg = g2.header_constants()
    N = spg * maxg + 5
    w, obs, rows, gvalue = v2.grad_case(12, (64, 64), (4,) * N, 4, 840)
    _run_grad(Weights(w), w, obs, rows, gvalue, pool, "vgrad2 12x64x64 many")


@pytest.mark.parametrize("cols,hidden,pool,n", v2.INT_CASES, ids=_ids)
def test_exact_integer_cases(cols, hidden, pool, n):
    """Small-integer weights, observations and gvalue: values and all six gradients EQUAL the float64 reference."""
    w, obs, rows, gvalue = v2.int_case(cols, hidden, pool, n)
    vals, want = v2.int_case_reference(pool, w, obs, rows, gvalue)
    W = Weights(w)
    dobs, drows, dgv = to_cuda(obs, rows, gvalue)
    v32, _ = _value(W, dobs, drows, pool)
    assert np.array_equal(v32.astype(np.float64), vals), (v32, vals)
    got = _vgrad(W, dobs, drows, pool, dgv)
    for name, x, y in zip(v2.NAMES, got, want):
        assert np.array_equal(x.astype(np.float64), y.reshape(x.shape)), (name, int((x != y.reshape(x.shape)).sum()), x.size)


@pytest.mark.parametrize("pool", v2.POOLS)
def test_row_count_conventions(pool):
    """A call made only of one-row states has the reference's (non-zero) gradient — the policy's gradient kernel would skip every
    one of them; states without rows among them, whatever their gvalue, contribute nothing; what lies beyond the live rows (-1
    padding or garbage) changes no bit of values or gradients."""
    w, obs, rows, gvalue = v2.grad_case(12, (128, 64), (1,) * 7, 5, 850)
    W = Weights(w)
    got = _run_grad(W, w, obs, rows, gvalue, pool, "vgrad2 one-row states")
    assert abs(got[5][0]) > 0 and all(np.abs(g).max() > 0 for g in got)
    assert abs(float(got[5][0]) - float(gvalue.astype(np.float64).sum())) <= 8 * v2.EPS * np.abs(gvalue).sum()
    rows2 = np.concatenate([rows[:3], np.array([0, -5], dtype=np.int32), rows[3:], np.array([0], dtype=np.int32)])
    obs2 = np.concatenate([obs[:3], obs[:2], obs[3:], obs[:1]])
    gv2 = np.concatenate([gvalue[:3], np.array([np.nan, 1e30], dtype=np.float32), gvalue[3:], np.array([-np.inf], dtype=np.float32)])
    got2 = _run_grad(W, w, obs2, rows2, gv2, pool, "vgrad2 one-row + rowless states")
    assert all(np.isfinite(x).all() for x in got2)
    # garbage against -1 padding beyond the live rows
    _, obs3, rows3, gv3 = v2.grad_case(12, (128, 64), (33, 1, 16, 0, 40), 40, 851, garbage=True)
    clean = pc.fill_padding(obs3, rows3, False)
    assert (clean != obs3).any()
    a = to_cuda(obs3, rows3, gv3); b = to_cuda(clean, rows3, gv3)
    assert _same(_value(W, a[0], a[1], pool), _value(W, b[0], b[1], pool))
    assert _same(_vgrad(W, a[0], a[1], pool, a[2]), _vgrad(W, b[0], b[1], pool, b[2]))


# ---- bit-for-bit relations -----------------------------------------------------------------------------------------------------
def _buffer_case(seed=860, S=23, hidden=(64, 128)):
    rows = np.resize(np.array((33, 0, 17, 1, 2, 64, 40, 5, 31, 32), dtype=np.int32), S)
    w, obs, rows, _ = v2.grad_case(12, hidden, rows, 40, seed)
    return w, obs, rows


@pytest.mark.parametrize("pool", v2.POOLS)
def test_indexed_calls_equal_the_contiguous_calls_on_gathered_arrays(pool):
    """An index out of order with repeated entries: values, gradients and the whole fit call equal, bit for bit, the calls without
    _at on obs[index], rows[index]."""
    w, obs, rows = _buffer_case()
    W = Weights(w)
    rng = np.random.default_rng(861)
    index = np.concatenate([rng.permutation(len(rows)), rng.integers(0, len(rows), size=14)]).astype(np.int32)
    gvalue = rng.normal(size=len(index)).astype(np.float32); targets = rng.normal(size=len(index)).astype(np.float32)
    dobs, drows, dindex, dgv, dtg = to_cuda(obs, rows, index, gvalue, targets)
    gobs, grows = to_cuda(obs[index], rows[index])
    assert _same(_value(W, dobs, drows, pool, dindex), _value(W, gobs, grows, pool))
    assert _same(_vgrad(W, dobs, drows, pool, dgv, dindex), _vgrad(W, gobs, grows, pool, dgv))
    fa = _fit(W, dobs, drows, pool, dtg, 0.25, dindex); fb = _fit(W, gobs, grows, pool, dtg, 0.25)
    assert _same(fa[:3], fb[:3]) and _same(fa[3], fb[3])


@pytest.mark.parametrize("pool", v2.POOLS)
def test_an_index_out_of_range_gives_nan_and_reads_nothing(pool):
    """Indices -1 and n_src: NaN values, coef 0, not counted, nothing contributed (gvalue NaN at those positions).  The recorded
    arrays handed to the calls lie INSIDE larger ones whose states -1 and n_src are a poisoned guard (2048 rows of huge entries):
    read there, they would give a finite value and move every gradient.  The gradients equal, bit for bit, those of the call in
    which these positions point at a state without rows instead (the same partition of the positions)."""
    import torch
    w, obs, rows = _buffer_case(870)
    rows[1] = 0                                                          # (a state without rows to stand in)
    W = Weights(w)
    S, R, cols = obs.shape
    big_obs = np.full((S + 2, R, cols), 1 << 20, dtype=np.int32); big_obs[1:S + 1] = obs
    big_rows = np.full(S + 2, 2048, dtype=np.int32); big_rows[1:S + 1] = rows
    gobs, grows = to_cuda(big_obs, big_rows)
    dobs, drows = gobs[1:S + 1], grows[1:S + 1]                          # (views: contiguous, the guards right in front and behind)
    assert dobs.is_contiguous() and dobs.data_ptr() == gobs.data_ptr() + 4 * R * cols
    rng = np.random.default_rng(871)
    index = rng.integers(0, S, size=19).astype(np.int32)
    bad = np.array([3, 11])
    index[bad] = (-1, S)
    keep = np.setdiff1d(np.arange(len(index)), bad)
    gvalue = rng.normal(size=len(index)).astype(np.float32); gvalue[bad] = np.nan
    targets = rng.normal(size=len(index)).astype(np.float32)
    dindex, dgv, dtg = to_cuda(index, gvalue, targets)
    v32, v64 = _value(W, dobs, drows, pool, dindex)
    assert np.isnan(v32[bad]).all() and np.isnan(v64[bad]).all() and np.isfinite(v32[keep]).all()
    got = _vgrad(W, dobs, drows, pool, dgv, dindex)
    standin = index.copy(); standin[bad] = 1
    assert _same(got, _vgrad(W, dobs, drows, pool, dgv, to_cuda(standin)[0]))
    want, A = v2.reference_grad2(w, obs[index[keep]], rows[index[keep]], gvalue[keep], pool)
    v2.check_grads(got, want, A, what="out of range")
    fv, fc, fs, fg = _fit(W, dobs, drows, pool, dtg, 0.5, dindex)
    assert np.isnan(fv[bad]).all() and (fc[bad] == 0.0).all() and fs[0] == len(keep) and fs[5] == len(bad)
    assert _same(fg, _vgrad(W, dobs, drows, pool, to_cuda(fc)[0], dindex))
    allbad = to_cuda(np.full(len(index), 7, dtype=np.int32))[0]           # a source of one state: every index is out of range
    fv, fc, fs, fg = _fit(W, dobs[:1], drows[:1], pool, dtg, 0.5, allbad)
    assert np.isnan(fv).all() and (fc == 0.0).all() and fs[0] == 0 and fs[5] == len(index) and all((g == 0).all() for g in fg)
    assert torch.equal(gobs[0], torch.full_like(gobs[0], 1 << 20)) and int(grows[0]) == 2048 and int(grows[-1]) == 2048


@pytest.mark.parametrize("pool", v2.POOLS)
def test_the_fit_call_is_its_three_parts_bit_for_bit(pool):
    """Values = bbx_pmlp2_value's; coef = the float32 recipe in numpy; gradients = bbx_pmlp2_value_grad's with d_gvalue = d_coef;
    statistics = numpy's double sums of the float32 terms (1e-12 relative; the counts exactly); d_stats NULL is accepted and changes
    nothing else; two calls give the same bits; n == 0 zeroes gradients and statistics."""
    import torch
    w, obs, rows = _buffer_case(880, S=1030)
    W = Weights(w)
    targets = np.random.default_rng(881).normal(size=len(rows)).astype(np.float32) * 3
    scale = 1.0 / len(rows)
    dobs, drows, dtg = to_cuda(obs, rows, targets)
    v, coef, stats, grads = _fit(W, dobs, drows, pool, dtg, scale)
    v32, _ = _value(W, dobs, drows, pool)
    assert np.array_equal(_bits(v), _bits(v32))
    want_coef, _, counted = vc.fit_recipe(v, targets, np.float32(scale))
    assert counted.all() and np.array_equal(_bits(coef), _bits(want_coef))
    assert _same(grads, _vgrad(W, dobs, drows, pool, to_cuda(coef)[0]))
    want = vc.fit_stats(v, targets, np.float32(scale))
    assert stats[0] == want[0] == len(rows) and stats[5] == want[5] == 0
    assert (np.abs(stats - want) <= 1e-12 * np.abs(want)).all(), (stats, want)
    again = _fit(W, dobs, drows, pool, dtg, scale)
    assert _same(again[:3], (v, coef, stats)) and _same(again[3], grads)
    quiet = _fit(W, dobs, drows, pool, dtg, scale, stats=False)
    assert quiet[2] is None and _same(quiet[:2], (v, coef)) and _same(quiet[3], grads)
    e_obs, e_rows = torch.zeros((0, 40, 12), dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
    z = _fit(W, e_obs, e_rows, pool, None, 1.0)
    assert (z[2] == 0).all() and all((g == 0).all() for g in z[3])
    z = _fit(W, e_obs, e_rows, pool, None, 1.0, stats=False)
    assert all((g == 0).all() for g in z[3])


def test_a_nan_position_of_the_fit_call_is_not_counted():
    """One index out of range among five: stats[0] = 4, stats[5] = 1, and the sums are those of the four counted positions."""
    w, obs, rows = _buffer_case(885, S=6)
    W = Weights(w)
    index = np.array([0, 2, 6, 4, 5], dtype=np.int32)
    targets = np.array([0.5, -1.0, 9.0, 2.0, 0.25], dtype=np.float32)
    dobs, drows, dindex, dtg = to_cuda(obs, rows, index, targets)
    v, coef, stats, _ = _fit(W, dobs, drows, "sum", dtg, 0.2, dindex)
    assert np.isnan(v[2]) and coef[2] == 0.0
    want = vc.fit_stats(v, targets, np.float32(0.2))
    assert stats[0] == 4 and stats[5] == 1 and (np.abs(stats - want) <= 1e-12 * np.abs(want)).all()


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def _param_grads(critic):
    l1, l2 = critic.embedding
    g = lambda t: t.grad.cpu().numpy()
    return (l1.weight.grad.t().contiguous().cpu().numpy(), g(l1.bias), l2.weight.grad.t().contiguous().cpu().numpy(), g(l2.bias),
            critic.head.weight.grad.reshape(-1).cpu().numpy(), critic.head.bias.grad.reshape(-1).cpu().numpy())


def _weights_of(critic):
    f = lambda t: t.detach().cpu().numpy().astype(np.float32)
    return [(f(l.weight).T.copy(), f(l.bias)) for l in critic.embedding] + [(f(critic.head.weight).reshape(-1), f(critic.head.bias).reshape(-1))]


@pytest.mark.parametrize("pool", v2.POOLS)
def test_evaluate_backward_equals_the_abi(pool):
    """PMLPValue(deep_kernels).evaluate(...).sum().backward(): the values are bbx_pmlp2_value's and the .grad of the six parameters
    bbx_pmlp2_value_grad's with gvalue = 1, bit for bit; evaluate_at on a buffer the same on the gathered states; the same module
    without deep_kernels takes the torch path, says so, and agrees within the bounds."""
    import torch
    w, obs, rows = _buffer_case(890)
    W = Weights(w)
    critic = v2.to_critic(w, pool, "cuda")
    dobs, drows = to_cuda(obs, rows)
    v = critic.evaluate(dobs, drows)
    assert critic.last_path == "kernels" and v.requires_grad and type(v.grad_fn).__name__.startswith("_PMLP2ValueEvaluate")
    v.sum().backward()
    want_v, _ = _value(W, dobs, drows, pool)
    assert np.array_equal(_bits(v.detach().cpu().numpy()), _bits(want_v))
    assert _same(_param_grads(critic), _vgrad(W, dobs, drows, pool, torch.ones(len(rows), device="cuda")))
    index = np.array([5, 5, 0, 22, 7, 3], dtype=np.int32)
    critic.zero_grad()
    va = critic.evaluate_at(dobs, drows, torch.from_numpy(index).cuda())
    assert type(va.grad_fn).__name__.startswith("_PMLP2ValueEvaluate")
    (2.0 * va).sum().backward()
    gobs, grows = to_cuda(obs[index], rows[index])
    assert _same(_param_grads(critic), _vgrad(W, gobs, grows, pool, torch.full((len(index),), 2.0, device="cuda")))
    assert np.array_equal(_bits(critic.values_at(dobs, drows, torch.from_numpy(index).cuda()).cpu().numpy()), _bits(_value(W, gobs, grows, pool)[0]))
    plain = v2.to_critic(w, pool, "cuda", deep_kernels=False)
    vt = plain.evaluate(dobs, drows)
    assert plain.last_path == "torch" and not type(vt.grad_fn).__name__.startswith("_PMLP")
    gv = np.linspace(-1, 1, len(rows)).astype(np.float32)
    (vt * torch.from_numpy(gv).cuda()).sum().backward()
    want, ref = vc.reference_values(w, obs, rows, pool)
    assert (np.abs(vt.detach().cpu().numpy() - want) <= vc.value_tol(ref, pool, want, c_v=v2.C_V2)).all()
    want_g, A = v2.reference_grad2(w, obs, rows, gv, pool, ref=ref)
    # (torch's float32 autograd is the baseline, not the code under test: its ratio is printed, and it is held to the float64
    # reference only through the kernels' agreement with both — on an MI355X it needed 138.6 of the unit at sum and mean)
    print("ratios %-50s %-4s N=%-5d r_vg2=%.3f (torch path)" % ("evaluate 12x64x128", pool, len(rows), gc.grad_ratio(_param_grads(plain), want_g, A)))
    assert all(np.isfinite(x).all() for x in _param_grads(plain))
    critic.zero_grad()
    (critic.evaluate(dobs, drows) * torch.from_numpy(gv).cuda()).sum().backward()
    v2.check_grads(_param_grads(critic), want_g, A, what="kernel path")


def test_fit_step_at_in_place_equals_fit_step_on_the_gathered_copy():
    """fit_step_at over a [T, B, R, cols] buffer in place and fit_step on states[index]: the same statistics, values and .grad,
    bit for bit; a second call ADDS to .grad; after an optimiser step the next call computes with the new weights."""
    import torch
    w, obs, rows = _buffer_case(900, S=24, hidden=(64, 64))
    critic = v2.to_critic(w, "mean", "cuda"); other = v2.to_critic(w, "mean", "cuda")
    dobs, drows = to_cuda(obs.reshape(4, 6, 40, 12), rows.reshape(4, 6))
    index = torch.from_numpy(np.array([23, 1, 1, 8, 15, 0, 4], dtype=np.int64)).cuda()
    targets = torch.linspace(-2, 2, 7, device="cuda")
    st_a, v_a = critic.fit_step_at(dobs, drows, index, targets)
    flat_obs, flat_rows = dobs.view(-1, 40, 12), drows.view(-1)
    st_b, v_b = other.fit_step(flat_obs[index], flat_rows[index], targets)
    assert critic.last_path == "kernels" and other.last_path == "kernels"
    assert torch.equal(st_a, st_b) and torch.equal(v_a, v_b)
    first = _param_grads(critic)
    assert _same(first, _param_grads(other))
    critic.fit_step_at(dobs, drows, index, targets)
    for x, y in zip(_param_grads(critic), first):
        assert np.array_equal(x, 2 * y)
    opt = torch.optim.SGD(critic.parameters(), lr=0.1)
    before = critic.values(flat_obs, flat_rows).clone()
    prepared = critic._deep_weights()["prepared"].value
    opt.step()
    after = critic.values(flat_obs, flat_rows)
    assert critic.last_path == "kernels" and not torch.equal(before, after)
    assert critic._deep_weights()["prepared"].value == prepared                  # (refilled in place)
    want, ref = vc.reference_values(_weights_of(critic), obs, rows, "mean")
    assert (np.abs(after.cpu().numpy() - want) <= vc.value_tol(ref, "mean", want, c_v=v2.C_V2)).all()


@pytest.mark.parametrize("pool", v2.POOLS)
def test_backward_reads_the_weights_of_its_own_forward_pass(pool):
    """The contract of tests/test_pmlp_weights_cache_gpu.py for the new kind: a backward behind a change of parameter storage
    (p.data = ...) differentiates the weights of its own forward pass; the next call sees the new ones."""
    import torch
    w, obs, rows = v2.value_case(6, (32, 32), (0, 1, 2, 4), 4, 9300)
    dobs, drows = to_cuda(obs, rows)
    cot = torch.tensor((0.5, -1.0, 2.0, 0.25), device="cuda")
    results = []
    for change in (False, True):
        m = v2.to_critic(w, pool, "cuda")
        out = m.evaluate(dobs, drows)
        assert type(out.grad_fn).__name__.startswith("_PMLP2ValueEvaluate")
        if change:
            with torch.no_grad():
                for p in m.parameters():
                    p.data = p.data + 0.25
            m._deep_weights()                                             # (the buffer, refilled in place, holds the new weights from here)
        out.backward(cot)
        results.append((out.detach().cpu().numpy(), [p.grad.cpu().numpy() for p in m.parameters()], m))
    (o0, g0, _), (o1, g1, moved) = results
    assert o0.tobytes() == o1.tobytes() and len(g0) == len(g1) == 6
    assert all(a.tobytes() == b.tobytes() for a, b in zip(g0, g1))
    assert moved.evaluate(dobs, drows).detach().cpu().numpy().tobytes() != o1.tobytes()


# ---- rollout and update loops ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rollout_pair():
    """The same fused rollout twice, same seeds: with a PMLP(64, 64) critic and without (3-20-10-weighted, B = 64, 32 steps, 128-row
    blocks in a state-keeping buffer)."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, PMLPValue, run_rollout_fused
    B, R, T = 64, 128, 32
    torch.manual_seed(5)
    policy = PMLPPolicy(12, (128,)).cuda()
    critic = PMLPValue(12, (64, 64), pool="mean", deep_kernels=True).cuda()
    out = []
    for cr in (critic, None):
        env = VecLeadMonomialsEnv("3-20-10-weighted", batch=B, k=2)
        env.seed(np.arange(B) + 100)
        env.reset()
        buf = DeviceTrajectoryBuffer(T, B, obs_shape=(R, 12))
        gen = torch.Generator(device="cuda"); gen.manual_seed(11)
        run_rollout_fused(env, policy, T, buf, obs_rows=R, generator=gen, critic=cr)
        torch.cuda.synchronize()
        out.append(buf)
    return critic, out[0], out[1]


def test_run_rollout_fused_fills_the_values_and_leaves_the_rollout_alone(rollout_pair):
    import torch
    critic, with_critic, without = rollout_pair
    R, cols = with_critic.states.shape[2:]
    assert with_critic.t == 32 and without.t == 32
    want = critic.values(with_critic.states.view(-1, R, cols), with_critic.rows.view(-1))
    assert critic.last_path == "kernels"
    assert torch.equal(with_critic.values.view(-1), want.to(torch.float64)) and float(with_critic.values.abs().max()) > 0
    assert (without.values == 0).all()
    for name in ("actions", "rewards", "logprobs", "dones", "rows", "states"):
        assert torch.equal(getattr(with_critic, name), getattr(without, name)), name


def test_value_update_lowers_the_mean_squared_error(rollout_pair):
    """Three epochs with Adam (lr 1e-3), a fixed seed: sum d^2 / counted positions (stats[1] / stats[0] over the epoch) falls."""
    import torch
    from deepgroebner_amd.rollout import value_update
    critic, buf, _ = rollout_pair
    assert int(buf.get_index(None)[0].numel()) > 64
    opt = torch.optim.Adam(critic.parameters(), lr=1e-3)
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    out = value_update(critic, buf, opt, 3, 64, generator=gen)
    mse = [float(o["stats"][:, 1].sum() / o["stats"][:, 0].sum()) for o in out]
    print("value_update mean squared errors", mse)
    assert critic.last_path == "kernels" and len(out) == 3 and all((o["stats"][:, 5] == 0).all() for o in out)
    assert mse[-1] < mse[0]
