"""The indexed training interface without a GPU: the four bbx_pmlp*_at symbols and their shape / argument answers,
DeviceTrajectoryBuffer.get_index against get() on CPU tensors, and PMLPPolicy.evaluate_at's gather path against evaluate on the
gathered tensors.  (tests/test_policy_indexed_gpu.py runs the kernels.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import policy_cases as pc

E_ARG, E_UNSUPPORTED = -1, -5


def test_abi_symbols_and_shape_answers():
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    for name in ("bbx_pmlp_logprob_at", "bbx_pmlp_grad_at", "bbx_pmlp2_logprob_at", "bbx_pmlp2_grad_at"):
        assert name in _ffi.SIGNATURES and getattr(lib, name) is not None
    z = C.c_void_p(16)
    one_l = lambda n_src, idx, n, R, cols, h: lib.bbx_pmlp_logprob_at(z, z, z, n_src, idx, n, R, cols, z, h, z, None, None)
    one_g = lambda n_src, idx, n, R, cols, h: lib.bbx_pmlp_grad_at(z, z, z, n_src, idx, n, R, cols, z, h, z, None, z, z, z, z, z, None)
    two_l = lambda n_src, idx, n, R, cols, h: lib.bbx_pmlp2_logprob_at(z, z, z, n_src, idx, n, R, cols, z, h, h, z, None, None)
    two_g = lambda n_src, idx, n, R, cols, h: lib.bbx_pmlp2_grad_at(z, z, z, n_src, idx, n, R, cols, z, h, h, z, None, z, z, z, z, z, z, z, None)
    # unsupported shapes are refused before anything is queued (no device needed to hear it)
    for f, wide in ((one_l, 257), (one_g, 257), (two_l, 129), (two_g, 129)):
        assert f(8, z, 4, 64, 12, wide) == E_UNSUPPORTED
        assert str(wide) in lib.bbx_last_error().decode()
        assert f(8, z, 4, 64, 65, 64) == E_UNSUPPORTED
        assert "65" in lib.bbx_last_error().decode()
        assert f(8, z, 4, 2049, 12, 64) == E_UNSUPPORTED
        assert "2049" in lib.bbx_last_error().decode()
    # (one layer takes up to 256 units: 129 is a shape of its own there; the two-layer pair refuses 129 / 65 / 2049 together too)
    for f in (two_l, two_g):
        assert f(8, z, 4, 2049, 65, 129) == E_UNSUPPORTED
    # the arguments the indexed entries add
    for f in (one_l, one_g, two_l, two_g):
        assert f(-1, z, 4, 64, 12, 64) == E_ARG
        assert f(8, None, 1, 64, 12, 64) == E_ARG
        assert f(8, z, -1, 64, 12, 64) == E_ARG


# ---- get_index ---------------------------------------------------------------------------------------------------------------
T, B, R, COLS = 7, 5, 4, 3
MODES = [(None, False, False), (None, True, False), (3, True, False), (3, False, True), (100, True, False)]


def _buffer(states=True, done=None):
    """Five environments: one never finishes, one is done at the last step only, one at every step, two at mixed steps; row counts
    0 .. 4 (0 and 1 included) in a pattern of its own."""
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer
    rng = np.random.default_rng(4)
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(R, COLS) if states else None, device="cpu")
    if done is None:
        done = np.zeros((T, B), dtype=bool)
        done[T - 1, 1] = True
        done[:, 2] = True
        done[[1, 4], 3] = True
        done[[0, 2, 3, 5], 4] = True
    rows = np.array([(3 * t + 2 * b + t * b) % 5 for t in range(T) for b in range(B)], dtype=np.int32).reshape(T, B)
    assert set(rows.ravel()) == {0, 1, 2, 3, 4}
    buf.rows.copy_(torch.from_numpy(rows))
    buf.dones.copy_(torch.from_numpy(done))
    buf.actions.copy_(torch.from_numpy(rng.integers(0, 4, size=(T, B)).astype(np.int32)))
    buf.rewards.copy_(torch.from_numpy(-rng.integers(1, 30, size=(T, B)).astype(np.float64)))
    buf.values.copy_(torch.from_numpy(rng.normal(size=(T, B))))
    buf.logprobs.copy_(torch.from_numpy(rng.normal(size=(T, B)).astype(np.float32)))
    if states:
        st = rng.integers(0, 9, size=(T, B, R, COLS)).astype(np.int32)
        st[np.arange(R)[None, None, :] >= rows[:, :, None]] = -1
        buf.states.copy_(torch.from_numpy(st))
    buf.t = T
    return buf


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("batch_size,sort,drop", MODES)
def test_get_index_selects_what_get_selects(batch_size, sort, drop, with_rows):
    buf = _buffer()
    want = buf.get(batch_size, sort=sort, drop_remainder=drop, with_rows=True)
    got = buf.get_index(batch_size, sort=sort, drop_remainder=drop, with_rows=with_rows)
    bare = _buffer(states=False).get_index(batch_size, sort=sort, drop_remainder=drop, with_rows=with_rows)
    if batch_size is None:
        want, got, bare = [want], [got], [bare]
    assert isinstance(got, (list, tuple)) and len(got) == len(want) == len(bare) and len(want) >= 1
    flat = buf.states.view(-1, R, COLS)
    total = 0
    for w, g, h in zip(want, got, bare):
        assert len(g) == (6 if with_rows else 5) and len(h) == len(g)
        idx = g[0]
        assert idx.dtype == torch.int32 and idx.dim() == 1
        assert _same(idx, h[0])                                        # a buffer without states: the same indices
        mr = int(w[5].max())
        assert _same(flat[idx.long()][:, :mr], w[0].contiguous())
        assert torch.equal(buf.rows.view(-1)[idx.long()], w[5]) and torch.equal(buf.actions.view(-1)[idx.long()], w[1])
        for k in range(1, len(g)):
            assert _same(g[k], w[k]) and _same(h[k], w[k])
        total += idx.numel()
    assert total > 0
    if batch_size is not None and len(got) > 1:                        # the tuples hold slices of ONE index tensor
        assert all(g[0]._base is not None and g[0]._base is got[0][0]._base for g in got)


def test_get_index_of_an_empty_selection():
    buf = _buffer(done=np.zeros((T, B), dtype=bool))                   # no episode ends: no complete step
    for with_rows in (False, True):
        got, want = buf.get_index(with_rows=with_rows), buf.get(with_rows=with_rows)
        assert got[0].dtype == torch.int32 and all(x.numel() == 0 for x in got)
        assert all(_same(a, b) for a, b in zip(got[1:], want[1:]))
        assert buf.get_index(batch_size=3, sort=True, with_rows=with_rows) == [] == buf.get(batch_size=3, sort=True, with_rows=with_rows)


# ---- evaluate_at on CPU tensors: the gather path -------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [(16,), (8, 8), (8, 4, 8)], ids=str)
@pytest.mark.parametrize("four_d", [False, True])
def test_evaluate_at_on_cpu_tensors_equals_evaluate_on_the_gathered_ones(hidden, four_d):
    buf = _buffer()
    pol = pc.to_policy(pc.make_weights(COLS, hidden, 7))
    pol.deep_kernels = True
    index = torch.tensor([3, 0, 34, 17, 17, 8, 21], dtype=torch.int32)
    st = buf.states if four_d else buf.states.view(-1, R, COLS)
    act = buf.actions if four_d else buf.actions.view(-1)
    rows = buf.rows if four_d else buf.rows.view(-1)
    lp, ent = pol.evaluate_at(st, act, rows, index)
    j = index.long()
    lp2, ent2 = pol.evaluate(buf.states.view(-1, R, COLS)[j], buf.actions.view(-1)[j], buf.rows.view(-1)[j])
    assert lp.shape == (len(index),) and lp.requires_grad
    assert torch.equal(torch.nan_to_num(lp, nan=7.0), torch.nan_to_num(lp2, nan=7.0)) and torch.equal(ent, ent2)
    g1 = torch.autograd.grad((torch.nan_to_num(lp) + ent).sum(), list(pol.parameters()))
    g2 = torch.autograd.grad((torch.nan_to_num(lp2) + ent2).sum(), list(pol.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
