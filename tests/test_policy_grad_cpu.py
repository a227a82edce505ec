"""tests/policy_grad_cases.py and the training-side interface without a GPU: the float64 gradient reference against torch
autograd in double precision, PMLPPolicy.evaluate_torch against the reference, the C ABI's shape answers, and
DeviceTrajectoryBuffer.get(with_rows=True).  (tests/test_policy_grad_gpu.py runs the kernels against the same reference.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import policy_cases as pc
from tests import policy_grad_cases as gc

SHAPES = [(1, (1,)), (12, (128,)), (13, (33,)), (64, (256,))]
R = 40
ROWS = (0, 1, 2, 33, R + 7, 17, 40)          # no row, one row, a tile and a row, more than the block holds


def _batch(cols, hidden, seed):
    w = pc.make_weights(cols, hidden, seed)
    rows = np.array(ROWS, dtype=np.int32)
    obs = pc.fill_padding(pc.random_blocks(len(rows), R, cols, seed + 1), rows, False)
    rng = np.random.default_rng(seed + 2)
    n = np.clip(rows, 0, R)
    actions = (rng.integers(0, 1 << 30, size=len(rows)) % np.maximum(n, 1)).astype(np.int32)
    glogp = rng.normal(size=len(rows)); gent = rng.normal(size=len(rows))
    return w, obs, rows, actions, glogp, gent


@pytest.mark.parametrize("cols,hidden", SHAPES, ids=[pc.label(*s) for s in SHAPES])
def test_reference_grad_equals_autograd_in_double_precision(cols, hidden):
    """L built from PMLPPolicy's forward in float64 (_forward64: masking by the -1 padding), gather and -(exp(lp) lp): its autograd gradients
    are reference_grad's to 1e-10 relative; the absolute contributions dominate the gradients they belong to."""
    w, obs, rows, actions, glogp, gent = _batch(cols, hidden, 11)
    pol = pc.to_policy(w, dtype=torch.float64)
    lp = _forward64(pol, torch.from_numpy(obs))
    n = torch.from_numpy(np.clip(rows, 0, R).astype(np.int64))
    live = torch.arange(R)[None, :] < n[:, None]
    logp = lp.gather(1, torch.from_numpy(actions.astype(np.int64))[:, None]).squeeze(1)
    lpl = torch.where(live, lp, torch.zeros_like(lp))
    ent = -(torch.exp(lpl) * lpl * live).sum(dim=1)
    has = n > 0
    loss = (torch.from_numpy(glogp) * logp)[has].sum() + (torch.from_numpy(gent) * ent)[has].sum()
    loss.backward()
    want = (pol.embedding[0].weight.grad.t().numpy(), pol.embedding[0].bias.grad.numpy(), pol.deciding.weight.grad.reshape(-1).numpy(),
            pol.deciding.bias.grad.reshape(-1).numpy())
    got, A = gc.reference_grad(w, obs, rows, actions, glogp, gent)
    for x, y, a in zip(got, want, A):
        assert x.shape == y.shape
        assert np.abs(x - y).max() <= 1e-10 * max(1.0, np.abs(y).max())
        assert (np.abs(x) <= a.sum(axis=0) * (1 + 1e-12) + 1e-300).all()
    # the value side, against the same module
    rl, rh, ref = gc.reference_eval(w, obs, rows, actions)
    assert np.abs(rl - logp.detach().numpy())[has.numpy()].max() <= 1e-12 and np.abs(rh - ent.detach().numpy())[has.numpy()].max() <= 1e-12
    assert (rl[~has.numpy()] == 0).all() and (rh[~has.numpy()] == 0).all()
    # the summed form of A
    K = gc.state_scale(ref)
    _, As = gc.reference_grad(w, obs, rows, actions, glogp, gent, scale=K)
    for a, b in zip(gc.grad_bounds(A, ref), gc.grad_bounds(As)):
        assert np.allclose(a, b, rtol=1e-12, atol=0)


# PMLPPolicy.forward casts its input to float32: the same forward with the cast to the float64 of the module under test
def _forward64(pol, batch):
    mask = batch[:, :, -1] != -1
    x = batch.to(torch.float64)
    for layer in pol.embedding:
        x = torch.relu(layer(x))
    x = pol.deciding(x).squeeze(-1)
    x = x + (~mask).to(torch.float64) * -1e9
    return torch.log_softmax(x, dim=-1)


def test_reference_conventions():
    """No rows: 0.0 and 0.0; one row: 0 and 0 and no gradient; a bad action: NaN, the entropy still there, no gradient."""
    w, obs, rows, actions, glogp, gent = _batch(12, (128,), 3)
    actions = actions.copy(); actions[3] = 33; actions[5] = -1
    lp, ent, ref = gc.reference_eval(w, obs, rows, actions)
    assert lp[0] == 0.0 and ent[0] == 0.0 and lp[1] == 0.0 and ent[1] == 0.0
    assert np.isnan(lp[3]) and np.isnan(lp[5]) and ent[3] > 0 and ent[5] > 0 and np.isfinite(lp[[2, 4, 6]]).all()
    g, A = gc.reference_grad(w, obs, rows, actions, glogp, gent)
    for i in (0, 3, 5):
        assert all((a[i] == 0).all() for a in A)
    only = np.zeros(len(rows)); only[[0, 1, 3, 5]] = 1.0
    g0, _ = gc.reference_grad(w, obs, rows, actions, glogp * only, gent * only)
    assert all(np.abs(x).max() <= 1e-15 for x in g0)


@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (13, (33,)), (12, (64, 64))], ids=["12x128", "13x33", "12x64x64"])
@pytest.mark.parametrize("garbage", [False, True], ids=["padded", "garbage"])
def test_evaluate_torch_agrees_with_the_reference(cols, hidden, garbage):
    """float32 on the CPU, masked by the padding (rows=None, -1 padding only) and by the row counts (also over garbage):
    logprob within policy_cases' tol, entropy within entropy_tol at the ceiling constant, the three conventions exact."""
    w, obs, rows, actions, _, _ = _batch(cols, hidden, 5)
    obs = pc.fill_padding(obs, rows, garbage, 9)
    actions = actions.copy(); actions[3] = 35
    pol = pc.to_policy(w)
    rl, rh, ref = gc.reference_eval(w, obs, rows, actions)
    calls = [torch.from_numpy(rows)] + ([] if garbage else [None])
    for r in calls:
        lp, ent = pol.evaluate(torch.from_numpy(obs), torch.from_numpy(actions), r)
        assert lp.dtype == torch.float32 and ent.dtype == torch.float32 and lp.requires_grad
        lp = lp.detach().numpy().astype(np.float64); ent = ent.detach().numpy().astype(np.float64)
        assert lp[0] == 0.0 and ent[0] == 0.0 and np.isnan(lp[3])
        ok = ~np.isnan(rl)
        assert (np.abs(lp - rl)[ok] <= ref.tol()[ok]).all()
        assert (np.abs(ent - rh) <= gc.entropy_tol(ref, pc.C_CEILING)).all()      # (C_H is the kernels' measurement: torch ops get the ceiling)


def test_evaluate_torch_is_differentiable_for_two_layers():
    w, obs, rows, actions, glogp, gent = _batch(12, (64, 64), 7)
    pol = pc.to_policy(w)
    lp, ent = pol.evaluate(torch.from_numpy(obs), torch.from_numpy(actions), torch.from_numpy(rows))
    (lp[2:] * torch.from_numpy(glogp[2:]).float()).sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in pol.parameters())
    assert float(pol.embedding[0].weight.grad.abs().max()) > 0


# ---- the C ABI without a device
def test_abi_symbols_and_shape_answers():
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    for name in ("bbx_pmlp_logprob", "bbx_pmlp_grad_workspace_floats", "bbx_pmlp_grad"):
        assert name in _ffi.SIGNATURES and getattr(lib, name) is not None
    f = lib.bbx_pmlp_grad_workspace_floats
    for cols, hidden in ((1, 1), (12, 128), (33, 65), (64, 256)):
        for n in (0, 1, 5, 4096, 1 << 20):
            assert f(n, 64, cols, hidden) > 0
    for args, word in (((16, 64, 65, 128), "65"), ((16, 64, 12, 257), "257"), ((16, 2049, 12, 128), "2049")):
        assert f(*args) == -5                                          # BBX_E_UNSUPPORTED
        assert word in lib.bbx_last_error().decode()
    # recompute, not store: the workspace does not grow with the rows, and stops growing with n
    for cols, hidden in ((12, 128), (64, 256)):
        assert abs(f(4096, 128, cols, hidden) - f(4096, 64, cols, hidden)) <= 4096
        assert abs(f(4096, 2048, cols, hidden) - f(4096, 1024, cols, hidden)) <= 4096
        assert f(4096, 2048, cols, hidden) < 4096 * 2048 * hidden // 64
        assert f(1 << 20, 64, cols, hidden) == f(1 << 16, 64, cols, hidden)
    # unsupported shapes are refused before anything is queued (no device needed to hear it)
    z = C.c_void_p(16)
    assert lib.bbx_pmlp_logprob(z, z, z, 4, 64, 65, z, 128, z, None, None) == -5
    assert lib.bbx_pmlp_grad(z, z, z, 4, 2049, 12, z, 128, z, None, z, z, z, z, z, None) == -5
    assert "2048" in lib.bbx_last_error().decode()


def test_partition_constants_are_in_the_header():
    spw, most = gc.header_constants()
    assert spw >= 1 and most >= 2


# ---- DeviceTrajectoryBuffer.get(with_rows=True)
def test_get_with_rows():
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer
    T, B, Rr, cols = 6, 3, 5, 4
    rng = np.random.default_rng(0)
    buf = DeviceTrajectoryBuffer(T, B, obs_shape=(Rr, cols), device="cpu")
    rows_all = rng.integers(1, Rr + 1, size=(T, B)).astype(np.int32)
    for t in range(T):
        rows = torch.from_numpy(rows_all[t])
        state = torch.full((B, Rr, cols), -1, dtype=torch.int32)
        for e in range(B):
            state[e, :rows_all[t, e]] = torch.from_numpy(rng.integers(0, 9, size=(rows_all[t, e], cols)).astype(np.int32))
        done = torch.tensor([t == T - 1 or (t == 2 and e == 1) for e in range(B)])
        buf.store(state, rows, torch.zeros(B, dtype=torch.int32), torch.from_numpy(rng.normal(size=B)), torch.zeros(B), torch.zeros(B, dtype=torch.float64), done)
    plain = buf.get()
    with6 = buf.get(with_rows=True)
    assert len(plain) == 5 and len(with6) == 6
    for x, y in zip(plain, with6[:5]):
        assert torch.equal(x, y)
    st, rows = with6[0], with6[5]
    assert rows.dtype == torch.int32 and rows.shape == (st.shape[0],) and (rows != 1).all()
    assert torch.equal((st[:, :, -1] != -1).sum(1).to(torch.int32), rows)
    want = torch.from_numpy(rows_all).transpose(0, 1).reshape(-1)
    assert torch.equal(rows, want[want != 1])
    # batches, sorted: the sixth element follows the same order and cuts
    b5 = buf.get(batch_size=4, sort=True)
    b6 = buf.get(batch_size=4, sort=True, with_rows=True)
    assert len(b5) == len(b6)
    for x, y in zip(b5, b6):
        assert len(x) == 5 and len(y) == 6 and all(torch.equal(p, q) for p, q in zip(x, y[:5]))
        assert torch.equal((y[0][:, :, -1] != -1).sum(1).to(torch.int32), y[5]) and (y[5][1:] >= y[5][:-1]).all()
