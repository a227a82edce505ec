"""tests/policy2_grad_cases.py and the two-layer training interface without a GPU: the float64 gradient reference against torch
autograd in double precision, its conventions, the exact-integer constructions, the C ABI's shape answers and PMLPPolicy's
dispatch.  (tests/test_policy2_grad_gpu.py runs the kernels against the same reference.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import policy_cases as pc
from tests import policy_grad_cases as gc
from tests import policy2_grad_cases as g2

SHAPES = [(1, (1, 1)), (12, (64, 64)), (13, (65, 64)), (64, (128, 128))]
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


def _forward64(pol, batch):
    mask = batch[:, :, -1] != -1
    x = batch.to(torch.float64)
    for layer in pol.embedding:
        x = torch.relu(layer(x))
    x = pol.deciding(x).squeeze(-1)
    x = x + (~mask).to(torch.float64) * -1e9
    return torch.log_softmax(x, dim=-1)


def _params_as_cases(pol):
    """The .grad of a two-layer policy's parameters in the layouts of reference_grad2."""
    l1, l2 = pol.embedding
    return (l1.weight.grad.t(), l1.bias.grad, l2.weight.grad.t(), l2.bias.grad, pol.deciding.weight.grad.reshape(-1), pol.deciding.bias.grad.reshape(-1))


@pytest.mark.parametrize("cols,hidden", SHAPES, ids=[pc.label(*s) for s in SHAPES])
def test_reference_grad2_equals_autograd_in_double_precision(cols, hidden):
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
    want = [t.numpy() for t in _params_as_cases(pol)]
    got, A = g2.reference_grad2(w, obs, rows, actions, glogp, gent)
    assert len(got) == 6 and len(A) == 6
    for x, y, a in zip(got, want, A):
        assert x.shape == y.shape and a.shape == (len(rows),) + x.shape
        assert np.abs(x - y).max() <= 1e-10 * max(1.0, np.abs(y).max())
        assert (np.abs(x) <= a.sum(axis=0) * (1 + 1e-12) + 1e-300).all()
    # the summed form of A
    ref = pc.reference(w, obs, rows)
    _, As = g2.reference_grad2(w, obs, rows, actions, glogp, gent, scale=gc.state_scale(ref))
    for a, b in zip(gc.grad_bounds(A, ref), gc.grad_bounds(As)):
        assert a.shape == b.shape and np.allclose(a, b, rtol=1e-12, atol=0)


def test_reference_conventions():
    """No rows: 0.0 and 0.0; one row: 0 and 0 and no gradient; a bad action: NaN, the entropy still there, no gradient."""
    w, obs, rows, actions, glogp, gent = _batch(12, (64, 64), 3)
    actions = actions.copy(); actions[3] = 33; actions[5] = -1
    lp, ent, ref = gc.reference_eval(w, obs, rows, actions)
    assert lp[0] == 0.0 and ent[0] == 0.0 and lp[1] == 0.0 and ent[1] == 0.0
    assert np.isnan(lp[3]) and np.isnan(lp[5]) and ent[3] > 0 and ent[5] > 0 and np.isfinite(lp[[2, 4, 6]]).all()
    g, A = g2.reference_grad2(w, obs, rows, actions, glogp, gent)
    for i in (0, 3, 5):
        assert all((a[i] == 0).all() for a in A)
    only = np.zeros(len(rows)); only[[0, 1, 3, 5]] = 1.0
    g0, _ = g2.reference_grad2(w, obs, rows, actions, glogp * only, gent * only)
    assert all(np.abs(x).max() <= 1e-15 for x in g0)
    assert any(np.abs(x).max() > 0 for x in g)


@pytest.mark.parametrize("n", g2.INT_ROWS)
@pytest.mark.parametrize("cols,hidden", g2.INT_SHAPES, ids=[pc.label(*s) for s in g2.INT_SHAPES])
@pytest.mark.parametrize("kind", ["a", "b"])
def test_integer_constructions_are_what_they_claim(kind, cols, hidden, n):
    """Equal logits per state, integer gradients with absolute sums below 2^24, the gradients that must vanish exactly zero,
    the others not degenerate (int_case_reference asserts all of it)."""
    w, obs, rows, actions, glogp = (g2.int_case_a if kind == "a" else g2.int_case_b)(cols, hidden, n)
    assert (glogp % n == 0).all() and obs[:, :n].min() >= 0 and obs[:, :n].max() <= 3
    want = g2.int_case_reference(kind, w, obs, rows, actions, glogp)
    assert [y.shape for y in want] == [(cols, hidden[0]), (hidden[0],), hidden, (hidden[1],), (hidden[1],), (1,)]


# ---- the C ABI without a device
def test_abi_symbols_and_shape_answers():
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    for name in ("bbx_pmlp2_logprob", "bbx_pmlp2_grad_workspace_floats", "bbx_pmlp2_grad"):
        assert name in _ffi.SIGNATURES and getattr(lib, name) is not None
    f = lib.bbx_pmlp2_grad_workspace_floats
    for cols, h1, h2 in ((1, 1, 1), (12, 64, 64), (33, 17, 128), (64, 128, 128)):
        for n in (0, 1, 5, 4096, 1 << 20):
            assert f(n, 64, cols, h1, h2) > 0
    for args, word in (((16, 64, 65, 128, 128), "65"), ((16, 64, 12, 129, 64), "129"), ((16, 64, 12, 64, 129), "129"), ((16, 2049, 12, 128, 128), "2049")):
        assert f(*args) == -5                                          # BBX_E_UNSUPPORTED
        assert word in lib.bbx_last_error().decode()
    # recompute, not store: the workspace does not depend on the rows, stops growing with n, and stays at or below 2^24 floats
    for cols, h1, h2 in ((12, 64, 64), (64, 128, 128)):
        assert f(4096, 64, cols, h1, h2) == f(4096, 2048, cols, h1, h2)
        assert f(1 << 20, 64, cols, h1, h2) == f(1 << 16, 64, cols, h1, h2)
    assert f(1 << 20, 2048, 64, 128, 128) <= 1 << 24
    # unsupported shapes are refused before anything is queued (no device needed to hear it)
    z = C.c_void_p(16)
    assert lib.bbx_pmlp2_logprob(z, z, z, 4, 64, 65, z, 128, 128, z, None, None) == -5
    assert "65" in lib.bbx_last_error().decode()
    assert lib.bbx_pmlp2_logprob(z, z, z, 4, 64, 12, z, 129, 128, z, None, None) == -5
    assert lib.bbx_pmlp2_grad(z, z, z, 4, 2049, 12, z, 128, 128, z, None, z, z, z, z, z, z, z, None) == -5
    assert "2049" in lib.bbx_last_error().decode()
    assert lib.bbx_pmlp2_grad(z, z, z, 4, 64, 12, z, 128, 129, z, None, z, z, z, z, z, z, z, None) == -5
    assert "129" in lib.bbx_last_error().decode()


def test_partition_constants_are_in_the_header():
    per, most = g2.header_constants()
    assert per >= 1 and most >= 2
    from deepgroebner_amd import _ffi
    f = _ffi.lib().bbx_pmlp2_grad_workspace_floats
    # the workspace is one slot per workgroup: it grows by whole slots up to `most` of them
    slot = f(1, 64, 12, 64, 64)
    assert f(per, 64, 12, 64, 64) == slot and f(per + 1, 64, 12, 64, 64) == 2 * slot
    assert f(per * most, 64, 12, 64, 64) == most * slot == f(per * most + 5, 64, 12, 64, 64)


# ---- PMLPPolicy
def test_deep_kernels_defaults_to_false_and_cpu_tensors_take_the_torch_path():
    from deepgroebner_amd.rollout import PMLPPolicy
    assert PMLPPolicy(12, (64, 64)).deep_kernels is False and PMLPPolicy(12, (128,)).deep_kernels is False
    w, obs, rows, actions, _, _ = _batch(12, (64, 64), 5)
    pol = PMLPPolicy(12, (64, 64), deep_kernels=True)
    assert pol.deep_kernels is True
    with torch.no_grad():
        for dst, src in zip(pol.parameters(), pc.to_policy(w).parameters()):
            dst.copy_(src)
    lp, ent = pol.evaluate(torch.from_numpy(obs), torch.from_numpy(actions), torch.from_numpy(rows))
    assert lp.requires_grad and not type(lp.grad_fn).__name__.startswith("_PMLP2Evaluate")
    lp2, ent2 = pol.evaluate_torch(torch.from_numpy(obs), torch.from_numpy(actions), torch.from_numpy(rows))
    assert torch.equal(lp, lp2) and torch.equal(ent, ent2)
    rl, rh, ref = gc.reference_eval(w, obs, rows, actions)
    assert (np.abs(lp.detach().numpy() - rl) <= ref.tol()).all()
