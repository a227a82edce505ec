"""The two-layer critic without a GPU: the float64 reference of tests/value2_cases.py against torch autograd in double precision, the
assertions of the exact-integer builders for every parameter set tests/test_value2_model_gpu.py uses, PMLPValue's deep_kernels flag
and its torch path on CPU tensors, the gathered fallbacks of the _at methods, and what the C ABI answers without a device: the
workspace sizes and the refusals."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import policy2_grad_cases as g2
from tests import policy_cases as pc
from tests import value2_cases as v2
from tests import value_cases as vc

_ids = lambda v: str(v).replace(" ", "")
E_ARG, E_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def lib():
    graft.build()
    from deepgroebner_amd import _ffi
    return _ffi.lib()


CASE = dict(cols=7, hidden=(33, 18), rows=(5, 0, 1, 12, -2, 20, 1, 9), R=12, seed=45)


@pytest.fixture(scope="module")
def case():
    w, obs, rows, gvalue = v2.grad_case(**CASE)
    return w, obs, rows, gvalue, pc.reference(w, obs, rows)


def _param_grads(cr):
    l1, l2 = cr.embedding
    return (l1.weight.grad.t().numpy(), l1.bias.grad.numpy(), l2.weight.grad.t().numpy(), l2.bias.grad.numpy(),
            cr.head.weight.grad.reshape(-1).numpy(), cr.head.bias.grad.reshape(-1).numpy())


@pytest.mark.parametrize("pool", v2.POOLS)
def test_reference_gradient_equals_autograd_in_float64(case, pool):
    """The reference values are PMLPValue.evaluate_torch's in float64 to 1e-12, the six reference gradients autograd's of
    L = sum_s gvalue_s V_s; states without rows (rows 0 and -2) contribute nothing, one-row states do."""
    import torch
    w, obs, rows, gvalue, ref = case
    want_v, _ = vc.reference_values(w, obs, rows, pool, ref=ref)
    want_g, A = v2.reference_grad2(w, obs, rows, gvalue, pool, ref=ref)
    cr = v2.to_critic(w, pool, dtype=torch.float64)
    v = cr.evaluate(torch.from_numpy(obs), torch.from_numpy(rows))
    assert cr.last_path == "torch"
    assert v.dtype == torch.float64 and np.abs(v.detach().numpy() - want_v).max() <= 1e-12 * (1 + np.abs(want_v).max())
    (torch.from_numpy(gvalue.astype(np.float64)) * v).sum().backward()
    for x, y in zip(_param_grads(cr), want_g):
        assert np.abs(x.reshape(y.shape) - y).max() <= 1e-11 * (1 + np.abs(y).max())
    assert all((a >= 0).all() for a in A) and A[5][0] > 0 and all(np.abs(y).max() > 0 for y in want_g)
    one = np.flatnonzero(ref.n == 1)[:1]
    g1, _ = v2.reference_grad2(w, obs[one], rows[one], gvalue[one], pool)
    assert np.abs(g1[5][0] - gvalue[one][0]) <= 1e-12 and np.abs(g1[4]).max() > 0
    none = np.flatnonzero(ref.n == 0)
    g0, A0 = v2.reference_grad2(w, obs[none], rows[none], np.full(len(none), 1e30), pool)
    assert all((y == 0).all() for y in g0) and all((a == 0).all() for a in A0)


@pytest.mark.parametrize("cols,hidden,pool,n", v2.INT_CASES, ids=_ids)
def test_integer_cases_keep_their_promises(cols, hidden, pool, n):
    """int_case_reference asserts integers, absolute sums below 2^24 and gradients that are not degenerate: for every parameter set
    of the GPU test."""
    w, obs, rows, gvalue = v2.int_case(cols, hidden, pool, n)
    vals, want = v2.int_case_reference(pool, w, obs, rows, gvalue)
    assert obs.shape == (v2.INT_N, n + 3, cols) and (obs[:, n:] != -1).any()              # (garbage behind the live rows)
    assert len(want) == 6 and want[0].shape == (cols, hidden[0]) and want[2].shape == hidden


def test_deep_kernels_defaults_to_false_and_cpu_tensors_take_the_torch_path(case):
    import torch
    from deepgroebner_amd.rollout import PMLPValue
    w, obs, rows, _, ref = case
    assert PMLPValue(7, (33, 18)).deep_kernels is False and PMLPValue(7, (33,)).deep_kernels is False
    assert PMLPValue(7, (33, 18), "mean", True).deep_kernels is True and PMLPValue(7, (33, 18), deep_kernels=True).pool == "sum"
    for pool in v2.POOLS:
        cr = v2.to_critic(w, pool)
        assert cr.deep_kernels is True
        want, _ = vc.reference_values(w, obs, rows, pool, ref=ref)
        tobs, trows = torch.from_numpy(obs), torch.from_numpy(rows)
        assert not cr.kernels_ok(tobs)
        v = cr.values(tobs, trows)
        assert cr.last_path == "torch" and (np.abs(v.numpy() - want) <= vc.value_tol(ref, pool, want, c_v=v2.C_V2)).all()
        cr.last_path = None
        e = cr.evaluate(tobs, trows)
        assert cr.last_path == "torch" and e.requires_grad and "PMLP2ValueEvaluate" not in type(e.grad_fn).__name__
        cr.last_path = None
        cr.fit_step(tobs, trows, torch.zeros(len(rows)))
        assert cr.last_path == "torch" and all(q.grad is not None for q in cr.parameters())


def test_gathered_fallbacks_on_cpu_buffers_equal_the_calls_on_gathered_arrays(case):
    """values_at / evaluate_at / fit_step_at on CPU buffers, flat and [T, B]: the calls on states[index], rows[index]."""
    import torch
    w, obs, rows, _, _ = case
    tobs, trows = torch.from_numpy(obs), torch.from_numpy(rows)
    index = torch.tensor([7, 0, 0, 3, 5, 2])
    targets = torch.linspace(-1, 1, len(index))
    for buf_obs, buf_rows in ((tobs, trows), (tobs.view(4, 2, *obs.shape[1:]), trows.view(4, 2))):
        a, b = v2.to_critic(w, "mean"), v2.to_critic(w, "mean")
        assert torch.equal(a.values_at(buf_obs, buf_rows, index), b.values(tobs[index], trows[index]))
        assert torch.equal(a.evaluate_at(buf_obs, buf_rows, index), b.evaluate(tobs[index], trows[index]))
        sa, va = a.fit_step_at(buf_obs, buf_rows, index, targets)
        sb, vb = b.fit_step(tobs[index], trows[index], targets)
        assert a.last_path == "torch" and torch.equal(sa, sb) and torch.equal(va, vb)
        for x, y in zip(a.parameters(), b.parameters()):
            assert torch.equal(x.grad, y.grad)


# ---- the C ABI: sizes and refusals need no device
P = C.c_void_p(4096)                                              # (never dereferenced: every call below is refused first)


def test_workspace_sizes(lib):
    """bbx_pmlp2_value_grad_workspace_floats is bbx_pmlp2_grad_workspace_floats over the shape table and the partition's batch sizes;
    the fit workspace is that plus four floats per position; both negative for cols 65, hidden 129 and obs_rows 2049."""
    spg, maxg = g2.header_constants()
    for cols in pc.TWO_COLS:
        for h1, h2 in pc.TWO_HIDDEN:
            for n in (0, 1, spg, spg + 1, 1030, spg * maxg + 5):
                g = lib.bbx_pmlp2_grad_workspace_floats(n, 136, cols, h1, h2)
                assert g > 0 and g % 4 == 0
                assert lib.bbx_pmlp2_value_grad_workspace_floats(n, 136, cols, h1, h2) == g, (cols, h1, h2, n)
                assert lib.bbx_pmlp2_value_fit_workspace_floats(n, 136, cols, h1, h2) == g + 4 * n, (cols, h1, h2, n)
    for fn in (lib.bbx_pmlp2_value_grad_workspace_floats, lib.bbx_pmlp2_value_fit_workspace_floats):
        assert fn(5, 136, 65, 128, 128) == E_UNSUPPORTED and fn(5, 136, 12, 129, 64) == E_UNSUPPORTED and fn(5, 136, 12, 64, 129) == E_UNSUPPORTED
        assert fn(5, 2049, 12, 128, 128) == E_UNSUPPORTED and fn(-1, 136, 12, 128, 128) == E_ARG
    assert lib.bbx_pmlp2_value_fit_workspace_floats(2 ** 30, 16, 12, 128, 128) == E_ARG      # (would not fit an int)


def _value(lib, cols=12, h1=128, h2=64, pool=0, obs_rows=16, values=P, values64=P, n=3):
    return lib.bbx_pmlp2_value(P, P, n, obs_rows, cols, P, h1, h2, pool, values, values64, None)


def _value_at(lib, cols=12, h1=128, h2=64, pool=0, obs_rows=16, values=P, values64=P, n=3, n_src=5, index=P):
    return lib.bbx_pmlp2_value_at(P, P, n_src, index, n, obs_rows, cols, P, h1, h2, pool, values, values64, None)


def _grad(lib, cols=12, h1=128, h2=64, pool=0, obs_rows=16, gvalue=P, n=3):
    return lib.bbx_pmlp2_value_grad(P, P, n, obs_rows, cols, P, h1, h2, pool, gvalue, P, P, P, P, P, P, P, None)


def _grad_at(lib, cols=12, h1=128, h2=64, pool=0, obs_rows=16, n=3, n_src=5, index=P):
    return lib.bbx_pmlp2_value_grad_at(P, P, n_src, index, n, obs_rows, cols, P, h1, h2, pool, P, P, P, P, P, P, P, P, None)


def _fit(lib, cols=12, h1=128, h2=64, pool=0, obs_rows=16, targets=P, coef=P, stats=P, n=3):
    return lib.bbx_pmlp2_value_fit(P, P, n, obs_rows, cols, P, h1, h2, pool, targets, C.c_float(0.5), P, coef, stats, P, P, P, P, P, P, P, None)


def _fit_at(lib, cols=12, h1=128, h2=64, pool=0, obs_rows=16, targets=P, coef=P, stats=P, n=3, n_src=5, index=P):
    return lib.bbx_pmlp2_value_fit_at(P, P, n_src, index, n, obs_rows, cols, P, h1, h2, pool, targets, C.c_float(0.5), P, coef, stats, P, P, P, P, P,
                                      P, P, None)


CALLS = (_value, _value_at, _grad, _grad_at, _fit, _fit_at)


@pytest.mark.parametrize("call", CALLS, ids=lambda f: f.__name__)
def test_abi_refuses_shapes_and_pools_before_anything_is_queued(lib, call):
    """The shapes bbx_pmlp2_logprob refuses, with its error codes and messages; a pool of -1 or 3: BBX_E_ARG."""
    for kw, word in ((dict(cols=0), b"cols"), (dict(cols=65), b"cols"), (dict(h1=0), b"hidden1"), (dict(h1=129), b"hidden1"), (dict(h2=0), b"hidden2"),
                     (dict(h2=129), b"hidden2")):
        assert call(lib, **kw) == E_UNSUPPORTED, kw
        assert word in lib.bbx_last_error()
    assert call(lib, obs_rows=2049) == E_UNSUPPORTED
    for pool in (-1, 3):
        assert call(lib, pool=pool) == E_ARG, pool
        assert b"pool" in lib.bbx_last_error()
    assert call(lib, n=-1) == E_ARG and call(lib, obs_rows=0) == E_ARG


def test_abi_refuses_the_nulls_it_names(lib):
    assert _value(lib, values=None, values64=None) == E_ARG and _value_at(lib, values=None, values64=None) == E_ARG
    assert _value_at(lib, index=None) == E_ARG and _value_at(lib, n_src=-1) == E_ARG
    assert _grad(lib, gvalue=None) == E_ARG and _grad_at(lib, index=None) == E_ARG
    for call in (_fit, _fit_at):
        for name in ("targets", "coef"):                              # (d_stats may be NULL: no statistics)
            assert call(lib, **{name: None}) == E_ARG, (call.__name__, name)
            assert b"null" in lib.bbx_last_error()
    assert _fit_at(lib, index=None) == E_ARG
