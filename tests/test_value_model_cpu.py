"""The critic without a GPU: the float64 reference of tests/value_cases.py against torch autograd in double precision, PMLPValue's
torch path against that reference, what the C ABI refuses before anything is queued (no device is needed for a refusal), the
workspace sizes, DeviceTrajectoryBuffer.fill_values on a CPU buffer, and run_rollout_fused's check of its critic argument."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import policy_cases as pc
from tests import policy_grad_cases as gc
from tests import value_cases as vc

_ids = lambda v: str(v).replace(" ", "")
E_ARG, E_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def lib():
    graft.build()
    from deepgroebner_amd import _ffi
    return _ffi.lib()


CASE = dict(cols=7, hidden=(33,), rows=(5, 0, 1, 12, -2, 20, 1, 9), R=12, seed=40)


@pytest.fixture(scope="module")
def case():
    w, obs, rows, gvalue = vc.grad_case(**CASE)
    return w, obs, rows, gvalue, pc.reference(w, obs, rows)


@pytest.mark.parametrize("pool", vc.POOLS)
def test_reference_gradient_equals_autograd_in_float64(case, pool):
    """The reference values are PMLPValue.evaluate_torch's in float64 to 1e-12, the reference gradients are autograd's of
    L = sum_s gvalue_s V_s; states without rows (rows 0 and -2) are worth 0 and contribute nothing, one-row states contribute."""
    import torch
    w, obs, rows, gvalue, ref = case
    want_v, _ = vc.reference_values(w, obs, rows, pool, ref=ref)
    want_g, A = vc.reference_grad(w, obs, rows, gvalue, pool, ref=ref)
    cr = vc.to_critic(w, pool, dtype=torch.float64)
    v = cr.evaluate_torch(torch.from_numpy(obs), torch.from_numpy(rows))
    assert cr.last_path == "torch"
    assert v.dtype == torch.float64 and np.abs(v.detach().numpy() - want_v).max() <= 1e-12 * (1 + np.abs(want_v).max())
    assert (v.detach().numpy()[ref.n == 0] == 0.0).all()
    (torch.from_numpy(gvalue.astype(np.float64)) * v).sum().backward()
    lin = cr.embedding[0]
    got = (lin.weight.grad.t().numpy(), lin.bias.grad.numpy(), cr.head.weight.grad.reshape(-1).numpy(), cr.head.bias.grad.reshape(-1).numpy())
    for x, y in zip(got, want_g):
        assert np.abs(x.reshape(y.shape) - y).max() <= 1e-11 * (1 + np.abs(y).max())
    assert all((a >= 0).all() for a in A) and A[3][0] > 0
    # a one-row state alone has a gradient (the policy kernels skip such states; the critic does not)
    one = np.flatnonzero(ref.n == 1)[:1]
    g1, _ = vc.reference_grad(w, obs[one], rows[one], gvalue[one], pool)
    assert np.abs(g1[3][0] - gvalue[one][0]) <= 1e-12 and np.abs(g1[2]).max() > 0


@pytest.mark.parametrize("pool", vc.POOLS)
def test_torch_path_in_float32_against_the_reference(case, pool):
    """values_torch in float32 (rows given, and derived from -1 padding) within the kernels' own bound of the reference; out and
    out64 receive the same numbers; two hidden layers take the same path."""
    import torch
    w, obs, rows, _, ref = case
    want, _ = vc.reference_values(w, obs, rows, pool, ref=ref)
    cr = vc.to_critic(w, pool)
    out = torch.zeros(len(rows)); out64 = torch.zeros(len(rows), dtype=torch.float64)
    v = cr.values(torch.from_numpy(obs), torch.from_numpy(rows), out=out, out64=out64)
    assert v is out and cr.last_path == "torch"
    assert (np.abs(out.numpy() - want) <= vc.value_tol(ref, pool, want)).all()
    assert np.array_equal(out64.numpy(), out.numpy().astype(np.float64))
    padded = pc.fill_padding(obs, rows, False)
    v2 = cr(torch.from_numpy(padded))
    assert (np.abs(v2.detach().numpy() - want) <= vc.value_tol(ref, pool, want)).all()
    deep = vc.to_critic(pc.make_weights(7, (16, 8), 3), pool)
    v3 = deep.values(torch.from_numpy(obs), torch.from_numpy(rows))
    assert deep.last_path == "torch" and v3.shape == (len(rows),) and torch.isfinite(v3).all() and (v3.numpy()[ref.n == 0] == 0.0).all()


def test_fit_step_torch_path_matches_the_recipe(case):
    """fit_step on CPU tensors: the statistics are the recipe's, the gradients those of 1/2 mean d^2."""
    import torch
    w, obs, rows, _, ref = case
    cr = vc.to_critic(w, "mean")
    targets = np.linspace(-1.0, 2.0, len(rows)).astype(np.float32)
    stats, values = cr.fit_step(torch.from_numpy(obs), torch.from_numpy(rows), torch.from_numpy(targets))
    want = vc.fit_stats(values.numpy(), targets, 1.0 / len(rows))
    assert np.allclose(stats.numpy(), want, rtol=1e-6, atol=1e-6) and stats.numpy()[0] == len(rows) and stats.numpy()[5] == 0
    coef, _, _ = vc.fit_recipe(values.numpy(), targets, 1.0 / len(rows))
    g, A = vc.reference_grad(w, obs, rows, coef, "mean", ref=ref)
    got = cr.head.bias.grad.numpy()
    assert abs(got[0] - g[3][0]) <= 1e-5 * (1 + abs(g[3][0]))


# ---- the C ABI: refusals need no device
P = C.c_void_p(4096)                                              # (never dereferenced: every call below is refused first)


def _value(lib, cols=12, hidden=128, pool=0, obs_rows=16, values=P, values64=P, n=3):
    return lib.bbx_pmlp_value(P, P, n, obs_rows, cols, P, hidden, pool, values, values64, None)


def _value_at(lib, cols=12, hidden=128, pool=0, obs_rows=16, values=P, values64=P, n=3, n_src=5, index=P):
    return lib.bbx_pmlp_value_at(P, P, n_src, index, n, obs_rows, cols, P, hidden, pool, values, values64, None)


def _grad(lib, cols=12, hidden=128, pool=0, obs_rows=16, gvalue=P, n=3):
    return lib.bbx_pmlp_value_grad(P, P, n, obs_rows, cols, P, hidden, pool, gvalue, P, P, P, P, P, None)


def _grad_at(lib, cols=12, hidden=128, pool=0, obs_rows=16, n=3, n_src=5, index=P):
    return lib.bbx_pmlp_value_grad_at(P, P, n_src, index, n, obs_rows, cols, P, hidden, pool, P, P, P, P, P, P, None)


def _fit(lib, cols=12, hidden=128, pool=0, obs_rows=16, targets=P, coef=P, stats=P, n=3):
    return lib.bbx_pmlp_value_fit(P, P, n, obs_rows, cols, P, hidden, pool, targets, C.c_float(0.5), P, coef, stats, P, P, P, P, P, None)


def _fit_at(lib, cols=12, hidden=128, pool=0, obs_rows=16, targets=P, coef=P, stats=P, n=3, n_src=5, index=P):
    return lib.bbx_pmlp_value_fit_at(P, P, n_src, index, n, obs_rows, cols, P, hidden, pool, targets, C.c_float(0.5), P, coef, stats, P, P, P, P, P, None)


CALLS = (_value, _value_at, _grad, _grad_at, _fit, _fit_at)


@pytest.mark.parametrize("call", CALLS, ids=lambda f: f.__name__)
def test_abi_refuses_shapes_and_pools_before_anything_is_queued(lib, call):
    """The shapes bbx_pmlp_prepared_floats refuses and a block taller than the kernels score: BBX_E_UNSUPPORTED with a message; a
    pool of -1 or 3: BBX_E_ARG."""
    for cols, hidden in ((0, 128), (65, 128), (12, 0), (12, 257)):
        assert lib.bbx_pmlp_prepared_floats(cols, hidden) == E_UNSUPPORTED
        assert call(lib, cols=cols, hidden=hidden) == E_UNSUPPORTED, (cols, hidden)
        assert b"not built into the policy kernel" in lib.bbx_last_error()
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
        for name in ("targets", "coef", "stats"):
            assert call(lib, **{name: None}) == E_ARG, (call.__name__, name)
            assert b"null" in lib.bbx_last_error()
    assert _fit_at(lib, index=None) == E_ARG


def test_workspace_sizes(lib):
    """bbx_pmlp_value_grad_workspace_floats is bbx_pmlp_grad_workspace_floats over the shape table and the partition's batch
    sizes; the fit workspace is that plus its documented tail, d^2 | V | target | flags: four floats per position."""
    spw, maxw = gc.header_constants()
    for cols in pc.ONE_COLS:
        for hidden in pc.ONE_HIDDEN:
            for n in (0, 1, spw, spw + 1, 1030, spw * maxw + 5):
                g = lib.bbx_pmlp_grad_workspace_floats(n, 136, cols, hidden)
                assert g > 0 and g % 4 == 0
                assert lib.bbx_pmlp_value_grad_workspace_floats(n, 136, cols, hidden) == g, (cols, hidden, n)
                assert lib.bbx_pmlp_value_fit_workspace_floats(n, 136, cols, hidden) == g + 4 * n, (cols, hidden, n)
    for fn in (lib.bbx_pmlp_value_grad_workspace_floats, lib.bbx_pmlp_value_fit_workspace_floats):
        assert fn(5, 136, 65, 128) == E_UNSUPPORTED and fn(5, 136, 12, 257) == E_UNSUPPORTED and fn(5, 2049, 12, 128) == E_UNSUPPORTED
        assert fn(-1, 136, 12, 128) == E_ARG
    assert lib.bbx_pmlp_value_fit_workspace_floats(2 ** 30, 16, 12, 128) == E_ARG      # (would not fit an int)


# ---- the Python surface on CPU tensors
def _toy_buffer():
    """Two environments, four steps, blocks of 2 rows x 2 columns; a critic whose value is the sum of a state's live entries
    (W1 = 1, b1 = 0, w2 = 1, b2 = 0, pool sum; the entries are non-negative).  gam = lam = 1/2: every number is exact."""
    import torch
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer
    w = [(np.ones((2, 1), dtype=np.float32), np.zeros(1, dtype=np.float32)), (np.ones(1, dtype=np.float32), np.zeros(1, dtype=np.float32))]
    values = np.array([[4, 8], [2, 4], [6, 2], [2, 10]], dtype=np.float64)
    rewards = np.array([[-1, -1], [-2, -1], [-3, -2], [-4, -5]], dtype=np.float64)
    dones = np.array([[0, 0], [1, 0], [0, 1], [1, 0]], dtype=bool)
    buf = DeviceTrajectoryBuffer(5, 2, gam=0.5, lam=0.5, obs_shape=(2, 2), device="cpu")
    for t in range(4):
        st = np.zeros((2, 2, 2), dtype=np.int32)
        st[:, 0, 0] = values[t] - 1; st[:, 1, 1] = 1
        buf.store(torch.from_numpy(st), torch.full((2,), 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.from_numpy(rewards[t]),
                  torch.zeros(2), None, torch.from_numpy(dones[t]))
    return buf, vc.to_critic(w, "sum"), values


def test_fill_values_on_a_cpu_buffer_gives_the_hand_computed_advantages():
    """Environment 0: episodes (t = 0, 1) and (2, 3); environment 1: episode (0, 1, 2) and an unfinished step.  By hand, with
    delta_t = r_t - v_t + v_{t+1} / 2 inside an episode and adv_t = delta_t + adv_{t+1} / 4:
      env 0: adv_1 = -2 - 2 = -4, adv_0 = (-1 - 4 + 1) - 1 = -5; adv_3 = -4 - 2 = -6, adv_2 = (-3 - 6 + 1) - 1.5 = -9.5
      env 1: adv_2 = -2 - 2 = -4, adv_1 = (-1 - 4 + 1) - 1 = -5, adv_0 = (-1 - 8 + 2) - 1.25 = -8.25; adv_3 = -5 - 10 = -15 (incomplete)."""
    buf, critic, values = _toy_buffer()
    buf.finish()
    assert buf.returns is not None and (buf.values == 0).all()
    buf.fill_values(critic)
    assert buf.returns is None and buf.advantages is None and buf.complete is None
    assert buf.values.dtype.is_floating_point and np.array_equal(buf.values[:4].numpy(), values) and (buf.values[4] == 0).all()
    ret, adv, comp = buf._finish_torch()
    assert np.array_equal(adv.numpy(), np.array([[-5, -8.25], [-4, -5], [-9.5, -4], [-6, -15]]))
    assert np.array_equal(ret.numpy(), np.array([[-2, -2], [-2, -2], [-5, -2], [-4, -5]]))
    assert np.array_equal(comp.numpy(), np.array([[1, 1], [1, 1], [1, 1], [1, 0]], dtype=bool))
    # a range of steps only
    buf.values.zero_()
    buf.fill_values(critic, 1, 3)
    assert np.array_equal(buf.values[1:3].numpy(), values[1:3]) and (buf.values[0] == 0).all() and (buf.values[3] == 0).all()
    idx = buf.get_index(None)[0]
    assert buf.returns is not None and idx.numel() == 7                   # get_index finished again: the complete steps


def test_fill_values_and_value_update_need_states():
    import torch
    import deepgroebner_amd
    from deepgroebner_amd import DeviceTrajectoryBuffer, PMLPValue, value_update     # (exported from the package, resolved on first use)
    from deepgroebner_amd import rollout
    assert PMLPValue is rollout.PMLPValue and value_update is rollout.value_update and not hasattr(deepgroebner_amd, "no_such_name")
    buf = DeviceTrajectoryBuffer(4, 2, device="cpu")
    critic = PMLPValue(2, (4,))
    with pytest.raises(ValueError):
        buf.fill_values(critic)
    with pytest.raises(ValueError):
        value_update(critic, buf, torch.optim.SGD(critic.parameters(), lr=0.1), 1, 4)
    with pytest.raises(ValueError):
        PMLPValue(2, (4,), pool="max")


def test_value_update_on_a_cpu_buffer_reduces_the_loss():
    """The torch path end to end: three epochs of value_update on the toy buffer report a falling loss, with every position counted."""
    import torch
    from deepgroebner_amd.rollout import PMLPValue, value_update
    buf, _, _ = _toy_buffer()
    torch.manual_seed(0)
    critic = PMLPValue(2, (8,), pool="mean")
    out = value_update(critic, buf, torch.optim.Adam(critic.parameters(), lr=1e-2), 3, 4, shuffle=False)
    assert len(out) == 3 and out[0]["stats"].shape == (2, 6) and out[0]["stats"][:, 0].sum() == 7
    assert out[-1]["loss"] < out[0]["loss"]
    assert all(np.isfinite(o["explained_variance"]) for o in out)


def test_run_rollout_fused_refuses_a_critic_without_states_before_touching_the_environment():
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, PMLPPolicy, PMLPValue, run_rollout_fused
    critic = PMLPValue(12, (128,))
    policy = PMLPPolicy(12, (128,))
    with pytest.raises(ValueError):
        run_rollout_fused(None, policy, 8, None, critic=critic)
    with pytest.raises(ValueError):
        run_rollout_fused(None, policy, 8, DeviceTrajectoryBuffer(8, 4, device="cpu"), critic=critic)
