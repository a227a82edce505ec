"""Cross-entropy training without a GPU: the float64 reference of tests/xent_cases.py against torch autograd in double precision,
action_value_targets against a hand-written loop, what the ten new entry points refuse, PMLPPolicy's torch path on CPU tensors, and
the conditions the GPU cases of tests/test_xent_gpu.py rest on."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import policy_cases as pc
from tests import xent_cases as xc

_ids = lambda v: str(v).replace(" ", "")
ALL = xc.SHAPES_ONE + xc.SHAPES_TWO


def _case(cols, hidden, bad=True, null_weights=False):
    w, obs, rows, targets = xc.source(cols, hidden)
    index = xc.index_of(bad=bad)
    wk = None if null_weights else xc.weights_for(index)
    return w, obs, rows, targets, index, wk


# ---- the reference against autograd in double --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,hidden", ALL, ids=_ids)
def test_reference_equals_autograd_in_double(cols, hidden):
    import torch
    w, obs, rows, targets, index, wk = _case(cols, hidden)
    scale = 1.0 / len(index)
    xr = xc.reference(w, obs, rows, targets, index, wk, scale)
    pol = pc.to_policy(w, dtype=torch.float64)
    j = np.where((index >= 0) & (index < len(rows)), index, 0).astype(np.int64)
    t = np.where(xr.counted[:, None], np.nan_to_num(targets[j].astype(np.float64), nan=0.0), 0.0)
    loss = xc.torch_loss(pol, obs[j], rows[j], t, xr.w, float(xc.f32(scale)))
    loss.backward()
    assert np.isclose(float(loss.detach()), float(xc.f32(scale)) * xr.stats[1], rtol=1e-10, atol=0)
    got = [l.weight.grad.t().numpy() for l in pol.embedding]
    got = [x for l, g in zip(pol.embedding, got) for x in (g, l.bias.grad.numpy())] + [pol.deciding.weight.grad.numpy().reshape(-1), pol.deciding.bias.grad.numpy()]
    for x, y, a in zip(got, xr.grads, xr.A):                          # (1e-12 of the absolute contributions: db2 = c (T sum_r p_r - T) cancels to nothing)
        assert (np.abs(x - y.reshape(x.shape)) <= 1e-10 * np.abs(y.reshape(x.shape)) + 1e-12 * a.sum(axis=0).reshape(x.shape)).all(), float(np.abs(x - y.reshape(x.shape)).max())
    assert any(np.abs(y).max() > 0 for y in xr.grads)
    # per position: l against -(t * log_softmax).sum()
    for k in np.flatnonzero(xr.counted)[:8]:
        one = xc.torch_loss(pol, obs[j[k]:j[k] + 1], rows[j[k]:j[k] + 1], t[k:k + 1], np.ones(1), 1.0)
        assert np.isclose(float(one), xr.l[k], rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("cols,hidden", ALL, ids=_ids)
def test_what_counts(cols, hidden):
    w, obs, rows, targets, index, wk = _case(cols, hidden)
    wk = wk.copy(); wk[0] = np.inf
    xr = xc.reference(w, obs, rows, targets, index, wk)
    src = np.where((index >= 0) & (index < len(rows)), index, -1)
    kinds = np.array(xc.KINDS + ("outside",))[src]
    assert not xr.counted[0] and not xr.counted[kinds == "outside"].any() and (kinds == "outside").sum() == 2
    assert not xr.counted[(kinds == "negative") | (kinds == "nan")].any()
    rest = ~np.isin(kinds, ("outside", "negative", "nan")); rest[0] = False
    assert xr.counted[rest].all() and np.isnan(xr.l[~xr.counted]).all() and (xr.c[~xr.counted] == 0).all()
    assert (xr.l[xr.counted & (xr.n <= 1)] == 0).all() and (xr.l[xr.counted & (kinds == "zero")] == 0).all()
    assert xr.stats[0] == xr.counted.sum() and xr.stats[0] + xr.stats[5] == len(index)
    assert np.isclose(xr.T[kinds == "unnormalised"], 3.5, rtol=1e-6).all() and (xr.T[xr.counted & (kinds == "onehot")] == 1).all()


# ---- the conditions the GPU cases rest on ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("null_weights", [False, True], ids=["weights", "null"])
@pytest.mark.parametrize("bad", [True, False], ids=["at", "plain"])
@pytest.mark.parametrize("cols,hidden", ALL, ids=_ids)
def test_cases_are_mostly_healthy_and_no_bound_hides_an_entry(cols, hidden, bad, null_weights):
    w, obs, rows, targets, index, wk = _case(cols, hidden, bad, null_weights)
    xr = xc.reference(w, obs, rows, targets, index, wk)
    assert xc.healthy_fraction(xr) >= 0.8
    assert {0, 1, 2, 31, 32, 33, 64, 65, 80} <= set(int(x) for x in xr.n) and int(rows.max()) == 200
    depth = len(hidden)
    for g, b in zip(xr.grads, xc.grad_bounds(xr, depth)):
        assert not ((b.reshape(g.shape) == 0) & (g != 0)).any()
    unit = xc.loss_unit(xr)
    assert not ((unit == 0) & xr.counted & (np.nan_to_num(xr.l) != 0)).any()
    assert wk is None or ((wk == 0).any() and (wk < 0).any())


# ---- action_value_targets ------------------------------------------------------------------------------------------------------------
def _targets_by_hand(q, rows, obs_rows, temperature):
    B, R = q.shape
    out = np.zeros((B, obs_rows), dtype=np.float32)
    for e in range(B):
        n = max(0, min(int(rows[e]), R, obs_rows))
        if n == 0:
            continue
        x = q[e, :n]
        if temperature > 0:
            y = x / temperature
            ex = np.exp(y - y.max())
            out[e, :n] = (ex / ex.sum()).astype(np.float32)
        else:
            best = 0
            for a in range(1, n):
                if x[a] > x[best]:
                    best = a
            out[e, best] = 1.0
    return out


@pytest.mark.parametrize("temperature", [1.0, 0.25, 0.0])
@pytest.mark.parametrize("R,obs_rows", [(7, 12), (12, 7), (9, 9)])
def test_action_value_targets_against_a_hand_written_loop(R, obs_rows, temperature):
    import torch
    from deepgroebner_amd.rollout import action_value_targets
    rng = np.random.default_rng(R * 100 + obs_rows)
    rows = np.array([0, 1, 2, R, R - 1, 5, 3, R], dtype=np.int32)
    B = len(rows)
    q = np.full((B, R), np.nan)
    for e in range(B):
        q[e, :rows[e]] = -rng.integers(1, 6, size=rows[e]).astype(np.float64) * 1.5          # (few distinct values: ties)
    q[6, :3] = -2.0                                                                          # a tie over every live row
    want = _targets_by_hand(q, rows, obs_rows, temperature)
    got = action_value_targets(torch.from_numpy(q), torch.from_numpy(rows), obs_rows, temperature)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, obs_rows)
    assert np.allclose(got.numpy(), want, rtol=0, atol=1e-7) and (got.numpy()[0] == 0).all()
    if temperature == 0:
        assert np.array_equal(got.numpy(), want) and got.numpy()[6, 0] == 1.0
    else:
        live = np.minimum(rows, min(R, obs_rows))
        assert np.allclose(got.numpy().sum(axis=1)[live > 0], 1.0, atol=1e-6)
    out = torch.full((B, obs_rows), 7.0)
    assert action_value_targets(q, rows, obs_rows, temperature, out=out) is out and torch.equal(out, got)
    with pytest.raises(ValueError):
        action_value_targets(q, rows, obs_rows, -1.0)


def test_the_buffer_keeps_targets_only_when_asked():
    import torch
    from deepgroebner_amd.rollout import DeviceTrajectoryBuffer, imitation_update
    plain = DeviceTrajectoryBuffer(3, 2, obs_shape=(4, 6), device="cpu")
    assert plain.targets is None
    z = torch.zeros(2)
    plain.store(torch.zeros((2, 4, 6), dtype=torch.int32), z.int(), z.int(), z.double(), z, None, z.bool())
    with pytest.raises(ValueError):
        plain.store(torch.zeros((2, 4, 6), dtype=torch.int32), z.int(), z.int(), z.double(), z, None, z.bool(), target=torch.zeros((2, 4)))
    with pytest.raises(ValueError):
        imitation_update(None, plain, None, 1, 2)
    with pytest.raises(ValueError):
        DeviceTrajectoryBuffer(3, 2, device="cpu", targets=True)
    buf = DeviceTrajectoryBuffer(3, 2, obs_shape=(4, 6), device="cpu", targets=True)
    assert buf.targets.dtype == torch.float32 and tuple(buf.targets.shape) == (3, 2, 4) and (buf.targets == 0).all()
    buf.store(torch.zeros((2, 4, 6), dtype=torch.int32), z.int(), z.int(), z.double(), z, None, z.bool(), target=torch.full((2, 4), 0.25))
    assert (buf.targets[0] == 0.25).all() and (buf.targets[1:] == 0).all() and buf.t == 1


# ---- the torch path on CPU tensors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (33, (40, 100)), (12, (16, 12, 8))], ids=_ids)
def test_xent_torch_on_cpu_tensors_against_the_reference(cols, hidden):
    import torch
    if len(hidden) == 3:
        w = pc.make_weights(cols, hidden, 900)
        _, obs, rows, targets = xc.source(cols, (8,))
    else:
        w, obs, rows, targets = xc.source(cols, hidden)
    index = xc.index_of(bad=False)
    wk = xc.weights_for(index)
    pol = pc.to_policy(w, dtype=torch.float64)
    st, rw, tg, idx = (torch.from_numpy(np.array(a)) for a in (obs, rows, targets, index))
    stats, losses, ent = pol.xent_step_at(st, rw, idx, tg, torch.from_numpy(wk))
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (6,)
    if len(hidden) < 3:
        xr = xc.reference(w, obs, rows, targets, index, wk, 1.0 / len(index))
        cn = xr.counted
        assert np.array_equal(np.isnan(losses.numpy()), ~cn)
        assert np.allclose(losses.numpy()[cn], xr.l[cn], rtol=1e-10, atol=1e-13) and np.allclose(ent.numpy(), xr.H, rtol=1e-10, atol=1e-13)
        assert np.allclose(stats.numpy(), xr.stats, rtol=1e-10, atol=1e-12)
        got = [x for l in pol.embedding for x in (l.weight.grad.t().numpy(), l.bias.grad.numpy())] + [pol.deciding.weight.grad.numpy().reshape(-1),
                                                                                                      pol.deciding.bias.grad.numpy()]
        sc = float(xc.f32(1.0 / len(index))) * len(index)               # (the reference rounds 1 / n to float32, the torch path does not)
        for x, y, a in zip(got, xr.grads, xr.A):
            assert (np.abs(x * sc - y.reshape(x.shape)) <= 1e-9 * np.abs(y.reshape(x.shape)) + 1e-12 * a.sum(axis=0).reshape(x.shape)).all()
    once = [q.grad.clone() for q in pol.parameters()]
    pol.xent_step_at(st, rw, idx, tg, torch.from_numpy(wk))              # adds, as backward() does
    assert all(torch.allclose(q.grad, 2 * g, rtol=1e-12, atol=0) for q, g in zip(pol.parameters(), once))
    l2, e2 = pol.xent_at(st, rw, idx, tg, torch.from_numpy(wk))
    assert torch.equal(torch.nan_to_num(l2), torch.nan_to_num(losses)) and not l2.requires_grad


def test_twenty_adam_steps_lower_the_loss_of_the_torch_path():
    """The descent check of tests/test_xent_gpu.py on synthetic inputs of its shapes: 256 states of 64 rows, PMLP(128), softmax targets."""
    import torch
    torch.manual_seed(11)
    from deepgroebner_amd.rollout import PMLPPolicy
    rng = np.random.default_rng(970)
    N, R, cols = 256, 64, 12
    rows = rng.integers(2, 40, size=N).astype(np.int32)
    obs = pc.fill_padding(pc.random_blocks(N, R, cols, 971), rows, False)
    targets = xc.targets_for(rows, R, ["soft"] * N, 972)
    pol = PMLPPolicy(cols, [128])
    st, rw, tg = torch.from_numpy(obs), torch.from_numpy(rows), torch.from_numpy(targets)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
    opt.zero_grad()
    means = []
    for _ in range(21):
        stats, _, _ = pol.xent_step(st, rw, tg)
        means.append(float(stats[1] / stats[4]))
        opt.step(); opt.zero_grad()
    assert stats[0] == N and np.isfinite(means).all() and means[-1] < means[0]


# ---- what the entry points refuse ------------------------------------------------------------------------------------------------
BBX_E_ARG, BBX_E_UNSUPPORTED = -1, -5
_HOST = (C.c_double * 64)()                                 # what every non-null pointer points to: a refused call reads none of it
VALID = {"n": 3, "n_src": 3, "obs_rows": 2, "cols": 6, "hidden": 33, "hidden1": 8, "hidden2": 8, "scale": 1.0, "stream": None}


def _params(two, grad, at):
    p = ["d_obs", "d_rows", "d_targets"] + (["n_src", "d_index"] if at else []) + ["n", "obs_rows", "cols", "d_prepared"]
    p += (["hidden1", "hidden2"] if two else ["hidden"]) + ["d_weights", "scale", "d_losses", "d_entropy"]
    if grad:
        p += ["d_coef", "d_stats", "d_workspace", "d_gw1", "d_gb1", "d_gw2", "d_gb2"] + (["d_gw3", "d_gb3"] if two else [])
    return p + ["stream"]


def _shared_faults(two, at, query=False):
    """[(label, {argument: value}, code)]: the shape, rows, bad and index faults of tests/test_pmlp_refusals_cpu.py."""
    f = [("cols=0", {"cols": 0}, BBX_E_UNSUPPORTED), ("cols=65", {"cols": 65}, BBX_E_UNSUPPORTED)]
    for name, over in ((("hidden1", 129), ("hidden2", 129)) if two else (("hidden", 257),)):
        f += [("%s=0" % name, {name: 0}, BBX_E_UNSUPPORTED), ("%s=%d" % (name, over), {name: over}, BBX_E_UNSUPPORTED)]
    f += [("obs_rows=2049", {"obs_rows": 2049}, BBX_E_UNSUPPORTED), ("obs_rows=0", {"obs_rows": 0}, BBX_E_ARG), ("n=-1", {"n": -1}, BBX_E_ARG)]
    if at and not query:
        f += [("n_src=-1", {"n_src": -1}, BBX_E_ARG), ("d_index=null", {"d_index": None}, BBX_E_ARG)]
    return f


def _entry_points():
    for two in (False, True):
        for grad in (False, True):
            for at in (False, True):
                yield ("bbx_pmlp2_xent" if two else "bbx_pmlp_xent") + ("_grad" if grad else "") + ("_at" if at else ""), two, grad, at


@pytest.fixture(scope="module")
def ffi_():
    import __graft_entry__ as graft
    graft.build()
    from deepgroebner_amd import _ffi
    return _ffi


def _call(ffi, name, params, changed):
    dll = ffi.lib()
    args = [changed[p] if p in changed else VALID[p] if p in VALID else C.addressof(_HOST) for p in params]
    rc = getattr(dll, name)(*args)
    return rc, dll.bbx_last_error().decode()


def _golden(name):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pmlp_refusals.json")) as f:
        g = json.load(f)
    return {label: g["outcomes"][i] for label, i in zip(g["calls"][name]["cases"], g["calls"][name]["outcome"])}


@pytest.mark.parametrize("name,two,grad,at", list(_entry_points()), ids=lambda v: v if isinstance(v, str) else "")
def test_refusals_of_the_entry_points(ffi_, name, two, grad, at):
    params = _params(two, grad, at)
    assert len(params) == len(ffi_.SIGNATURES[name][1]), name
    for p, t in zip(params, ffi_.SIGNATURES[name][1]):
        assert (p.startswith("d_") or p == "stream") == (t is C.c_void_p), (name, p)
    # the faults the PPO / log-probability entries know: the same code and the same words
    twin = _golden(name.replace("_xent_grad", "_ppo_grad").replace("_xent", "_logprob"))
    required = ["d_obs", "d_rows", "d_prepared"] + (["d_workspace", "d_gw1", "d_gb1", "d_gw2", "d_gb2"] + (["d_gw3", "d_gb3"] if two else []) if grad else ["d_losses"])
    faults = _shared_faults(two, at) + [("%s=null" % a, {a: None}, BBX_E_ARG) for a in required]
    for label, changed, code in faults:
        rc, msg = _call(ffi_, name, params, changed)
        assert rc == code and msg and "launch failed" not in msg, (name, label, rc, msg)
        assert [rc, msg] == twin[label.replace("d_losses", "d_logprobs")], (name, label, rc, msg)
    # the call's own, each alone
    own = [("d_targets=null", {"d_targets": None}, "null argument")]
    if grad:
        own += [("d_coef=null", {"d_coef": None}, "null argument"), ("d_stats=null", {"d_stats": None}, "null argument")]
    own += [("scale=nan", {"scale": float("nan")}, "scale"), ("scale=inf", {"scale": float("inf")}, "scale"), ("scale=-inf", {"scale": float("-inf")}, "scale")]
    for label, changed, words in own:
        rc, msg = _call(ffi_, name, params, changed)
        assert rc == BBX_E_ARG and words in msg, (name, label, rc, msg)
    # a shape fault outranks the call's own; so does a null pointer of the states
    rc, msg = _call(ffi_, name, params, {"cols": 65, "scale": float("nan")})
    assert rc == BBX_E_UNSUPPORTED
    rc, msg = _call(ffi_, name, params, {"d_obs": None, "scale": float("nan")})
    assert rc == BBX_E_ARG and msg == "null argument"
    # what may be left out is no fault, but the call then reaches a launcher: nothing here tries it


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
def test_refusals_of_the_workspace_queries(ffi_, two):
    name = "bbx_pmlp2_xent_workspace_floats" if two else "bbx_pmlp_xent_workspace_floats"
    params = ["n", "obs_rows", "cols"] + (["hidden1", "hidden2"] if two else ["hidden"])
    twin = _golden(name.replace("_xent_", "_ppo_"))
    for label, changed, code in _shared_faults(two, False, query=True):
        rc, msg = _call(ffi_, name, params, changed)
        assert rc == code and [rc, msg] == twin[label], (name, label, rc, msg)
    dll = ffi_.lib()
    h = (8, 8) if two else (33,)
    grad = getattr(dll, name.replace("_xent_", "_grad_"))
    for n in (0, 1, 3, 4097):
        assert getattr(dll, name)(n, 2, 6, *h) == grad(n, 2, 6, *h) + 5 * n
    big = 2 ** 31 - 1
    rc = getattr(dll, name)(big, 2, 6, *h)
    assert rc == BBX_E_ARG and "would not fit an int" in dll.bbx_last_error().decode()
