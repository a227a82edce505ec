"""The PPO call without a GPU: the six bbx_pmlp[2]_ppo_* symbols and their refusals, the float64 reference of tests/ppo_cases.py
against torch autograd in double precision, the placed ratios' distance from the clip bounds, and PMLPPolicy.ppo_step_at /
ppo_update on CPU tensors (the torch path).  (tests/test_ppo_gpu.py runs the kernels.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import policy_cases as pc
from tests import policy_grad_cases as gc
from tests import ppo_cases as pp

E_ARG, E_UNSUPPORTED = -1, -5
NAMES = ("bbx_pmlp_ppo_workspace_floats", "bbx_pmlp_ppo_grad", "bbx_pmlp_ppo_grad_at",
         "bbx_pmlp2_ppo_workspace_floats", "bbx_pmlp2_ppo_grad", "bbx_pmlp2_ppo_grad_at")


def _calls():
    """The four entries with every pointer a (never followed) non-null address; keyword overrides name what a case changes."""
    from deepgroebner_amd import _ffi
    lib = _ffi.lib()
    z = C.c_void_p(16)
    f = C.c_float

    def make(name, two, at):
        def call(n=4, R=64, cols=12, h=64, n_src=8, idx=z, mode=1, eps=0.2, old=z, adv=z, coef=z, stats=z, ws=z, gw1=z):
            src = (z, z, z) + ((n_src, idx, n) if at else (n,)) + (R, cols, z) + ((h, h) if two else (h,))
            outs = (gw1, z, z, z) + ((z, z) if two else ())
            return getattr(lib, name)(*src, old, adv, mode, f(0.25), f(eps), f(0.01), f(0.0), None, None, coef, stats, ws, *outs, None)
        return call
    return lib, [(make("bbx_pmlp_ppo_grad", False, False), 257, False), (make("bbx_pmlp_ppo_grad_at", False, True), 257, True),
                 (make("bbx_pmlp2_ppo_grad", True, False), 129, False), (make("bbx_pmlp2_ppo_grad_at", True, True), 129, True)]


def test_abi_symbols_and_refusals():
    from deepgroebner_amd import _ffi
    lib, calls = _calls()
    for name in NAMES:
        assert name in _ffi.SIGNATURES and getattr(lib, name) is not None
    for call, wide, at in calls:
        # unsupported shapes are refused before anything is queued (no device needed to hear it)
        assert call(h=wide) == E_UNSUPPORTED and str(wide) in lib.bbx_last_error().decode()
        assert call(cols=65) == E_UNSUPPORTED and "65" in lib.bbx_last_error().decode()
        assert call(R=2049) == E_UNSUPPORTED and "2049" in lib.bbx_last_error().decode()
        # the arguments of the loss
        for mode in (-1, 3):
            assert call(mode=mode) == E_ARG and "mode" in lib.bbx_last_error().decode()
        assert call(eps=-0.01) == E_ARG
        assert call(eps=float("nan")) == E_ARG
        for null in ("old", "adv", "coef", "stats", "ws", "gw1"):
            assert call(**{null: None}) == E_ARG, null
        assert call(n=-1) == E_ARG
        if at:
            assert call(n_src=-1) == E_ARG
            assert call(idx=None, n=1) == E_ARG
    # the workspace: the gradient kernels' own and four floats per position behind it; the shapes' refusals
    for n in (0, 1, 5, 4096):
        assert lib.bbx_pmlp_ppo_workspace_floats(n, 64, 12, 128) == lib.bbx_pmlp_grad_workspace_floats(n, 64, 12, 128) + 4 * n
        assert lib.bbx_pmlp2_ppo_workspace_floats(n, 64, 12, 128, 64) == lib.bbx_pmlp2_grad_workspace_floats(n, 64, 12, 128, 64) + 4 * n
    assert lib.bbx_pmlp_ppo_workspace_floats(4, 64, 12, 257) == E_UNSUPPORTED
    assert lib.bbx_pmlp2_ppo_workspace_floats(4, 64, 12, 129, 64) == E_UNSUPPORTED
    assert lib.bbx_pmlp_ppo_workspace_floats(4, 64, 65, 64) == E_UNSUPPORTED
    assert lib.bbx_pmlp_ppo_workspace_floats(4, 2049, 12, 64) == E_UNSUPPORTED
    assert lib.bbx_pmlp_ppo_workspace_floats(-1, 64, 12, 64) == E_ARG
    assert lib.bbx_pmlp_ppo_workspace_floats(2 ** 31 - 1, 64, 12, 64) == E_ARG       # (4 n floats do not fit an int)


# ---- the float64 reference against autograd in double precision ------------------------------------------------------------------
def _random_positions(n=2000, seed=1):
    """Log-probabilities, ratios on both sides of both bounds (and exactly on neither), advantages of both signs with zeros."""
    rng = np.random.default_rng(seed)
    new = -rng.uniform(0.05, 6.0, size=n)
    old, t = pp.placed_old(new, seed)
    old[n // 2:] = pp.far_old(new, seed)[n // 2:]
    adv = pp.advantages(n, seed)
    H = rng.uniform(0.0, 3.0, size=n)
    return new, H, old, adv


class _NumpyExp(torch.autograd.Function):
    """exp with the values numpy's exp gives (torch's differs from it in the last bit on some processors; the comparison below
    is about the loss's formulae, which are to agree to the last bit, not about two exponential routines)."""

    @staticmethod
    def forward(ctx, x):
        y = torch.from_numpy(np.exp(x.detach().numpy()))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_reference_coefficients_equal_autograd_in_double(mode):
    new, H, old, adv = _random_positions()
    loss = pp.Loss(mode, len(new), ent_coef=0.01, c_kl=0.3)
    u, gl, ge, clipped, counted, r, d = pp.reference_loss(loss, new, H, old, adv)
    tn = torch.tensor(new, dtype=torch.float64, requires_grad=True); tH = torch.tensor(H, dtype=torch.float64, requires_grad=True)
    to, tA = torch.tensor(old.astype(np.float64)), torch.tensor(adv.astype(np.float64))
    tr = _NumpyExp.apply(tn - to)
    if mode == 0:
        tu = tn * tA
    elif mode == 1:
        tu = torch.min(tr * tA, torch.clamp(tr, loss.lo, loss.hi) * tA)
    else:
        tu = tr * tA - loss.c_kl * (to - tn)
    L = -tu.sum() * loss.scale - (loss.scale * loss.ent_coef) * tH.sum()
    L.backward()
    assert counted.all() and (adv == 0).any() and (adv > 0).any() and (adv < 0).any()
    assert float(np.abs(tn.grad.numpy() - gl).max()) == 0.0
    assert float(np.abs(tH.grad.numpy() - ge).max()) == 0.0
    assert float(np.abs(tu.detach().numpy() - u).max()) == 0.0
    if mode == 1:
        assert clipped.any() and (~clipped).any() and ((gl == 0) == (clipped | (adv == 0))).all()
    st = pp.reference_stats(loss, new, H, old, adv)
    assert st[0] == len(new) and st[5] == 0 and st[4] == clipped.sum()
    assert abs(st[1] - float(tu.detach().sum())) <= 1e-9 and abs(st[3] - float((to - tn.detach()).sum())) <= 1e-9


def test_uncounted_positions_of_the_reference():
    new, H, old, adv = _random_positions(40, 2)
    new[[3, 17]] = np.nan
    for mode in (0, 1, 2):
        loss = pp.Loss(mode, 40, c_kl=0.3)
        u, gl, ge, clipped, counted, r, d = pp.reference_loss(loss, new, H, old, adv)
        assert not counted[[3, 17]].any() and (u[[3, 17]] == 0).all() and (gl[[3, 17]] == 0).all() and (ge[[3, 17]] == 0).all()
        st = pp.reference_stats(loss, new, H, old, adv)
        assert st[0] == 38 and st[5] == 2 and np.isfinite(st).all()


def test_every_placed_ratio_keeps_its_distance_from_the_clip_bounds():
    """The condition under which a float32 clip decision must agree with the reference: no position is excluded anywhere."""
    for seed in range(7):
        new, H, old, adv = _random_positions(700, seed)
        placed, t = pp.placed_old(new, seed)
        assert set(np.round(t, 2)) == set(pp.PLACED)
        assert pp.distance_from_bounds(new, placed) >= pp.MARGIN
        assert pp.distance_from_bounds(new, pp.far_old(new, seed)) >= pp.MARGIN
        far = np.abs(new - pp.far_old(new, seed).astype(np.float64))
        assert 9.9 < far.max() <= 10.0 + 1e-5
    # ... and for the log-probabilities of the GPU tests' recorded states, whatever the weights
    t = pp.header_constants()
    for cols, hidden in pp.ONE + pp.TWO:
        for index in (np.arange(pp.S), np.resize(np.arange(pp.S), 2 * t + 1)):
            new64 = pp.reference_at(cols, hidden, index)[0]
            assert np.isnan(new64).any() and np.isfinite(new64).any()
            for old in (pp.placed_old(new64, cols)[0], pp.far_old(new64, cols)):
                assert pp.distance_from_bounds(new64, old) >= pp.MARGIN


# ---- PMLPPolicy.ppo_step_at on CPU tensors: the torch path -----------------------------------------------------------------------
T, B, R, COLS = 7, 5, 4, 3


def _buffer():
    from tests.test_policy_indexed_cpu import _buffer as make
    return make()


def _torch_loss(mode, logp, ent, old, adv, clip, ent_coef, c_kl):
    ratio = torch.exp(logp - old)
    if mode == "pg":
        u = logp * adv
    elif mode == "clip":
        u = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv)
    else:
        u = ratio * adv - c_kl * (old - logp)
    return -u.mean() - ent_coef * ent.mean(), u


@pytest.mark.parametrize("mode", ["pg", "clip", "penalty"])
@pytest.mark.parametrize("hidden", [(16,), (8, 8), (8, 4, 8)], ids=str)
def test_ppo_step_at_on_cpu_tensors_equals_evaluate_at_and_the_torch_loss(hidden, mode):
    buf = _buffer()
    pol = pc.to_policy(pc.make_weights(COLS, hidden, 7))
    rows = buf.rows.view(-1)
    ok = (rows >= 1) & (buf.actions.view(-1) < rows)
    # 16 positions (1 / n exact), some of them twice, every log-probability a number
    index = torch.from_numpy(np.resize(torch.nonzero(ok).view(-1).numpy(), 16).astype(np.int32))
    assert ok.sum() >= 8
    g = torch.Generator().manual_seed(3)
    adv = torch.randn(16, generator=g); adv[::5] = 0.0
    with torch.no_grad():
        lp0, _ = pol.evaluate_at(buf.states, buf.actions, buf.rows, index)
    old = lp0 - torch.log(torch.tensor(np.resize(np.array(pp.PLACED), 16), dtype=torch.float32))
    ent_coef = 2.0 ** -7
    logp, ent = pol.evaluate_at(buf.states, buf.actions, buf.rows, index)
    loss, u = _torch_loss(mode, logp, ent, old, adv, 0.2, ent_coef, 0.3)
    want = torch.autograd.grad(loss, list(pol.parameters()))
    pol.zero_grad(set_to_none=True)
    stats, lp, en = pol.ppo_step_at(buf.states, buf.actions, buf.rows, index, old, adv, clip=0.2, ent_coef=ent_coef, mode=mode, c_kl=0.3)
    assert torch.equal(lp, logp.detach()) and torch.equal(en, ent.detach()) and not lp.requires_grad
    got = [q.grad for q in pol.parameters()]
    assert all(a is not None and torch.equal(a, b) for a, b in zip(got, want))
    assert any(float(a.abs().max()) > 0 for a in got)
    assert stats.dtype == torch.float64 and stats.shape == (6,)
    ratio = torch.exp(logp.detach() - old)
    clipped = (ratio * adv > torch.clamp(ratio, 0.8, 1.2) * adv).sum() if mode == "clip" else 0
    want_stats = [16.0, float(u.detach().double().sum()), float(ent.detach().double().sum()), float((old - logp.detach()).double().sum()), float(clipped), 0.0]
    assert np.allclose(stats.numpy(), want_stats, rtol=0, atol=1e-12)
    # a second call ADDS to .grad, as backward() would
    pol.ppo_step_at(buf.states, buf.actions, buf.rows, index, old, adv, clip=0.2, ent_coef=ent_coef, mode=mode, c_kl=0.3)
    assert all(torch.equal(q.grad, 2 * b) for q, b in zip(pol.parameters(), want))


def test_ppo_step_on_cpu_tensors_and_positions_that_do_not_count():
    buf = _buffer()
    pol = pc.to_policy(pc.make_weights(COLS, (16,), 8))
    index = torch.arange(T * B, dtype=torch.int32)
    with torch.no_grad():
        lp0, _ = pol.evaluate_at(buf.states, buf.actions, buf.rows, index)
    bad = torch.isnan(lp0)
    assert bad.any() and (~bad).any()                                  # actions outside the live rows among them
    old = torch.where(bad, torch.zeros_like(lp0), lp0) + 0.1
    adv = torch.linspace(-1, 1, T * B)
    stats, lp, en = pol.ppo_step_at(buf.states, buf.actions, buf.rows, index, old, adv)
    assert stats[0] == (~bad).sum() and stats[5] == bad.sum() and torch.isfinite(stats).all()
    got = [q.grad.clone() for q in pol.parameters()]
    assert all(torch.isfinite(x).all() for x in got)
    # the gathered form on the same states: the same numbers
    pol.zero_grad(set_to_none=True)
    j = index.long()
    st2, lp2, en2 = pol.ppo_step(buf.states.view(-1, R, COLS)[j], buf.actions.view(-1)[j], buf.rows.view(-1)[j], old, adv)
    assert torch.equal(stats, st2) and torch.equal(torch.nan_to_num(lp), torch.nan_to_num(lp2))
    assert all(torch.equal(q.grad, x) for q, x in zip(pol.parameters(), got))
    with pytest.raises(KeyError):
        pol.ppo_step_at(buf.states, buf.actions, buf.rows, index, old, adv, mode="nonsense")


# ---- ppo_update --------------------------------------------------------------------------------------------------------------
def _spy(pol):
    seen = []
    inner = pol.ppo_step_at

    def step(states, actions, rows, index, old, adv, **kw):
        seen.append((index.clone(), old.clone(), adv.clone()))
        return inner(states, actions, rows, index, old, adv, **kw)
    pol.ppo_step_at = step
    return seen


def test_ppo_update_covers_the_index_list_once_per_epoch_and_respects_epochs():
    from deepgroebner_amd.rollout import ppo_update
    buf = _buffer()
    pol = pc.to_policy(pc.make_weights(COLS, (16,), 9))
    opt = torch.optim.SGD(pol.parameters(), lr=0.01)
    idx, _, old, adv, _ = buf.get_index()
    n = int(idx.numel())
    assert n > 6
    seen = _spy(pol)
    before = [q.detach().clone() for q in pol.parameters()]
    g = torch.Generator().manual_seed(5)
    out = ppo_update(pol, buf, opt, epochs=3, batch_size=4, ent_coef=0.01, generator=g)
    per_epoch = (n + 3) // 4
    assert len(out) == 3 and len(seen) == 3 * per_epoch
    orders = []
    for e in range(3):
        calls = seen[e * per_epoch:(e + 1) * per_epoch]
        assert [c[0].numel() for c in calls] == [4] * (n // 4) + ([n % 4] if n % 4 else [])
        ci, co, ca = (torch.cat([c[k] for c in calls]) for k in range(3))
        assert torch.equal(torch.sort(ci).values, torch.sort(idx).values)           # every step once
        where = torch.tensor([int(np.flatnonzero(idx.numpy() == v)[0]) for v in ci.numpy()])
        assert torch.equal(co, old[where]) and torch.equal(ca, adv[where])           # with ITS log-probability and advantage
        orders.append(ci)
        st = out[e]["stats"]
        assert st.shape == (per_epoch, 6) and st[:, 0].sum() + st[:, 5].sum() == n and np.isfinite(st).all()
        assert np.isfinite([out[e][k] for k in ("loss", "entropy", "kl", "clip_frac")]).all()
    assert not torch.equal(orders[0], orders[1]) or not torch.equal(orders[1], orders[2])      # a new permutation per epoch
    assert any(not torch.equal(a, b) for a, b in zip(before, pol.parameters()))
    assert all(q.grad is None or float(q.grad.abs().max()) == 0 for q in pol.parameters())     # zero_grad after the last step
    # shuffle=False: the list in get_index's order
    seen.clear()
    ppo_update(pol, buf, opt, epochs=1, batch_size=100, shuffle=False)
    assert len(seen) == 1 and torch.equal(seen[0][0], idx)


def test_ppo_update_stops_on_the_kl_limit():
    from deepgroebner_amd.rollout import ppo_update
    buf = _buffer()
    pol = pc.to_policy(pc.make_weights(COLS, (16,), 9))
    opt = torch.optim.SGD(pol.parameters(), lr=0.0)
    # the buffer's recorded log-probabilities are random numbers: mean old - new is what it is, and no step changes it (lr = 0)
    first = ppo_update(pol, buf, opt, epochs=1, batch_size=8, shuffle=False)[0]["kl"]
    assert np.isfinite(first)
    out = ppo_update(pol, buf, opt, epochs=4, batch_size=8, kld_limit=first - 0.5)
    assert len(out) == 1                                               # stopped after the first epoch
    out = ppo_update(pol, buf, opt, epochs=4, batch_size=8, kld_limit=first + 0.5)
    assert len(out) == 4 and all(abs(o["kl"] - first) < 1e-4 for o in out)      # (shuffled minibatches: float32 rounding apart)
