"""Cross-entropy training of the PMLP policy against per-row target distributions — bbx_pmlp[2]_xent[_at], bbx_pmlp[2]_xent_grad[_at],
PMLPPolicy.xent_step[_at], imitation_update — against float64.  Plain numpy on top of tests/policy_cases.py, tests/policy_grad_cases.py
and tests/policy2_grad_cases.py, importable without a GPU (tests/test_xent_cpu.py checks the reference against torch autograd in
double precision, and the conditions the GPU cases rest on).

Per position k of a call, about recorded state s with n live rows, logits z_r, p = softmax(z), target row t_r = targets[s][r] (r < n),
weight w_k (None: 1):
    T = sum_r t_r      l = -sum_r t_r log p_r      H = -sum_r p_r log p_r      c = scale w_k      g_r = c (T p_r - t_r) = dL/dz_r
of L = scale sum_k w_k l_k.  Not counted (l = NaN, c = 0, in no sum and no gradient): an index out of range, a live t_r that is
negative or not finite, a w_k that is not finite.  What lies beyond the live rows is never read.  No live row: counted, l = H = 0.
stats = counted positions, sum w l, sum w T, sum H, sum w, positions not counted.

What the kernels are held to, K_s = max_r S_r + |logZ_s| + 1 (policy_grad_cases.state_scale):
    |l - l64|  <= C_X 2^-24 K_s T (1 + log max(n, 1))
    |H - H64|  <= the depth's entropy_tol
    |g - g64|  <= C_G 2^-24 sum_k K_s A_theta,k   (the depth's grad_bounds and constant), A as in reference_grad with |g_r| taken as
                  |c_k| (T p_r + t_r)
    stats[0], stats[5] exact; stats[1..4] within the sums of their terms' bounds:
        w l: |w| bound(l) + 2^-24 |w l|         (one float32 product)
        w T: |w| bound(T) + 2^-24 |w T|,  bound(T) = (ceil(n / 64) + 7) 2^-24 T: a lane adds at most ceil(n / 64) of the non-negative
             float32 targets, the wave sum is six more additions, every partial sum is at most T, one rounding each, one to spare
        H: entropy_tol        w: exact to 2^-40 (a double sum of float32 numbers)

C_X: R_X is the largest |l - l64| in units of 2^-24 K_s T (1 + log max(n, 1)) over every case of tests/test_xent_gpu.py that prints it
(pytest -s); C_X is the next power of two at or above 4 R_X (the rule of policy_grad_cases.py and ppo_cases.py); 64 (policy_cases.C_CEILING)
is the ceiling: a ratio above it is a finding about the kernel, not a constant.  R_GX1 / R_GX2: the gradient ratios of the same cases in
units of the depth's bound at constant 1, held against the existing C_G = 64 and C_G2 = 16."""
import numpy as np

from tests import policy_cases as pc
from tests import policy_grad_cases as gc
from tests import policy2_grad_cases as g2

EPS = pc.EPS
# Measured on an MI355X over the 34 calls of tests/test_xent_gpu.py that print their ratios, against the float64 reference with the
# constant at the ceiling (64): R_X = 0.355 (12x128, the partition case n = 4100; the five shapes of the float64 cases: 0.064 .. 0.282)
# -> 4 R_X = 1.42 -> C_X = 2.
# The gradients: R_GX1 = 3.360 (40x256, the indexed call with weights) against C_G = 64; R_GX2 = 4.306 (33x40x100, the indexed call
# with weights; 12x128x128: 0.297) against C_G2 = 16 — inside the existing constant with a margin of 3.7 where the rule asks 4 of a new
# one; the constant is policy2_grad_cases', and stays.
R_X = 0.355
C_X = 2.0
R_GX1, R_GX2 = 3.360, 4.306

OBS_ROWS = 80
SHAPES_ONE = [(12, (128,)), (5, (20,)), (40, (256,))]
SHAPES_TWO = [(12, (128, 128)), (33, (40, 100))]
# the recorded states of a case: live rows around the tiles of 16 / 32 / 64, none, one, more than obs_rows (clamped)
SRC_ROWS = (0, 1, 2, 31, 32, 33, 64, 65, 80, 200, 17, 48)
N_SRC = len(SRC_ROWS)
# what each state's target row is
KINDS = ("soft", "soft", "soft", "unnormalised", "onehot", "zero", "negative", "nan", "soft", "onehot", "soft", "unnormalised")
HEALTHY = (2, 3, 4, 8, 9, 10, 11)             # counted, n >= 2, T > 0
N_POS = 42


def f32(x):
    return np.float32(x)


def targets_for(rows, obs_rows, kinds, seed):
    """float32 [len(rows)][obs_rows]: the rows' kinds over the live entries, NaN beyond them (never read)."""
    rng = np.random.default_rng(seed)
    out = np.full((len(rows), obs_rows), np.nan, dtype=np.float32)
    for s, (r, kind) in enumerate(zip(rows, kinds)):
        n = int(np.clip(r, 0, obs_rows))
        if n == 0:
            continue
        t = rng.uniform(0.05, 1.0, size=n)
        if kind == "soft":
            t = t / t.sum()
        elif kind == "unnormalised":
            t = 3.5 * t / t.sum()
        elif kind == "onehot":
            a = int(rng.integers(0, n)); t = np.zeros(n); t[a] = 1.0
        elif kind == "zero":
            t = np.zeros(n)
        elif kind == "negative":
            t = t / t.sum(); t[n // 2] = -0.25
        elif kind == "nan":
            t = t / t.sum(); t[n - 1] = np.nan
        out[s, :n] = t.astype(np.float32)
    return out


_sources = {}


def source(cols, hidden, obs_rows=OBS_ROWS, rows=SRC_ROWS, kinds=KINDS, seed=900):
    """(weights, obs, rows, targets) of a case's recorded states: garbage beyond the live rows of the blocks, NaN beyond those of the
    targets (read-only, shared between tests)."""
    key = (cols, tuple(hidden), obs_rows, tuple(rows), tuple(kinds), seed)
    if key not in _sources:
        w = pc.make_weights(cols, hidden, seed)
        r = np.array(rows, dtype=np.int32)
        obs = pc.fill_padding(pc.random_blocks(len(r), obs_rows, cols, seed + 1), r, True, seed + 2)
        t = targets_for(r, obs_rows, kinds, seed + 3)
        for a in (obs, r, t):
            a.setflags(write=False)
        _sources[key] = (w, obs, r, t)
    return _sources[key]


def index_of(n_pos=N_POS, n_src=N_SRC, healthy=HEALTHY, bad=True, seed=0):
    """n_pos positions over the recorded states: every state once, the rest repeats of the healthy ones, and (bad) one -1 and one n_src."""
    rng = np.random.default_rng(910 + seed)
    idx = list(range(n_src))
    idx += [int(x) for x in rng.choice(np.array(healthy), size=n_pos - n_src - (2 if bad else 0))]
    idx = [int(x) for x in rng.permutation(np.array(idx))]
    if bad:
        idx.insert(5, -1); idx.insert(n_pos // 2, n_src)
    return np.array(idx, dtype=np.int32)


def weights_for(index, healthy=HEALTHY, seed=0):
    """float32 [n]: positive weights, one 0 and one negative among the healthy positions."""
    rng = np.random.default_rng(920 + seed)
    w = rng.uniform(0.5, 1.5, size=len(index)).astype(np.float32)
    good = [k for k, s in enumerate(index) if s in healthy]
    if len(good) > 4:
        w[good[1]] = 0.0; w[good[3]] = -0.75
    return w


def _backprop(weights, x, grow, absolute):
    """The gradient terms of one state from its row coefficients (policy_grad_cases.reference_grad / policy2_grad_cases.reference_grad2,
    whose formulae these are); absolute: |x|, |W2|, |w| with the relu masks and activations kept."""
    f = lambda t: np.asarray(t, dtype=np.float64)
    m = np.abs if absolute else (lambda t: t)
    if len(weights) == 2:
        W1, b1, w2 = f(weights[0][0]), f(weights[0][1]), f(weights[1][0])
        h = x @ W1 + b1
        act = np.maximum(h, 0.0); on = (h > 0).astype(np.float64)
        dh = grow[:, None] * m(w2)[None, :] * on
        return (m(x).T @ dh, dh.sum(axis=0), grow @ act, np.array([grow.sum()]))
    W1, b1, W2, b2, w3 = f(weights[0][0]), f(weights[0][1]), f(weights[1][0]), f(weights[1][1]), f(weights[2][0])
    z1 = x @ W1 + b1; a1 = np.maximum(z1, 0.0); on1 = (z1 > 0).astype(np.float64)
    z2 = a1 @ W2 + b2; a2 = np.maximum(z2, 0.0); on2 = (z2 > 0).astype(np.float64)
    dz2 = grow[:, None] * m(w3)[None, :] * on2
    dz1 = (dz2 @ m(W2).T) * on1
    return (m(x).T @ dz1, dz1.sum(axis=0), a1.T @ dz2, dz2.sum(axis=0), grow @ a2, np.array([grow.sum()]))


class XRef:
    """reference()'s result, per position: l (NaN: not counted), H (NaN: index out of range), T, counted, c, n; stats [6]; grads and A
    (A: per position, leading axis [n]); ref: the policy_cases.Ref of the positions (an index out of range: state 0, unused)."""


def reference(weights, obs, rows, targets, index=None, w=None, scale=None):
    obs = np.asarray(obs); rows = np.asarray(rows)
    n_src = len(rows)
    index = np.arange(n_src) if index is None else np.asarray(index).astype(np.int64)
    N = len(index)
    inside = (index >= 0) & (index < n_src)
    j = np.where(inside, index, 0)
    scale = float(f32(1.0 / N if N else 0.0)) if scale is None else float(f32(scale))
    wk = np.ones(N) if w is None else np.asarray(w, dtype=np.float64)
    ref = pc.reference(weights, obs[j], rows[j]) if n_src else None
    out = XRef()
    out.ref, out.n = ref, (np.where(inside, ref.n, 0) if n_src else np.zeros(N, dtype=np.int64))
    out.l = np.full(N, np.nan); out.H = np.full(N, np.nan); out.T = np.zeros(N); out.c = np.zeros(N)
    out.counted = np.zeros(N, dtype=bool)
    grads = A = None
    for k in range(N):
        if not inside[k]:
            continue
        n = int(ref.n[k])
        t = np.asarray(targets[j[k], :n], dtype=np.float64)
        logp = ref.logsm[k, :n]; p = np.exp(logp)
        out.H[k] = -(p * logp).sum()
        bad = bool(((t < 0) | ~np.isfinite(t)).any())
        if bad or not np.isfinite(wk[k]):
            continue
        out.counted[k] = True
        out.T[k] = t.sum(); out.l[k] = -(t * logp).sum(); out.c[k] = scale * wk[k]
        if n == 0:
            continue
        x = obs[j[k], :n].astype(np.float64)
        gr = out.c[k] * (out.T[k] * p - t)
        ga = abs(out.c[k]) * (out.T[k] * p + t)
        gs, As = _backprop(weights, x, gr, False), _backprop(weights, x, ga, True)
        if grads is None:
            grads = [np.zeros_like(g) for g in gs]; A = [np.zeros((N,) + g.shape) for g in gs]
        for i in range(len(gs)):
            grads[i] += gs[i]; A[i][k] = As[i]
    if grads is None:
        shapes = _grad_shapes(weights, obs.shape[2])
        grads = [np.zeros(s) for s in shapes]; A = [np.zeros((N,) + s) for s in shapes]
    out.grads, out.A = tuple(grads), tuple(A)
    cn = out.counted
    z = lambda x: np.where(cn, x, 0.0)
    out.w = z(wk)
    out.stats = np.array([cn.sum(), (out.w * z(out.l)).sum(), (out.w * out.T).sum(), z(out.H).sum(), out.w.sum(), (~cn).sum()], dtype=np.float64)
    return out


def _grad_shapes(weights, cols):
    h = [W.shape[1] for W, _ in weights[:-1]]
    return ((cols, h[0]), (h[0],), (h[0],), (1,)) if len(h) == 1 else ((cols, h[0]), (h[0],), (h[0], h[1]), (h[1],), (h[1],), (1,))


def state_scale(xr):
    return gc.state_scale(xr.ref)


def loss_unit(xr):
    """2^-24 K_s T (1 + log max(n, 1)) per position (0 where the position is not counted)."""
    return np.where(xr.counted, EPS * state_scale(xr) * xr.T * (1.0 + np.log(np.maximum(xr.n, 1))), 0.0)


def loss_tol(xr, c_x=None):
    return (C_X if c_x is None else c_x) * loss_unit(xr)


def entropy_tol(xr, depth):
    return gc.entropy_tol(xr.ref) if depth == 1 else g2.entropy_tol(xr.ref)


def total_tol(xr):
    return np.where(xr.counted, (np.ceil(xr.n / 64.0) + 7.0) * EPS * xr.T, 0.0)


def stats_tol(xr, depth, c_x=None):
    """The bounds of stats[1..4]."""
    w = np.abs(xr.w)
    l = np.where(xr.counted, xr.l, 0.0)
    b1 = (w * loss_tol(xr, c_x) + EPS * w * np.abs(l)).sum()
    b2 = (w * total_tol(xr) + EPS * w * xr.T).sum()
    b3 = np.where(xr.counted, entropy_tol(xr, depth), 0.0).sum()
    b4 = 2.0 ** -40 * w.sum()
    return b1, b2, b3, b4


def grad_bounds(xr, depth, c_g=None):
    c = (gc.C_G if depth == 1 else g2.C_G2) if c_g is None else c_g
    return gc.grad_bounds(xr.A, xr.ref, c)


def loss_ratio(xr, losses):
    """The largest |l - l64| in units of loss_unit (a position whose unit is 0 must be exact: inf otherwise)."""
    err = np.abs(np.where(xr.counted, np.asarray(losses, dtype=np.float64) - np.where(xr.counted, xr.l, 0.0), 0.0))
    unit = loss_unit(xr)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(unit > 0, err / unit, np.where(err > 0, np.inf, 0.0))
    return float(q.max(initial=0.0))


def grad_ratio(xr, got):
    return gc.grad_ratio(got, xr.grads, xr.A, xr.ref)


def check_grads(xr, got, depth, what=""):
    names = ("dW1", "db1", "dw2", "db2") if depth == 1 else g2.NAMES
    for name, x, y, b in zip(names, got, xr.grads, grad_bounds(xr, depth)):
        x = np.asarray(x, dtype=np.float64).reshape(b.shape)
        assert np.isfinite(x).all(), (what, name, "not finite")
        bad = np.abs(x - y) > b
        assert not bad.any(), (what, name, "entries off (index, got, want, bound)",
                               [(int(i), float(x.reshape(-1)[i]), float(y.reshape(-1)[i]), float(b.reshape(-1)[i])) for i in np.flatnonzero(bad)[:5]],
                               int(bad.sum()))


def healthy_fraction(xr):
    """The share of positions that are counted and have n >= 2 and T > 0."""
    return float((xr.counted & (xr.n >= 2) & (xr.T > 0)).mean()) if len(xr.n) else 1.0


# ---- the partition boundaries: small blocks, every state healthy
def partition_case(cols, hidden, obs_rows, n, seed=930):
    """n recorded states of obs_rows rows, live rows 2 .. obs_rows, soft and unnormalised targets."""
    w = pc.make_weights(cols, hidden, seed)
    rows = (2 + np.arange(n) % (obs_rows - 1)).astype(np.int32)
    obs = pc.fill_padding(pc.random_blocks(n, obs_rows, cols, seed + 1), rows, True, seed + 2)
    kinds = np.resize(np.array(("soft", "unnormalised", "onehot", "soft")), n)
    return w, obs, rows, targets_for(rows, obs_rows, kinds, seed + 3)


def torch_loss(policy, obs, rows, targets, w, scale):
    """L = scale sum_k w_k (-(t * log_softmax(z)).sum()) over the counted positions with torch ops in the policy's dtype: what
    autograd differentiates in tests/test_xent_cpu.py.  obs, rows, targets: gathered, one per position."""
    import torch
    R = obs.shape[1]
    n = torch.clamp(torch.as_tensor(np.asarray(rows).astype(np.int64)), 0, R)
    live = torch.arange(R)[None, :] < n[:, None]
    z = policy._logits(torch.as_tensor(np.asarray(obs)))
    lp = torch.log_softmax(torch.where(live, z, torch.full_like(z, -1e9)), dim=-1)
    t = torch.where(live, torch.as_tensor(np.asarray(targets)).to(z.dtype), torch.zeros_like(z))
    l = -(t * torch.where(live, lp, torch.zeros_like(lp))).sum(dim=1)
    return scale * (torch.as_tensor(np.asarray(w)).to(z.dtype) * l).sum()
