"""The PMLP critic — bbx_pmlp_value, bbx_pmlp_value_grad, bbx_pmlp_value_fit, PMLPValue — against float64: the pooled value of a
state's row scores and the gradient of
    L = sum_s gvalue[s] V_s
with respect to W1 [cols][hidden], b1 [hidden], w2 [hidden], b2 [1].  Plain numpy on top of tests/policy_cases.py, importable
without a GPU (tests/test_value_model_cpu.py checks the reference against torch autograd in double precision).

Conventions (include/bbx.h): the row count masks; a state without live rows is worth 0.0 and has no gradient; a state with ONE
live row contributes like any other.

What the kernels are held to, per state with n live rows, S_r the per-row scale of policy_cases (the network evaluated with |W|,
|b|, |x|), EPS = 2^-24:
    sum    |V - ref| <= EPS (C_V + 8 + n / 64) sum_r S_r      the logit error per row (C_V: policy_cases.C_L = 64 until measured, 4 since: below), plus
                                                              an fp32 sum of n terms over 64 lanes and a six-level tree
    mean   that bound / n + EPS |ref|                         (one more rounding: the division)
    lse    Ref.tol()                                          the log-partition is held to this inside the log-probability bound
    |g - g_ref| <= C_VG EPS sum_s K_s A_theta,s               A_theta,s as in policy_grad_cases with |g_r| = |gvalue_s| dV/dz_r;
                                                              K_s = 1 for sum and mean (the coefficient carries at most one
                                                              rounding), policy_grad_cases.state_scale for lse (a probability
                                                              inherits the logit's error)."""
import numpy as np

from tests import policy_cases as pc
from tests import policy_grad_cases as gc

EPS = pc.EPS
POOLS = ("sum", "mean", "lse")
POOL_ID = {"sum": 0, "mean": 1, "lse": 2}                         # BBX_POOL_*
# Measured on an MI355X over every case of tests/test_value_model_gpu.py (each prints the ratio it needed: pytest -s): R_V, the
# largest |V - ref| of the sum and mean pools in units of EPS sum_r S_r (mean: of EPS (sum_r S_r / n + |ref|)) — the whole error
# charged to the constant, nothing to the 8 + n / 64 of the summation — and R_VG, the largest |g - g_ref| in units of
# EPS sum_s K_s A_theta,s.  A constant is lowered from policy_cases' 64, for the value bounds only, where the next power of two at
# or above 4 x the measured ratio is below 64; a ratio above 64 is a finding about the kernel, not a constant.
# R_V = 0.961 (21x1, sum, the nine-state row sweep; mean at most 0.631) -> 4 R_V = 3.84 -> C_V = 4.  (The lse pool is held to
# Ref.tol() with policy_cases' own C_L; it needed 2.318 of that bound's unit.)
# R_VG = 28.161 (64x256, mean, N = 5; sum 27.170; with K_s = 1 the unit is the bare sum of absolute terms, and an entry of dW1 adds
# up to 165 rows of 64-term dots in fp32; lse at most 2.905; 1030 four-row states at most 7.306) -> 4 R_VG = 112.6: C_VG stays 64.
R_V, R_VG = 0.961, 28.161
C_V, C_VG = 4.0, gc.C_G

LIVE_ROWS = (1, 2, 31, 32, 33, 63, 64, 65, 129)
TALL_ROWS = (2047, 2048)
BATCHES = (1, 5, 9)


def to_critic(weights, pool, device="cpu", dtype=None):
    """A PMLPValue holding `weights` (policy_cases' layout)."""
    import torch
    from deepgroebner_amd.rollout import PMLPValue
    cr = PMLPValue(weights[0][0].shape[0], [W.shape[1] for W, _ in weights[:-1]], pool=pool)
    with torch.no_grad():
        for lin, (W, b) in zip(cr.embedding, weights[:-1]):
            lin.weight.copy_(torch.from_numpy(np.ascontiguousarray(W.T))); lin.bias.copy_(torch.from_numpy(b))
        cr.head.weight.copy_(torch.from_numpy(weights[-1][0].reshape(1, -1))); cr.head.bias.copy_(torch.from_numpy(weights[-1][1].reshape(1)))
    if dtype is not None:
        cr = cr.to(dtype)
    return cr.to(device)


def _live(ref):
    return np.arange(ref.logits.shape[1])[None, :] < ref.n[:, None]


def reference_values(weights, obs, rows, pool, ref=None):
    """float64 values [N] (0.0 where a state has no live row) and the policy_cases.Ref they come from."""
    if ref is None:
        ref = pc.reference(weights, obs, rows)
    live = _live(ref)
    z = np.where(live, ref.logits, 0.0)
    if pool == "lse":
        v = ref.logz
    else:
        v = z.sum(axis=1)
        if pool == "mean":
            v = v / np.maximum(ref.n, 1)
    return np.where(ref.n > 0, v, 0.0), ref


def value_tol(ref, pool, vref, c_v=None):
    """The bound on |V - ref| per state (module docstring)."""
    if pool == "lse":
        return ref.tol()
    c = C_V if c_v is None else c_v
    ssum = np.where(_live(ref), ref.scale, 0.0).sum(axis=1)
    b = EPS * (c + 8.0 + ref.n / 64.0) * ssum
    if pool == "mean":
        b = b / np.maximum(ref.n, 1) + EPS * np.abs(vref)
    return b


def value_ratio(ref, pool, got, vref):
    """The largest |got - ref| in units of the bound with the constant's term set to 1: EPS sum_r S_r for sum, EPS (sum_r S_r / n +
    |ref|) for mean, Ref.tol(1) for lse (states without rows must be exact: inf otherwise)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - vref)
    if pool == "lse":
        unit = ref.tol(1.0)
    else:
        unit = EPS * np.where(_live(ref), ref.scale, 0.0).sum(axis=1)
        if pool == "mean":
            unit = unit / np.maximum(ref.n, 1) + EPS * np.abs(vref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(unit > 0, err / unit, np.where(err > 0, np.inf, 0.0))
    return float(r.max(initial=0.0))


def grad_scale(ref, pool):
    """K_s"""
    return gc.state_scale(ref) if pool == "lse" else np.ones(len(ref.n))


def reference_grad(weights, obs, rows, gvalue, pool, ref=None):
    """float64 gradients (gW1 [cols][hidden], gb1 [hidden], gw2 [hidden], gb2 [1]) of L for a ONE-hidden-layer critic, and the
    absolute contributions summed with their scales, A = sum_s K_s A_theta,s, in the gradients' shapes (what
    policy_grad_cases.grad_ratio / check_grads take with ref=None).  A state without live rows contributes nothing, whatever
    its gvalue."""
    assert len(weights) == 2, "one hidden layer"
    obs = np.asarray(obs)
    if ref is None:
        ref = pc.reference(weights, obs, rows)
    N, R, cols = obs.shape
    W1 = weights[0][0].astype(np.float64); b1 = weights[0][1].astype(np.float64); w2 = weights[1][0].astype(np.float64)
    hidden = W1.shape[1]
    gvalue = np.asarray(gvalue, dtype=np.float64)
    K = grad_scale(ref, pool)
    g = [np.zeros((cols, hidden)), np.zeros(hidden), np.zeros(hidden), np.zeros(1)]
    A = [np.zeros((cols, hidden)), np.zeros(hidden), np.zeros(hidden), np.zeros(1)]
    for s in range(N):
        n = int(ref.n[s])
        if n <= 0:
            continue
        x = obs[s, :n].astype(np.float64)
        if pool == "sum":
            c = np.ones(n)
        elif pool == "mean":
            c = np.full(n, 1.0 / n)
        else:
            c = np.exp(ref.logsm[s, :n])
        gr = gvalue[s] * c
        ga = np.abs(gr)
        h = x @ W1 + b1
        act = np.maximum(h, 0.0); on = (h > 0).astype(np.float64)
        dh = gr[:, None] * w2[None, :] * on
        g[0] += x.T @ dh; g[1] += dh.sum(axis=0); g[2] += gr @ act; g[3] += gr.sum()
        dha = ga[:, None] * np.abs(w2)[None, :] * on
        for i, a in enumerate((np.abs(x).T @ dha, dha.sum(axis=0), ga @ act, np.array([ga.sum()]))):
            A[i] += K[s] * a
    return tuple(g), tuple(A)


def fit_recipe(values, targets, scale):
    """The fit epilogue in float32 numpy, in the kernels' order: (coef, u = d^2, counted) — a NaN value is not counted."""
    v = np.asarray(values, dtype=np.float32); t = np.asarray(targets, dtype=np.float32)
    counted = ~np.isnan(v)
    d = (np.where(counted, v, np.float32(0)) - t).astype(np.float32)
    u = (d * d).astype(np.float32)
    coef = (np.float32(scale) * d).astype(np.float32)
    zero = np.float32(0)
    return np.where(counted, coef, zero), np.where(counted, u, zero), counted


def fit_stats(values, targets, scale):
    """double [6] as bbx_pmlp_value_fit defines them, summed by numpy in double over the float32 terms."""
    _, u, counted = fit_recipe(values, targets, scale)
    v = np.asarray(values, dtype=np.float32)[counted].astype(np.float64)
    t32 = np.asarray(targets, dtype=np.float32)[counted]
    tt = (t32 * t32).astype(np.float32).astype(np.float64)
    return np.array([counted.sum(), u[counted].astype(np.float64).sum(), v.sum(), t32.astype(np.float64).sum(), tt.sum(), (~counted).sum()],
                    dtype=np.float64)


# ---- seeded case builders: small exponents (entries 0..3), so that the row scores stay of order one
def value_case(cols, hidden, rows, R, seed, garbage=True, emax=3):
    """(weights, obs int32 [N, R, cols], rows int32 [N]): one state per entry of `rows` (which may exceed R, be 0 or negative)."""
    w = pc.make_weights(cols, hidden, seed)
    rows = np.array(rows, dtype=np.int32)
    obs = pc.fill_padding(pc.random_blocks(len(rows), R, cols, seed + 1, emax=emax), rows, garbage, seed + 2)
    return w, obs, rows


def grad_case(cols, hidden, rows, R, seed, garbage=True, emax=3):
    """value_case plus gvalue float32 [N] of both signs."""
    w, obs, rows = value_case(cols, hidden, rows, R, seed, garbage, emax)
    gvalue = np.random.default_rng(seed + 3).normal(size=len(rows)).astype(np.float32)
    return w, obs, rows, gvalue
