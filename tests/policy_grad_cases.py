"""The training side of the one-hidden-layer PMLP policy — bbx_pmlp_logprob, bbx_pmlp_grad, PMLPPolicy.evaluate — against
float64: the log-probability of a recorded action, the entropy over a state's rows, and the gradient of
    L = sum_s glogp[s] logprob_s + gent[s] entropy_s
with respect to W1 [cols][hidden], b1 [hidden], w2 [hidden], b2 [1].  Plain numpy on top of tests/policy_cases.py, importable
without a GPU (tests/test_policy_grad_cpu.py checks the reference against torch autograd in double precision).

Conventions (include/bbx.h): the row count masks; a state without live rows has logprob 0.0 and entropy 0.0 and no gradient;
an action outside the live rows gives logprob NaN (entropy still computed) and no gradient.

What the kernels are held to, per state with n live rows, K_s = max_r S_r + |logZ_s| + 1 (policy_cases' logit-error scale):
    |logprob - ref|  <= Ref.tol()                                     (policy_cases: the existing bound and constant)
    |entropy - ref|  <= C_H 2^-24 K_s (1 + log n)
    |g - g_ref|      <= C_G 2^-24 sum_s K_s A_theta,s                 for every gradient entry theta
A_theta,s: the state's contribution to the entry with every term replaced by its absolute value — |g_r| taken as
|glogp| (delta_{r,a} + p_r) + |gent| p_r (|log p_r| + H), times |dz_r / dtheta| evaluated with |x|, |w2| and relu(h).  (A probability
inherits the logit's error, hence K_s; the sums over rows and states are what fp32 accumulation errors are proportional to.)"""
import numpy as np

from tests import policy_cases as pc

EPS = pc.EPS
# Measured on an MI355X over every case of tests/test_policy_grad_gpu.py (each prints the ratio it needed: pytest -s):
# R_H, the largest |entropy - ref| in units of 2^-24 K_s (1 + log n), and R_G, the largest |g - g_ref| in units of
# 2^-24 sum_s K_s A_theta,s.  Each constant is then the next power of two at or above 4 x the measured ratio; 64 (policy_cases'
# ceiling) is where they stood before, and a ratio above it is a finding about the kernel, not a constant.
# Measured on an MI355X: R_H = 0.407 (21x1 and 64x1, the row sweeps), R_G = 9.626 (64x256, N = 5, gent = NULL: without the entropy
# term A is at its smallest; with it the largest ratio is 2.434) -> 4 R_H = 1.63 -> C_H = 2; 4 R_G = 38.5 -> C_G = 64.
R_H, R_G = 0.407, 9.626
C_H, C_G = 2.0, 64.0


def entropy_tol(ref, c_h=None):
    return (C_H if c_h is None else c_h) * EPS * (ref.smax() + np.abs(ref.logz) + 1.0) * (1.0 + np.log(np.maximum(ref.n, 1)))


def state_scale(ref):
    """K_s"""
    return ref.smax() + np.abs(ref.logz) + 1.0


def reference_eval(weights, obs, rows, actions, ref=None):
    """float64 (logprob [N], entropy [N], the policy_cases.Ref they come from)."""
    if ref is None:
        ref = pc.reference(weights, obs, rows)
    a = np.asarray(actions).astype(np.int64)
    N = len(ref.n)
    ok = (a >= 0) & (a < ref.n)
    lp = ref.logsm[np.arange(N), np.where(ok, a, 0)] if ref.logsm.shape[1] else np.zeros(N)
    logprob = np.where(ref.n > 0, np.where(ok, lp, np.nan), 0.0)
    live = np.arange(ref.logsm.shape[1])[None, :] < ref.n[:, None]
    l = np.where(live, ref.logsm, 0.0)
    entropy = -(np.where(live, np.exp(l), 0.0) * l).sum(axis=1)
    return logprob, entropy, ref


def reference_grad(weights, obs, rows, actions, glogp, gent=None, scale=None, ref=None):
    """float64 gradients (gW1 [cols][hidden], gb1 [hidden], gw2 [hidden], gb2 [1]) of L for a ONE-hidden-layer policy, and the
    absolute contributions A = (A_W1 [N][cols][hidden], A_b1 [N][hidden], A_w2 [N][hidden], A_b2 [N][1]) per state.
    scale [N] (K_s) given: A is returned summed, sum_s scale_s A_theta,s, in the gradients' shapes (large N)."""
    assert len(weights) == 2, "one hidden layer"
    obs = np.asarray(obs); a = np.asarray(actions).astype(np.int64)
    if ref is None:
        ref = pc.reference(weights, obs, rows)
    N, R, cols = obs.shape
    W1 = weights[0][0].astype(np.float64); b1 = weights[0][1].astype(np.float64); w2 = weights[1][0].astype(np.float64)
    hidden = W1.shape[1]
    glogp = np.asarray(glogp, dtype=np.float64)
    gent = np.zeros(N) if gent is None else np.asarray(gent, dtype=np.float64)
    g = [np.zeros((cols, hidden)), np.zeros(hidden), np.zeros(hidden), np.zeros(1)]
    if scale is None:
        A = [np.zeros((N, cols, hidden)), np.zeros((N, hidden)), np.zeros((N, hidden)), np.zeros((N, 1))]
    else:
        A = [np.zeros((cols, hidden)), np.zeros(hidden), np.zeros(hidden), np.zeros(1)]
    for s in range(N):
        n = int(ref.n[s])
        if n <= 0 or a[s] < 0 or a[s] >= n:
            continue
        x = obs[s, :n].astype(np.float64)
        logp = ref.logsm[s, :n]; p = np.exp(logp)
        H = -(p * logp).sum()
        delta = np.zeros(n); delta[a[s]] = 1.0
        gr = glogp[s] * (delta - p) - gent[s] * p * (logp + H)
        ga = np.abs(glogp[s]) * (delta + p) + np.abs(gent[s]) * p * (np.abs(logp) + H)
        h = x @ W1 + b1
        act = np.maximum(h, 0.0); on = (h > 0).astype(np.float64)
        dh = gr[:, None] * w2[None, :] * on
        g[0] += x.T @ dh; g[1] += dh.sum(axis=0); g[2] += gr @ act; g[3] += gr.sum()
        dha = ga[:, None] * np.abs(w2)[None, :] * on
        As = (np.abs(x).T @ dha, dha.sum(axis=0), ga @ act, np.array([ga.sum()]))
        for i in range(4):
            if scale is None:
                A[i][s] = As[i]
            else:
                A[i] += scale[s] * As[i]
    return tuple(g), tuple(A)


def grad_bounds(A, ref=None, c_g=None):
    """C_G 2^-24 sum_s K_s A_theta,s per gradient entry, from per-state A and the reference (ref=None: A is already the sum)."""
    c = (C_G if c_g is None else c_g) * EPS
    if ref is None:
        return tuple(c * x for x in A)
    K = state_scale(ref)
    return tuple(c * np.tensordot(K, x, axes=(0, 0)) for x in A)


def grad_ratio(got, want, A, ref=None):
    """The largest |got - want| over all four gradients in units of 2^-24 sum_s K_s A_theta,s (entries whose bound is 0 must
    be exact: inf otherwise)."""
    worst = 0.0
    for x, y, b in zip(got, want, grad_bounds(A, ref, 1.0)):
        err = np.abs(np.asarray(x, dtype=np.float64).reshape(b.shape) - y.reshape(b.shape))
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))
        worst = max(worst, float(r.max(initial=0.0)))
    return worst


def check_grads(got, want, A, ref=None, c_g=None, what=""):
    names = ("dW1", "db1", "dw2", "db2")
    for name, x, y, b in zip(names, got, want, grad_bounds(A, ref, c_g)):
        x = np.asarray(x, dtype=np.float64).reshape(b.shape); y = y.reshape(b.shape)
        assert np.isfinite(x).all(), (what, name, "not finite")
        bad = np.abs(x - y) > b
        assert not bad.any(), (what, name, "entries off (index, got, want, bound)",
                               [(int(i), float(x.reshape(-1)[i]), float(y.reshape(-1)[i]), float(b.reshape(-1)[i])) for i in np.flatnonzero(bad)[:5]],
                               int(bad.sum()))


def header_constants():
    """The partition constants of the gradient kernel, read from the kernels' shape header (not guessed)."""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "deepgroebner_amd", "csrc", "bbx_pmlp_shape.h")).read()
    get = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    return get("PMLP_GRAD_STATES_PER_WAVE"), get("PMLP_GRAD_MAX_WAVES")
