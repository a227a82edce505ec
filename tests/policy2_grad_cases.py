"""The training side of the TWO-hidden-layer PMLP policy — bbx_pmlp2_logprob, bbx_pmlp2_grad, PMLPPolicy.evaluate with
deep_kernels — against float64: the log-probability of a recorded action, the entropy over a state's rows, and the gradient of
    L = sum_s glogp[s] logprob_s + gent[s] entropy_s
with respect to W1 [cols][h1], b1 [h1], W2 [h1][h2], b2 [h2], w3 [h2], b3 [1].  Plain numpy on top of tests/policy_cases.py and
tests/policy_grad_cases.py (whose reference_eval, bounds and ratios hold for any depth), importable without a GPU
(tests/test_policy2_grad_cpu.py checks the reference against torch autograd in double precision).

Conventions and bounds are those of tests/policy_grad_cases.py, with K_s = max_r S_r + |logZ_s| + 1:
    |logprob - ref|  <= Ref.tol()
    |entropy - ref|  <= C_H2 2^-24 K_s (1 + log n)
    |g - g_ref|      <= C_G2 2^-24 sum_s K_s A_theta,s                for every gradient entry theta
A_theta,s: the state's contribution to the entry with every term replaced by its absolute value through BOTH layers — |g_r| as
|glogp| (delta_{r,a} + p_r) + |gent| p_r (|log p_r| + H), |w3|, |W2|, |x|, the relu masks and the (non-negative) activations kept."""
import numpy as np

from tests import policy_cases as pc
from tests import policy_grad_cases as gc

EPS = pc.EPS
# R_H2: the largest |entropy - ref| in units of 2^-24 K_s (1 + log n), R_G2: the largest |g - g_ref| in units of
# 2^-24 sum_s K_s A_theta,s, over every case of tests/test_policy2_grad_gpu.py (each prints the ratio it needed: pytest -s).
# Each constant is the next power of two at or above 4 x the measured ratio (the rule of tests/policy_grad_cases.py); 64
# (policy_cases' ceiling) is where they start, and a ratio above it is a finding about the kernel, not a constant.
# Measured on an MI355X: R_H2 = 0.211 (1x1x1, the row sweep) -> 4 R_H2 = 0.84 -> C_H2 = 1; R_G2 = 3.084 (13x65x64, N = 5, gent = NULL:
# without the entropy term A is at its smallest; with it the largest ratio is 2.521, the autograd case) -> 4 R_G2 = 12.3 -> C_G2 = 16.
# (A takes the activations at their float64 values, so it only bounds a kernel whose recomputed activations are good to a
# RELATIVE 2^-24: with both pre-activations recomputed in fp32 an activation of 5e-4 left by cancellation among terms of size 3.5
# was off by 2e-4 of itself and two cases needed 139.7 and 97.6.  The backward kernel therefore recomputes them with f64
# accumulation: DESIGN.md 4.4.3.)
R_H2, R_G2 = 0.211, 3.084
C_H2, C_G2 = 1.0, 16.0
NAMES = ("dW1", "db1", "dW2", "db2", "dw3", "db3")


def entropy_tol(ref, c_h=None):
    return gc.entropy_tol(ref, C_H2 if c_h is None else c_h)


def reference_grad2(weights, obs, rows, actions, glogp, gent=None, scale=None, ref=None):
    """float64 gradients (gW1 [cols][h1], gb1 [h1], gW2 [h1][h2], gb2 [h2], gw3 [h2], gb3 [1]) of L for a TWO-hidden-layer policy, and
    the absolute contributions A per state, each with a leading [N] axis.  scale [N] (K_s) given: A is returned summed,
    sum_s scale_s A_theta,s, in the gradients' shapes (large N)."""
    assert len(weights) == 3, "two hidden layers"
    obs = np.asarray(obs); a = np.asarray(actions).astype(np.int64)
    if ref is None:
        ref = pc.reference(weights, obs, rows)
    N, R, cols = obs.shape
    f = lambda t: np.asarray(t, dtype=np.float64)
    W1, b1, W2, b2, w3 = f(weights[0][0]), f(weights[0][1]), f(weights[1][0]), f(weights[1][1]), f(weights[2][0])
    h1, h2 = W1.shape[1], W2.shape[1]
    glogp = f(glogp)
    gent = np.zeros(N) if gent is None else f(gent)
    shapes = ((cols, h1), (h1,), (h1, h2), (h2,), (h2,), (1,))
    g = [np.zeros(sh) for sh in shapes]
    A = [np.zeros(sh if scale is not None else (N,) + sh) for sh in shapes]
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
        z1 = x @ W1 + b1; a1 = np.maximum(z1, 0.0); on1 = (z1 > 0).astype(np.float64)
        z2 = a1 @ W2 + b2; a2 = np.maximum(z2, 0.0); on2 = (z2 > 0).astype(np.float64)
        for grow, w3v, W2v, xv, out, k in ((gr, w3, W2, x, g, None), (ga, np.abs(w3), np.abs(W2), np.abs(x), A, 1.0 if scale is None else scale[s])):
            dz2 = grow[:, None] * w3v[None, :] * on2
            dz1 = (dz2 @ W2v.T) * on1
            terms = (xv.T @ dz1, dz1.sum(axis=0), a1.T @ dz2, dz2.sum(axis=0), grow @ a2, np.array([grow.sum()]))
            for i, t in enumerate(terms):
                if k is None:
                    out[i] += t
                elif scale is None:
                    out[i][s] = t
                else:
                    out[i] += k * t
    return tuple(g), tuple(A)


def grad_ratio(got, want, A, ref=None):
    return gc.grad_ratio(got, want, A, ref)


def check_grads(got, want, A, ref=None, c_g=None, what=""):
    for name, x, y, b in zip(NAMES, got, want, gc.grad_bounds(A, ref, C_G2 if c_g is None else c_g)):
        x = np.asarray(x, dtype=np.float64).reshape(b.shape); y = y.reshape(b.shape)
        assert np.isfinite(x).all(), (what, name, "not finite")
        bad = np.abs(x - y) > b
        assert not bad.any(), (what, name, "entries off (index, got, want, bound)",
                               [(int(i), float(x.reshape(-1)[i]), float(y.reshape(-1)[i]), float(b.reshape(-1)[i])) for i in np.flatnonzero(bad)[:5]],
                               int(bad.sum()))


def header_constants():
    """(states per workgroup, the most workgroups) of the two-layer gradient kernel, read from the kernels' shape header."""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "deepgroebner_amd", "csrc", "bbx_pmlp_shape.h")).read()
    get = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    return get("PMLP2_GRAD_STATES_PER_GROUP"), get("PMLP2_GRAD_MAX_GROUPS")


# ---- exact-integer constructions: every logit of a state is equal although its rows differ, so p_r = 1 / n exactly (n a power
# of two); with glogp a multiple of n and gent NULL every g_r is an integer, and every product and sum of the backward pass is an
# integer far below 2^24: the kernel's outputs equal the float64 reference exactly, and a row, column or unit of a permuted
# operand in the wrong place changes almost every entry.
INT_SHAPES = [(12, (128, 128)), (33, (70, 66)), (12, (64, 64)), (64, (128, 128))]
INT_ROWS = (16, 32, 64)
INT_N = 6


def _int_batch(rng, cols, n, multiples):
    rows = np.full(INT_N, n, dtype=np.int32)
    obs = pc.fill_padding(rng.integers(0, 4, size=(INT_N, n + 3, cols)).astype(np.int32), rows, True, 1)
    actions = rng.integers(0, n, size=INT_N).astype(np.int32)
    glogp = (n * rng.choice(np.array(multiples), size=INT_N)).astype(np.float32)
    return obs, rows, actions, glogp


def int_case_a(cols, hidden, n, seed=0):
    """The SECOND-layer units in pairs with the same W2 column and bias and opposite w3: every logit is b3.  Exercises dW2, db2, dw3
    (about half of their entries non-zero); dz1 cancels pair by pair, so dW1 and db1 are exactly 0."""
    h1, h2 = hidden
    rng = np.random.default_rng(seed)
    W1 = rng.integers(-1, 2, size=(cols, h1)); b1 = rng.integers(-6, 4, size=h1)
    half = h2 // 2
    W2h = rng.integers(-1, 2, size=(h1, half)); b2h = rng.integers(-20, 21, size=half); w3h = rng.integers(-2, 3, size=half)
    W2 = np.concatenate([W2h, W2h], axis=1); b2 = np.concatenate([b2h, b2h]); w3 = np.concatenate([w3h, -w3h])
    if h2 % 2:
        W2 = np.concatenate([W2, np.zeros((h1, 1))], axis=1); b2 = np.append(b2, 0); w3 = np.append(w3, 0)
    f = lambda t: np.ascontiguousarray(t, dtype=np.float32)
    w = [(f(W1), f(b1)), (f(W2), f(b2)), (f(w3), np.array([1.0], dtype=np.float32))]
    return (w,) + _int_batch(rng, cols, n, (-1, 1))


def int_case_b(cols, hidden, n, seed=0):
    """The FIRST-layer units in pairs with the same W1 column and bias and opposite W2 rows: z2 = b2 exactly, whatever the row.
    Exercises dW1, db1 and dW2 through per-row relu masks of the first layer; db2 and dw3 (sum_r g_r = 0 times a constant) are
    exactly 0."""
    h1, h2 = hidden
    rng = np.random.default_rng(seed)
    half = h1 // 2
    W1h = rng.integers(-1, 2, size=(cols, half)); b1h = rng.integers(-6, 4, size=half)
    W1 = np.concatenate([W1h, W1h], axis=1); b1 = np.concatenate([b1h, b1h])
    W2h = rng.integers(-2, 3, size=(half, h2)); W2 = np.concatenate([W2h, -W2h], axis=0)
    if h1 % 2:
        W1 = np.concatenate([W1, np.zeros((cols, 1))], axis=1); b1 = np.append(b1, 0); W2 = np.concatenate([W2, np.zeros((1, h2))], axis=0)
    b2 = rng.integers(-3, 6, size=h2); w3 = rng.integers(-3, 4, size=h2)
    f = lambda t: np.ascontiguousarray(t, dtype=np.float32)
    w = [(f(W1), f(b1)), (f(W2), f(b2)), (f(w3), np.array([1.0], dtype=np.float32))]
    return (w,) + _int_batch(rng, cols, n, (-3, -2, -1, 1, 2, 3))


def int_case_reference(kind, w, obs, rows, actions, glogp):
    """The reference of an integer case after asserting what the construction promises: equal logits per state, integer gradients,
    absolute sums below 2^24, the gradients that must vanish exactly 0 and the exercised ones not degenerate.  Returns np.rint(g)."""
    ref = pc.reference(w, obs, rows)
    n = int(rows[0])
    assert (ref.logits[:, :n] == ref.logits[:, :1]).all(), "the logits of a state differ"
    want, A = reference_grad2(w, obs, rows, actions, glogp, None, ref=ref)
    assert all(np.abs(y - np.rint(y)).max() <= 1e-8 for y in want), "not integers"
    assert max(float(a.sum(axis=0).max()) for a in A) < 2.0 ** 24, "absolute sums reach 2^24"
    want = tuple(np.rint(y) for y in want)
    nz = [int((y != 0).sum()) for y in want]
    if kind == "a":
        assert nz[0] == 0 and nz[1] == 0, "dW1, db1 must vanish"
        assert nz[2] > want[2].size // 4 and nz[3] > want[3].size // 4 and nz[4] > want[4].size // 4, ("the case is degenerate", nz)
    else:
        assert nz[3] == 0 and nz[4] == 0, "db2, dw3 must vanish"
        assert nz[0] > want[0].size // 8 and nz[1] > want[1].size // 8 and nz[2] > want[2].size // 8, ("the case is degenerate", nz)
    return want
