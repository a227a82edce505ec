"""The PPO loss between the forward and the gradient kernels — bbx_pmlp_ppo_grad[_at], bbx_pmlp2_ppo_grad[_at],
PMLPPolicy.ppo_step[_at] — against float64: per position the surrogate value u, the coefficients gl = dL/dlogprob, ge = dL/dH of
    L = -scale sum_k u_k - scale ent_coef sum_k H_k
and the six statistics.  Plain numpy on top of tests/policy_grad_cases.reference_eval, importable without a GPU
(tests/test_ppo_cpu.py checks gl / ge against torch autograd in double precision).

    new = logprob_k   old = old_logprobs[k]   A = advantages[k]   d = new - old   r = exp(d)   sA = scale A
    mode 0:  u = new A                            gl = -sA
    mode 1:  a = r A, b = clamp(r, lo, hi) A      u = min(a, b)    gl = -(sA r) if a <= b else 0      (lo = 1 - eps, hi = 1 + eps)
    mode 2:  u = r A - c_kl (old - new)           gl = -(sA r) - scale c_kl
    ge = -(scale ent_coef)
A position whose log-probability is NaN is not counted: gl = ge = 0, nothing in any sum.

What the kernels are held to (tol = policy_cases.Ref.tol(), the log-probability's own bound; E = 2^-24 (1 + |new - old|)):
    the clip decision, stats[0], stats[4], stats[5]                   exact
    |gl - gl64| <= |scale A| r64 (tol + C_R E)                        (mode 0: r64 taken as 1; mode 2: + C_R 2^-24 |scale c_kl|)
    |u - u64|   <= |A| rho (tol + C_R E)                              rho = r64; mode 0: |new| + 1 (u = new A: the factor of A is new
                                                                      itself); mode 1: max(r64, lo) (a ratio clipped from below leaves
                                                                      u = lo A, whose rounding does not shrink with r);
                                                                      mode 2: + |c_kl| (tol + C_R E) for the penalty term
    |ge - ge64| <= 2^-24 |ge64|                                       one float32 product
    stats[1], [2], [3]: within the sums of the bounds of u, of the entropy (policy_grad_cases / policy2_grad_cases) and of
    old - new (tol + C_R E)
The exact decisions need every ratio away from the clip bounds by more than the float32 error of r: the cases PLACE the ratios, at
least 0.5 % from 1 +- eps (tests/test_ppo_cpu.py checks it), against a relative error of r of about tol + 2^-24 (1 + |d|) < 1e-4.

C_R: R_R is the largest |gl - gl64'| in units of |scale A| r64' 2^-24 (1 + |d|) over every case of tests/test_ppo_gpu.py (each prints
the ratio it needed: pytest -s), gl64' being the float64 formula at the kernel's OWN float32 log-probability — the epilogue's
arithmetic alone, without the logit error tol stands for.  C_R is the next power of two at or above 4 R_R; 64 is the ceiling
(policy_cases'): a ratio above it is a finding about the kernel, not a constant."""
import numpy as np

from tests import policy_cases as pc
from tests import policy_grad_cases as gc

EPS = pc.EPS
# Measured on an MI355X over the 70 cases of tests/test_ppo_gpu.py that print it: R_R = 2.076 (12x128 and 12x128x128, mode 1,
# n = 1023; the ratio printed is the larger of gl's and u's) -> 4 R_R = 8.3 -> C_R = 16.
R_R = 2.076
C_R = 16.0
CLIP = 0.2
PLACED = (0.5, 0.79, 0.81, 1.0, 1.19, 1.21, 2.0)      # ratios on both sides of both bounds of eps = 0.2, and far outside
MARGIN = 0.005                                # every placed ratio is at least this far (relative) from 1 +- eps


def f32(x):
    return np.float32(x)


class Loss:
    """mode and the four float32 constants of a call, as float64 numbers."""

    def __init__(self, mode, n, eps=CLIP, ent_coef=0.01, c_kl=0.0, scale=None):
        self.mode = mode
        self.scale = float(f32(1.0 / n if n else 0.0)) if scale is None else float(f32(scale))
        self.eps, self.ent_coef, self.c_kl = float(f32(eps)), float(f32(ent_coef)), float(f32(c_kl))
        # (the kernel forms 1.f - eps and 1.f + eps in float32)
        self.lo, self.hi = float(f32(1.0) - f32(eps)), float(f32(1.0) + f32(eps))

    def args(self):
        return self.mode, self.scale, self.eps, self.ent_coef, self.c_kl


def reference_loss(loss, new, H, old, adv):
    """float64 (u, gl, ge, clipped, counted, r, d) per position from log-probabilities `new` (NaN: not counted), entropies H,
    old log-probabilities and advantages."""
    new = np.asarray(new, dtype=np.float64); old = np.asarray(old, dtype=np.float64); A = np.asarray(adv, dtype=np.float64)
    counted = ~np.isnan(new)
    nw = np.where(counted, new, old)
    d = nw - old
    r = np.exp(d)
    sA = loss.scale * A
    clipped = np.zeros(len(nw), dtype=bool)
    if loss.mode == 0:
        u, gl = nw * A, -sA
    elif loss.mode == 1:
        a, b = r * A, np.clip(r, loss.lo, loss.hi) * A
        u = np.minimum(a, b)
        clipped = a > b
        gl = np.where(clipped, 0.0, -(sA * r))
    else:
        u, gl = r * A - loss.c_kl * (old - nw), -(sA * r) - loss.scale * loss.c_kl
    ge = np.full(len(nw), -(loss.scale * loss.ent_coef))
    z = lambda x: np.where(counted, x, 0.0)
    return z(u), z(gl), z(ge), clipped & counted, counted, r, d


def reference_stats(loss, new, H, old, adv):
    u, gl, ge, clipped, counted, r, d = reference_loss(loss, new, H, old, adv)
    H = np.where(counted, np.asarray(H, dtype=np.float64), 0.0)
    return np.array([counted.sum(), u.sum(), H.sum(), np.where(counted, -d, 0.0).sum(), clipped.sum(), (~counted).sum()], dtype=np.float64)


def bounds(loss, new, old, adv, tol, c_r=None):
    """(bound of gl, bound of u, bound of old - new) per position; tol: the log-probability's bound per position."""
    c = C_R if c_r is None else c_r
    new = np.asarray(new, dtype=np.float64); old = np.asarray(old, dtype=np.float64); A = np.abs(np.asarray(adv, dtype=np.float64))
    counted = ~np.isnan(new)
    nw = np.where(counted, new, old)
    d = nw - old
    r = np.exp(d)
    rel = tol + c * EPS * (1.0 + np.abs(d))
    if loss.mode == 0:
        bg, bu = loss.scale * A * rel, A * (np.abs(nw) + 1.0) * rel
    elif loss.mode == 1:
        bg, bu = loss.scale * A * r * rel, A * np.maximum(r, loss.lo) * rel
    else:
        bg = loss.scale * A * r * rel + c * EPS * abs(loss.scale * loss.c_kl)
        bu = A * r * rel + abs(loss.c_kl) * rel
    z = lambda x: np.where(counted, x, 0.0)
    return z(bg), z(bu), z(rel)


def needed_ratio(loss, gl, u, new32, old, adv):
    """R_R of one call: the largest |gl - gl64'| in units of |scale A| r 2^-24 (1 + |d|) and the largest |u - u64'| in units of
    |A| rho 2^-24 (1 + |d|) (bounds()' factors), gl64' and u64' the float64 formulae at the kernel's own float32 log-probabilities
    new32 (positions with a zero unit must be exact: inf otherwise); the larger of the two."""
    u64, g64, ge, clipped, counted, r, d = reference_loss(loss, new32, np.zeros(len(gl)), old, adv)
    one = Loss(loss.mode, 1, loss.eps, loss.ent_coef, loss.c_kl, loss.scale)
    bg, bu, _ = bounds(one, new32, old, adv, 0.0, 1.0)
    worst = 0.0
    for got, want, unit in ((gl, g64, bg), (u, u64, bu)):
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(unit > 0, err / unit, np.where(err > 0, np.inf, 0.0))
        worst = max(worst, float(np.where(counted, q, 0.0).max(initial=0.0)))
    return worst


# ---- inputs
ONE = [(1, (1,)), (12, (128,)), (33, (65,)), (64, (256,))]          # the shapes of tests/test_policy_indexed_gpu.py
TWO = [(12, (128, 128)), (33, (65, 64)), (1, (1, 1))]
S, R = 37, 40
ROWS = (33, 0, 40, 1, 2, 45, -3, 17, 31, 32)      # the tile of 32 and around it, none, one, more than obs_rows
_sources = {}


def source(cols, hidden, n_src=S, rr=R, seed=600):
    """Recorded states: row counts cycling through ROWS, garbage beyond the live rows, a few actions out of range
    (read-only, shared between tests)."""
    key = (cols, tuple(hidden), n_src, rr, seed)
    if key not in _sources:
        w = pc.make_weights(cols, hidden, seed)
        rows = np.resize(np.array(ROWS, dtype=np.int32), n_src)
        obs = pc.fill_padding(pc.random_blocks(n_src, rr, cols, seed + 1), rows, True, seed + 2)
        rng = np.random.default_rng(seed + 3)
        live = np.clip(rows, 0, rr)
        actions = (rng.integers(0, 1 << 30, size=n_src) % np.maximum(live, 1)).astype(np.int32)
        if n_src > 4:
            actions[4] = -1
        if n_src > 7:
            actions[7] = rr
        for a in (obs, rows, actions):
            a.setflags(write=False)
        _sources[key] = (w, obs, rows, actions)
    return _sources[key]


def reference_at(cols, hidden, index):
    """float64 (logprob, entropy, tol, entropy_tol) of the positions of `index` over source(cols, hidden); an index out of range:
    NaN, NaN and zero bounds."""
    from tests import policy2_grad_cases as g2
    w, obs, rows, actions = source(cols, hidden)
    index = np.asarray(index).astype(np.int64)
    inside = (index >= 0) & (index < len(rows))
    j = np.where(inside, index, 0)
    lp, H, ref = gc.reference_eval(w, obs[j], rows[j], actions[j])
    etol = gc.entropy_tol(ref) if len(hidden) == 1 else g2.entropy_tol(ref)
    nan = lambda x: np.where(inside, x, np.nan)
    return nan(lp), nan(H), np.where(inside, ref.tol(), 0.0), np.where(inside, etol, 0.0)


STAT_THREADS_NS = lambda t: (0, 1, t - 1, t, t + 1, 2 * t + 1)      # n around the statistics kernel's partition boundaries

def placed_old(new64, seed=0):
    """Old log-probabilities that PLACE the ratios: old = new64 - log(t), t cycling through PLACED (float32; NaN positions get 0)."""
    new64 = np.asarray(new64, dtype=np.float64)
    t = np.resize(np.array(PLACED), len(new64))
    t = np.roll(t, seed % len(PLACED))
    return np.where(np.isnan(new64), 0.0, new64 - np.log(t)).astype(np.float32), t


def far_old(new64, seed=0):
    """The extra set: |new - old| up to 10, both signs; where the ratio comes within 1 % of a clip bound of eps = 0.2 the position
    gets ratio 1 instead (so that the clip decision stays one a float32 evaluation must agree with)."""
    new64 = np.asarray(new64, dtype=np.float64)
    rng = np.random.default_rng(100 + seed)
    d = rng.uniform(-10.0, 10.0, size=len(new64))
    d[:2] = (10.0, -10.0)[:len(d)]
    near = (np.abs(np.exp(d) / (1 + CLIP) - 1) < 2 * MARGIN) | (np.abs(np.exp(d) / (1 - CLIP) - 1) < 2 * MARGIN)
    d[near] = 0.0
    return np.where(np.isnan(new64), 0.0, new64 - d).astype(np.float32)


def advantages(n, seed=0):
    """Both signs, exact zeros among them (every fifth)."""
    a = np.random.default_rng(200 + seed).normal(size=n).astype(np.float32)
    a[::5] = 0.0
    if n > 1:
        a[1] = -abs(a[1]) - 0.5
    if n > 2:
        a[2] = abs(a[2]) + 0.5
    return a


def distance_from_bounds(new64, old, eps=CLIP):
    """The smallest relative distance of any counted ratio exp(new64 - old) from 1 - eps and 1 + eps, in float64."""
    new64 = np.asarray(new64, dtype=np.float64)
    counted = ~np.isnan(new64)
    r = np.exp(np.where(counted, new64 - np.asarray(old, dtype=np.float64), 0.0))
    lo, hi = float(f32(1.0) - f32(eps)), float(f32(1.0) + f32(eps))
    dist = np.minimum(np.abs(r / lo - 1.0), np.abs(r / hi - 1.0))
    return float(np.where(counted, dist, np.inf).min(initial=np.inf))


def header_constants():
    """The statistics kernel's partition constant, read from the kernels' shape header (not guessed)."""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "deepgroebner_amd", "csrc", "bbx_pmlp_shape.h")).read()
    return int(re.search(r"constexpr int PMLP_PPO_STAT_THREADS = (\d+);", text).group(1))
