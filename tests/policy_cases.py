"""The floating-point side of the library — the PMLP policy kernels (bbx_pmlp_act, bbx_pmlp2_act, bbx_pmlp3_act and the same tile
code inside the step kernels) — against a float64 evaluation: the reference, the checker of a kernel's draws, and seeded
builders of the cases tests/test_policy_parity.py runs.  Plain numpy, importable without a GPU (tests/test_policy_cases_cpu.py
checks that reference, checker and builders are what they claim to be).

Weights are a list [(W1, b1), ..., (wd, bd)] of float32 arrays in the layouts include/bbx.h hands to the prepare calls:
W [inputs][units] (torch.nn.Linear(...).weight.t()), b [units]; the deciding layer last, wd [units], bd [1].

What a kernel's draw is held to, per environment with n live rows, reference log-partition logZ, reference CDF F and the
per-row scale S_r (the network evaluated with |W|, |b|, |x|: what an fp32 rounding error of a logit is proportional to):
    |logprob - ref_logsoftmax[action]| <= tol = C_L 2^-24 (max_r S_r + |logZ| + 1)
    F[action - 1] - delta <= u <= F[action] + delta,   delta = 2 C_L 2^-24 max_r S_r + C_S 2^-24 (8 + n / 64)
(a logit off by e moves every probability by a factor within e^(+-2e): the first term; the fp32 sum of n exponentials in 64
lanes, the fast exponential and the rounding of u * sum: the second)."""
import numpy as np

MAXROWS = 2048                                # BBX_POLICY_MAX_ROWS
EPS = 2.0 ** -24
# To be measured on an MI355X against reference() below over every case of tests/test_policy_parity.py (each prints its
# ratios: pytest -s): R_L, the largest |logprob - ref| any draw needs in units of 2^-24 (max S + |logZ| + 1), and R_S, the
# largest distance of a draw from its reference CDF interval in units of 2^-24 (8 + n / 64) after the logit term at the chosen
# C_L.  Each constant is then the next power of two at or above 4 x the measured ratio (the accumulation order of the
# MFMA chains and the fast __expf / __logf are fixed by the code: the spread between cases is small, the margin is for inputs
# the cases do not cover).  64 is the ceiling: a ratio above it is a finding about the kernel, not a constant.
C_CEILING = 64.0
R_L, R_S = None, None                         # UNMEASURED: no MI355X run has set these yet; the constants stand at the ceiling
C_L, C_S = C_CEILING, C_CEILING

# ---- the edges of the kernels' instantiation table (bbx_pmlp_shape.h) and of their tiles
ONE_COLS = (1, 2, 6, 7, 12, 13, 20, 21, 32, 33, 63, 64)          # k-steps of two columns: 3 | 6 | 10 | 16 | 32
ONE_HIDDEN = (1, 31, 32, 33, 64, 65, 128, 129, 255, 256)          # blocks of 32 units: 1 | 2 | 4 | 8
TWO_COLS = (1, 12, 13, 32, 33, 64)                                # k-steps of four columns: 3 | 8 | 16
TWO_HIDDEN = ((1, 1), (64, 64), (65, 64), (64, 65), (17, 128), (128, 128))
THREE_HIDDEN = ((1, 1, 1), (64, 64, 64), (64, 65, 17), (128, 128, 128))
THREE_COLS = (12, 33, 64)
LIVE_ROWS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
TALL_ROWS = (1023, 1024, 1025, 2047, 2048)
BATCHES = (1, 5, 9)


def one_layer_shapes():
    """(cols, (hidden,)): the four corners, then every column count and every hidden size at least once."""
    out = [(c, (h,)) for c in (ONE_COLS[0], ONE_COLS[-1]) for h in (ONE_HIDDEN[0], ONE_HIDDEN[-1])]
    for i, c in enumerate(ONE_COLS):
        s = (c, (ONE_HIDDEN[(i + 3) % len(ONE_HIDDEN)],))
        if s not in out:
            out.append(s)
    return out


def two_layer_shapes():
    out = [(c, h) for c in (TWO_COLS[0], TWO_COLS[-1]) for h in (TWO_HIDDEN[0], TWO_HIDDEN[-1])]
    for i, c in enumerate(TWO_COLS):
        s = (c, TWO_HIDDEN[(i + 2) % len(TWO_HIDDEN)])
        if s not in out:
            out.append(s)
    return out


def three_layer_shapes():
    out = [(THREE_COLS[0], THREE_HIDDEN[-1]), (THREE_COLS[-1], THREE_HIDDEN[0])]
    for i, h in enumerate(THREE_HIDDEN):
        s = (THREE_COLS[(i + 1) % len(THREE_COLS)], h)
        if s not in out:
            out.append(s)
    return out


def label(cols, hidden):
    return "%dx%s" % (cols, "x".join(str(h) for h in hidden))


# ---- weights
def make_weights(cols, hidden, seed, scale=0.3, decide_scale=None):
    """torch.nn.Linear's default initialisation (weights and biases uniform in +-1/sqrt(inputs)) from numpy's generator, the
    weight matrices times `scale` (the deciding layer's times `decide_scale` where given), float32."""
    rng = np.random.default_rng(seed)
    dims = [cols] + list(hidden) + [1]
    out = []
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        k = 1.0 / np.sqrt(a)
        last = i == len(dims) - 2
        sc = decide_scale if (last and decide_scale is not None) else scale
        W = (rng.uniform(-k, k, size=(a, b)) * sc).astype(np.float32)
        bias = rng.uniform(-k, k, size=b).astype(np.float32)
        out.append((W[:, 0].copy(), bias) if last else (W, bias))
    return out


def weights_of(policy):
    """The weights of a deepgroebner_amd.rollout.PMLPPolicy in this module's layout."""
    f = lambda t: t.detach().cpu().numpy().astype(np.float32)
    out = [(f(l.weight).T.copy(), f(l.bias)) for l in policy.embedding]
    out.append((f(policy.deciding.weight).reshape(-1), f(policy.deciding.bias).reshape(-1)))
    return out


def to_policy(weights, device="cpu", dtype=None):
    """A PMLPPolicy holding `weights`."""
    import torch
    from deepgroebner_amd.rollout import PMLPPolicy
    pol = PMLPPolicy(weights[0][0].shape[0], [W.shape[1] for W, _ in weights[:-1]])
    with torch.no_grad():
        for lin, (W, b) in zip(pol.embedding, weights[:-1]):
            lin.weight.copy_(torch.from_numpy(np.ascontiguousarray(W.T))); lin.bias.copy_(torch.from_numpy(b))
        pol.deciding.weight.copy_(torch.from_numpy(weights[-1][0].reshape(1, -1))); pol.deciding.bias.copy_(torch.from_numpy(weights[-1][1].reshape(1)))
    if dtype is not None:
        pol = pol.to(dtype)
    return pol.to(device)


# ---- the reference
class Ref:
    """reference()'s result, arrays over [environment, row]: n [B] live rows; logits, logsm (log-softmax), cdf (inclusive),
    scale (S_r) [B, R'] — nan / 1.0 / 0 beyond the live rows; logz [B]."""

    def __init__(self, n, logits, logsm, cdf, scale, logz):
        self.n, self.logits, self.logsm, self.cdf, self.scale, self.logz = n, logits, logsm, cdf, scale, logz

    def take(self, idx):
        """The reference of a batch made of copies idx[i] of this one's environments."""
        return Ref(*[a[idx] for a in (self.n, self.logits, self.logsm, self.cdf, self.scale, self.logz)])

    def smax(self):
        live = np.arange(self.scale.shape[1])[None, :] < self.n[:, None]
        return np.where(live, self.scale, 0.0).max(axis=1, initial=0.0)

    def tol(self, c_l=None):
        return (C_L if c_l is None else c_l) * EPS * (self.smax() + np.abs(self.logz) + 1.0)

    def delta(self, c_l=None, c_s=None):
        return 2.0 * (C_L if c_l is None else c_l) * EPS * self.smax() + (C_S if c_s is None else c_s) * EPS * (8.0 + self.n / 64.0)


def reference(weights, obs, rows):
    """float64: logit_r = wd . relu(... relu(W1^T x_r + b1) ...) + bd over rows 0 .. min(rows, obs_rows, 2048) - 1 of every
    environment (the row COUNT masks — whatever the rows beyond it hold, -1 padding or not, plays no part: include/bbx.h),
    log-softmax and CDF over them, and the scale S_r of every row."""
    obs = np.asarray(obs); rows = np.asarray(rows).astype(np.int64)
    B, R, cols = obs.shape
    Rm = min(R, MAXROWS)
    n = np.clip(np.minimum(rows, Rm), 0, None)
    W64 = [(np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)) for W, b in weights]
    logits = np.empty((B, Rm)); scale = np.empty((B, Rm))
    step = max(1, (1 << 17) // max(Rm, 1))
    for e0 in range(0, B, step):
        h = obs[e0:e0 + step, :Rm].astype(np.float64); s = np.abs(h)
        for W, b in W64[:-1]:
            h = np.maximum(h @ W + b, 0.0); s = s @ np.abs(W) + np.abs(b)
        wd, bd = W64[-1]
        logits[e0:e0 + step] = h @ wd + bd[0]; scale[e0:e0 + step] = s @ np.abs(wd) + abs(bd[0])
    live = np.arange(Rm)[None, :] < n[:, None]
    mx = np.where(live, logits, -np.inf).max(axis=1, initial=-np.inf)
    mx = np.where(n > 0, mx, 0.0)
    ex = np.where(live, np.exp(np.where(live, logits - mx[:, None], 0.0)), 0.0)
    se = ex.sum(axis=1)
    logz = np.where(n > 0, mx + np.log(np.where(n > 0, se, 1.0)), 0.0)
    logsm = np.where(live, logits - logz[:, None], np.nan)
    p = np.where(live, np.exp(np.where(live, logsm, 0.0)), 0.0)
    cdf = np.cumsum(p, axis=1)
    return Ref(n, np.where(live, logits, np.nan), logsm, cdf, np.where(live, scale, 0.0), logz)


def act_float32(weights, obs, rows, u):
    """The kernels' computation in plain float32 numpy (row count masks, softmax, inverse CDF: the first row whose cumulative
    weight exceeds u times the total, the last one on round-off): a stand-in for a kernel where there is no GPU."""
    obs = np.asarray(obs); rows = np.asarray(rows); u = np.asarray(u, dtype=np.float32)
    B, R, _ = obs.shape
    Rm = min(R, MAXROWS)
    h = obs[:, :Rm].astype(np.float32)
    for W, b in weights[:-1]:
        h = np.maximum(h @ W.astype(np.float32) + b.astype(np.float32), np.float32(0))
    lg = (h @ weights[-1][0].astype(np.float32) + np.float32(weights[-1][1][0])).astype(np.float32)
    a = np.zeros(B, dtype=np.int32); l = np.zeros(B, dtype=np.float32)
    for e in range(B):
        n = int(max(0, min(int(rows[e]), Rm)))
        if n == 0:
            continue
        x = lg[e, :n]
        mx = x.max()
        ex = np.exp(x - mx).astype(np.float32)
        c = np.cumsum(ex, dtype=np.float32)
        a[e] = min(int((c <= np.float32(u[e]) * c[-1]).sum()), n - 1)
        l[e] = x[a[e]] - (mx + np.log(c[-1]))
    return a, l


# ---- the checker
def draw_errors(ref, u, actions, logprobs):
    """Per environment (n > 0; 0 elsewhere): |logprob - ref_logsoftmax[action]| and the distance of u from the action's
    reference CDF interval [F[a - 1], F[a]] (the last row's reaches up to any u).  Actions must lie inside the rows."""
    u = np.asarray(u, dtype=np.float64); a = np.asarray(actions).astype(np.int64); l = np.asarray(logprobs, dtype=np.float64)
    B = len(ref.n)
    e = np.arange(B)
    ok = ref.n > 0
    ac = np.where(ok, np.clip(a, 0, np.maximum(ref.n - 1, 0)), 0)
    lerr = np.where(ok, np.abs(l - np.where(ok, ref.logsm[e, ac], 0.0)), 0.0)
    lo = np.where(ac > 0, ref.cdf[e, np.maximum(ac - 1, 0)], 0.0)
    hi = np.where(ac >= ref.n - 1, np.inf, ref.cdf[e, ac])
    dist = np.where(ok, np.maximum(np.maximum(lo - u, u - hi), 0.0), 0.0)
    return lerr, dist


def ratios(ref, u, actions, logprobs, c_l=None):
    """What these draws need: (the largest |logprob error| in units of 2^-24 (max S + |logZ| + 1), the largest distance from
    the CDF interval beyond the logit term 2 c_l 2^-24 max S in units of 2^-24 (8 + n / 64), the same without taking the logit
    term off)."""
    lerr, dist = draw_errors(ref, u, actions, logprobs)
    r_l = float((lerr / ref.tol(1.0)).max(initial=0.0))
    unit = EPS * (8.0 + ref.n / 64.0)
    r_s = float(((dist - 2.0 * (C_L if c_l is None else c_l) * EPS * ref.smax()) / unit).max(initial=0.0))
    return r_l, max(r_s, 0.0), float((dist / unit).max(initial=0.0))


def check_draws(weights, obs, rows, u, actions, logprobs, c_l=None, c_s=None, ref=None, what=""):
    """Holds the output of ANY policy kernel to the reference: every action inside [0, n); n <= 0: action 0 and log-probability
    exactly 0.0; the action admissible for u (module docstring); the log-probability within tol of the reference's for that
    row.  Raises AssertionError naming the first offenders.  Returns the number of draws that only the delta band admitted
    (u outside the row's own reference interval), so that callers can cap it."""
    if ref is None:
        ref = reference(weights, obs, rows)
    a = np.asarray(actions).astype(np.int64); l = np.asarray(logprobs)
    u = np.asarray(u)
    assert a.shape == ref.n.shape and l.shape == ref.n.shape and u.shape == ref.n.shape, (what, "shapes")
    dead = ref.n <= 0
    bad = dead & ((a != 0) | (l != 0.0))
    assert not bad.any(), (what, "no rows: action 0 and log-probability 0.0", np.flatnonzero(bad)[:5].tolist(), a[bad][:5].tolist(), l[bad][:5].tolist())
    bad = ~dead & ((a < 0) | (a >= ref.n))
    assert not bad.any(), (what, "action outside the rows", np.flatnonzero(bad)[:5].tolist(), a[bad][:5].tolist(), ref.n[bad][:5].tolist())
    assert np.isfinite(l).all(), (what, "log-probability not finite", np.flatnonzero(~np.isfinite(l))[:5].tolist())
    lerr, dist = draw_errors(ref, u, a, l)
    tol, delta = ref.tol(c_l), ref.delta(c_l, c_s)
    bad = lerr > tol
    assert not bad.any(), (what, "log-probability (env, action, error, tol)",
                           [(int(i), int(a[i]), float(lerr[i]), float(tol[i])) for i in np.flatnonzero(bad)[:5]], int(bad.sum()))
    bad = dist > delta
    assert not bad.any(), (what, "action not admissible for u (env, action, u, distance, delta)",
                           [(int(i), int(a[i]), float(u[i]), float(dist[i]), float(delta[i])) for i in np.flatnonzero(bad)[:5]], int(bad.sum()))
    return int((dist > 0).sum())


def near_boundary(ref, u, c_l=None, c_s=None):
    """How many draws the reference predicts the delta band may decide: u within delta of an interior CDF boundary."""
    u = np.asarray(u, dtype=np.float64)
    delta = ref.delta(c_l, c_s)
    interior = np.arange(ref.cdf.shape[1])[None, :] < (ref.n - 1)[:, None]
    return int((interior & (np.abs(ref.cdf - u[:, None]) <= delta[:, None])).any(axis=1).sum())


# ---- blocks
def fill_padding(obs, rows, garbage, seed=0):
    """Rows beyond rows[e]: -1 (the reference's padding), or large garbage the kernels must ignore just the same."""
    obs = obs.copy()
    R = obs.shape[1]
    dead = np.arange(R)[None, :] >= np.clip(rows, 0, None)[:, None]
    if garbage:
        g = np.random.default_rng(seed).choice(np.array([2 ** 31 - 1, -2 ** 31, 10 ** 9, -123456789, 65536], dtype=np.int64), size=obs.shape)
        obs[dead] = g[dead].astype(obs.dtype)
    else:
        obs[dead] = -1
    return obs


def random_blocks(B, R, cols, seed, emax=9):
    return np.random.default_rng(seed).integers(0, emax + 1, size=(B, R, cols)).astype(np.int32)


# ---- case builders: (weights, obs, rows, u) and what the case expects
class Case:
    """A launch: `base` blocks [nb, R, cols] with `base_rows`, environment i a copy of base[src[i]] (the device replicates:
    tall sweeps are hundreds of megabytes), its uniform u[i]; expect[i] >= 0: the action the case pins; ref: the reference of
    the base blocks (take(src): of the launch)."""

    def __init__(self, name, weights, base, base_rows, src, u, expect=None):
        self.name, self.weights, self.base, self.base_rows = name, weights, base, np.asarray(base_rows, dtype=np.int32)
        self.src = np.asarray(src, dtype=np.int64); self.u = np.asarray(u, dtype=np.float32)
        self.expect = np.full(len(self.src), -1, dtype=np.int64) if expect is None else np.asarray(expect, dtype=np.int64)
        self.base_ref = reference(weights, base, self.base_rows)
        self.ref = self.base_ref.take(self.src)

    @property
    def rows(self):
        return self.base_rows[self.src]

    @property
    def obs(self):
        return self.base[self.src]

    def as_tuple(self):
        return self.weights, self.obs, self.rows, self.u


def sweep_case(weights, base, base_rows, name="sweep", c_l=None, c_s=None):
    """Row sweep: every base environment replicated once per live row j with u = (F[j - 1] + F[j]) / 2: the draw must be row
    j, its log-probability the reference's.  A row is pinned unless p_j < 2 delta (expect = -1 there; skipped: their share)."""
    base_rows = np.asarray(base_rows, dtype=np.int32)
    ref = reference(weights, base, base_rows)
    delta = ref.delta(c_l, c_s)
    src, u, expect = [], [], []
    for b in range(len(ref.n)):
        n = int(ref.n[b])
        F = np.concatenate([[0.0], ref.cdf[b, :n]])
        mid = ((F[:-1] + F[1:]) / 2).astype(np.float32)
        p = np.diff(F)
        pinned = (p >= 2 * delta[b]) & (mid.astype(np.float64) > F[:-1]) & (mid.astype(np.float64) < F[1:]) & (mid < 1.0)
        src += [b] * n; u += mid.tolist(); expect += np.where(pinned, np.arange(n), -1).tolist()
    case = Case(name, weights, base, base_rows, src, u, expect)
    case.skipped = float((case.expect < 0).mean()) if len(case.expect) else 0.0
    return case


def row_sweep(cols, hidden, live_rows, seed, R=None, garbage=False, scale=0.3, decide_scale=None, c_l=None, c_s=None):
    """The row sweep over one random block (entries 0..9) per live-row count, in blocks of R rows (default: the largest count)."""
    R = max(live_rows) if R is None else R
    w = make_weights(cols, hidden, seed, scale, decide_scale)
    rows = np.array(live_rows, dtype=np.int32)
    base = fill_padding(random_blocks(len(rows), R, cols, seed + 1), rows, garbage, seed + 2)
    return sweep_case(w, base, rows, "sweep %s rows %s" % (label(cols, hidden), list(live_rows)), c_l, c_s)


def tie_case(cols, hidden, n, seed, R=None):
    """All n live rows identical, u a grid of 4n + 1 points j / 4n: away from the boundaries (the grid points that are no
    multiple of 1 / n) the draw is floor(u n) with log-probability -log n; non-decreasing in u.  Where n is a power of two
    every quantity of the kernel is exact (e^0 = 1, sums of ones, u n), so the boundaries are pinned as well: u = j / n draws
    row j — "the first row whose cumulative probability EXCEEDS u" — and u = 1.0 the last row."""
    R = n if R is None else R
    w = make_weights(cols, hidden, seed)
    row = np.random.default_rng(seed + 1).integers(0, 10, size=cols).astype(np.int32)
    base = np.full((1, R, cols), -1, dtype=np.int32); base[0, :n] = row
    g = np.arange(4 * n + 1)
    u = (g / (4.0 * n)).astype(np.float32)
    exact = (n & (n - 1)) == 0
    expect = np.where((g % 4 != 0) | exact, np.minimum(g // 4, n - 1), -1)
    return Case("ties %s n=%d" % (label(cols, hidden), n), w, base, [n], np.zeros(len(u), dtype=np.int64), u, expect)


def monotone_case(cols, hidden, n, seed, points=1024):
    """One random block, `points` sorted uniforms including 0.0, the float just below 1.0 and 1.0: draws non-decreasing,
    u = 0 draws row 0, u = 1.0 row n - 1."""
    w = make_weights(cols, hidden, seed)
    base = random_blocks(1, n, cols, seed + 1)
    u = np.sort(np.random.default_rng(seed + 2).random(points - 3).astype(np.float32))
    u = np.concatenate([[0.0], u, [np.nextafter(np.float32(1), np.float32(0)), 1.0]]).astype(np.float32)
    expect = np.full(points, -1); expect[0] = 0; expect[-1] = n - 1
    return Case("monotone %s n=%d" % (label(cols, hidden), n), w, base, [n], np.zeros(points, dtype=np.int64), u, expect)


BOUNDARY_OFFSETS = (-4096, -1024, -256, -64, -16, -4, -2, -1, 0, 1, 2, 4, 16, 64, 256, 1024, 4096)


def boundary_case(cols, hidden, n, seed):
    """One random block; for every interior CDF boundary F[j] the uniforms float32(F[j]) + k 2^-24 for k in BOUNDARY_OFFSETS:
    where the kernel's own boundary lies is measured to one ulp of u (the delta it needs), and the draws of a boundary's
    uniforms are non-decreasing."""
    w = make_weights(cols, hidden, seed)
    base = random_blocks(1, n, cols, seed + 1)
    F = reference(w, base, [n]).cdf[0, :n - 1]
    u = np.float32(F)[:, None] + np.float32(EPS) * np.array(BOUNDARY_OFFSETS, dtype=np.float32)[None, :]
    u = np.clip(u, 0.0, np.nextafter(np.float32(1), np.float32(0))).astype(np.float32).reshape(-1)
    return Case("boundaries %s n=%d" % (label(cols, hidden), n), w, base, [n], np.zeros(len(u), dtype=np.int64), u)


# (largest exponent entry, weights x default init): entries up to 255 under 1.0 x default init are left out — the highest logit
# any row of such entries reaches is 13 to 59 for the 128-unit networks of one to three layers, no row can lead by 100
PEAKED = ((255, 3.0), (65535, 1.0), (65535, 3.0))
PEAK_MARGIN = 100.0


def peaked_case(cols, hidden, emax, scale, seed, B=48, R=40):
    """Exponent entries up to emax, weights at scale x default init, random row counts; only environments whose leading row is
    more than PEAK_MARGIN ahead of every other (in the reference) are kept (at most B), so in fp32 every other row's
    exponential underflows. Random u, the first one 1.0 and the second 0.0.  expect: the leading row wherever u <= 0.999 and the margin
    exceeds 2 tol + 30 (every other row together below 1e-10)."""
    w = make_weights(cols, hidden, seed, scale)
    rng = np.random.default_rng(seed + 1)
    # the leading row: every entry 0 or emax, whichever scores higher (two greedy passes), then a few entries lowered at random
    # per environment; at a random place among rows with entries in the lowest sixteenth of the range (a relu network is close
    # to homogeneous: their logits are about a sixteenth of its own)
    lead = np.full(cols, emax // 2, dtype=np.int32)
    for k in list(range(cols)) * 2:
        two = np.stack([lead, lead]); two[0, k] = 0; two[1, k] = emax
        lead[k] = (0, emax)[int(np.argmax(reference(w, two[None], [2]).logits[0]))]
    cand = rng.integers(0, emax // 16 + 1, size=(4 * B, R, cols)).astype(np.int32)
    rows = rng.integers(2, R + 1, size=4 * B).astype(np.int32)
    leads = np.clip(lead[None, :] - rng.integers(0, emax // 8 + 1, size=(4 * B, cols)) * (rng.random((4 * B, cols)) < 0.25), 0, emax)
    cand[np.arange(4 * B), rng.integers(0, rows)] = leads.astype(np.int32)
    ref = reference(w, cand, rows)
    srt = np.sort(np.where(np.isnan(ref.logits), -np.inf, ref.logits), axis=1)
    keep = np.flatnonzero(srt[:, -1] - srt[:, -2] > PEAK_MARGIN)[:B]
    base = fill_padding(cand[keep], rows[keep], False); rows = rows[keep]
    u = rng.random(len(keep)).astype(np.float32)
    u[:2] = (1.0, 0.0)
    case = Case("peaked %s emax=%d x%.1f" % (label(cols, hidden), emax, scale), w, base, rows, np.arange(len(keep)), u)
    lg = np.where(np.isnan(case.ref.logits), -np.inf, case.ref.logits)
    s = np.sort(lg, axis=1)
    case.margin = s[:, -1] - s[:, -2]
    case.expect = np.where((case.margin > 2 * case.ref.tol() + 30) & (case.u <= 0.999), lg.argmax(axis=1), -1)
    return case


def edge_case(cols, hidden, B, R, rows, seed, garbage):
    """B environments in blocks of R rows with the given row counts (cycled; may exceed R, be 0 or negative), random u."""
    w = make_weights(cols, hidden, seed)
    rows = np.resize(np.array(rows, dtype=np.int32), B)
    base = fill_padding(random_blocks(B, R, cols, seed + 1), rows, garbage, seed + 2)
    u = np.random.default_rng(seed + 3).random(B).astype(np.float32)
    return Case("edges %s B=%d R=%d rows=%s" % (label(cols, hidden), B, R, rows.tolist()[:6]), w, base, rows, np.arange(B), u)


def check_case(case, actions, logprobs, c_l=None, c_s=None):
    """check_draws plus what the case pins: the expected rows, and draws non-decreasing in u within one block."""
    a = np.asarray(actions).astype(np.int64)
    band = check_draws(case.weights, None, None, case.u, a, logprobs, c_l, c_s, ref=case.ref, what=case.name)
    pinned = case.expect >= 0
    bad = pinned & (a != case.expect)
    assert not bad.any(), (case.name, "pinned draws (env, u, action, expected)",
                           [(int(i), float(case.u[i]), int(a[i]), int(case.expect[i])) for i in np.flatnonzero(bad)[:5]], int(bad.sum()))
    for b in np.unique(case.src):
        m = np.flatnonzero(case.src == b)
        order = m[np.argsort(case.u[m], kind="stable")]
        assert (np.diff(a[order]) >= 0).all(), (case.name, "draws decrease while u grows", int(b))
    return band
