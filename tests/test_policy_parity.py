"""The PMLP policy kernels on the device against the float64 reference of tests/policy_cases.py (tests/test_policy_cases_cpu.py
checks reference, checker and builders on the CPU): bbx_pmlp_act / bbx_pmlp2_act / bbx_pmlp3_act through PMLPPolicy.act at every
boundary of their instantiation tables and tiles, the later rounds of the deep kernels' grid-stride loop, the prepared weights
element by element, and the same tile code inside the step kernels.  Every draw is held to check_draws: the action admissible
for its uniform number, the log-probability within tol of the reference — tolerances that scale with the network's own
magnitude (C_L, C_S: policy_cases.py).  Each case prints the ratios it needed before it asserts (pytest -s)."""
import numpy as np
import pytest

from tests import policy_cases as pc

pytestmark = pytest.mark.gpu
_ids = lambda v: str(v).replace(" ", "")


def _act(case):
    """The case through PMLPPolicy.act on the device — through the HIP kernel of its depth, never the torch path."""
    import torch
    pol = pc.to_policy(case.weights, "cuda")
    cols, R = case.base.shape[2], case.base.shape[1]
    hidden = [l.out_features for l in pol.embedding]
    assert (len(hidden) == 1 and pol.fused_ok(cols, hidden[0]) and R <= 2048) or (pol.deep_ok(cols) and R <= pol.deep_max_rows()), "no kernel for this case"
    base = torch.from_numpy(case.base).cuda()
    obs = base[torch.from_numpy(case.src).cuda()].contiguous()
    rows = torch.from_numpy(case.rows.astype(np.int32)).cuda(); u = torch.from_numpy(case.u).cuda()
    a = torch.full((len(case.src),), -7, dtype=torch.int32, device="cuda"); l = torch.full((len(case.src),), float("nan"), device="cuda")
    pol.act(obs, rows, u, a, l)
    torch.cuda.synchronize()
    return a.cpu().numpy(), l.cpu().numpy()


def _check(case, a, l):
    r_l, r_s, r_raw = pc.ratios(case.ref, case.u, a, l)
    lerr = pc.draw_errors(case.ref, case.u, np.clip(a, 0, None), l)[0].max(initial=0.0)
    print("ratios %-60s B=%-5d r_l=%.3f r_s=%.3f (without the logit term: %.3f) max |logprob error| %.2e" % (case.name, len(case.u), r_l, r_s, r_raw, lerr))
    return pc.check_case(case, a, l)


def _run(case):
    return _check(case, *_act(case))


# ---- every instantiation boundary: row sweeps and block edges ----------------------------------------------------------------
def _shape_cases(cols, hidden, seed):
    """Row sweep over LIVE_ROWS twice (-1 padding in blocks of exactly 129 rows: obs_rows == rows for the tallest; garbage
    padding in blocks of 136), then the block edges: obs_rows 1 (B = 1), obs_rows 15 with rows above it, 0 and -3 (B = 5), rows
    40 in blocks of 24 next to 0, -3 and tile-edge counts (B = 9)."""
    yield pc.row_sweep(cols, hidden, pc.LIVE_ROWS, seed, R=129, garbage=False)
    yield pc.row_sweep(cols, hidden, pc.LIVE_ROWS, seed + 10, R=136, garbage=True)
    yield pc.edge_case(cols, hidden, 1, 1, (1,), seed, False)
    yield pc.edge_case(cols, hidden, 1, 1, (5,), seed + 1, True)
    yield pc.edge_case(cols, hidden, 5, 15, (15, 0, 7, -3, 20), seed + 2, True)
    yield pc.edge_case(cols, hidden, 9, 24, (40, 0, 24, -3, 1, 15, 16, 17, 40), seed + 3, False)
    yield pc.edge_case(cols, hidden, 9, 24, (0, 40, -3, 24, 23, 2, 17, 0, 9), seed + 4, True)


@pytest.mark.parametrize("cols,hidden", pc.one_layer_shapes() + pc.two_layer_shapes() + pc.three_layer_shapes(), ids=_ids)
def test_kernel_draws_every_row_at_every_instantiation_boundary(cols, hidden):
    """Per shape: the row sweep (copy j of a block gets the uniform in the middle of row j's reference interval: the draw is
    row j, its log-probability the reference's — EVERY row's logit is looked at, not the drawn one's) at every live-row count
    around the tiles of 16 and 32 rows and the wave of 64, and the obs_rows / rows / batch edges.  No draw of a sweep may
    need the delta band except on an unpinned row; at most 5 % of its rows may be unpinned (policy_cases.sweep_case)."""
    for case in _shape_cases(cols, hidden, 100):
        band = _run(case)
        if case.name.startswith("sweep"):
            assert case.skipped <= 0.05 and band <= (case.expect < 0).sum(), (case.name, case.skipped, band)


TALL = [((128,), n) for n in pc.TALL_ROWS] + [((128, 128), n) for n in pc.TALL_ROWS] + \
       [((128, 128, 128), n) for n in pc.TALL_ROWS[:2]] + [((64, 64, 64), n) for n in pc.TALL_ROWS[2:]]


@pytest.mark.parametrize("hidden,n", TALL, ids=_ids)
def test_row_sweep_on_tall_blocks(hidden, n):
    """1023 .. 2048 live rows (three layers wider than 64 units: up to their ceiling of 1024, the taller counts at 64 units),
    the deciding layer flattened (x 0.03) so that every row keeps a probability near 1 / n: n copies, row j drawn in copy j."""
    case = pc.row_sweep(12, hidden, (n,), 200, decide_scale=0.03)
    band = _run(case)
    assert case.skipped <= 0.05 and band <= (case.expect < 0).sum(), (case.skipped, band)


# ---- ties, monotone draws, CDF boundaries, peaked and large inputs -----------------------------------------------------------
DEPTH_SHAPES = [(12, (128,)), (12, (128, 128)), (12, (128, 128, 128))]
ODD_COLS_SHAPES = [s for s in pc.one_layer_shapes() + pc.two_layer_shapes() + pc.three_layer_shapes() if s[0] in (13, 33)]


@pytest.mark.parametrize("cols,hidden", DEPTH_SHAPES + ODD_COLS_SHAPES, ids=_ids)
def test_ties_monotone_draws_and_cdf_boundaries(cols, hidden):
    """Identical rows on a grid of 4n + 1 uniforms (draw floor(u n), log-probability -log n; with n a power of two the kernel's
    arithmetic is exact and u = j / n must draw row j, u = 1.0 the last row: a '>=' for the '>' of the inverse CDF fails
    here); 1024 sorted uniforms from 0.0 to 1.0 on one block (draws never decrease, u = 0 draws row 0, u = 1.0 the last);
    and uniforms a few units of 2^-24 to either side of every CDF boundary (where the kernel's own boundary lies)."""
    for n, R in ((16, 16), (33, 40), (64, 64), (129, 129), (256, 300)):
        _run(pc.tie_case(cols, hidden, n, 300 + n, R=R))
    for n in (40, 129):
        _run(pc.monotone_case(cols, hidden, n, 400 + n))
    for n in (33, 129):
        _run(pc.boundary_case(cols, hidden, n, 500 + n))


PEAKED_SHAPES = DEPTH_SHAPES + [(13, (255,)), (33, (32,)), (13, (17, 128)), (33, (128, 128, 128))]


@pytest.mark.parametrize("emax,scale", pc.PEAKED)
@pytest.mark.parametrize("cols,hidden", PEAKED_SHAPES, ids=_ids)
def test_peaked_and_large_inputs(cols, hidden, emax, scale):
    """Exponent entries up to 255 / 65535 under weights at 1.0 x / 3.0 x default init, one row more than 100 ahead: every
    other row's __expf underflows, the leading row is drawn with log-probability ~0, u = 1.0 draws the last row with ITS
    log-probability; tol scales with the network's magnitude (S_r), which is why the checker carries it."""
    case = pc.peaked_case(cols, hidden, emax, scale, 600)
    assert len(case.u) >= 8, len(case.u)
    _run(case)


# ---- the later rounds of the deep kernels' grid-stride loop ------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [(64, 64), (128, 128), (128, 128, 128)], ids=_ids)
def test_deep_kernels_beyond_one_round_of_the_grid(hidden):
    """B = 16 CUs + 27: the launcher caps the grid at 2 x CUs workgroups of 8 waves (1 x CUs of 16), so 27 environments run in
    a second round of bbx_pmlp2_act_kernel's loop — the non-prefetch path that reuses the workgroup's queue and row counts
    across barriers.  Even environments have one tile of rows, odd ones three, and the last 64 environments are copies (block,
    rows, u) of the first 64: a wave slot that scored one tile in round 0 scores three in round 1 and the reverse, and the
    copies must return the same bits in whichever round they land."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, R, cols = 16 * cus + 27, 48, 12
    e = np.arange(B)
    rows = np.where(e % 2 == 0, 1 + (e * 7) % 16, 33 + (e * 5) % 16).astype(np.int32)
    src = e.copy(); src[B - 64:] = np.arange(64)
    w = pc.make_weights(cols, hidden, 700)
    base = pc.fill_padding(pc.random_blocks(B, R, cols, 701), rows, True, 702)
    u = np.random.default_rng(703).random(B).astype(np.float32)
    case = pc.Case("later rounds %s B=%d" % (pc.label(cols, hidden), B), w, base, rows, src, u[src])
    assert (B - 64) % 2 == 1 and np.array_equal(case.rows[B - 64:], rows[:64])
    a, l = _act(case)
    band = _check(case, a, l)
    assert band <= pc.near_boundary(case.ref, case.u) + 2
    assert np.array_equal(a[B - 64:], a[:64]) and np.array_equal(l[B - 64:].view(np.int32), l[:64].view(np.int32))


# ---- the prepared weights, element by element --------------------------------------------------------------------------------
def _ks1(cols): return next(k for k in (3, 6, 10, 16, 32) if (cols + 1) // 2 <= k)
def _nb(hidden): return next(k for k in (1, 2, 4, 8) if (hidden + 31) // 32 <= k)
def _ks2(cols): return next(k for k in (3, 8, 16) if (cols + 3) // 4 <= k)
def _hp(hidden): return 64 if hidden <= 64 else 128


def _padded(W, r, c):
    out = np.zeros((r, c), dtype=np.float32); out[:W.shape[0], :W.shape[1]] = W
    return out


def _permuted(W, HPI, HPO):
    """A[blk][s4][lane][j] = W[k(4 s4 + j, lane >> 4)][16 blk + (lane & 15)],  k(s, g) = 16 (s >> 2) + 4 g + (s & 3)  (bbx_pmlp2.hip)"""
    Wp = _padded(W, HPI, HPO)
    blk, s4, lane, j = np.meshgrid(np.arange(HPO // 16), np.arange(HPI // 16), np.arange(64), np.arange(4), indexing="ij")
    s = 4 * s4 + j
    return Wp[16 * (s >> 2) + 4 * (lane >> 4) + (s & 3), 16 * blk + (lane & 15)].reshape(-1)


def _vec(b, n):
    out = np.zeros(n, dtype=np.float32); out[:len(b)] = b
    return out


@pytest.mark.parametrize("hidden", [31, 33, 100, 255])                # blocks of 32 units: 1 | 2 | 4 | 8
@pytest.mark.parametrize("cols", [5, 11, 13, 21, 33])                 # k-steps of two columns: 3 | 6 | 10 | 16 | 32
def test_prepared_weights_of_one_layer_are_the_documented_layout(cols, hidden):
    """bbx_pmlp_prepare's output read back, against bbx_pmlp_shape.h: W1p [2 KS][32 NB] | b1p [32 NB] | w2p [32 NB] | b2 | pad to
    a multiple of 4 — every float, the zero padding included."""
    w = pc.make_weights(cols, (hidden,), 800, scale=1.0)
    got = pc.to_policy(w, "cuda")._fused_weights()["keep"].cpu().numpy()
    K2, HP = 2 * _ks1(cols), 32 * _nb(hidden)
    want = np.concatenate([_padded(w[0][0], K2, HP).reshape(-1), _vec(w[0][1], HP), _vec(w[1][0], HP), _vec(w[1][1], 4)])
    assert got.shape == want.shape == ((K2 + 2) * HP + 4,)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.flatnonzero(got != want)[:8]


@pytest.mark.parametrize("hidden", [(17, 60), (65, 64), (64, 100), (128, 127), (10, 20, 30), (64, 65, 17), (128, 3, 5)], ids=_ids)
@pytest.mark.parametrize("cols", [5, 13, 33])                         # k-steps of four columns: 3 | 8 | 16
def test_prepared_weights_of_the_deep_kernels_are_the_documented_layout(cols, hidden):
    """bbx_pmlp2_prepare / bbx_pmlp3_prepare read back, against bbx_pmlp_shape.h and the head of bbx_pmlp2.hip:
    W1p [4 KS][HP1] | b1p [HP1] | [AM [HPM / 16][HP1 / 16][64][4]] | A2 [HP2 / 16][HPI / 16][64][4] | [bMp [HPM]] | b2p [HP2] | wdp [HP2] |
    bd, pad — the lane permutation of the matrices behind the first, every padding float, the bd / pad tail.  Two layers are
    padded to 64 or 128 units one by one, three all to the widest."""
    w = pc.make_weights(cols, hidden, 801, scale=1.0)
    got = pc.to_policy(w, "cuda")._deep_weights()["keep"][0].cpu().numpy()
    K1 = 4 * _ks2(cols)
    if len(hidden) == 2:
        HP1, HPM, HP2 = _hp(hidden[0]), 0, _hp(hidden[1])
        mid = []
    else:
        HP1 = HPM = HP2 = _hp(max(hidden))
        mid = [_permuted(w[1][0], HP1, HPM)]
    HPI = HPM or HP1
    want = np.concatenate([_padded(w[0][0], K1, HP1).reshape(-1), _vec(w[0][1], HP1)] + mid + [_permuted(w[-2][0], HPI, HP2)] +
                          ([_vec(w[1][1], HPM)] if HPM else []) + [_vec(w[-2][1], HP2), _vec(w[-1][0], HP2), _vec(w[-1][1], 4)])
    assert got.shape == want.shape == ((K1 + 1) * HP1 + HP1 * HPM + HPI * HP2 + HPM + 2 * HP2 + 4,)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.flatnonzero(got != want)[:8]


# ---- the policy inside the step kernels ----------------------------------------------------------------------------------------
# the number of draws the reference predicts the delta band may decide (u within delta of a CDF boundary) for the seeds below,
# per path: stated in the test's docstring, asserted as a cap (+ 2).  Unmeasured so far, like C_L and C_S: placeholders
PREDICTED_BAND = {"step": 0, "rollout": 0, "rollout-lds16": 0, "rollout-5var": 0, "rollout2-128x128": 0, "rollout2-100x48": 0}
STEP_PATHS = [("step", "3-20-10-weighted", 2, (128,), None, 64), ("rollout", "3-20-10-weighted", 2, (128,), None, 64),
              ("rollout-lds16", "3-20-10-weighted", 2, (128,), {"lds_max_basis": 16}, 64), ("rollout-5var", "5-10-5-uniform", 1, (64,), None, 256),
              ("rollout2-128x128", "3-20-10-weighted", 2, (128, 128), None, 64), ("rollout2-100x48", "3-20-10-weighted", 2, (100, 48), None, 64)]


@pytest.mark.parametrize("path,dist,k,hidden,caps,R", STEP_PATHS, ids=[p[0] for p in STEP_PATHS])
def test_policy_inside_the_step_kernels_against_the_reference(path, dist, k, hidden, caps, R):
    """B = 64 environments, T = 24 steps; every step's (block, row counts, u, action, log-probability) through check_draws:
    bbx_policy_step_device (the fused register/LDS-resident class), bbx_policy_rollout_device with default capacities
    (environments move to the HBM-resident kernel mid-launch) and with the register/LDS class capped at 16 basis elements,
    the HBM-resident kernel from the start (5-10-5-uniform), bbx_policy2_rollout_device with (128, 128) and (100, 48).
    Draws the reference predicts within delta of a CDF boundary for these seeds, and so the cap on draws only the delta
    band admits (+ 2): step 0, rollout 0, rollout-lds16 0, rollout-5var 0, rollout2-128x128 0, rollout2-100x48 0 — PLACEHOLDERS
    until the test has run on an MI355X (it prints the predicted count; the blocks depend on the actions drawn there)."""
    import torch
    from deepgroebner_amd import VecLeadMonomialsEnv
    B, T = 64, 24
    env = VecLeadMonomialsEnv(dist, batch=B, k=k, caps=caps)
    env.seed(np.arange(B) + 900); env.reset(); env.accounting(False)
    w = pc.make_weights(env.cols, hidden, 901)
    pol = pc.to_policy(w, "cuda")
    s = torch.cuda.current_stream().cuda_stream
    u = torch.rand((T, B), device="cuda", generator=torch.Generator(device="cuda").manual_seed(902))
    A = torch.zeros((T, B), dtype=torch.int32, device="cuda"); L = torch.zeros((T, B), dtype=torch.float32, device="cuda")
    N = torch.zeros((T, B), dtype=torch.int32, device="cuda")
    O = torch.full((T, B, R, env.cols), -1, dtype=torch.int32, device="cuda")
    if path == "step":
        p = pol._fused_weights()
        rew = torch.zeros(B, dtype=torch.float64, device="cuda"); done = torch.zeros(B, dtype=torch.uint8, device="cuda")
        obs = torch.full((B, R, env.cols), -1, dtype=torch.int32, device="cuda"); rows = torch.zeros(B, dtype=torch.int32, device="cuda")
        env.rollout_device("first", 0, False, s, rew, done, rows, obs, R, True, False); env.sync()
        for t in range(T):
            O[t].copy_(obs); N[t].copy_(rows)
            env.policy_step_device(p["prepared"], p["hidden"], u[t], A[t], L[t], rew, done, rows, obs, R, 1, s)
            env.sync()
    elif len(hidden) == 1:
        p = pol._fused_weights()
        env.policy_rollout_device(p["prepared"], p["hidden"], T, u, A, L, None, None, N, O, R, B * R * env.cols, s)
        env.sync()
    else:
        p = pol._deep_weights()
        env.policy2_rollout_device(p["prepared"], p["hidden"][0], p["hidden"][1], T, u, A, L, None, None, N, O, R, B * R * env.cols, s)
        env.sync()
    torch.cuda.synchronize()
    obs, rows = O.reshape(T * B, R, env.cols).cpu().numpy(), N.reshape(-1).cpu().numpy()
    uu, a, l = u.reshape(-1).cpu().numpy(), A.reshape(-1).cpu().numpy(), L.reshape(-1).cpu().numpy()
    assert rows.min() >= 1 and rows.max() <= R and len(np.unique(rows)) > 5
    ref = pc.reference(w, obs, rows)
    r_l, r_s, r_raw = pc.ratios(ref, uu, a, l)
    predicted = pc.near_boundary(ref, uu)
    print("ratios %-60s B=%-5d r_l=%.3f r_s=%.3f (without the logit term: %.3f) near a boundary: %d" % ("step kernels " + path, T * B, r_l, r_s, r_raw, predicted))
    band = pc.check_draws(w, obs, rows, uu, a, l, ref=ref, what=path)
    print("band %s: %d" % (path, band))
    assert band <= PREDICTED_BAND[path] + 2, (band, predicted)
