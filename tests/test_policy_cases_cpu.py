"""tests/policy_cases.py on the CPU: the float64 reference against an independent evaluation (the torch module in double
precision), every case builder against what it claims, and check_draws against planted errors — on a plain float32 numpy
evaluation standing in for the kernels (tests/test_policy_parity.py runs the same checker on the MI355X)."""
import numpy as np
import pytest

from tests import policy_cases as pc

CEIL = pc.C_CEILING


def _mixed(cols, hidden, seed, B=7, R=24):
    w = pc.make_weights(cols, hidden, seed)
    rows = np.resize(np.array([1, 5, 16, 17, 24, 40, 0], dtype=np.int32), B)
    obs = pc.fill_padding(pc.random_blocks(B, R, cols, seed + 1), rows, False)
    u = np.random.default_rng(seed + 2).random(B).astype(np.float32)
    return w, obs, rows, u


# ---- the reference against an independent evaluation -------------------------------------------------------------------------
@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (7, (33,)), (12, (128, 128)), (13, (65, 17)), (33, (64, 65, 17))])
def test_reference_equals_the_torch_module_in_double_precision(cols, hidden):
    """PMLPPolicy(...).double() on the CPU masks by the -1 padding, the reference by the row count: on -1-padded blocks whose
    rows fit, the log-softmax over the live rows agrees to 1e-12, and act_torch in float64 draws the same rows on random u."""
    import torch
    w, obs, rows, u = _mixed(cols, hidden, 5)
    rows = np.clip(rows, 1, obs.shape[1]).astype(np.int32)
    obs = pc.fill_padding(obs, rows, False)
    ref = pc.reference(w, obs, rows)
    pol = pc.to_policy(w, dtype=torch.float64)
    for got, want in zip(pc.weights_of(pol), w):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    pol.forward = lambda batch, f=pol.forward: f(batch.to(torch.float64))      # (the module casts its input to float32)
    x = torch.from_numpy(obs).to(torch.float64)
    for layer in pol.embedding:
        x = torch.relu(layer(x))
    lg = pol.deciding(x).squeeze(-1)
    for e in range(len(rows)):
        n = int(rows[e])
        lp = torch.log_softmax(lg[e, :n], dim=0).detach().numpy()
        assert np.abs(lp - ref.logsm[e, :n]).max() <= 1e-12
        assert np.isnan(ref.logsm[e, n:]).all() and abs(ref.cdf[e, n - 1] - 1.0) < 1e-12
    # the draws of act_torch, double precision end to end
    lp = torch.log_softmax(lg + (torch.arange(obs.shape[1])[None, :] >= torch.from_numpy(rows)[:, None].long()) * -1e9, dim=1)
    p = torch.exp(lp)
    cdf = torch.cumsum(p, dim=1).detach().numpy()
    uu = np.random.default_rng(9).random((50, len(rows)))
    for k in range(50):
        a = np.minimum((cdf <= uu[k][:, None] * cdf[:, -1:]).sum(axis=1), rows - 1)
        l = lp.detach().numpy()[np.arange(len(rows)), a]
        assert pc.check_draws(w, obs, rows, uu[k], a, l, c_l=1e-3, c_s=1e-3, ref=ref) == 0


def test_reference_masks_by_the_row_count_not_by_the_padding():
    """Garbage, -1 or live-looking rows beyond the count change nothing; rows above the block or above 2048 are clamped; rows
    <= 0 leave an environment without rows."""
    w, obs, rows, u = _mixed(12, (64,), 3)
    a = pc.reference(w, pc.fill_padding(obs, rows, False), rows)
    b = pc.reference(w, pc.fill_padding(obs, rows, True), rows)
    for x, y in ((a.logsm, b.logsm), (a.cdf, b.cdf), (a.scale, b.scale)):
        assert np.array_equal(x, y, equal_nan=True)
    assert a.n.tolist() == [1, 5, 16, 17, 24, 24, 0]
    assert pc.reference(w, obs, np.full(7, -3)).n.tolist() == [0] * 7
    tall = pc.reference(pc.make_weights(2, (4,), 1), pc.random_blocks(1, 2100, 2, 1), [2100])
    assert tall.n[0] == 2048 and tall.cdf.shape[1] == 2048
    assert (a.scale[a.scale > 0] >= np.abs(a.logits[a.scale > 0])).all()


# ---- the builders are what they claim ----------------------------------------------------------------------------------------
def test_edge_lists_hold_every_value_of_the_instantiation_table():
    from_header = lambda f, vals: sorted({f(v) for v in vals})
    ks1 = lambda c: next(k for k in (3, 6, 10, 16, 32) if (c + 1) // 2 <= k)
    ks2 = lambda c: next(k for k in (3, 8, 16) if (c + 3) // 4 <= k)
    nb = lambda h: next(k for k in (1, 2, 4, 8) if (h + 31) // 32 <= k)
    assert pc.ONE_COLS == (1, 2, 6, 7, 12, 13, 20, 21, 32, 33, 63, 64) and from_header(ks1, pc.ONE_COLS) == [3, 6, 10, 16, 32]
    assert pc.ONE_HIDDEN == (1, 31, 32, 33, 64, 65, 128, 129, 255, 256) and from_header(nb, pc.ONE_HIDDEN) == [1, 2, 4, 8]
    assert pc.TWO_COLS == (1, 12, 13, 32, 33, 64) and from_header(ks2, pc.TWO_COLS) == [3, 8, 16]
    assert pc.TWO_HIDDEN == ((1, 1), (64, 64), (65, 64), (64, 65), (17, 128), (128, 128))
    assert pc.THREE_HIDDEN == ((1, 1, 1), (64, 64, 64), (64, 65, 17), (128, 128, 128)) and pc.THREE_COLS == (12, 33, 64)
    assert pc.LIVE_ROWS == (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129) and pc.TALL_ROWS == (1023, 1024, 1025, 2047, 2048)
    assert pc.BATCHES == (1, 5, 9)
    one, two, three = pc.one_layer_shapes(), pc.two_layer_shapes(), pc.three_layer_shapes()
    assert {c for c, _ in one} == set(pc.ONE_COLS) and {h[0] for _, h in one} == set(pc.ONE_HIDDEN)
    assert {(1, (1,)), (1, (256,)), (64, (1,)), (64, (256,))} <= set(one)
    assert {c for c, _ in two} == set(pc.TWO_COLS) and {h for _, h in two} == set(pc.TWO_HIDDEN)
    assert {c for c, _ in three} == set(pc.THREE_COLS) and {h for _, h in three} == set(pc.THREE_HIDDEN)
    assert len(set(one)) == len(one) and len(set(two)) == len(two) and len(set(three)) == len(three)


@pytest.mark.parametrize("cols,hidden", pc.one_layer_shapes() + pc.two_layer_shapes() + pc.three_layer_shapes(), ids=lambda v: str(v).replace(" ", ""))
def test_row_sweep_skips_at_most_five_per_cent_at_the_ceiling(cols, hidden):
    """With delta at C_L = C_S = 64 (the ceiling) the reference alone leaves at most 5 % of a case's rows unpinned, every
    live row count is there once per row, and the pinned uniforms lie strictly inside their rows' intervals."""
    case = pc.row_sweep(cols, hidden, pc.LIVE_ROWS, 11, garbage=True, c_l=CEIL, c_s=CEIL)
    assert case.skipped <= 0.05, case.skipped
    assert len(case.src) == sum(pc.LIVE_ROWS) and np.array_equal(np.bincount(case.src), pc.LIVE_ROWS)
    F = np.concatenate([np.zeros((len(case.src), 1)), case.ref.cdf], axis=1)
    e = np.flatnonzero(case.expect >= 0)
    j = case.expect[e]
    d = case.ref.delta(CEIL, CEIL)[e]
    assert (case.u[e] - F[e, j] >= d * 0.99).all() and (F[e, j + 1] - case.u[e] >= d * 0.99).all()


@pytest.mark.parametrize("n", pc.TALL_ROWS)
@pytest.mark.parametrize("hidden", [(128,), (128, 128), (64, 64, 64)])
def test_tall_row_sweep_stays_inside_the_cap_with_a_flattened_deciding_layer(hidden, n):
    case = pc.row_sweep(12, hidden, (n,), 13, decide_scale=0.03, c_l=CEIL, c_s=CEIL)
    assert case.skipped <= 0.05, case.skipped
    assert len(case.u) == n


def test_tie_rows_are_identical_and_the_grid_pins_what_it_says():
    for n in (5, 16, 33):
        case = pc.tie_case(12, (64,), n, 3, R=40)
        assert (case.base[0, :n] == case.base[0, 0]).all() and (case.base[0, n:] == -1).all()
        assert len(case.u) == 4 * n + 1 and case.u[0] == 0.0 and case.u[-1] == 1.0
        assert np.abs(case.ref.logsm[0, :n] + np.log(n)).max() < 1e-12
        g = np.arange(4 * n + 1)
        inner = g % 4 != 0
        assert np.array_equal(case.expect[inner], g[inner] // 4)
        assert (case.expect[~inner] >= 0).all() == (n == 16)
        if n == 16:
            assert case.expect[-1] == n - 1 and np.array_equal(case.expect[~inner][:-1], g[~inner][:-1] // 4)


def test_monotone_and_boundary_cases():
    case = pc.monotone_case(13, (65,), 33, 4)
    assert len(case.u) == 1024 and (np.diff(case.u) >= 0).all() and case.u[0] == 0.0 and case.u[-1] == 1.0
    assert case.u[-2] == np.nextafter(np.float32(1), np.float32(0)) and case.expect[0] == 0 and case.expect[-1] == 32
    case = pc.boundary_case(12, (128,), 33, 4)
    assert len(case.u) == 32 * len(pc.BOUNDARY_OFFSETS) and (case.u >= 0).all() and (case.u < 1).all()
    k0 = pc.BOUNDARY_OFFSETS.index(0)
    assert np.array_equal(case.u.reshape(32, -1)[:, k0], np.float32(case.ref.cdf[0, :32]))


@pytest.mark.parametrize("emax,scale", pc.PEAKED)
@pytest.mark.parametrize("cols,hidden", [(12, (128,)), (13, (128, 128)), (33, (128, 128, 128))])
def test_peaked_cases_underflow_in_float32(cols, hidden, emax, scale):
    case = pc.peaked_case(cols, hidden, emax, scale, 21)
    assert len(case.u) >= 16 and int(case.base.max()) > emax * 0.9
    assert (case.margin > pc.PEAK_MARGIN).all()
    assert (np.exp(-case.margin.astype(np.float32)) < np.finfo(np.float32).tiny).all()      # below the normal range: flushed
    a, l = pc.act_float32(*case.as_tuple())
    p = np.exp(l[case.u < 0.999].astype(np.float64))
    assert (p == 1.0).all()                                       # (every other row's exponential is gone in float32)


# ---- the checker ---------------------------------------------------------------------------------------------------------------
def _sweep(cols=12, hidden=(128,), seed=31, rows=(15, 16, 17, 33, 40)):
    return pc.row_sweep(cols, hidden, rows, seed, R=48, c_l=CEIL, c_s=CEIL)


@pytest.mark.parametrize("hidden", [(128,), (100, 48), (64, 65, 17)])
def test_checker_accepts_the_float32_evaluation(hidden):
    """The untouched stand-in passes every case kind at the ceiling constants, with no draw left to the delta band on random
    uniforms."""
    for case in (_sweep(hidden=hidden), pc.tie_case(12, hidden, 16, 2), pc.tie_case(12, hidden, 33, 2), pc.monotone_case(12, hidden, 40, 2),
                 pc.boundary_case(12, hidden, 33, 2), pc.edge_case(12, hidden, 9, 24, (40, 0, 24, -3, 1, 15), 2, True),
                 pc.peaked_case(12, hidden, 255, 3.0, 2), pc.peaked_case(12, hidden, 65535, 1.0, 2)):
        a, l = pc.act_float32(*case.as_tuple())
        band = pc.check_case(case, a, l, CEIL, CEIL)
        if not case.name.startswith(("boundaries", "ties")):
            assert band <= 1, (case.name, band)
        r_l, r_s, r_s_raw = pc.ratios(case.ref, case.u, a, l, CEIL)
        assert r_l <= CEIL and r_s == 0.0, (case.name, r_l, r_s, r_s_raw)


def test_checker_rejects_an_action_shifted_by_one():
    case = _sweep()
    a, l = pc.act_float32(*case.as_tuple())
    i = int(np.flatnonzero((case.expect >= 1) & (case.expect < case.ref.n - 1))[7])
    for d in (1, -1):
        b = a.copy(); b[i] += d
        lb = l.copy(); lb[i] = case.ref.logsm[i, b[i]]            # (with that row's own log-probability: only the draw is wrong)
        with pytest.raises(AssertionError, match="not admissible"):
            pc.check_draws(*case.as_tuple(), b, lb, CEIL, CEIL)
    b = a.copy(); b[i] = case.ref.n[i]
    with pytest.raises(AssertionError, match="outside the rows"):
        pc.check_draws(*case.as_tuple(), b, l, CEIL, CEIL)


def test_checker_rejects_a_log_probability_off_by_ten_tolerances():
    case = _sweep()
    a, l = pc.act_float32(*case.as_tuple())
    for sign in (1, -1):
        lb = l.copy(); lb[11] += sign * 10 * case.ref.tol(CEIL)[11]
        with pytest.raises(AssertionError, match="log-probability"):
            pc.check_draws(*case.as_tuple(), a, lb, CEIL, CEIL)


def test_checker_rejects_rows_without_an_environment_that_report_something():
    case = pc.edge_case(12, (64,), 5, 24, (3, 0, -3, 24, 40), 1, False)
    a, l = pc.act_float32(*case.as_tuple())
    assert pc.check_case(case, a, l, CEIL, CEIL) == 0
    for arr, v in ((a, 1), (l, -0.5)):
        x = arr.copy(); x[2] = v
        with pytest.raises(AssertionError, match="no rows"):
            pc.check_draws(*case.as_tuple(), *((x, l) if arr is a else (a, x)), CEIL, CEIL)


@pytest.mark.parametrize("hidden", [(128,), (100, 48), (64, 65, 17)])
def test_checker_rejects_planted_arithmetic_errors(hidden):
    """A stand-in evaluation with one hidden unit's deciding weight zeroed, with the last column dropped, with the row count cut
    at the tile boundary: each fails the row sweep held against the true weights, block and rows."""
    case = _sweep(hidden=hidden)
    w, obs, rows, u = case.as_tuple()
    x = obs[0, :int(rows[0])].astype(np.float64)
    for W, b in w[:-1]:
        x = np.maximum(x @ W + b, 0.0)
    wd = w[-1][0].copy()
    h = int(np.argmax(np.abs(wd) * x.std(axis=0)))                # the unit that tells the first block's rows apart most
    wd[h] = 0.0
    with pytest.raises(AssertionError):
        pc.check_case(case, *pc.act_float32(w[:-1] + [(wd, w[-1][1])], obs, rows, u), CEIL, CEIL)
    cut = obs.copy(); cut[:, :, -1] = 0
    with pytest.raises(AssertionError):
        pc.check_case(case, *pc.act_float32(w, cut, rows, u), CEIL, CEIL)
    with pytest.raises(AssertionError):
        pc.check_case(case, *pc.act_float32(w, obs, np.minimum(rows, 16 * ((rows - 1) // 16)), u), CEIL, CEIL)
    pc.check_case(case, *pc.act_float32(w, obs, rows, u), CEIL, CEIL)


def test_checker_rejects_an_off_by_one_at_an_exact_boundary():
    """Ties over a power of two of rows: u = j / n must draw row j (">" in "cumulative probability exceeds u"), which a ">="
    gets wrong although both rows are admissible within delta."""
    case = pc.tie_case(12, (128,), 16, 2)
    a, l = pc.act_float32(*case.as_tuple())
    pc.check_case(case, a, l, CEIL, CEIL)
    b = a.copy(); b[8] -= 1                                       # u = 2 / 16 drawing row 1
    with pytest.raises(AssertionError, match="pinned"):
        pc.check_case(case, b, l, CEIL, CEIL)


def test_constants_are_powers_of_two_under_the_ceiling():
    for c, r in ((pc.C_L, pc.R_L), (pc.C_S, pc.R_S)):
        assert c <= pc.C_CEILING and np.log2(c) == int(np.log2(c))
        if r is not None:
            assert c >= 4 * r and (c / 2 < 4 * r or c == 1.0)
        else:
            assert c == pc.C_CEILING
