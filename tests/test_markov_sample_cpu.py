"""The numpy mirror of the linear-time joint posterior draws (gpcc_amd.markov.prior_draw, sample, MarkovObjective.sample_markov_batch;
DESIGN.md 4.19) against dense algebra on the oracle's matrices, with the dense draws' own bar (tests/_markov_sample_cases.py):

  covariance   a draw is mu + G xi: every unit normal pushed through sample() gives G, and G G' must be the witness's
               C - kB*' K^-1 kB*; the draw of xi = 0 must be the witness's mean.  Every injected mistake must miss that bar.
  Matheron     on the 72 cases of the predictions (N = 110), sample() against mu_pred + g~ - kB*' K^-1 r~ + noise of the same prior draw
  normals      one block per POINT, whatever the merge order; a stream of its own; the mixture's rows are rng.pick_rows
  fit level    Predictor.sample and DelayAveragedPredictor.sample with solver="markov" over MarkovObjective."""
import numpy as np
import pytest

import _markov_cases as MC
import _markov_sample_cases as SC
import _sample_witness as SW
from gpcc_amd import fit, markov, rng

SMALL = SC.small_cases()
CASES = SC.cpu_cases()
_maps = {}


def _draw_map(case, slip=None):
    """(the draw of xi = 0, G) of a case: draw = mean + G xi (cached)."""
    cid, k, data, delays, alpha, rho, mb, tests = case
    if (cid, slip) not in _maps:
        N, T = SC.dims(case)
        zero = np.zeros((N + T + 1, 4))
        base, _, info = markov.sample(k, *data, delays, alpha, rho, tests[0], tests[2], mb, normals=zero, _slip=slip)
        assert info == 0, cid
        G = np.empty((T, 4 * (N + T + 1)))
        for e in range(N + T + 1):
            for c in range(4):
                xi = zero.copy()
                xi[e, c] = 1.0
                G[:, 4 * e + c] = markov.sample(k, *data, delays, alpha, rho, tests[0], tests[2], mb, normals=xi, _slip=slip)[0] - base
        _maps[(cid, slip)] = (base, G)
    return _maps[(cid, slip)]


def test_small_cases_cover_the_ties():
    assert len(SMALL) == 18
    for cid, k, (t, y, s), delays, alpha, rho, mb, (tt, _, st) in SMALL:
        N, T = SC.dims((cid, k, (t, y, s), delays, alpha, rho, mb, (tt, None, st)))
        assert 6 <= N <= 15 and 3 <= T <= 7
        sh = [t[l] - delays[l] for l in range(len(t))]
        ts = [tt[l] - delays[l] for l in range(len(t))]
        assert all(len(np.unique(a)) < len(a) for a in t)                                     # inside a band
        assert all(np.intersect1d(tt[l], t[l]).size for l in range(len(t)))                   # a test point on a training point
        if len(t) > 1:
            assert all(np.intersect1d(sh[0], sh[l]).size and np.intersect1d(sh[0], ts[l]).size for l in range(1, len(t)))


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_covariance_and_mean_against_witness(oracle, kernel):
    wc, wm = MC.Worst("mirror draw covariance %s" % kernel), MC.Worst("mirror draw of zero normals %s" % kernel)
    for case in SMALL:
        if case[1] != kernel:
            continue
        mean, cov, _, cond, _ = SC.witness(oracle, case)
        base, G = _draw_map(case)
        wc.add(float(np.max(np.abs(G @ G.T - cov))), SW.bar(cond, cov), case[0])
        wm.add(float(np.max(np.abs(base - mean))), SW.bar(cond, mean), case[0])
    wc.report()
    wm.report()


# the slips the covariance of a draw can show, and the cases where each one changes anything ("merged_index" permutes the normals: the
# distribution cannot show it, test_point_normals_do_not_follow_the_merge does)
SLIPS = {"no_flip": lambda c: c[1] != "OU", "tie_both": lambda c: True, "no_prior": lambda c: True, "no_obs_noise": lambda c: True,
         "no_offset_draw": lambda c: c[6], "plus": lambda c: True}


@pytest.mark.parametrize("slip", sorted(SLIPS))
def test_bar_catches_slips(oracle, slip):
    """Each mistake misses the bar of the covariance (or of the mean) on at least one small case; by how much is printed."""
    worst, caught, n = 0.0, 0, 0
    for case in SMALL:
        if not SLIPS[slip](case):
            continue
        mean, cov, _, cond, _ = SC.witness(oracle, case)
        base, G = _draw_map(case, slip)
        ratio = max(float(np.max(np.abs(G @ G.T - cov))) / SW.bar(cond, cov), float(np.max(np.abs(base - mean))) / SW.bar(cond, mean))
        worst, caught, n = max(worst, ratio), caught + (ratio > 1.0), n + 1
    print("%s: misses the bar on %d of %d cases, by up to %.3g times" % (slip, caught, n, worst))
    assert caught >= 1


def _process_noise_40_digits(kernel, d, rho):
    """Q(d) = Pinf - A Pinf A' scaled by diag(Pinf)^-1/2, by the difference in 60-digit arithmetic (mpmath)."""
    import mpmath as mp
    mp.mp.dps = 60
    lam = mp.sqrt({"OU": 1, "matern32": 3, "matern52": 5}[kernel]) / mp.mpf(rho)
    d = mp.mpf(d)
    x, e = lam * d, mp.exp(-lam * d)
    if kernel == "OU":
        A, P = mp.matrix([[e]]), mp.matrix([[1]])
    elif kernel == "matern32":
        A, P = e * mp.matrix([[1 + x, d], [-lam * lam * d, 1 - x]]), mp.matrix([[1, 0], [0, lam ** 2]])
    else:
        l2 = lam * lam
        A = e * mp.matrix([[1 + x + x * x / 2, d * (1 + x), d * d / 2], [-l2 * lam * d * d / 2, 1 + x - x * x, d * (1 - x / 2)],
                           [l2 * x * (x / 2 - 1), lam * x * (x - 3), 1 - 2 * x + x * x / 2]])
        P = mp.matrix([[1, 0, -l2 / 3], [0, l2 / 3, 0], [-l2 / 3, 0, lam ** 4]])
    Q = P - A * P * A.T
    n = Q.rows
    return np.array([[float(Q[i, j] / mp.sqrt(P[i, i] * P[j, j])) for j in range(n)] for i in range(n)])


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_process_noise_factor_against_40_digits(kernel):
    """C C' against Q = Pinf - A Pinf A' formed in 60-digit arithmetic, in the units of diag(Pinf), at lags from one grid step to the
    prior and rho = 0.1 .. 300.  Bar: 512 eps of sqrt(Q_ii Q_jj), RELATIVE to the entries -- each integral of process_noise_scaled is
    a sum of positive terms (a few eps), an entry combines up to five of them with coefficients up to 5 (the sum of their magnitudes
    is at most ~12 times the entry for x <= 1), and the last Schur complement of the factor is 1/36 of its diagonal entry:
    12 x 36 eps.  Beyond x = 1, by the difference, Q is of the order of Pinf and eps of Pinf is within the same bar.  Q by the
    difference at every lag ("q_by_difference") misses it by many orders where x is small: at rho = 300 its first pivot is rounding."""
    eps = np.finfo(np.float64).eps
    worst, worst_diff = 0.0, 0.0
    for rho in (0.1, 3.0, 20.0, 300.0):
        lam = markov.rate(kernel, rho)
        sc = 1.0 / np.sqrt(np.diag(markov.stationary(kernel, rho)))
        for d in [2.0 ** -10 * k for k in (1, 3, 17, 100, 256, 277, 301, 1000, 5000)] + [0.3 / lam, 0.999 / lam, 1.001 / lam, 50.0 * rho]:
            Qx = _process_noise_40_digits(kernel, d, rho)
            scale = np.sqrt(np.outer(np.diag(Qx), np.diag(Qx)))
            for diff in (False, True):
                C = markov._sim_factor(kernel, d, rho, diff)
                err = float(np.max(np.abs(sc[:, None] * (C @ C.T) * sc[None, :] - Qx) / scale))
                if diff:
                    worst_diff = max(worst_diff, err)
                else:
                    worst = max(worst, err)
                    assert err <= 512 * eps, (kernel, rho, d, err / eps)
        assert not markov._sim_factor(kernel, 0.0, rho).any()                                 # tied points share one state
        C = markov._sim_factor(kernel, None, rho)
        assert np.allclose(C @ C.T, markov.stationary(kernel, rho), rtol=8 * eps, atol=0)     # the first point: the stationary draw
    print("%s: C C' - Q at most %.3g eps of sqrt(Q_ii Q_jj) (bar 512); Q by the difference: %.3g eps" % (kernel, worst / eps, worst_diff / eps))
    if kernel != "OU":
        assert worst_diff > 512 * eps


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_sample_against_dense_matheron(oracle, kernel):
    w = MC.Worst("mirror draw against the dense Matheron draw %s" % kernel)
    for idx, case in enumerate(CASES):
        cid, k, data, delays, alpha, rho, mb, tests = case
        if k != kernel:
            continue
        kw = dict(seed=77, s=idx, m=(rng.MIXROW if idx % 2 else 3))
        rt, gt, noise = markov.prior_draw(k, *data, delays, alpha, rho, tests[0], tests[2], mb, **kw)
        draw, ll, info = markov.sample(k, *data, delays, alpha, rho, tests[0], tests[2], mb, **kw)
        assert info == 0 and ll == markov.loglik(k, *data, delays, alpha, rho, mb)[0], cid
        ref, b = SC.matheron(oracle, case, rt, gt, noise)
        w.add(float(np.max(np.abs(draw - ref))), b, cid)
    w.report()


def test_point_normals_do_not_follow_the_merge():
    """The normals belong to points: a delay that reorders the merge leaves every point's own noise term as it was.  Indexed by merged
    position ("merged_index") they move."""
    cid, k, (t, y, s), delays, alpha, rho, mb, (tt, _, st) = SMALL[10]            # L = 2
    N, T = sum(map(len, t)), sum(map(len, tt))
    xi = rng.point_normals(5, N + T + 1, [2], [0])[0]
    other = delays + np.array([0.0, 3.0])
    assert markov.merge_order([np.sort(a) for a in t], delays) != markov.merge_order([np.sort(a) for a in t], other)
    sd = np.sqrt(markov.JITTER + np.concatenate(st) ** 2)
    for d in (delays, other):
        rt, gt, noise = markov.prior_draw(k, t, y, s, d, alpha, rho, tt, st, mb, seed=5, s=2, m=0)
        assert np.array_equal(noise, sd * xi[N:N + T, 3])
    a = markov.prior_draw(k, t, y, s, delays, alpha, rho, tt, st, mb, seed=5, s=2, m=0, _slip="merged_index")[2]
    b = markov.prior_draw(k, t, y, s, other, alpha, rho, tt, st, mb, seed=5, s=2, m=0, _slip="merged_index")[2]
    assert not np.array_equal(a, b)
    # explicit normals and the seed's are the same draw
    one = markov.sample(k, t, y, s, delays, alpha, rho, tt, st, mb, seed=5, s=2, m=0)[0]
    assert np.array_equal(one, markov.sample(k, t, y, s, delays, alpha, rho, tt, st, mb, normals=xi)[0])


def test_stream_shares_no_counter_and_keeps_the_old_bits():
    """Counter word 3: 0 for rng.normals, 1 for the row picks, 2 for the point blocks -- whatever the other three words are, the
    counters differ.  The blocks are Philox4x64-10 of (e, s, m, 2) under key (seed, 0), Box-Muller as rng.normals."""
    assert (rng.STREAM_NORMALS, rng.STREAM_PICK, rng.STREAM_POINTS) == (0, 1, 2)
    seed, S = 1234, 3
    z = rng.point_normals(seed, 5, range(S), [rng.MIXROW] * S)
    assert z.shape == (S, 5, 4)
    x = rng.philox4x64(np.array([4, 2, rng.MIXROW, 2], dtype=np.uint64), np.array([seed, 0], dtype=np.uint64))
    u1, u2 = rng.uniform53_open0(x[0]), rng.uniform53(x[1])
    assert z[2, 4, 0] == np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    dense = rng.normals(seed, 20, range(S), [rng.MIXROW] * S).reshape(S, 5, 4)
    assert not np.any(z == dense)
    # the same three leading words in stream 1 give the row picks' word
    pick = rng.philox4x64(np.array([2, 0, rng.MIXROW, 1], dtype=np.uint64), np.array([seed, 0], dtype=np.uint64))
    assert rng.uniform53(pick[0]) == rng.pick_uniforms(seed, S)[2]
    assert not np.array_equal(pick, rng.philox4x64(np.array([2, 0, rng.MIXROW, 2], dtype=np.uint64), np.array([seed, 0], dtype=np.uint64)))


def test_batch_rows_modes_and_codes():
    t, y, s, delays = MC.lightcurves([12, 9], seed=31, kind="ties")
    obj = markov.MarkovObjective(t, y, s, "matern32")
    tt = [np.array([1.0, 7.5, 7.5]), np.array([3.25])]
    D = np.stack([delays, delays + 0.5, delays - 0.25])
    A = np.array([[1.0, 0.7], [1.2, 0.9], [0.8, 1.1]])
    R = np.array([2.0, 3.0, 1.0])
    w = np.array([0.5, 0.0, 1.5])
    draws, rows, ll, info = obj.sample_markov_batch(D, A, R, tt, 6, 9, weights=w)
    assert draws.shape == (6, 4) and np.array_equal(rows, rng.pick_rows(9, 6, w)) and np.isfinite(draws).all()
    assert info[1] == -14 and np.isnan(ll[1]) and info[0] == 0 and info[2] == 0
    for o in range(6):
        assert np.array_equal(draws[o], markov.sample("matern32", t, y, s, D[rows[o]], A[rows[o]], R[rows[o]], tt, seed=9, s=o,
                                                      m=rng.MIXROW)[0])
    A[1, 0] = -1.0
    draws, rows, ll, info = obj.sample_markov_batch(D, A, R, tt, 2, 9)
    assert draws.shape == (6, 4) and np.array_equal(rows, [0, 0, 1, 1, 2, 2]) and list(info) == [0, -1, 0]
    assert np.isnan(draws[2:4]).all() and np.isfinite(draws[:2]).all() and np.isfinite(draws[4:]).all()
    assert np.array_equal(draws[5], markov.sample("matern32", t, y, s, D[2], A[2], R[2], tt, seed=9, s=1, m=2)[0])
    with pytest.raises(ValueError):
        obj.sample_markov_batch(D, A, R, tt, 0, 9)
    with pytest.raises(ValueError):
        obj.sample_markov_batch(D, A, R, tt, 2, 9, weights=[1.0, -1.0, 1.0])


def test_predictors_sample_in_linear_time_without_a_gpu():
    t, y, s, delays = MC.lightcurves([20, 15], seed=32, kind="plain")
    obj = markov.MarkovObjective(t, y, s, "matern52")
    cand = np.stack([np.zeros(3), delays[1] + np.array([-0.5, 0.0, 0.5])], 1)
    alpha, rho = np.array([[1.0, 0.8]] * 3), np.array([2.0, 3.0, 4.0])
    grid = np.linspace(-1.0, 31.0, 5)
    pred = fit.Predictor(obj, cand[1], alpha[1], rho[1], solver="markov")
    out = pred.sample(grid, 4, 11, solver="markov")
    assert len(out) == 2 and all(a.shape == (4, 5) and np.isfinite(a).all() for a in out)
    out = pred.sample([grid, grid[:2]], 3, 11, sigmatest=[np.full(5, 0.1), np.full(2, 0.2)], solver="markov")
    assert [a.shape for a in out] == [(3, 5), (3, 2)] and all(np.isfinite(a).all() for a in out)
    avg = fit.DelayAveragedPredictor(obj, cand, alpha, rho, [0.2, 0.5, 0.3], solver="markov")
    bands, rows = avg.sample(grid, 5, 12, solver="markov")
    assert [a.shape for a in bands] == [(5, 5), (5, 5)] and all(np.isfinite(a).all() for a in bands)
    assert np.array_equal(rows, rng.pick_rows(12, 5, [0.2, 0.5, 0.3]))
    with pytest.raises(ValueError):
        pred.sample(grid, 2, 1, solver="sparse")
    with pytest.raises(AttributeError):
        pred.sample(grid, 2, 1)                         # solver None stays dense: the mirror has no dense draws
