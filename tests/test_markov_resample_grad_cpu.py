"""The gradient of rows with their own resampled data set on the CPU (gpcc_amd.markov.loglik_grad_resampled, the numpy restatement of
csrc/gpcc_markov_resample_grad.hip.h): every cell of tests/_markov_resample_grad_cases.py against the extended-precision dense gradient
of its reduced fresh data set under that gradient's own bar; the slips the comparator must reject, on named cells; value and info
against loglik_resampled, the own-y rows against loglik_grad; bfgs.BatchedBFGS against scipy's BFGS; fit.realisation_refits with the
BFGS optimiser and fit.realisation_peaks on the mirror."""
import numpy as np
import pytest

import _grad_highprec as H
import _markov_cases as MC
import _markov_resample_cases as SC
import _markov_resample_grad_cases as GC
from gpcc_amd import bfgs, fit, markov, synthetic

CASES = GC.cases((110,))
TIES = "OU-N110-L2-b1-rho300-ties"       # OU, two bands, marginalised offsets, exact cross-band ties in shifted time


def _mirror(case, rows=None, slip=None):
    """The mirror's (loglik, grad, info) of a case's rows (one per realisation, or the realisations `rows`), "own" constants."""
    cid, k, data, delays, alpha, rho, mb, N = case
    Y, counts = SC.realisations(case)
    d, a, rh, real = SC.rows(case)
    sel = np.arange(SC.R) if rows is None else np.asarray(rows)
    mean, vb = markov.resample_constants(data[0], Y, counts, mb)
    return markov.loglik_grad_resampled(k, *data, Y, counts, real[sel], d[sel], a[sel], rh[sel], mb, mean=mean, sigma_b=vb, _slip=slip)


@pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_mirror_against_the_reduced_data_sets_reference(kernel):
    picked = [c for c in CASES if c[1] == kernel]
    assert len(picked) == 3 * 2 * 3
    worst = GC.Worst("mirror gradient %s N = 110, 4 realisations" % kernel)
    for case in picked:
        ll, grad, info = markov.MarkovObjective(*case[2], case[1], marginalise_b=case[6]).loglik_grad_markov_resampled(
            SC.realisations(case)[0], *SC.rows(case)[:3], SC.rows(case)[3], counts=SC.realisations(case)[1])
        assert grad.shape == (SC.R, 2 * len(case[3]) + 1) and (info == 0).all(), case[0]
        for r in range(SC.R):
            worst.add(H.ratio(grad[r], GC.reference(case, r)), (case[0], SC.KINDS[r]))
    worst.report()


@pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)
@pytest.mark.parametrize("slip,cid,r", [("lag_from_merged", TIES, 2), ("lag_from_merged", "matern32-N110-L3-b0-rho3-before", 3),
                                        ("handle_sigma_b", TIES, 1), ("handle_sigma_b", "matern52-N110-L2-b1-rho3-plain", 3),
                                        ("one_sided", TIES, 0), ("one_sided", TIES, 2)])
def test_the_comparator_rejects_the_slips(slip, cid, r):
    """Each slip exceeds the bar on its named cell, where the mirror without it is under the bar.  (TIES, 2) is random subset
    selection: points are dropped next to a change of band, and kept points of the two bands still tie."""
    case = next(c for c in CASES if c[0] == cid)
    ref = GC.reference(case, r)
    good, bad = _mirror(case, [r])[1][0], _mirror(case, [r], slip)[1][0]
    print("%s on (%s, %s): error / bar %.3g with the slip, %.3g without" % (slip, cid, SC.KINDS[r], H.ratio(bad, ref), H.ratio(good, ref)))
    assert H.ratio(good, ref) <= 1.0 < H.ratio(bad, ref)


def test_value_and_info_are_loglik_resampleds_and_own_y_rows_are_loglik_grads():
    for case in [c for c in CASES if c[5] == 3.0 and len(c[3]) == 3]:
        cid, k, data, delays, alpha, rho, mb, N = case
        Y, counts = SC.realisations(case)
        d, a, rh, real = SC.rows(case)
        a2, r2 = a.copy(), rh.copy()
        a2[1, 0], r2[2] = -1.0, 0.0
        obj = markov.MarkovObjective(*data, k, marginalise_b=mb)
        ll, grad, info = obj.loglik_grad_markov_resampled(Y, d, a2, r2, real, counts=counts)
        vl, vinfo = obj.loglik_markov_resampled(Y, d, a2, r2, real, counts=counts)
        assert np.array_equal(ll, vl, equal_nan=True) and np.array_equal(info, vinfo) and list(info) == [0, -1, -2, 0]
        assert np.isnan(grad[1:3]).all() and np.isfinite(grad[[0, 3]]).all()
        # realisation 0 is the case's own y with counts of 1: with the handle's constants the row is loglik_grad's, exactly
        ll, grad, info = obj.loglik_grad_markov_resampled(Y, d[:1], a[:1], rh[:1], [0], counts=counts, center="handle", sigma_b="handle")
        pl, pg, pinfo = markov.loglik_grad(k, *data, delays, alpha, rho, mb)
        assert pinfo == 0 and info[0] == 0 and ll[0] == pl and np.array_equal(grad[0], pg), cid
    # a realisation that keeps nothing: 0.0, a zero gradient, info 0
    t, y, s, d0 = MC.lightcurves([20, 15], seed=2, kind="plain")
    Y, counts = [np.asarray(v, np.float64)[None, :] for v in y], [np.zeros((1, len(v)), dtype=np.int64) for v in y]
    ll, grad, info = markov.loglik_grad_resampled("matern32", t, y, s, Y, counts, [0], d0, [1.0, 1.0], 2.0, False)
    assert ll[0] == 0.0 and info[0] == 0 and (grad[0] == 0.0).all()
    with pytest.raises(ValueError):
        markov.loglik_grad_resampled("matern32", t, y, s, Y, counts, [1], d0, [1.0, 1.0], 2.0, False)


def test_ou_tie_among_kept_points_across_a_dropped_point():
    """A dropped point between two kept points that tie across bands: the tau entries are the mean of the two tie orders of the KEPT
    points, and equal the plain mirror's gradient of the reduced data set exactly."""
    t, y, s, d0, Y, counts, (b, i) = GC.tie_case()
    mean, vb = markov.resample_constants(t, Y, counts, False)
    ll, grad, info = markov.loglik_grad_resampled("OU", t, y, s, Y, counts, [0], d0, [1.0, 0.8], 2.0, False, mean=mean, sigma_b=vb)
    _, one, _ = markov.loglik_grad_resampled("OU", t, y, s, Y, counts, [0], d0, [1.0, 0.8], 2.0, False, mean=mean, sigma_b=vb,
                                             _slip="one_sided")
    fl, fg_, finfo = markov.loglik_grad("OU", *SC.reduced((t, y, s), Y, counts, 0), d0, [1.0, 0.8], 2.0, False)
    assert info[0] == 0 and finfo == 0 and np.array_equal(grad[0], fg_) and ll[0] == fl
    assert not np.array_equal(grad[0, 3:], one[0, 3:]) and np.array_equal(grad[0, :3], one[0, :3])


def _problems(P, n, seed):
    rg = np.random.default_rng(seed)
    A = [(lambda m: m @ m.T + np.eye(n))(rg.normal(size=(n, n))) for _ in range(P)]
    b = rg.normal(size=(P, n))

    def one(p, x):
        if p % 2 == 0:                                   # a convex quadratic
            return 0.5 * x @ A[p] @ x - b[p] @ x, A[p] @ x - b[p]
        z = x - b[p]                                     # a shifted Rosenbrock function
        f = sum(100.0 * (z[i + 1] - z[i] ** 2) ** 2 + (1.0 - z[i]) ** 2 for i in range(n - 1))
        g = np.zeros(n)
        for i in range(n - 1):
            g[i] += -400.0 * z[i] * (z[i + 1] - z[i] ** 2) - 2.0 * (1.0 - z[i])
            g[i + 1] += 200.0 * (z[i + 1] - z[i] ** 2)
        return f, g

    def fg(pidx, X):
        out = [one(int(p), x) for p, x in zip(pidx, X)]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])

    return fg, one, rg.normal(size=(P, n))


def test_batched_bfgs_alone():
    """What needs no reference: every problem converges, problems that stop at different rounds do not disturb one another (each equals
    its solo run bitwise), the run is deterministic, a value that is not finite counts as +inf, the iterations bound the accepted steps."""
    P, n = 8, 3
    fg, one, x0 = _problems(P, n, seed=0)
    opt = bfgs.BatchedBFGS(x0, fg, iterations=500, g_tol=1e-8)
    x, f = opt.run()
    assert opt.converged.all() and opt.rounds < opt.f_calls and len(set(opt.iterations_done)) > 2      # they stop at different rounds
    assert (np.abs(opt.gmin).max(axis=1) <= 1e-8).all() and np.array_equal(f, fg(np.arange(P), x)[0])
    for p in range(P):
        solo = bfgs.BatchedBFGS(x0[p:p + 1], lambda pi, X: fg([p] * len(pi), X), iterations=500, g_tol=1e-8)
        xs, fs = solo.run()
        assert np.array_equal(xs[0], x[p]) and fs[0] == f[p] and solo.iterations_done[0] == opt.iterations_done[p]
    again = bfgs.BatchedBFGS(x0, fg, iterations=500, g_tol=1e-8)
    assert np.array_equal(again.run()[0], x) and again.rounds == opt.rounds                                # deterministic
    # a value that is not finite counts as +inf: the trial is rejected, a start of this kind ends at once
    wall = lambda pi, X: (np.where(X[:, 0] > 0.5, np.nan, ((X - 1.0) ** 2).sum(axis=1)), 2.0 * (X - 1.0))
    o = bfgs.BatchedBFGS(np.array([[0.0, 0.0], [2.0, 0.0]]), wall, iterations=50, g_tol=1e-8)
    x, f = o.run()
    assert np.isfinite(f[0]) and f[0] < 2.0 and x[0, 0] <= 0.5 and f[1] == np.inf and not o.converged[1] and o.iterations_done[1] == 0
    # iterations spent
    o = bfgs.BatchedBFGS(x0, fg, iterations=2, g_tol=1e-8)
    o.run()
    assert (o.iterations_done <= 2).all() and not o.converged.all()


def test_batched_bfgs_against_scipy():
    """The same minimisers as scipy.optimize.minimize(method="BFGS") to 1e-6, on the convex quadratics and shifted Rosenbrock functions."""
    minimize = pytest.importorskip("scipy.optimize").minimize
    P, n = 8, 3
    fg, one, x0 = _problems(P, n, seed=0)
    x, f = bfgs.BatchedBFGS(x0, fg, iterations=500, g_tol=1e-8).run()
    for p in range(P):
        ref = minimize(lambda v: one(p, v)[0], x0[p], jac=lambda v: one(p, v)[1], method="BFGS", options=dict(gtol=1e-10))
        assert np.max(np.abs(ref.x - x[p])) <= 1e-6, (p, ref.x, x[p])


def _softmax(ll, logprior=None):
    """getprobabilities without the library (which needs a device)."""
    v = np.asarray(ll, np.float64) + (0.0 if logprior is None else np.asarray(logprior, np.float64))
    e = np.exp(v - v.max())
    return e / e.sum()


@pytest.fixture(scope="module")
def small_fit():
    t, y, s, _ = synthetic.simulate_lightcurves((55, 55))
    grid = np.array([0.0, 1.0, 2.0, 3.0, 8.0])
    cand = np.stack([np.zeros_like(grid), grid], 1)
    Y, counts = synthetic.resample(y, s, 3, seed=3)
    obj = markov.MarkovObjective(t, y, s, "matern32")
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    start = (np.tile(alpha0, (5, 1)), np.full(5, min(rho0, 19.0)))
    return obj, cand, Y, counts, start


def test_realisation_refits_with_bfgs_on_the_mirror(small_fit):
    obj, cand, Y, counts, start = small_fit
    R, G, g_tol = 3, 5, 1e-6
    out = fit.realisation_refits(obj, cand, Y, counts, iterations=25, start=start, optimiser="bfgs", probabilities=_softmax)
    assert out.loglikel.shape == (R, G) and out.alpha.shape == (R, G, 2) and out.rho.shape == (R, G)
    assert np.isfinite(out.loglikel).all() and (out.loglikel >= out.start_loglikel).all() and (out.loglikel > out.start_loglikel).any()
    assert np.all(np.abs(out.delays.prob.sum(axis=1) - 1.0) <= 1e-12) and out.rounds < out.f_calls
    # re-evaluated at the returned (alpha, rho): the value, and the gradient taken to the optimiser's own coordinates out.x
    real = np.repeat(np.arange(R), G)
    assert out.x.shape == (R, G, 3) and np.array_equal(fit.makepositive(out.x[..., :2]) + 1e-8, out.alpha)
    assert np.array_equal(fit.transformbetween(out.x[..., 2], 0.1, 20.0), out.rho)
    ll, grad, info = obj.loglik_grad_markov_resampled(Y, np.tile(cand, (R, 1)), out.alpha.reshape(-1, 2), out.rho.reshape(-1), real, counts=counts)
    assert (info == 0).all() and np.array_equal(ll, out.loglikel.reshape(-1))
    gx = np.abs(fit.unpack_grad(out.x.reshape(-1, 3), grad[:, :3], 2, 0.1, 20.0)).max(axis=1)
    print("refits with bfgs on the mirror: %d rounds, %d f_calls, %d of %d cells converged, their worst re-evaluated gradient %.3g"
          % (out.rounds, out.f_calls, out.converged.sum(), R * G, gx[out.converged.reshape(-1)].max(initial=0.0)))
    assert out.converged.shape == (R, G) and out.converged.any()
    assert (gx[out.converged.reshape(-1)] <= g_tol).all()
    with pytest.raises(ValueError):
        fit.realisation_refits(obj, cand, Y, counts, iterations=1, start=start, optimiser="newton", probabilities=_softmax)
    # the default is the Nelder-Mead path, exactly
    a = fit.realisation_refits(obj, cand, Y, counts, iterations=2, start=start, probabilities=_softmax)
    b = fit.realisation_refits(obj, cand, Y, counts, iterations=2, start=start, optimiser="neldermead", probabilities=_softmax)
    assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("loglikel", "alpha", "rho", "start_loglikel"))
    assert (a.f_calls, a.rounds) == (b.f_calls, b.rounds) and np.array_equal(a.delays.prob, b.delays.prob)
    assert a.converged is None and a.x.shape == (R, G, 3) and np.array_equal(a.x, b.x)


def test_realisation_peaks_on_the_mirror(small_fit):
    obj, cand, Y, counts, start = small_fit
    R, g_tol = 3, 1e-6
    pk = fit.realisation_peaks(obj, cand, Y, counts, start=start, iterations=40, g_tol=g_tol, probabilities=_softmax)
    assert pk.delays.shape == (R, 2) and pk.alpha.shape == (R, 2) and pk.rho.shape == (R,) and pk.converged.shape == (R,)
    assert (pk.loglikel >= pk.start_loglikel).all() and (pk.delays[:, 0] == 0.0).all()
    assert (pk.delays[:, 1] >= 0.0).all() and (pk.delays[:, 1] <= 8.0).all() and (pk.rho > 0.1).all() and (pk.rho < 20.0).all()
    ll, grad, info = obj.loglik_grad_markov_resampled(Y, pk.delays, pk.alpha, pk.rho, np.arange(R), counts=counts)
    assert (info == 0).all() and np.array_equal(ll, pk.loglikel)
    # the gradient taken to the optimiser's own coordinates pk.x: alpha, rho, then the free delay, tau = 8 logistic(x)
    assert pk.x.shape == (R, 4) and np.array_equal(fit.makepositive(pk.x[:, :2]) + 1e-8, pk.alpha)
    gx = fit.unpack_grad(pk.x[:, :3], grad[:, :3], 2, 0.1, 20.0)
    u = 1.0 / (1.0 + np.exp(-pk.x[:, 3]))
    gt = grad[:, 4] * (8.0 * u * (1.0 - u))
    worst = np.maximum(np.abs(gx).max(axis=1), np.abs(gt))
    print("peaks on the mirror: %d rounds, %d f_calls, converged %s, delays %s, re-evaluated gradient %s"
          % (pk.rounds, pk.f_calls, pk.converged, pk.delays[:, 1], worst))
    assert pk.converged.any() and (worst[pk.converged] <= g_tol).all()
    # from a RealisationRefits: the start is each realisation's best cell with its refitted hyper-parameters
    ref = fit.realisation_refits(obj, cand, Y, counts, iterations=3, start=start, optimiser="bfgs", probabilities=_softmax)
    p2 = fit.realisation_peaks(obj, cand, Y, counts, start=ref, iterations=3)
    cell = ref.delays.map_index
    assert (p2.loglikel >= p2.start_loglikel).all() and np.allclose(p2.start_loglikel, ref.loglikel[np.arange(R), cell], rtol=1e-10, atol=0)
    with pytest.raises(ValueError):
        fit.realisation_peaks(obj, cand, Y, counts, start=start, iterations=1, free_delays=[0], probabilities=_softmax)
