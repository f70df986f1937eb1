"""The numpy mirror of the linear-time predictions, held-out log-likelihoods and offsets' posterior (gpcc_amd.markov.predict, heldout,
posterior_offsets) against the dense witnesses, with the dense entries' own bars (tests/_markov_predict_cases.py); every injected
mistake must exceed the bar somewhere; identities; the fit and the predictors without a GPU."""
import math

import numpy as np
import pytest

import _markov_cases as MC
import _markov_predict_cases as PC
from gpcc_amd import fit, markov

CASES = PC.cpu_cases()


def test_case_count():
    assert len(CASES) == 3 * 3 * 2 * len(MC.RHOS)
    assert any(len(a) == 0 for c in CASES for a in c[7][0]) and {c[0].split("-")[-1] for c in CASES} == {"ties", "before", "plain"}


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_predict_against_witness(oracle, kernel):
    wm, wv = MC.Worst("mirror mu %s" % kernel), MC.Worst("mirror var %s" % kernel)
    for case in CASES:
        cid, k, data, delays, alpha, rho, mb, tests = case
        if k != kernel:
            continue
        mu, var, ll, info = markov.predict(k, *data, delays, alpha, rho, tests[0], mb)
        assert info == 0, cid
        assert ll == markov.loglik(k, *data, delays, alpha, rho, mb)[0], cid       # the taps do not split the filter's chain
        rmu, rvar, bmu, bvar = PC.predict_reference(oracle, case)
        wm.add(float(np.max(np.abs(mu - rmu))), bmu, cid)
        wv.add(float(np.max(np.abs(var - rvar))), bvar, cid)
    wm.report()
    wv.report()


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_heldout_against_witness(oracle, kernel):
    w = MC.Worst("mirror held-out %s" % kernel)
    for case in CASES:
        cid, k, data, delays, alpha, rho, mb, tests = case
        if k != kernel:
            continue
        held, ll, info = markov.heldout(k, *data, delays, alpha, rho, *tests, mb)
        assert info == 0 and ll == markov.loglik(k, *data, delays, alpha, rho, mb)[0], cid
        ref, b = PC.heldout_reference(oracle, case)
        w.add(abs(held - ref), b, cid)
    w.report()


def test_posterior_offsets_against_reference_formulas(oracle):
    n = 0
    for case in CASES:
        cid, k, data, delays, alpha, rho, mb, _ = case
        if not mb:
            continue
        mu, Sig, ll, info = markov.posterior_offsets(k, *data, delays, alpha, rho)
        assert info == 0 and ll == markov.loglik(k, *data, delays, alpha, rho, True)[0], cid
        PC.assert_postb(mu, Sig, *PC.postb_reference(oracle, k, *data, delays, alpha, rho))
        n += 1
    assert n == 36


@pytest.mark.parametrize("slip", ["no_flip", "tie_both", "no_prior", "no_jitter"])
def test_bar_catches_predict_slips(oracle, slip):
    """Each mistake exceeds the bar on at least one case ("no_jitter" can only show where b is not marginalised: with Sigma_b in the
    scale the bar is above 1e-8)."""
    caught = 0
    for case in CASES:
        cid, k, data, delays, alpha, rho, mb, tests = case
        mu, var, _, info = markov.predict(k, *data, delays, alpha, rho, tests[0], mb, _slip=slip)
        rmu, rvar, bmu, bvar = PC.predict_reference(oracle, case)
        if info != 0 or np.max(np.abs(mu - rmu)) > bmu or np.max(np.abs(var - rvar)) > bvar:
            caught += 1
    print("%s: caught on %d of %d cases" % (slip, caught, len(CASES)))
    assert caught >= 1


@pytest.mark.parametrize("slip", ["no_jitter", "test_mean"])
def test_bar_catches_heldout_slips(oracle, slip):
    caught = 0
    for case in CASES:
        cid, k, data, delays, alpha, rho, mb, tests = case
        held, _, info = markov.heldout(k, *data, delays, alpha, rho, *tests, mb, _slip=slip)
        ref, b = PC.heldout_reference(oracle, case)
        if info != 0 or abs(held - ref) > b:
            caught += 1
    print("%s: caught on %d of %d cases" % (slip, caught, len(CASES)))
    assert caught >= 1


def test_far_test_point_returns_the_prior():
    """OU, b not marginalised: more than 40 rho from every training point the posterior is the prior, mu_b and alpha^2 + JITTER."""
    t, y, s, delays = MC.lightcurves([60, 50], seed=21, kind="plain")
    alpha, rho = np.array([0.8, 1.7]), 0.5
    tt = [np.array([-25.0, 30.0 + delays[0] + 45 * rho]), np.array([60.0 + delays[1], -40.0])]
    mu, var, _, info = markov.predict("OU", t, y, s, delays, alpha, rho, tt, False)
    assert info == 0
    means = np.repeat([np.mean(a) for a in y], 2)
    np.testing.assert_allclose(mu, means, rtol=0, atol=8 * np.finfo(float).eps * np.max(np.abs(means)) + 1e-15)
    np.testing.assert_allclose(var, np.repeat(alpha ** 2, 2) + markov.JITTER, rtol=8 * np.finfo(float).eps)


@pytest.mark.parametrize("kernel,mb", [("OU", True), ("matern32", False), ("matern52", True)])
def test_heldout_of_one_point_is_the_predictive_density(kernel, mb):
    t, y, s, delays = MC.lightcurves([60, 50], seed=22, kind="ties")
    alpha, rho = np.array([1.1, 0.6]), 3.0
    for band, tstar, ystar, sstar in ((0, 12.5, 0.3, 0.25), (1, float(np.sort(t[0])[7] + delays[1]), 0.9, 0.1)):
        tt = [np.array([tstar]) if l == band else np.zeros(0) for l in range(2)]
        yt = [np.array([ystar]) if l == band else np.zeros(0) for l in range(2)]
        st = [np.array([sstar]) if l == band else np.zeros(0) for l in range(2)]
        mu, var, _, _ = markov.predict(kernel, t, y, s, delays, alpha, rho, tt, mb)
        held, _, info = markov.heldout(kernel, t, y, s, delays, alpha, rho, tt, yt, st, mb)
        v = var[0] + sstar ** 2
        want = -0.5 * (markov.LOG2PI + math.log(v) + (ystar - mu[0]) ** 2 / v)
        assert info == 0 and abs(held - want) <= 1e-9 * max(1.0, abs(want))


def test_failures_and_codes():
    t, y, s, delays = MC.lightcurves([60, 50], seed=23, kind="plain")
    tt, yt, st = PC.test_points(t, delays, 5, -1)
    N, T = 110, sum(len(a) for a in tt)
    mu, var, ll, info = markov.predict("OU", t, y, s, delays, [1.0, -1.0], 2.0, tt)
    assert info == -1 and np.isnan(mu).all() and len(mu) == T and math.isnan(ll)
    assert markov.heldout("OU", t, y, s, delays, [1.0, 1.0], 0.0, tt, yt, st)[2] == -2
    st[1][3] = np.nan                                                             # a non-finite sigma*: that test point's variance
    held, ll, info = markov.heldout("OU", t, y, s, delays, [1.0, 1.0], 2.0, tt, yt, st)
    assert info == N + len(tt[0]) + 3 + 1 and math.isnan(held) and ll == markov.loglik("OU", t, y, s, delays, [1.0, 1.0], 2.0)[0]


def test_fit_and_predictors_without_a_gpu():
    t, y, s, delays = MC.lightcurves([40, 30], seed=24, kind="plain")
    cand = np.stack([np.zeros(3), delays[1] + np.array([-0.5, 0.0, 0.5])], 1)
    obj = markov.MarkovObjective(t, y, s, "matern32")
    res = fit.gpcc_grid(t, y, s, kernel="matern32", candidatedelays=cand, iterations=30, rhomax=20.0, objective=obj, solver="markov")
    assert np.isfinite(res.loglikel).all()
    pred = fit.Predictor(obj, cand[1], res.alpha[1], res.rho[1], solver="markov")
    grid = np.linspace(-2.0, 33.0, 15)
    mus, sds = pred(grid)
    ref = markov.predict("matern32", t, y, s, cand[1], res.alpha[1], res.rho[1], [grid, grid])
    assert len(mus) == 2 and np.array_equal(np.concatenate(mus), ref[0])
    assert np.array_equal(np.concatenate(sds), np.sqrt(np.maximum(ref[1], 1e-6)))
    tt, yt, st = PC.test_points(t, cand[1], 6, -1)
    assert pred(tt, yt, st) == markov.heldout("matern32", t, y, s, cand[1], res.alpha[1], res.rho[1], tt, yt, st)[0]
    w = np.exp(res.loglikel - res.loglikel.max())
    avg = fit.DelayAveragedPredictor(obj, cand, res.alpha, res.rho, w, solver="markov")
    mmu, msd = avg(grid)
    rows = [markov.predict("matern32", t, y, s, cand[g], res.alpha[g], res.rho[g], [grid, grid]) for g in range(3)]
    import _predict_witness as PW
    wmu, wvar = PW.mixture(np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), w)
    np.testing.assert_allclose(np.concatenate(mmu), wmu, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(np.concatenate(msd), np.sqrt(np.maximum(wvar, 1e-6)), rtol=1e-10)
    assert np.isfinite(avg.loglik(tt, yt, st))
    with pytest.raises(ValueError):
        fit.Predictor(obj, cand[1], res.alpha[1], res.rho[1], solver="sparse")
