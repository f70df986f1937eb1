"""Many flux realisations per parameter row on the CPU (gpcc_amd.markov.loglik_realisations, the numpy restatement of
csrc/gpcc_markov_multi.hip.h): against the dense reference of tests/_markov_realisations_cases.py under that module's bar (the
family's, measured on the reference side, per realisation), through the explicit dense route and through the shortcuts; its columns
against markov.loglik; what the two centrings do to a shifted band; fit.realisation_delays against the host loop;
synthetic.flux_randomise."""
import numpy as np
import pytest

import _markov_cases as MC
import _markov_realisations_cases as RC
from gpcc_amd import fit, markov, synthetic

CASES = RC.cases((110,))


def test_the_cases_cover_the_delay_kinds():
    assert len(CASES) == 3 * 3 * 2 * len(RC.RHOS)
    for kind in ("ties", "before", "plain"):
        for kernel in MC.KERNELS:
            assert any(c[0].endswith(kind) and c[1] == kernel for c in CASES), (kind, kernel)


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_mirror_against_the_dense_reference(oracle, kernel):
    """|mirror - reference| <= MC.bar(e_dense, N, F) |reference| per realisation, with the handle's means (mean=None) and with each
    realisation's own; every other case without marginalise_b takes the shortcut for the own means (the fresh data set's reference)."""
    worst = {w: MC.Worst("mirror %s N = 110, %s" % (kernel, w)) for w in ("handle means", "own means", "own means, fresh data set")}
    n = 0
    for case in CASES:
        cid, k, data, delays, alpha, rho, mb, N = case
        if k != kernel:
            continue
        n += 1
        Y = RC.realisations(case)
        own = RC.own_means(Y)
        ll_h, info_h = markov.loglik_realisations(k, *data, Y, delays, alpha, rho, mb)
        ll_o, info_o = markov.loglik_realisations(k, *data, Y, delays, alpha, rho, mb, mean=own)
        assert ll_h.shape == ll_o.shape == (1, RC.R) and info_h[0] == 0 and info_o[0] == 0, cid
        handle = np.tile(markov._setup(k, *data, delays, alpha, rho, mb)[7], (RC.R, 1))
        for r, (ref, b, _) in enumerate(RC.general_reference(oracle, case, Y, handle)):
            worst["handle means"].add(abs(ll_h[0, r] - ref) / abs(ref), b, (cid, r))
        if not mb and n % 2 == 0:
            for r in range(RC.R):
                ref, b, _ = RC.fresh_reference(oracle, case, Y, r)
                worst["own means, fresh data set"].add(abs(ll_o[0, r] - ref) / abs(ref), b, (cid, r))
        else:
            for r, (ref, b, _) in enumerate(RC.general_reference(oracle, case, Y, own)):
                worst["own means"].add(abs(ll_o[0, r] - ref) / abs(ref), b, (cid, r))
    assert n == 3 * 2 * len(RC.RHOS)
    for w in worst.values():
        assert w.where is not None
        w.report()


def test_rescaled_realisations_reach_the_fresh_reference(oracle):
    """With marginalise_b a realisation whose bands were rescaled to the handle's band means and variances has the handle's Sigma_b: its
    value is the fresh data set's, with either centring."""
    worst = MC.Worst("mirror, rescaled realisations against the fresh data set (marginalise_b)")
    picked = [c for c in CASES if c[6] and c[5] == 3.0]
    assert len(picked) == 9
    for case in picked:
        cid, k, data, delays, alpha, rho, mb, N = case
        Y = RC.rescale_to(data[1], RC.realisations(case))
        ll_h, _ = markov.loglik_realisations(k, *data, Y, delays, alpha, rho, mb)
        ll_o, _ = markov.loglik_realisations(k, *data, Y, delays, alpha, rho, mb, mean=RC.own_means(Y))
        for r in range(RC.R):
            ref, b, _ = RC.fresh_reference(oracle, case, Y, r, tag="rescaled")
            worst.add(abs(ll_h[0, r] - ref) / abs(ref), b, (cid, r, "handle"))
            worst.add(abs(ll_o[0, r] - ref) / abs(ref), b, (cid, r, "own"))
    worst.report()


def test_columns_against_loglik(oracle):
    """mean=None: the column of the handle's own y is markov.loglik of the handle's data; own means without marginalise_b: a column is
    markov.loglik of the fresh data set.  Both to the bar (two orders of rounding of one algorithm: twice the bar)."""
    for case in CASES[::5]:
        cid, k, data, delays, alpha, rho, mb, N = case
        Y = RC.realisations(case)
        ref, b, _ = MC.reference_and_bar(oracle, case)
        ll_h, _ = markov.loglik_realisations(k, *data, Y, delays, alpha, rho, mb)
        single, info = markov.loglik(k, *data, delays, alpha, rho, mb)
        assert info == 0 and abs(ll_h[0, 0] - single) <= 2 * b * abs(ref), cid
        if not mb:
            ll_o, _ = markov.loglik_realisations(k, *data, Y, delays, alpha, rho, mb, mean=RC.own_means(Y))
            for r in range(RC.R):
                fr, fb, _ = RC.fresh_reference(oracle, case, Y, r)
                single, info = markov.loglik(k, data[0], [a[r] for a in Y], data[2], delays, alpha, rho, mb)
                assert info == 0 and abs(ll_o[0, r] - single) <= 2 * fb * abs(fr), (cid, r)


def test_shifted_band(oracle):
    """Realisation 4 is realisation 1 with its last band shifted by a constant: the same value under own means, another under the
    handle's."""
    for case in CASES[::7]:
        cid, k, data, delays, alpha, rho, mb, N = case
        Y = RC.realisations(case)
        own = RC.own_means(Y)
        ll_o, _ = markov.loglik_realisations(k, *data, Y, delays, alpha, rho, mb, mean=own)
        ll_h, _ = markov.loglik_realisations(k, *data, Y, delays, alpha, rho, mb)
        refs = RC.general_reference(oracle, case, Y, own)
        assert abs(ll_o[0, 4] - ll_o[0, 1]) <= (refs[1][1] + refs[4][1]) * abs(refs[1][0]), cid
        # (with marginalise_b the offset's prior is nearly flat and the shift costs little -- but far more than any rounding)
        assert abs(ll_h[0, 4] - ll_h[0, 1]) > 1000 * (refs[1][1] + refs[4][1]) * abs(refs[1][0]), cid
        if not mb:
            assert abs(ll_h[0, 4] - ll_h[0, 1]) > 1e-2 * abs(ll_h[0, 1]), cid


def test_rows_codes_and_nonfinite_fluxes():
    t, y, s, d0 = MC.lightcurves([30, 20], seed=3, kind="plain")
    Y = synthetic.flux_randomise(y, s, 4, seed=1)
    delays = np.stack([d0, d0 + [0.0, 0.5], d0, d0])
    alpha = np.array([[1.0, 1.2], [0.7, 1.1], [1.0, 0.0], [1.0, 1.0]])
    rho = np.array([2.0, 3.0, 2.0, -1.0])
    ll, info = markov.loglik_realisations("matern32", t, y, s, Y, delays, alpha, rho)
    assert ll.shape == (4, 4) and list(info) == [0, 0, -1, -2]
    assert np.isfinite(ll[:2]).all() and np.isnan(ll[2:]).all()
    for m in (0, 1):                                                     # a row is its own single-row call; Y as one (R, N) array
        one, _ = markov.loglik_realisations("matern32", t, y, s, np.concatenate(Y, axis=1), delays[m], alpha[m], rho[m])
        assert np.array_equal(one[0], ll[m])
    Y[1][2, 5] = np.inf
    Y[0][3, 0] = np.nan
    bad, _ = markov.loglik_realisations("matern32", t, y, s, Y, delays[:2], alpha[:2], rho[:2])
    assert np.isnan(bad[:, 2:]).all() and np.array_equal(bad[:, :2], ll[:2, :2])
    with pytest.raises(ValueError):
        markov.loglik_realisations("rbf", t, y, s, Y, delays[0], alpha[0], rho[0])
    with pytest.raises(ValueError):
        markov.loglik_realisations("OU", t, y, s, [Y[0]], delays[0], alpha[0], rho[0])


def _softmax(ll, logprior=None):
    x = np.asarray(ll, np.float64) + (0.0 if logprior is None else np.asarray(logprior, np.float64))
    w = np.exp(x - x.max())
    return w / w.sum()


def test_realisation_delays_is_the_host_loop():
    t, y, s, _ = synthetic.simulate_lightcurves((25, 25), seed=2)
    cand = np.stack([np.zeros(7), np.arange(0.0, 7.0, 1.0)], 1)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    alpha, rho = np.tile(alpha0, (7, 1)) * np.linspace(0.9, 1.1, 7)[:, None], np.linspace(2.0, 4.0, 7)
    obj = markov.MarkovObjective(t, y, s, "matern32", marginalise_b=False)
    Y = [np.concatenate([np.asarray(a)[None, :], b]) for a, b in zip(y, synthetic.flux_randomise(y, s, 5, seed=4))]
    for center in ("own", "handle"):
        for logprior in (None, np.linspace(-1.0, 0.0, 7)):
            res = fit.realisation_delays(obj, cand, alpha, rho, Y, logprior=logprior, center=center, probabilities=_softmax)
            assert res.prob.shape == (6, 7) and res.map_index.shape == (6,) and res.mean_delay.shape == (6, 2)
            ll, info = obj.loglik_markov_realisations(Y, cand, alpha, rho, center=center)
            assert (info == 0).all()
            for r in range(6):
                p = _softmax(ll[:, r], logprior)
                assert np.array_equal(res.prob[r], p) and res.map_index[r] == int(np.argmax(p))
                assert np.all(np.abs(res.mean_delay[r] - p @ cand) <= 8 * np.finfo(float).eps * (p @ np.abs(cand)))    # (7 terms, any order)
            assert np.allclose(res.prob.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    # the unrandomised y under own means is the data set's own likelihood: the loop over fresh objectives
    own, _ = obj.loglik_markov_realisations(Y, cand, alpha, rho, center="own")
    for r in (0, 3):
        fresh = markov.MarkovObjective(t, [a[r] for a in Y], s, "matern32", marginalise_b=False)
        ll, _ = fresh.loglik_markov_batch(cand, alpha, rho)
        assert np.all(np.abs(own[:, r] - ll) <= 1e-11 * np.abs(ll))
    with pytest.raises(ValueError):
        fit.realisation_delays(obj, cand, -alpha, rho, Y, probabilities=_softmax)


def test_flux_randomise():
    t, y, s, _ = MC.lightcurves([40, 30], seed=9, kind="plain")
    a = synthetic.flux_randomise(y, s, 4000, seed=11)
    b = synthetic.flux_randomise(y, s, 4000, seed=11)
    c = synthetic.flux_randomise(y, s, 4000, seed=12)
    assert [x.shape for x in a] == [(4000, 40), (4000, 30)]
    assert all(np.array_equal(x, z) for x, z in zip(a, b)) and not np.array_equal(a[0], c[0])
    for l in range(2):
        z = (a[l] - y[l][None, :]) / s[l][None, :]                       # standard normal: 4000 draws per point
        n = z.shape[0]
        assert np.all(np.abs(z.mean(axis=0)) <= 5.0 / np.sqrt(n))        # 5 standard errors of the mean
        assert np.all(np.abs(z.var(axis=0, ddof=1) - 1.0) <= 5.0 * np.sqrt(2.0 / (n - 1)))      # ... and of the variance
        assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) <= 5.0 / np.sqrt(n)
    with pytest.raises(ValueError):
        synthetic.flux_randomise(y, s, 0, seed=1)
