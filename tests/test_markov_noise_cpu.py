"""The numpy mirror of the linear-time log-likelihood under a per-row noise model (gpcc_amd.markov.loglik_noise, loglik_grad_noise) on
the CPU: value and all 4L+1 gradient entries against the extended-precision reference on the effective error bars
(tests/_markov_noise_cases.py), every injected slip rejected, kappa = 1 and nu = 0 exactly the plain mirror, the codes, and
fit.gpcc_grid_noise with fit.effective_std over markov.MarkovObjective."""
import math
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _grad_highprec as H
import _markov_cases as MC
import _markov_noise_cases as NC
from gpcc_amd import fit, markov

extended = pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


def _references(pool, cases):
    refs = list(pool.map(NC.reference_job, [NC.job(c) for c in cases]))
    for c, r in zip(cases, refs):
        assert r[0].info == 0, c[0]
    return refs


@extended
@pytest.mark.parametrize("N", [110, 150, 767])
def test_mirror_against_extended_reference(oracle, pool, N):
    cases = NC.cases(N)
    assert len(cases) == (72 if N != 767 else 12)
    assert sum(c[8][0] == 0.0 for c in cases) == len(cases) // 2         # every second case: band 1 without its reported error bars
    refs = _references(pool, cases)
    worst = {g: NC.GC.Worst("mirror %s N = %d" % (g, N)) for g in ("value", "alpha rho tau", "kappa nu")}
    for case, reference in zip(cases, refs):
        cid, k, data, delays, alpha, rho, mb, _, kappa, nu = case
        ll, g, info = markov.loglik_grad_noise(k, *data, delays, alpha, rho, kappa, nu, mb)
        assert info == 0 and g.shape == (4 * len(alpha) + 1,), cid
        assert (ll, 0) == markov.loglik_noise(k, *data, delays, alpha, rho, kappa, nu, mb), cid
        rv, rg, rn = NC.ratios(ll, g, oracle, case, reference)
        print("%s: error / bar %.3g (value) %.3g (alpha, rho, tau) %.3g (kappa, nu)" % (cid, rv, rg, rn))
        worst["value"].add(rv, cid)
        worst["alpha rho tau"].add(rg, cid)
        worst["kappa nu"].add(rn, cid)
    for w in worst.values():
        w.report()


@extended
def test_every_slip_misses_a_bar(oracle, pool):
    """Each mistake of markov.loglik_grad_noise's _slip breaks the value's or a gradient bar on at least one case at N = 110 (here: on
    how many is printed); the same comparator passes the mirror without a slip in test_mirror_against_extended_reference."""
    cases = NC.cases(110)[::3]
    refs = _references(pool, cases)
    for slip in NC.SLIPS:
        missed, closest = 0, 0.0
        for case, reference in zip(cases, refs):
            cid, k, data, delays, alpha, rho, mb, _, kappa, nu = case
            ll, g, info = markov.loglik_grad_noise(k, *data, delays, alpha, rho, kappa, nu, mb, _slip=slip)
            if info != 0:      # (nu kappa^2 with kappa = 0 leaves a band without noise, and a tie then fails the filter: not counted)
                continue
            r = max(NC.ratios(ll, g, oracle, case, reference))
            missed += r > 1.0
            closest = max(closest, r)
        print("slip %-16s misses a bar on %d of %d cases, largest error / bar %.3g" % (slip, missed, len(cases), closest))
        assert missed >= 1, slip


def test_unit_noise_is_the_plain_mirror_exactly():
    for case in MC.cpu_cases()[5:72:11]:
        cid, k, data, delays, alpha, rho, mb, _ = case
        L = len(alpha)
        plain = markov.loglik(k, *data, delays, alpha, rho, mb)
        pl, pg, pinfo = markov.loglik_grad(k, *data, delays, alpha, rho, mb)
        for kappa, nu in ((np.ones(L), np.zeros(L)), (None, None), (np.ones(L), None), (None, np.zeros(L))):
            assert markov.loglik_noise(k, *data, delays, alpha, rho, kappa, nu, mb) == plain, cid
            ll, g, info = markov.loglik_grad_noise(k, *data, delays, alpha, rho, kappa, nu, mb)
            assert ll == pl and info == pinfo == 0 and np.array_equal(g[:2 * L + 1], pg) and np.isfinite(g).all(), cid
    t, y, s, d0 = MC.lightcurves([30, 20], seed=3, kind="plain")
    obj = markov.MarkovObjective(t, y, s, "matern32")
    d, a, r = np.tile(d0, (3, 1)), np.tile([1.0, 0.8], (3, 1)), [2.0, 3.0, 4.0]
    ll, info = obj.loglik_markov_noise_batch(d, a, r)
    pl, pinfo = obj.loglik_markov_batch(d, a, r)
    assert np.array_equal(ll, pl) and np.array_equal(info, pinfo)
    gl, gg, ginfo = obj.loglik_grad_markov_noise_batch(d, a, r, [1.0, 1.0], np.zeros((3, 2)))
    assert np.array_equal(gl, pl) and gg.shape == (3, 9) and np.array_equal(gg[:, :5], markov.loglik_grad_batch("matern32", t, y, s, d, a, r)[1])


def test_codes_and_their_precedence():
    t, y, s, d0 = MC.lightcurves([30, 20], seed=3, kind="plain")
    M = 8
    d, a, r = np.tile(d0, (M, 1)), np.tile([1.0, 0.8], (M, 1)), np.full(M, 2.0)
    kappa, nu = np.tile([1.3, 0.7], (M, 1)), np.tile([0.01, 0.0], (M, 1))
    good, gg, ginfo = markov.loglik_grad_noise_batch("OU", t, y, s, d, a, r, kappa, nu)
    assert (ginfo == 0).all() and np.isfinite(gg).all()
    a[1, 0] = 0.0          # -1
    kappa[1, 1] = -1.0     # ... before -3
    r[2] = 0.0             # -2
    nu[2, 0] = -0.5        # ... before -3
    kappa[3, 0] = -1e-300  # -3
    nu[4, 1] = -1e-300     # -3
    kappa[5, 1] = np.nan   # -3
    nu[6, 0] = np.inf      # -3
    ll, g, info = markov.loglik_grad_noise_batch("OU", t, y, s, d, a, r, kappa, nu)
    vl, vinfo = markov.loglik_noise_batch("OU", t, y, s, d, a, r, kappa, nu)
    assert list(info) == [0, -1, -2, -3, -3, -3, -3, 0] and np.array_equal(info, vinfo)
    assert np.isnan(ll[1:7]).all() and np.isnan(g[1:7]).all() and np.isnan(vl[1:7]).all()
    for m in (0, 7):       # the neighbouring rows are untouched
        assert ll[m] == good[m] == vl[m] and np.array_equal(g[m], gg[m])
    with pytest.raises(ValueError):
        markov.loglik_noise("rbf", t, y, s, d0, [1.0, 1.0], 2.0)
    with pytest.raises(ValueError):
        markov.loglik_noise_batch("OU", t, y, s, d, a, r, np.ones((M, 3)), None)
    # kappa = 0 and nu = 0: a band without noise is legal; its positive code is the filter's
    ll0, info0 = markov.loglik_noise("OU", t, y, s, d0, [1.0, 0.8], 2.0, [0.0, 1.0], [0.0, 0.0], False)
    assert info0 == 0 and math.isfinite(ll0)


# ---- the fit ------------------------------------------------------------------------------------------------------------------
SEED = 1                    # chosen on the CPU: with it the shared-kappa profile of the mirror over {1, 1.5, 2, 2.5, 3} peaks at 2
PROFILE = (1.0, 1.5, 2.0, 2.5, 3.0)


def misreported(seed):
    """MC.lightcurves([60, 50], "plain")-sized data of the model itself: a draw of alpha_l f(t - tau_l) + b_l with an OU f (rho = 3),
    observed with noise of standard deviation 2 sigma but REPORTED as sigma.  -> (t, y, s, delays, alpha, rho)."""
    t, _, s, delays = MC.lightcurves([60, 50], seed=seed, kind="plain")
    rg = np.random.default_rng(seed)
    alpha, rho = np.array([1.0, 0.8]), 3.0
    u = np.concatenate([t[l] - delays[l] for l in range(2)])
    K = np.exp(-np.abs(u[:, None] - u[None, :]) / rho)
    f = np.linalg.cholesky(K + 1e-12 * np.eye(len(u))) @ rg.standard_normal(len(u))
    y = [alpha[0] * f[:60] + 2.0 * s[0] * rg.standard_normal(60), 0.3 + alpha[1] * f[60:] + 2.0 * s[1] * rg.standard_normal(50)]
    return t, y, s, delays, alpha, rho


def test_grid_noise_recovers_the_error_bar_scale(oracle):
    t, y, s, delays, alpha, rho = misreported(SEED)
    obj = markov.MarkovObjective(t, y, s, "OU")
    prof, info = obj.loglik_markov_noise_batch(np.tile(delays, (5, 1)), np.tile(alpha, (5, 1)), np.full(5, rho),
                                               np.repeat(np.array(PROFILE)[:, None], 2, 1), None)
    print("shared-kappa profile at the generating (alpha, rho, tau):", dict(zip(PROFILE, np.round(prof, 3))))
    assert (info == 0).all() and int(np.argmax(prof)) == 2
    cand = np.stack([np.zeros(5), delays[1] + np.array([-1.0, -0.5, 0.0, 0.5, 1.0])], 1)
    res = fit.gpcc_grid_noise(obj, cand, iterations=60, noise="scale", shared=True, start=(np.tile(alpha, (5, 1)), np.full(5, rho)))
    assert isinstance(res, fit.NoiseGridFit) and res.kappa.shape == (5, 2) and res.nu.shape == (5, 2) and res.alpha.shape == (5, 2)
    assert (res.loglikel >= res.start_loglikel).all() and res.f_calls > 0 and res.rounds > 0
    assert np.array_equal(res.kappa[:, 0], res.kappa[:, 1]) and (res.nu == 0.0).all()        # shared; nu stays at its argument
    plain, _ = obj.loglik_markov_batch(cand, np.tile(alpha, (5, 1)), np.full(5, rho))
    assert np.allclose(res.start_loglikel, plain, rtol=1e-9, atol=0.0)                        # kappa = 1, nu fixed at 0: the plain model
    print("fitted kappa over the 5 delays:", np.round(res.kappa[:, 0], 3), "loglikel", np.round(res.loglikel, 3))
    assert 1.5 <= res.kappa[2, 0] <= 2.5
    # effective_std round-trips: the plain mirror on it gives loglik_noise's value, to the value's bar
    g = 2
    eff = fit.effective_std(s, res.kappa[g], res.nu[g])
    assert all(np.allclose(e, res.kappa[g, l] * s[l]) for l, e in enumerate(eff))
    fresh = markov.loglik("OU", t, y, eff, cand[g], res.alpha[g], res.rho[g], True)
    assert fresh[1] == 0
    d, dinfo = oracle.loglik_batch("OU", t, y, eff, cand[g][None, :], res.alpha[g][None, :], [res.rho[g]], True)
    if H.EXTENDED:
        ref = H.evaluate("OU", t, y, eff, cand[g], res.alpha[g], res.rho[g], True, value_only=True).loglik
        e = abs(d[0] - ref) / abs(ref)
    else:
        ref, e = d[0], MC.dense_pair_error("OU", (t, y, eff), cand[g], res.alpha[g], res.rho[g], True, d[0])
    b = MC.bar(e, 110, MC.factor(res.alpha[g], eff))
    assert abs(fresh[0] - res.loglikel[g]) <= b * abs(ref) and abs(fresh[0] - ref) <= b * abs(ref)
    # the other modes run: both parts per band from random candidates; the reference's unused global-noise model
    both = fit.gpcc_grid_noise(obj, cand[2:3], iterations=5, noise="both", seed=3)
    assert both.start_loglikel is None and np.isfinite(both.loglikel).all() and (both.kappa > 0).all() and (both.nu > 0).all()
    glob = fit.gpcc_grid_noise(obj, cand[2:3], iterations=5, noise="excess", shared=True, kappa=0.0, start=(alpha[None, :], [rho]))
    assert (glob.kappa == 0.0).all() and glob.nu[0, 0] / np.mean(s[0] ** 2) == pytest.approx(glob.nu[0, 1] / np.mean(s[1] ** 2))
    assert (glob.loglikel >= glob.start_loglikel).all()
    with pytest.raises(ValueError):
        fit.gpcc_grid_noise(obj, cand, iterations=1, noise="none")
