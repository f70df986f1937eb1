"""The numpy mirror of the linear-time Hessian under a per-row noise model (gpcc_amd.markov.loglik_hess_noise) on the
CPU: every block against the extended-precision reference on the effective error bars under the reference's own bars
(tests/_markov_noise_hess_cases.py), every injected slip rejected, the plain model and the contract -- a row's leading block is a
fresh data set's on effective_std -- and the outputs' contract."""
import math
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _hess_highprec as HH
import _markov_cases as MC
import _markov_grad_cases as GC
import _markov_noise_cases as NC
import _markov_noise_hess_cases as NH
from gpcc_amd import markov

extended = pytest.mark.skipif(not HH.EXTENDED, reason=HH.SKIP_REASON)


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


@pytest.fixture(scope="module")
def references(pool):
    """{case id: NoiseReference} of the 144 cases."""
    cases = NH.cases()
    refs = list(pool.map(NH.reference_job, [NH.job(c) for c in cases]))
    for c, r in zip(cases, refs):
        assert r.info == 0, c[0]
    return dict(zip((c[0] for c in cases), refs))


# ---- the mirror against the extended-precision reference ------------------------------------------------------------------------
@extended
def test_mirror_against_extended_reference(pool, references):
    cases = NH.cases()
    assert len(cases) == 144
    worst = {b: GC.Worst("mirror noise Hessian block %s" % b) for b in NH.BLOCKS}
    for case, (ll, g, H, info) in zip(cases, pool.map(NH.mirror_job, cases)):
        cid, L = case[0], len(case[4])
        assert info == 0 and H.shape == (3 * L + 1, 3 * L + 1) and np.array_equal(H, H.T), cid
        for b, r in NH.ratios(H, references[cid], case).items():
            worst[b].add(r, cid)
    for w in worst.values():
        w.report()


# ---- every slip misses a bar ----------------------------------------------------------------------------------------------------
# Where a slip cannot show: "kappa_linear" on a case whose every kappa is 0 (the one-band cases with the global-noise shape): dvar =
# kappa sigma^2 and 2 kappa sigma^2 are both 0; "noise_noise_diag_only" with one band: there is no pair of noise parameters on two
# bands.  There the slip must change nothing that is observed.  Every slip shows on every kernel.
def _shows(slip, case):
    kappa = case[8]
    if slip == "kappa_linear":
        return bool(np.any(kappa != 0.0))
    if slip == "noise_noise_diag_only":
        return len(kappa) > 1
    return True


@extended
def test_every_slip_misses_a_bar(pool, references):
    """Each slip on every third case at N = 110 (24 cases: all kernels, band counts and both b-modes): it misses a bar on EVERY case it
    can show on -- more than the one case per kernel that is asked for -- and changes nothing observed where it cannot."""
    cases = NH.cases(110)[::3]
    assert {c[1] for c in cases} == set(MC.KERNELS) and {len(c[4]) for c in cases} == {1, 2, 3}
    for slip in NH.SLIPS:
        jobs = [(c[1], *c[2], c[3], c[4], c[5], c[8], c[9], c[6], slip) for c in cases]
        closest, shown = math.inf, {k: 0 for k in MC.KERNELS}
        for case, (_, _, H, info) in zip(cases, pool.map(NH.hess_noise_job, jobs)):
            assert info == 0
            r = NH.worst(NH.ratios(H, references[case[0]], case))
            if _shows(slip, case):
                closest = min(closest, r)
                shown[case[1]] += 1
                assert r > 1.0, (slip, case[0], r)
            else:
                assert r <= 1.0, (slip, case[0], r)
        assert all(v > 0 for v in shown.values()), (slip, shown)
        print("slip %-22s closest miss: error / bar %.3g (cases per kernel %s)" % (slip, closest, shown))


# ---- the plain model, and the contract on a fresh data set ------------------------------------------------------------------------
@extended
def test_plain_model_and_the_fresh_handle_contract(pool, references):
    """On every sixth case at N = 110.  At kappa = 1, nu = 0 the leading (L+1)^2 block is loglik_hess_hyper's within the plain block's
    bars (_hess_highprec.add_bars on the reported error bars); with the case's noise model it is loglik_hess_hyper's on effective_std
    within the case's bars: the value of a fresh handle."""
    import _markov_hess_cases as HC
    cases = NH.cases(110)[::6]
    plain = list(pool.map(HH.reference_job, [HC.job(c[:8]) for c in cases]))
    w0, w1 = GC.Worst("kappa = 1, nu = 0: leading block against loglik_hess_hyper"), GC.Worst("leading block against loglik_hess_hyper on effective_std")
    for case, pref in zip(cases, plain):
        cid, k, (t, y, s), delays, alpha, rho, mb, N, kappa, nu = case
        L = len(alpha)
        assert pref.info == 0
        unit = markov.loglik_hess_noise(k, t, y, s, delays, alpha, rho, None, None, mb)
        hyper = markov.loglik_hess_hyper(k, t, y, s, delays, alpha, rho, mb)
        assert unit[3] == 0 == hyper[3] and unit[0] == hyper[0] and np.array_equal(unit[1][:2 * L + 1], hyper[1])
        w0.add(HC.ratio(unit[2][:L + 1, :L + 1], pref, case[:8], against=hyper[2]), cid)
        full = markov.loglik_hess_noise(k, t, y, s, delays, alpha, rho, kappa, nu, mb)
        fresh = markov.loglik_hess_hyper(k, t, y, NC.effective(s, kappa, nu), delays, alpha, rho, mb)
        assert full[3] == 0 == fresh[3]
        ref = references[cid]
        w1.add(NH.worst(NH.ratios(full[2][:L + 1, :L + 1], ref, case, against=fresh[2])), cid)
        w1.add(NH.worst(NH.ratios(fresh[2], ref, case)), cid)
    w0.report()
    w1.report()


# ---- the outputs' contract --------------------------------------------------------------------------------------------------------
def test_outputs_codes_and_the_objective():
    t, y, s, d0 = MC.lightcurves([30, 20], seed=3, kind="plain")
    with pytest.raises(ValueError):
        markov.loglik_hess_noise("rbf", t, y, s, d0, [1.0, 1.0], 2.0)
    kap, exc = [0.8, 1.5], [0.01, 0.0]
    ll, g, H, info = markov.loglik_hess_noise("matern32", t, y, s, d0, [1.0, 1.2], 2.0, kap, exc)
    gl, gg, ginfo = markov.loglik_grad_noise("matern32", t, y, s, d0, [1.0, 1.2], 2.0, kap, exc)
    assert info == 0 == ginfo and ll == gl and np.array_equal(g, gg) and H.shape == (7, 7) and np.array_equal(H, H.T) and np.isfinite(H).all()
    # the noise noise pair on two bands is not zero: the filter couples the bands
    assert H[3, 4] != 0.0 and H[5, 6] != 0.0 and H[3, 6] != 0.0
    for args, code in ((([0.0, 1.0], 2.0, kap, exc), -1), (([1.0, 1.0], -1.0, kap, exc), -2), (([1.0, 1.0], 2.0, [-0.5, 1.0], exc), -3),
                       (([1.0, 1.0], 2.0, kap, [0.0, math.inf]), -3), (([0.0, 1.0], 2.0, [-1.0, 1.0], exc), -1)):
        ll, g, H, info = markov.loglik_hess_noise("OU", t, y, s, d0, *args)
        assert info == code and math.isnan(ll) and np.isnan(g).all() and np.isnan(H).all() and H.shape == (7, 7)
    obj = markov.MarkovObjective(t, y, s, "matern32")
    delays, alpha, rho = [d0, d0, d0], [[1.0, 1.2], [1.0, 1.0], [0.9, 1.1]], [2.0, 2.0, 3.0]
    kappa, nu = [[0.8, 1.5], [1.0, -1.0], [0.0, 1.0]], [[0.01, 0.0], [0.0, 0.0], [0.02, 0.01]]
    bl, bg, bh, binfo = obj.loglik_hess_markov_noise_batch(delays, alpha, rho, kappa, nu)
    assert list(binfo) == [0, -3, 0] and bh.shape == (3, 7, 7) and bg.shape == (3, 9) and np.isnan(bh[1]).all() and np.isfinite(bh[[0, 2]]).all()
    one = markov.loglik_hess_noise("matern32", t, y, s, d0, [0.9, 1.1], 3.0, [0.0, 1.0], [0.02, 0.01])
    assert bl[2] == one[0] and np.array_equal(bg[2], one[1]) and np.array_equal(bh[2], one[2])
    # central differences of the mirror's own gradient: the block's entries are derivatives of the gradient's (h = 1e-5 relative, second
    # order: truncation ~1e-10 relative, rounding ~1e-16 / 1e-5 of the gradient's size)
    x0 = np.array([1.0, 1.2, 2.0, 0.8, 1.5, 0.01, 0.005])
    ll, g, H, info = markov.loglik_hess_noise("matern32", t, y, s, d0, x0[:2], x0[2], x0[3:5], x0[5:])
    idx = [0, 1, 2, 5, 6, 7, 8]
    for i in range(7):
        e = np.zeros(7)
        e[i] = 1e-5 * x0[i]
        gp = markov.loglik_grad_noise("matern32", t, y, s, d0, (x0 + e)[:2], (x0 + e)[2], (x0 + e)[3:5], (x0 + e)[5:])[1][idx]
        gm = markov.loglik_grad_noise("matern32", t, y, s, d0, (x0 - e)[:2], (x0 - e)[2], (x0 - e)[3:5], (x0 - e)[5:])[1][idx]
        fd = (gp - gm) / (2 * e[i])
        assert np.max(np.abs(fd - H[i])) <= 1e-6 * np.max(np.abs(H)), (i, fd, H[i])
    # five bands: with marginalised offsets refused, without them fine
    t5, y5, s5, d5 = MC.lightcurves([30, 25, 20, 25, 30], seed=12, kind="ties")
    a5 = np.linspace(0.6, 1.4, 5)
    with pytest.raises(ValueError):
        markov.loglik_hess_noise("OU", t5, y5, s5, d5, a5, 2.0, None, None, True)
    assert markov.loglik_hess_noise("OU", t5, y5, s5, d5, a5, 2.0, None, None, False)[2].shape == (16, 16)
