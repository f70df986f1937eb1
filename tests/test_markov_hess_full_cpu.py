"""The linear-time full Hessian's numpy mirror (gpcc_amd.markov.loglik_hess: the rows of tau) on the CPU: all six blocks
against the extended-precision reference under its own per-block bars times the filter's conditioning factor
(tests/_markov_hess_full_cases.py), the NaN contract on OU rows with a cross-band tie, every injected slip rejected in the blocks it
touches with the (alpha, rho) block's bits unchanged, the outputs' contract, and fit.delay_covariance over the mirror."""
import math
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _hess_highprec as HH
import _markov_cases as MC
import _markov_hess_full_cases as FC
from gpcc_amd import fit, markov, synthetic

extended = pytest.mark.skipif(not HH.EXTENDED, reason=HH.SKIP_REASON)


@pytest.fixture(scope="module")
def references():
    """{case id: Reference with its bars over the six blocks} of the 144 cases."""
    cases = FC.cases()
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as pool:
        refs = list(pool.map(FC.reference_job, [FC.job(c) for c in cases]))
    for c, r in zip(cases, refs):
        assert r.info == 0, c[0]
    return dict(zip((c[0] for c in cases), refs))


@extended
def test_mirror_against_extended_reference(references):
    """132 cases within 1 bar in every block; the 12 OU cases with a tie: NaN in every tau entry, info 0, the leading block
    loglik_hess_hyper's."""
    cases = FC.cases()
    assert len(cases) == 144
    worst = {(k, b): FC.Worst("mirror Hessian %s %s" % (k, b)) for k in MC.KERNELS for b in HH.BLOCKS}
    tied = 0
    for case in cases:
        cid, k, data, delays, alpha, rho, mb, _ = case
        L = len(alpha)
        ll, g, H, info = markov.loglik_hess(k, *data, delays, alpha, rho, mb)
        hl, hg, hyper, hinfo = markov.loglik_hess_hyper(k, *data, delays, alpha, rho, mb)
        assert info == 0 == hinfo and ll == hl and np.array_equal(g, hg), cid
        assert np.array_equal(H[:L + 1, :L + 1], hyper) and np.array_equal(H, H.T, equal_nan=True) and H.shape == (2 * L + 1, 2 * L + 1), cid
        ref = references[cid]
        if FC.ou_tie(case):
            tied += 1
            assert ref.ties, cid
            tau = np.zeros(H.shape, bool)
            tau[L + 1:, :] = tau[:, L + 1:] = True
            assert np.isnan(H[tau]).all() and np.isfinite(H[~tau]).all(), cid
            continue
        assert np.isfinite(H).all(), cid
        if L == 1:
            assert not H[2, :].any() and not H[:, 2].any(), cid          # exact zeros
        for b, r in FC.ratios(H, ref, case).items():
            worst[(k, b)].add(r, cid)
    assert tied == 12
    for w in worst.values():
        w.report()


@extended
def test_every_slip_misses_the_bar(references):
    """Each slip over the N = 110 cases with L >= 2 and without an OU tie (42): it misses the bar in every block it touches on at least
    40 of them and leaves the (alpha, rho) block's bits unchanged."""
    cases = [c for c in FC.cases(110) if len(c[4]) >= 2 and not FC.ou_tie(c)]
    assert len(cases) == 42
    good = {c[0]: markov.loglik_hess(c[1], *c[2], c[3], c[4], c[5], c[6])[2] for c in cases}
    for slip, blocks in FC.SLIPS.items():
        missed = dict.fromkeys(blocks, 0)
        closest = dict.fromkeys(blocks, math.inf)
        for case in cases:
            cid, k, data, delays, alpha, rho, mb, _ = case
            L = len(alpha)
            H = markov.loglik_hess(k, *data, delays, alpha, rho, mb, _slip=slip)[2]
            assert np.array_equal(H[:L + 1, :L + 1], good[cid][:L + 1, :L + 1]), (slip, cid)
            r = FC.ratios(H, references[cid], case)
            for b in blocks:
                if r[b] > 1.0:
                    missed[b] += 1
                    closest[b] = min(closest[b], r[b])
        print("slip %-12s cases missed of 42: %s; closest miss: %s" % (slip, missed, {b: "%.3g" % v for b, v in closest.items()}))
        for b in blocks:
            assert missed[b] >= 40, (slip, b, missed[b])


def test_outputs_codes_and_the_objective():
    t, y, s, d0 = MC.lightcurves([30, 20], seed=3, kind="plain")
    with pytest.raises(ValueError):
        markov.loglik_hess("rbf", t, y, s, d0, [1.0, 1.0], 2.0)
    ll, g, H, info = markov.loglik_hess("matern32", t, y, s, d0, [1.0, 1.2], 2.0)
    gl, gg, ginfo = markov.loglik_grad("matern32", t, y, s, d0, [1.0, 1.2], 2.0)
    hyper = markov.loglik_hess_hyper("matern32", t, y, s, d0, [1.0, 1.2], 2.0)[2]
    assert info == 0 == ginfo and ll == gl and np.array_equal(g, gg) and H.shape == (5, 5) and np.array_equal(H, H.T)
    assert np.isfinite(H).all() and np.array_equal(H[:3, :3], hyper)
    # a common shift of every delay changes nothing: the tau rows sum to zero (up to rounding of sums of entries of this size)
    assert np.max(np.abs(H[:, 3:].sum(1))) <= 1e-9 * np.max(np.abs(H))
    for args, code in ((([0.0, 1.0], 2.0), -1), (([1.0, 1.0], -1.0), -2)):
        ll, g, H, info = markov.loglik_hess("OU", t, y, s, d0, *args)
        assert info == code and math.isnan(ll) and np.isnan(g).all() and np.isnan(H).all() and H.shape == (5, 5)
    # one band: every c is 0, the tau entries are exact zeros
    t1, y1, s1, d1 = MC.lightcurves([40], seed=4, kind="plain")
    H1 = markov.loglik_hess("OU", t1, y1, s1, d1, [1.1], 2.0)[2]
    assert H1.shape == (3, 3) and np.isfinite(H1).all() and not H1[2, :].any() and not H1[:, 2].any()
    # an OU tie made by hand: the delay equals a difference of two observation times
    tie = np.array([0.0, t[1][3] - t[0][5]])
    assert t[1][3] - tie[1] == t[0][5]
    ll, g, H, info = markov.loglik_hess("OU", t, y, s, tie, [1.0, 1.2], 2.0)
    assert info == 0 and np.isfinite(ll) and np.isfinite(g).all() and np.isfinite(H[:3, :3]).all()
    assert np.isnan(H[3:, :]).all() and np.isnan(H[:, 3:]).all()
    assert np.isfinite(markov.loglik_hess("matern32", t, y, s, tie, [1.0, 1.2], 2.0)[2]).all()
    obj = markov.MarkovObjective(t, y, s, "matern32")
    delays, alpha, rho = [d0, d0, d0], [[1.0, 1.2], [0.0, 1.0], [0.9, 1.1]], [2.0, 2.0, 3.0]
    bl, bg, bh, binfo = obj.loglik_hess_markov_batch(delays, alpha, rho)
    assert list(binfo) == [0, -1, 0] and bh.shape == (3, 5, 5) and bg.shape == (3, 5) and np.isnan(bh[1]).all()
    one = markov.loglik_hess("matern32", t, y, s, d0, [0.9, 1.1], 3.0)
    assert bl[2] == one[0] and np.array_equal(bg[2], one[1]) and np.array_equal(bh[2], one[2])
    t5, y5, s5, d5 = MC.lightcurves([30, 25, 20, 25, 30], seed=12, kind="ties")
    with pytest.raises(ValueError):
        markov.loglik_hess("OU", t5, y5, s5, d5, np.linspace(0.6, 1.4, 5), 2.0, True)


def test_delay_covariance_over_the_mirror():
    """fit.delay_covariance over MarkovObjective at the README size: the covariance of (alpha, rho, tau_2) is laplace_covariance of the
    mirror's Hessian, ok = False where an entry it needs is NaN (OU at a tie) or the point cannot be evaluated, ValueError for another
    solver or a free set with every delay."""
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    delays = np.array(FC.README_DELAYS)
    a0, r0 = FC.README_MODE["matern32"]
    obj = markov.MarkovObjective(t, y, s, "matern32")
    cov, ok = fit.delay_covariance(obj, delays, a0, r0, solver="markov")
    H = markov.loglik_hess("matern32", t, y, s, delays, a0, r0)[2]
    want, wok = fit.laplace_covariance(H, [0, 1, 2, 4])
    assert ok and wok and cov.shape == (4, 4) and np.array_equal(cov, want) and (np.diag(cov) > 0).all()
    only, ok1 = fit.delay_covariance(obj, delays, a0, r0, free=[4], solver="markov")
    assert ok1 and only[0, 0] == pytest.approx(-1.0 / H[4, 4], rel=1e-12)
    with pytest.raises(ValueError):
        fit.delay_covariance(obj, delays, a0, r0, solver="sparse")
    with pytest.raises(ValueError):
        fit.delay_covariance(obj, delays, a0, r0, free=[0, 3, 4], solver="markov")
    bad, okb = fit.delay_covariance(obj, delays, [0.0, 1.0], r0, solver="markov")
    assert not okb and np.isnan(bad).all() and bad.shape == (4, 4)
    ou = markov.MarkovObjective(t, y, s, "OU")
    a0, r0 = FC.README_MODE["OU"]
    assert fit.delay_covariance(ou, delays, a0, r0, solver="markov")[1]
    ts = [np.sort(np.asarray(a, np.float64)) for a in t]
    tie = np.array([0.0, ts[1][7] - ts[0][9]])
    nan, okt = fit.delay_covariance(ou, tie, a0, r0, solver="markov")
    assert FC.tie_rows(t, tie)[0] and not okt and np.isnan(nan).all()
    hyper, okh = fit.delay_covariance(ou, tie, a0, r0, free=[0, 1, 2], solver="markov")      # (needs no tau entry: never NaN by the tie)
    assert okh == fit.laplace_covariance(markov.loglik_hess_hyper("OU", t, y, s, tie, a0, r0)[2], [0, 1, 2], L=2)[1]
    assert np.isfinite(hyper).all() == okh
