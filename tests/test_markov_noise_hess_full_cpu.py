"""The numpy mirror of the linear-time full Hessian under a per-row noise model (gpcc_amd.markov.loglik_hess_full_noise)
on the CPU: every block against the extended-precision reference on the effective error bars under the reference's own bars
(tests/_markov_noise_hess_full_cases.py), the NaN contract on the OU rows with a cross-band tie, every injected slip rejected, the
sub-blocks that other entries own, and fit.delay_covariance with a noise model on a MarkovObjective."""
import math
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _hess_highprec as HH
import _markov_cases as MC
import _markov_grad_cases as GC
import _markov_noise_cases as NC
import _markov_noise_hess_full_cases as NF
from gpcc_amd import fit, markov, synthetic

extended = pytest.mark.skipif(not HH.EXTENDED, reason=HH.SKIP_REASON)


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


@pytest.fixture(scope="module")
def split():
    """(the 132 cases held to their bars, the 12 OU cases with a cross-band tie)."""
    cases = NF.cases()
    ties = [c for c in cases if NF.is_tie(c)]
    assert len(cases) == 144 and len(ties) == 12
    assert all(c[0].endswith("-ties") and c[1] == "OU" for c in ties)
    assert sum(c[7] == 110 for c in ties) == 6
    return [c for c in cases if not NF.is_tie(c)], ties


@pytest.fixture(scope="module")
def references(pool, split):
    """{case id: NoiseReference over 4L + 1} of the 132 cases."""
    held = split[0]
    refs = list(pool.map(NF.reference_job, [NF.job(c) for c in held]))
    for c, r in zip(held, refs):
        assert r.info == 0, c[0]
    return dict(zip((c[0] for c in held), refs))


@pytest.fixture(scope="module")
def mirrors(pool, split):
    """{case id: (loglik, grad, hess, info)} of markov.loglik_hess_full_noise on all 144 cases."""
    cases = split[0] + split[1]
    return dict(zip((c[0] for c in cases), pool.map(NF.mirror_job, cases)))


# ---- the mirror against the extended-precision reference ------------------------------------------------------------------------
@extended
def test_mirror_against_extended_reference(split, references, mirrors):
    held = split[0]
    assert len(held) == 132
    worst = {b: GC.Worst("mirror full noise Hessian block %s" % b) for b in NF.BLOCKS}
    for case in held:
        cid, L = case[0], len(case[4])
        ll, g, H, info = mirrors[cid]
        assert info == 0 and H.shape == (4 * L + 1, 4 * L + 1) and np.array_equal(H, H.T) and np.isfinite(H).all(), cid
        r = NF.ratios(H, references[cid], case)
        assert set(r) == set(NF.BLOCKS), cid
        for b, v in r.items():
            worst[b].add(v, cid)
    for w in worst.values():
        w.report()


def test_nan_contract_on_the_tie_cases(split, mirrors):
    """OU with a cross-band tie: every entry with a tau index is NaN, info stays 0, value, gradient and the [alpha, rho, kappa, nu]
    sub-block are loglik_hess_noise's."""
    for case in split[1]:
        cid, kernel, data, delays, alpha, rho, mb, N, kappa, nu = case
        L = len(alpha)
        ll, g, H, info = mirrors[cid]
        assert info == 0 and math.isfinite(ll) and np.isfinite(g).all(), cid
        tm = NF.tau_mask(L)
        assert np.isnan(H[tm]).all() and np.isfinite(H[~tm]).all(), cid
        nl, ng, nH, ninfo = markov.loglik_hess_noise(kernel, *data, delays, alpha, rho, kappa, nu, mb)
        ix = NF.noise_index(L)
        assert ninfo == 0 and nl == ll and np.array_equal(ng, g) and np.array_equal(H[np.ix_(ix, ix)], nH), cid


# ---- the sub-blocks that other entries own ----------------------------------------------------------------------------------------
def test_common_sub_block_is_loglik_hess_noise_exactly(split, mirrors):
    """On the indices {0..L, 2L+1..4L} the block equals markov.loglik_hess_noise's exactly; value and gradient are loglik_grad_noise's.
    Every twelfth case (12 cases: all kernels and band counts)."""
    cases = (split[0] + split[1])[::12]
    assert {c[1] for c in cases} == set(MC.KERNELS) and {len(c[4]) for c in cases} == {1, 2, 3}
    for case in cases:
        cid, kernel, data, delays, alpha, rho, mb, N, kappa, nu = case
        L = len(alpha)
        ll, g, H, info = mirrors[cid]
        nl, ng, nH, ninfo = markov.loglik_hess_noise(kernel, *data, delays, alpha, rho, kappa, nu, mb)
        ix = NF.noise_index(L)
        assert info == 0 == ninfo and nl == ll and np.array_equal(ng, g) and np.array_equal(H[np.ix_(ix, ix)], nH), cid


@extended
def test_plain_model_leading_block_is_loglik_hess(pool, split):
    """At kappa = 1, nu = 0 the leading (2L+1)^2 block is markov.loglik_hess's within 2 bars of the plain full Hessian's reference
    (_markov_hess_full_cases: both sides are held to 1 bar of it).  Every sixth case at N = 110 that is not a tie case."""
    import _markov_hess_full_cases as FC
    cases = [c for c in NF.cases(110) if not NF.is_tie(c)][::6]
    plain = list(pool.map(FC.reference_job, [FC.job(c[:8]) for c in cases]))
    w = GC.Worst("kappa = 1, nu = 0: leading block against loglik_hess")
    for case, pref in zip(cases, plain):
        cid, k, (t, y, s), delays, alpha, rho, mb, N, kappa, nu = case
        L = len(alpha)
        assert pref.info == 0
        unit = markov.loglik_hess_full_noise(k, t, y, s, delays, alpha, rho, None, None, mb, pairs=NF.pairs_of(L, ("aa", "ar", "rr", "at", "rt", "tt")))
        full = markov.loglik_hess(k, t, y, s, delays, alpha, rho, mb)
        assert unit[3] == 0 == full[3] and unit[0] == full[0] and np.array_equal(unit[1][:2 * L + 1], full[1])
        w.add(max(FC.ratios(unit[2][:2 * L + 1, :2 * L + 1], pref, case[:8], against=full[2]).values()), cid, limit=2.0)
    w.report()


def test_one_band_tau_entries_are_exact_zeros(split, mirrors):
    seen = 0
    for case in split[0]:
        if len(case[4]) != 1:
            continue
        H = mirrors[case[0]][2]
        assert H.shape == (5, 5) and np.all(H[NF.tau_mask(1)] == 0.0), case[0]
        seen += 1
    assert seen >= 40


# ---- every slip misses a bar ----------------------------------------------------------------------------------------------------
@extended
def test_every_slip_misses_a_bar(pool, split, references):
    """Each slip on every third held case at N = 110 with more than one band (with one band every tau entry is an exact zero whatever
    the slip): the pairs of the blocks it touches alone are walked (pairs=).  It must exceed the bar of a block it touches on at least
    one case of every kernel; the case and the factor are named."""
    cases = [c for c in split[0] if c[7] == 110 and len(c[4]) > 1][::3]
    assert {c[1] for c in cases} == set(MC.KERNELS) and {len(c[4]) for c in cases} == {2, 3}
    for slip, blocks in NF.SLIPS.items():
        jobs = [(c, slip, NF.pairs_of(len(c[4]), blocks)) for c in cases]
        best, missed = (0.0, None), {k: 0 for k in MC.KERNELS}
        for case, (_, _, H, info) in zip(cases, pool.map(NF.slip_job, jobs)):
            assert info == 0
            r = NF.worst(NF.ratios(H, references[case[0]], case, blocks=blocks))
            if r > best[0]:
                best = (r, case[0])
            missed[case[1]] += r > 1.0
        print("slip %-20s largest miss: error / bar %.3g on %s (cases over the bar per kernel: %s of %d)" % (slip, best[0], best[1], missed, len(cases)))
        assert all(v > 0 for v in missed.values()), (slip, best, missed)


# ---- fit.delay_covariance with a noise model --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def readme():
    """The README-size data, the point (README_DELAYS, README_MODE["matern32"]) and its MarkovObjective."""
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    alpha, rho = NF.README_MODE["matern32"]
    return (t, y, s), np.array(NF.README_DELAYS), np.array(alpha), rho, markov.MarkovObjective(t, y, s, "matern32")


def _readme_case(readme, kappa, nu):
    data, delays, alpha, rho, _ = readme
    return ("readme-matern32", "matern32", data, delays, alpha, rho, True, 110, np.asarray(kappa, np.float64), np.asarray(nu, np.float64))


@extended
def test_delay_covariance_noise_fixed_is_the_fresh_objective(readme):
    """noise_free all False: the covariance over (alpha, rho, tau_2) at a fixed noise model is delay_covariance of a fresh
    MarkovObjective on effective_std.  PROPAGATION: both Hessians are within 1 bar per block of the reference on effective_std (the
    first test's claim), so their entries differ by at most E = 2 bar_B / scale, B the entry's block (aa, ar, rr, at, rt, tt); cov =
    (-H_ff)^-1 then differs entrywise by at most _markov_noise_hess_full_cases.inverse_bound(cov, E) = 2 |cov| E |cov|."""
    data, delays, alpha, rho, obj = readme
    kappa, nu = [1.2, 0.9], [0.01, 0.02]
    case = _readme_case(readme, kappa, nu)
    ref = NF.reference_job(NF.job(case))
    assert ref.info == 0
    cov, ok = fit.delay_covariance(obj, delays, alpha, rho, solver="markov", kappa=kappa, nu=nu, noise_free=[False] * 4)
    fresh = markov.MarkovObjective(data[0], data[1], NC.effective(data[2], kappa, nu), "matern32")
    cov0, ok0 = fit.delay_covariance(fresh, delays, alpha, rho, solver="markov")
    assert ok and ok0 and cov.shape == (4, 4) == cov0.shape
    free = [0, 1, 2, 4]
    E = NF.entry_bars(ref, case, 2.0)[np.ix_(free, free)]
    bound = NF.inverse_bound(cov0, E)
    print("noise fixed: largest |cov - cov_fresh| / bound %.3g (delay variance %.6g)" % (float(np.max(np.abs(cov - cov0) / bound)), cov[3, 3]))
    assert np.all(np.abs(cov - cov0) <= bound)


def test_delay_variance_grows_with_a_free_noise_model(readme):
    """kappa free at kappa = 1.2, nu = 0.01: both results are ok and the delay's variance is not smaller than with the noise fixed.  For
    any positive definite A = -H the block of A^-1 over a subset dominates the inverse of A's block over it (Schur complement), so the
    claim needs no tolerance beyond the rounding of the two Cholesky solves: 64 eps cond_2(A) relative."""
    data, delays, alpha, rho, obj = readme
    kappa, nu = [1.2, 1.2], [0.01, 0.01]
    fixed, ok0 = fit.delay_covariance(obj, delays, alpha, rho, solver="markov", kappa=kappa, nu=nu, noise_free=[False] * 4)
    free, ok1 = fit.delay_covariance(obj, delays, alpha, rho, solver="markov", kappa=kappa, nu=nu, noise_free=[True, True, False, False])
    assert ok0 and ok1 and fixed.shape == (4, 4) and free.shape == (6, 6)
    cond = np.linalg.cond(free)
    print("delay variance: noise fixed %.8g, kappa free %.8g, cond %.3g" % (fixed[3, 3], free[3, 3], cond))
    assert free[3, 3] >= fixed[3, 3] * (1.0 - 64 * 2.0 ** -53 * cond)
    # the default noise_free: every kappa_l > 0 and nu_l > 0
    full, ok2 = fit.delay_covariance(obj, delays, alpha, rho, solver="markov", kappa=kappa, nu=nu)
    assert full.shape == (8, 8) and (not ok2 or full[3, 3] >= free[3, 3] * (1.0 - 64 * 2.0 ** -53 * np.linalg.cond(full)))


def test_delay_covariance_arguments(readme):
    data, delays, alpha, rho, obj = readme
    kappa, nu = [1.2, 1.2], [0.01, 0.0]
    with pytest.raises(ValueError, match="Fisher information in kappa, nu does not exist yet"):
        fit.delay_covariance(obj, delays, alpha, rho, solver="dense", kappa=kappa, nu=nu)
    with pytest.raises(ValueError, match="Fisher information in kappa, nu does not exist yet"):
        fit.delay_covariance(obj, delays, alpha, rho, solver="markov", curvature="fisher", kappa=kappa, nu=nu)
    with pytest.raises(ValueError, match="every delay"):
        fit.delay_covariance(obj, delays, alpha, rho, solver="markov", kappa=kappa, nu=nu, free=[0, 1, 2, 3, 4, 5])
    # nu_2 = 0 sits on its lower bound: left out of the default noise_free -> alpha_1, alpha_2, rho, tau_2, kappa_1, kappa_2, nu_1
    cov, ok = fit.delay_covariance(obj, delays, alpha, rho, solver="markov", kappa=kappa, nu=nu)
    same, ok2 = fit.delay_covariance(obj, delays, alpha, rho, solver="markov", kappa=kappa, nu=nu, free=[0, 1, 2, 4, 5, 6, 7])
    assert cov.shape == (7, 7) and ok == ok2 and np.array_equal(cov, same, equal_nan=True)
    # kappa given alone: nu = 0, left out
    assert fit.delay_covariance(obj, delays, alpha, rho, solver="markov", kappa=kappa)[0].shape == (6, 6)


def test_delay_covariance_without_a_noise_model_is_unchanged(readme):
    """kappa = nu = None: bitwise the result of the Hessian entry the call has always used, for both solvers' objects at hand."""
    data, delays, alpha, rho, obj = readme
    cov, ok = fit.delay_covariance(obj, delays, alpha, rho, solver="markov", kappa=None, nu=None, noise_free=None)
    _, _, H, info = obj.loglik_hess_markov_batch(delays[None, :], alpha[None, :], [rho])
    want, wok = fit.laplace_covariance(H[0], [0, 1, 2, 4], 2)
    assert info[0] == 0 and ok == wok and ok and np.array_equal(cov, want)
    fcov, fok = fit.delay_covariance(obj, delays, alpha, rho, solver="markov", curvature="fisher")
    _, _, F, _ = obj.loglik_fisher_markov_batch(delays[None, :], alpha[None, :], [rho])
    fwant, _ = fit.laplace_covariance(-F[0], [0, 1, 2, 4], 2)
    assert fok and np.array_equal(fcov, fwant)


def test_outputs_codes_pairs_and_the_objective():
    t, y, s, d0 = MC.lightcurves([30, 20], seed=3, kind="plain")
    with pytest.raises(ValueError):
        markov.loglik_hess_full_noise("rbf", t, y, s, d0, [1.0, 1.0], 2.0)
    kap, exc = [0.8, 1.5], [0.01, 0.0]
    ll, g, H, info = markov.loglik_hess_full_noise("matern32", t, y, s, d0, [1.0, 1.2], 2.0, kap, exc)
    gl, gg, ginfo = markov.loglik_grad_noise("matern32", t, y, s, d0, [1.0, 1.2], 2.0, kap, exc)
    assert info == 0 == ginfo and ll == gl and np.array_equal(g, gg) and H.shape == (9, 9) and np.array_equal(H, H.T) and np.isfinite(H).all()
    # a (tau_l, noise_m) pair on two bands is not zero: the filter couples the bands
    assert H[3, 6] != 0.0 and H[4, 5] != 0.0 and H[3, 8] != 0.0
    # a common shift of all delays changes nothing: the rows of tau sum to zero (to rounding)
    assert np.max(np.abs(H[3] + H[4])) <= 1e-9 * np.max(np.abs(H))
    some = markov.loglik_hess_full_noise("matern32", t, y, s, d0, [1.0, 1.2], 2.0, kap, exc, pairs=[(5, 3), (4, 4)])[2]
    assert some[3, 5] == H[3, 5] == some[5, 3] and some[4, 4] == H[4, 4] and np.isnan(some).sum() == 81 - 3
    for args, code in ((([0.0, 1.0], 2.0, kap, exc), -1), (([1.0, 1.0], -1.0, kap, exc), -2), (([1.0, 1.0], 2.0, [-0.5, 1.0], exc), -3)):
        ll, g, H, info = markov.loglik_hess_full_noise("OU", t, y, s, d0, *args)
        assert info == code and math.isnan(ll) and np.isnan(g).all() and np.isnan(H).all() and H.shape == (9, 9)
    obj = markov.MarkovObjective(t, y, s, "matern32")
    delays, alpha, rho = [d0, d0, d0], [[1.0, 1.2], [1.0, 1.0], [0.9, 1.1]], [2.0, 2.0, 3.0]
    kappa, nu = [[0.8, 1.5], [1.0, -1.0], [0.0, 1.0]], [[0.01, 0.0], [0.0, 0.0], [0.02, 0.01]]
    bl, bg, bh, binfo = obj.loglik_hess_full_markov_noise_batch(delays, alpha, rho, kappa, nu)
    assert list(binfo) == [0, -3, 0] and bh.shape == (3, 9, 9) and bg.shape == (3, 9) and np.isnan(bh[1]).all() and np.isfinite(bh[[0, 2]]).all()
    one = markov.loglik_hess_full_noise("matern32", t, y, s, d0, [0.9, 1.1], 3.0, [0.0, 1.0], [0.02, 0.01])
    assert bl[2] == one[0] and np.array_equal(bg[2], one[1]) and np.array_equal(bh[2], one[2])
