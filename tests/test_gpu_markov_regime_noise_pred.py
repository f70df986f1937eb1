"""The noise-model predictions, held-out scores, offsets' posterior, leave-one-out scores and draws, and the gradient of rows with their
own resampled data set, on the device over tests/_markov_regime_noise_pred_cases.py: lambda x lag down to 5e-8, 4 and 8 bands (fixed
offsets <P, 0> at 8; <3, 4> among the cases: these entries ship it) with three or more bands tied on one shifted time, subset
resampling that drops points out of a tie of three bands, rho up to 3e5 for the gradient.  Against the extended-precision references
under max(the family's existing bar, 16 e_mirror) -- no e_mirror term in the control tier (k = 0).  As in
tests/test_gpu_markov_regime_noise.py every call carries the case's row as the last of 65 (a second, ragged wave), every row with its
own (tau, alpha, rho, kappa, nu): all rows info 0 and finite, and the case's row bitwise the same row sent alone; loglik and info of
every noise entry are loglik_markov_noise_batch's bits, those of the resampled gradient loglik_markov_resampled's.  The references and
the mirror's errors are computed in a pool of CPU processes that never touch the GPU; the worst error / bar of each group is printed
with the number of (case, quantity) pairs in which the e_mirror term was active."""
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _grad_highprec as H
import _loo_highprec as LH
import _markov_regime_cases as RC
import _markov_regime_noise_cases as RN
import _markov_regime_noise_pred_cases as RP
import _markov_resample_cases as SC
import _predict_highprec as PH
import gpcc_amd

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)]

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
ROWS = RN.ROWS
K_TIERS = RC.TIERS[:4]


@pytest.fixture(scope="module")
def pool(oracle):
    """The workers reach the CPU oracle through RC._oracle(), which loads it: the session's oracle fixture has built it before they start."""
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


def alone(x):
    return tuple(v[-1:] for v in x)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("tier", K_TIERS)
def test_noise_predict_heldout_and_postb(pool, tier):
    """predict_markov_noise_batch, heldout_loglik_markov_noise_batch and posterior_offsets_markov_noise_batch (marginalised b)."""
    cases = RP.small(tier)
    refs = list(pool.map(RP.predict_job, cases))
    assert len(cases) == 9 and sum(1 for c in cases if not RC.ships_hessian(c)) == 1      # <3, 4> is compared like the others
    worst = {w: RC.Worst("device noise %s, tier %s" % (w, tier)) for w in ("predict", "held-out", "postb")}
    for case, (ref, mirror) in zip(cases, refs):
        cid, k, data, delays, alpha, rho, mb, N, kappa, nu = case
        tests = RC.TESTS[cid]
        d, a, r, kap, exc = args = RN.batch(case, seed=300 + len(alpha))
        d1, a1, r1, kap1, exc1 = alone(args)
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            vl, vinfo = obj.loglik_markov_noise_batch(*args)
            mu, var, pl, pinfo, _, _ = obj.predict_markov_noise_batch(d, a, r, tests[0], kap, exc)
            held, hl, hinfo, _ = obj.heldout_loglik_markov_noise_batch(d, a, r, *tests, kap, exc)
            mu1, var1, _, _, _, _ = obj.predict_markov_noise_batch(d1, a1, r1, tests[0], kap1, exc1)
            held1 = obj.heldout_loglik_markov_noise_batch(d1, a1, r1, *tests, kap1, exc1)[0]
            got = {"mu": mu[-1], "var": var[-1], "held": held[-1]}
            assert (vinfo == 0).all() and same(pinfo, vinfo) and same(hinfo, vinfo) and same(pl, vl) and same(hl, vl), cid
            assert same(mu1[0], mu[-1]) and same(var1[0], var[-1]) and held1[0] == held[-1], cid
            assert np.isfinite(vl).all() and np.isfinite(mu).all() and np.isfinite(var).all() and np.isfinite(held).all(), cid
            if mb:
                pmu, pS, bl, binfo = obj.posterior_offsets_markov_noise_batch(d, a, r, kap, exc)
                p1 = obj.posterior_offsets_markov_noise_batch(d1, a1, r1, kap1, exc1)
                assert same(binfo, vinfo) and same(bl, vl) and same(p1[0][0], pmu[-1]) and same(p1[1][0], pS[-1]), cid
                assert np.isfinite(pmu).all() and np.isfinite(pS).all(), cid
                got["pmu"], got["pS"] = pmu[-1], pS[-1]
        em = RP.e_mirror(ref, mirror)
        assert set(got) == set(ref.bar) == set(em) and ref.second == "mirror", cid
        for q, value in got.items():
            RC.add_pair(worst[RP.GROUP[q]], cid, q, PH.err(value, getattr(ref, q)), ref.bar[q], em[q])
    assert worst["postb"].pairs == 2 * 6
    RC.report(worst.values())


@pytest.mark.parametrize("tier", K_TIERS)
def test_noise_leave_one_out(pool, tier):
    """loo_markov_noise_batch: the case's row and its second row (1.3 kappa, nu + 0.01; weights 0.75, 0.25) behind 63 rows of weight 0;
    the two rows sent alone give the same bits, the mixture included."""
    cases = RP.small(tier)
    refs = list(pool.map(RP.loo_job, cases))
    worst = RC.Worst("device noise leave-one-out, tier %s" % tier)
    for case, (ref, mirror) in zip(cases, refs):
        (cid, k, data, delays, alpha, rho, mb, N), kappa, nu = RP.loo_entry(case)
        L = alpha.shape[1]
        d, a, r, kap, exc = (x[:ROWS - 2] for x in RN.batch(case, seed=400 + L))
        d, a, r = np.concatenate([d, delays]), np.concatenate([a, alpha]), np.concatenate([r, rho])
        kap, exc = np.concatenate([kap, kappa]), np.concatenate([exc, nu])
        w = np.concatenate([np.zeros(ROWS - 2), LH.WEIGHTS])
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            vl, vinfo = obj.loglik_markov_noise_batch(d, a, r, kap, exc)
            res = obj.loo_markov_noise_batch(d, a, r, kap, exc, weights=w)
            two = obj.loo_markov_noise_batch(d[-2:], a[-2:], r[-2:], kap[-2:], exc[-2:], weights=LH.WEIGHTS)
        assert len(vl) == ROWS and (vinfo == 0).all() and same(res.info, vinfo) and same(res.loglik, vl), cid
        assert all(np.isfinite(x).all() for x in (vl, res.mu, res.var, res.lp, res.loo, res.mix_lp)) and np.isfinite(res.mix_loo), cid
        got = {"mu": res.mu[-2:], "var": res.var[-2:], "lp": res.lp[-2:], "loo": res.loo[-2:], "mix_lp": res.mix_lp, "mix_loo": res.mix_loo}
        alone2 = {"mu": two.mu, "var": two.var, "lp": two.lp, "loo": two.loo, "mix_lp": two.mix_lp, "mix_loo": two.mix_loo}
        em = RP.e_mirror(ref, mirror)
        for q in LH.QUANTITIES:
            assert same(np.asarray(got[q]), np.asarray(alone2[q])), (cid, q)
            RC.add_pair(worst, cid, "loo " + q, PH.err(got[q], getattr(ref, q)), ref.bar[q], em[q])
    assert worst.pairs == 9 * len(LH.QUANTITIES)
    RC.report([worst])


@pytest.mark.parametrize("tier", K_TIERS)
def test_noise_draws(pool, tier):
    """sample_markov_noise_batch, 3 draws of every row: the case's row is row 64, so its normals are those of (seed, row 64) -- the
    reference is built for that row, and a row sent alone (row 0, other normals) is another draw.  The latent curve (sigmatest=None) on
    the odd-numbered cases.  loglik and info are the noise value entry's, and those of the case's row sent alone are row 64's bits."""
    cases = RP.small(tier)
    refs = list(pool.map(RP.sample_job, [(c, i) for i, c in enumerate(cases)]))
    worst = RC.Worst("device noise draws, tier %s" % tier)
    S = RP.S
    latent = 0
    for i, (case, (ref, mirror)) in enumerate(zip(cases, refs)):
        (cid, k, data, delays, alpha, rho, mb, tests), kappa, nu = RP.sample_entry(case, i)
        d, a, r, kap, exc = args = RN.batch(case, seed=500 + len(alpha))
        latent += tests[2] is None
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            vl, vinfo = obj.loglik_markov_noise_batch(*args)
            draws, rows, ll, info = obj.sample_markov_noise_batch(d, a, r, kap, exc, tests[0], S, RP.SAMPLE_SEED + i, sigmatest=tests[2])
            dr1, _, l1, i1 = obj.sample_markov_noise_batch(*alone(args), tests[0], S, RP.SAMPLE_SEED + i, sigmatest=tests[2])
        assert l1[0] == ll[-1] and i1[0] == 0 and dr1.shape == (S, draws.shape[1]) and np.isfinite(dr1).all(), cid
        assert (vinfo == 0).all() and same(info, vinfo) and same(ll, vl) and np.isfinite(vl).all() and np.isfinite(draws).all(), cid
        assert draws.shape == (ROWS * S, sum(len(x) for x in tests[0])) and same(rows, np.repeat(np.arange(ROWS), S)), cid
        assert ref.second == "mirror" and (tests[2] is None) == bool(i % 2), cid
        RC.add_pair(worst, cid, "draws", PH.err(draws[-S:], ref.draws), ref.bar, float(np.max(PH.err(mirror, ref.draws))))
    assert latent == 4 and worst.pairs == 9
    RC.report([worst])


@pytest.mark.parametrize("tier", RC.TIERS)
def test_resampled_gradient(pool, tier):
    """loglik_grad_markov_resampled on every cell of the N <= 120 cases (k tiers) and on the "flux + subset" cell of the N = 370 cases
    (rho tiers), each cell with its own center and sigma_b, against the gradient of the reduced fresh data set in all 2L + 1 entries
    (OU's tau entries at its ties: the mean of the two tie orders): 64 rows with their own (tau, alpha, rho) on the cells in turn, then
    the case's row once per cell."""
    cases = RN.resample_cases(tier)
    assert len(cases) == (9 if tier in K_TIERS else 6)
    refs = RP.regrad_references(pool, cases)
    worst = RC.Worst("device resampled gradient, tier %s" % tier)
    for case in cases:
        cid, k, data, delays, alpha, rho, mb, N = case
        L = len(alpha)
        cells = RN.cells(case)
        Y, counts = RN.realisations(case)
        d, a, r = RN.batch(RN.noise_case(case), seed=700 + L)[:3]
        nc = len(cells)
        D, A, Rh = (np.concatenate([x[:-1]] + [x[-1:]] * nc) for x in (d, a, r))
        real = np.concatenate([np.array(cells)[np.arange(ROWS - 1) % nc], cells])
        last = slice(ROWS - 1, None)
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            vl, vinfo = obj.loglik_markov_resampled(Y, D, A, Rh, real, counts=counts)
            ll, grad, info = obj.loglik_grad_markov_resampled(Y, D, A, Rh, real, counts=counts)
            l1, g1, i1 = obj.loglik_grad_markov_resampled(Y, D[last], A[last], Rh[last], real[last], counts=counts)
        assert (info == 0).all() and same(info, vinfo) and same(ll, vl) and np.isfinite(ll).all(), cid
        assert grad.shape == (ROWS - 1 + nc, 2 * L + 1) and np.isfinite(grad).all(), cid
        assert same(l1, ll[last]) and same(g1, grad[last]) and (i1 == 0).all(), cid
        for j, c in enumerate(cells):
            ref, mll, mg = refs[(cid, c)]
            RC.add_pair(worst, cid, "cell %d (%s)" % (c, SC.KINDS[c]), RP.grad_error(grad[ROWS - 1 + j], ref), H.bar(ref), RP.grad_error(mg, ref))
    assert worst.pairs == sum(len(RN.cells(c)) for c in cases)
    RC.report([worst])
