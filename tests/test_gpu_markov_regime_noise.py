"""The linear-time entries that take a per-row noise model or a per-row data set, on the device over tests/_markov_regime_noise_cases.py:
lambda x lag down to 5e-8, rho up to 3e5, 4 and 8 bands (fixed-offset rows <P, 0> at 8) with three or more bands tied on one shifted
time, OU twins without cross-band ties for the tau blocks, subset resampling that drops points out of a tie of three bands.  Against the
extended-precision references under max(the family's existing bar, 16 e_mirror) -- no e_mirror term in the control tier (k = 0).  As in
tests/test_gpu_markov_regime.py every call carries the case's row as the last of 65 (a second, ragged wave), every row with its own
(alpha, rho, kappa, nu): all rows info 0, and the case's row bitwise the same row sent alone.  The references and the mirror's errors
are computed in a pool of CPU processes that never touch the GPU; the worst error / bar of each group is printed with the number of
(case, quantity) pairs in which the e_mirror term was active."""
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _grad_highprec as H
import _markov_cases as MC
import _markov_hess_full_cases as FC
import _markov_noise_hess_cases as NH
import _markov_noise_hess_full_cases as NF
import _markov_regime_cases as RC
import _markov_regime_noise_cases as RN
import _markov_resample_cases as SC
import gpcc_amd

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)]

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
UNSUPPORTED = -3
ROWS = RN.ROWS
K_TIERS = RC.TIERS[:4]
BANDS = {"L2-4": (2, 4), "L8": (8,)}         # the Hessians' tests, 8 bands apart: the mirror walks 561 pairs there


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


def alone(x):
    return tuple(v[-1:] for v in x)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- value and gradient under the noise model, every case ---------------------------------------------------------------------------
@pytest.mark.parametrize("tier", RC.TIERS)
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_noise_value_and_gradient(oracle, pool, kernel, tier):
    cases = RN.cases(tier, kernel)
    assert len(cases) == len(RC.tier(tier, kernel)) >= 2
    refs = RN.grad_references(pool, cases)
    worst = {q: RC.Worst("device noise %s %s, tier %s" % (q, kernel, tier)) for q in ("value", "grad", "noise")}
    for case in cases:
        cid, k, data, delays, alpha, rho, mb, N, kappa, nu = case
        L = len(alpha)
        b = RN.GradBars(oracle, case, refs[cid])
        args = RN.batch(case, seed=L)
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll, info = obj.loglik_markov_noise_batch(*args)
            gl, grad, ginfo = obj.loglik_grad_markov_noise_batch(*args)
            l1, i1 = obj.loglik_markov_noise_batch(*alone(args))
            g1l, g1, g1i = obj.loglik_grad_markov_noise_batch(*alone(args))
        assert (info == 0).all() and np.isfinite(ll).all() and np.isfinite(grad).all() and grad.shape == (ROWS, 4 * L + 1), cid
        assert same(gl, ll) and same(ginfo, info), cid                         # value and info bitwise the same from both entries
        assert l1[0] == ll[-1] and g1l[0] == ll[-1] and i1[0] == 0 and g1i[0] == 0 and same(g1[0], grad[-1]), cid
        b.add(worst, ll[-1], grad[-1])
    RC.report(worst.values())


# ---- the two Hessians under the noise model at the N <= 120 shapes --------------------------------------------------------------------
@pytest.mark.parametrize("bands", list(BANDS))
@pytest.mark.parametrize("tier", K_TIERS)
def test_noise_hessians(pool, tier, bands):
    """loglik_hess_markov_noise_batch on aa, ar, rr, an, rn, nn and loglik_hess_full_markov_noise_batch on all ten blocks; value, gradient
    and the [alpha, rho, kappa, nu] sub-block bitwise the siblings'; <3, 4> refused by both while the gradient entry answers; OU rows with
    a cross-band tie (the case's own row always): NaN in exactly the tau rows and columns."""
    cases = [c for c in RN.cases(tier, small=True) if len(c[4]) in BANDS[bands]]
    refs = RN.hess_references(pool, cases)
    assert (len(cases), len(refs)) == ((6, 5) if bands == "L2-4" else (3, 3))
    worst = {w: RC.Worst("device %s, tier %s, %s" % (w, tier, bands)) for w in ("noise Hessian block", "full noise Hessian")}
    for case in cases:
        cid, k, data, delays, alpha, rho, mb, N, kappa, nu = case
        L = len(alpha)
        args = RN.batch(case, seed=200 + L)
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            gl, gg, ginfo = obj.loglik_grad_markov_noise_batch(*args)
            assert (ginfo == 0).all() and np.isfinite(gg).all(), cid
            if not RN.ships_hessian(case):
                for entry in (obj.loglik_hess_markov_noise_batch, obj.loglik_hess_full_markov_noise_batch):
                    with pytest.raises(gpcc_amd.GpccError) as ei:
                        entry(*args)
                    assert ei.value.code == UNSUPPORTED, cid
                assert (obj.loglik_grad_markov_noise_batch(*args)[2] == 0).all(), cid          # the handle still serves the gradient
                continue
            nl, ng, nh, ninfo = obj.loglik_hess_markov_noise_batch(*args)
            fl, fg, fh, finfo = obj.loglik_hess_full_markov_noise_batch(*args)
            n1 = obj.loglik_hess_markov_noise_batch(*alone(args))
            f1 = obj.loglik_hess_full_markov_noise_batch(*alone(args))
        ref, mh = refs[cid]
        ix = NF.noise_index(L)
        tau = NF.tau_mask(L)
        tied = FC.tie_rows(data[0], args[0]) if k == "OU" else np.zeros(ROWS, bool)
        assert tied[-1] == RN.tied(case) == (k == "OU"), cid
        for ll, grad, info in ((nl, ng, ninfo), (fl, fg, finfo)):
            assert same(ll, gl) and same(grad, gg) and same(info, ginfo), cid                   # bitwise the gradient entry's
        assert nh.shape == (ROWS, 3 * L + 1, 3 * L + 1) and fh.shape == (ROWS, 4 * L + 1, 4 * L + 1), cid
        assert same(fh[:, ix][:, :, ix], nh) and np.isfinite(nh).all(), cid
        assert same(nh, np.swapaxes(nh, 1, 2)) and same(fh, np.swapaxes(fh, 1, 2)), cid
        assert np.array_equal(np.isnan(fh), tied[:, None, None] & tau[None, :, :]), cid
        for one, many in ((n1, (nl, ng, nh, ninfo)), (f1, (fl, fg, fh, finfo))):
            assert all(same(x[0], z[-1]) for x, z in zip(one, many)), cid
        for b, e, existing, em in RN.hess_pairs(ref, case, nh[-1], mh, NH.BLOCKS, index=ix):
            RC.add_pair(worst["noise Hessian block"], cid, b, e, existing, em)
        for b, e, existing, em in RN.hess_pairs(ref, case, fh[-1], mh, NF.BLOCKS):
            RC.add_pair(worst["full noise Hessian"], cid, b, e, existing, em)
    RC.report(worst.values())


# ---- OU's tau blocks at 2, 4 and 8 bands -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bands", list(BANDS))
@pytest.mark.parametrize("tier", K_TIERS)
def test_ou_tau_blocks_without_ties(pool, tier, bands):
    """The tier's three OU twins (the one with 8 bands in a test of its own) through loglik_hess_markov_batch, loglik_fisher_markov_batch and loglik_hess_full_markov_noise_batch: the
    twin's row finite in every entry, at, rt, tt and tn held to their bars like every other block.  At L = 8 the 28 off-diagonal
    (tau, tau) reference entries are pairwise distinct by more than their bar, so a wrong decoding of a pair's slot cannot pass by a
    symmetry of the data."""
    twins = [c for c in RN.twins(tier) if len(c[4]) in BANDS[bands]]
    assert [len(c[4]) for c in twins] == list(BANDS[bands])
    refs = RN.hess_references(pool, twins)
    plain = RC.hess_references(pool, [c[:8] for c in twins])
    worst = {w: RC.Worst("device twin %s, tier %s, %s" % (w, tier, bands)) for w in ("Hessian", "Fisher", "full noise Hessian")}
    for case in twins:
        cid, k, data, delays, alpha, rho, mb, N, kappa, nu = case
        L = len(alpha)
        args = RN.batch(case, seed=600 + L)
        d, a, r = args[:3]
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            gl, gg, ginfo = obj.loglik_grad_markov_batch(d, a, r)
            hl, hg, hh, hinfo = obj.loglik_hess_markov_batch(d, a, r)
            sl, sg, sf, sinfo = obj.loglik_fisher_markov_batch(d, a, r)
            fl, fg, fh, finfo = obj.loglik_hess_full_markov_noise_batch(*args)
            h1 = obj.loglik_hess_markov_batch(*alone((d, a, r)))
            s1 = obj.loglik_fisher_markov_batch(*alone((d, a, r)))
            f1 = obj.loglik_hess_full_markov_noise_batch(*alone(args))
        assert (ginfo == 0).all() and same(hinfo, ginfo) and same(sinfo, ginfo) and (finfo == 0).all(), cid
        assert same(hl, gl) and same(sl, gl) and same(hg, gg) and same(sg, gg), cid
        for one, many in ((h1, (hl, hg, hh, hinfo)), (s1, (sl, sg, sf, sinfo)), (f1, (fl, fg, fh, finfo))):
            assert all(same(x[0], z[-1]) for x, z in zip(one, many)), cid
        tied = FC.tie_rows(data[0], d)
        assert not tied[-1] and np.isfinite(hh[-1]).all() and np.isfinite(sf[-1]).all() and np.isfinite(fh[-1]).all(), cid
        assert np.array_equal(np.isnan(hh), tied[:, None, None] & FC.tau_mask(L)[None, :, :]), cid
        assert np.array_equal(np.isnan(fh), tied[:, None, None] & NF.tau_mask(L)[None, :, :]), cid
        pref, hyper_bars, ph, pf = plain[cid]
        ref, mh = refs[cid]
        assert not pref.ties, cid
        bars = {}
        for which, got, mirror in (("H", hh[-1], ph), ("F", sf[-1], pf)):
            for q, e, existing, em in RC.hess_pairs(pref, hyper_bars, case[:8], which, got, mirror):
                bars[q] = RC.regime_bar(existing, em, cid)[0]
                RC.add_pair(worst["Hessian" if which == "H" else "Fisher"], cid, q, e, existing, em)
        assert {"H at", "H rt", "H tt", "F at", "F rt", "F tt"} <= set(bars), cid
        held = RN.hess_pairs(ref, case, fh[-1], mh, NF.BLOCKS)
        assert [p[0] for p in held] == list(NF.BLOCKS), cid
        for b, e, existing, em in held:
            bars[b] = RC.regime_bar(existing, em, cid)[0]
            RC.add_pair(worst["full noise Hessian"], cid, b, e, existing, em)
        if L == 8:
            for name, gap in (("noise", RN.tau_pairs_distinct(ref.H, L, bars["tt"])), ("plain", RN.tau_pairs_distinct(pref.H, L, bars["H tt"]))):
                print("%s: the 28 off-diagonal (tau, tau) entries of the %s reference differ by at least %.3g (bar %.3g)" % (cid, name, *gap))
                assert gap[0] > gap[1], (cid, name, gap)
    RC.report(worst.values())


# ---- the per-row data sets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", RC.TIERS)
def test_resampled_and_realisations(oracle, pool, tier):
    """loglik_markov_resampled on every cell of the N <= 120 cases (k tiers) and on the "flux + subset" cell of the N = 370 cases (rho
    tiers), each cell with its own center and sigma_b, against the reduced fresh data set: 64 rows with their own (tau, alpha, rho) on
    the cells in turn, then the case's row once per cell.  loglik_markov_realisations (each realisation's own band means, the handle's
    offset prior variances) on the cells where that is the reduced data set's model (RN.same_model); there the two entries agree within
    twice the cell's bar, and with sigma_b="handle" the resampled entry agrees with the "flux" cell of the other under marginalised
    offsets too."""
    cases = RN.resample_cases(tier)
    assert len(cases) == (9 if tier in K_TIERS else 6)
    refs = RN.cell_references(pool, cases)
    worst = {w: RC.Worst("device %s, tier %s" % (w, tier)) for w in ("resampled", "realisations", "resampled against realisations (of 2 bars)")}
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
            ll, info = obj.loglik_markov_resampled(Y, D, A, Rh, real, counts=counts)
            l1, i1 = obj.loglik_markov_resampled(Y, D[last], A[last], Rh[last], real[last], counts=counts)
            if N <= RC.SMALL:
                multi, minfo = obj.loglik_markov_realisations(Y, d, a, r, center="own")
                m1, _ = obj.loglik_markov_realisations(Y, *alone((d, a, r)), center="own")
                hl, hinfo = obj.loglik_markov_resampled(Y, d[-1:], a[-1:], r[-1:], [1], center="own", sigma_b="handle")
        assert (info == 0).all() and np.isfinite(ll).all() and same(l1, ll[last]) and (i1 == 0).all(), cid
        bar = {}
        for j, c in enumerate(cells):
            ref, existing, mll, mmulti = refs[(cid, c)]
            q = "cell %d (%s)" % (c, SC.KINDS[c])
            RC.add_pair(worst["resampled"], cid, q, RN.rel(ll[ROWS - 1 + j], ref), existing, RN.rel(mll, ref))
            bar[c] = (ref, existing, float(RC.regime_bar(existing, RN.rel(mll, ref), cid)[0]))
        if N <= RC.SMALL:
            assert (minfo == 0).all() and multi.shape == (ROWS, RN.R) and np.isfinite(multi).all() and same(m1[0], multi[-1]) and hinfo[0] == 0, cid
            for c in cells:
                ref, existing, mll, mmulti = refs[(cid, c)]
                q = "cell %d (%s)" % (c, SC.KINDS[c])
                if RN.same_model(case, c):
                    RC.add_pair(worst["realisations"], cid, q, RN.rel(multi[-1, c], ref), existing, RN.rel(mmulti, ref))
                    RC.add_pair(worst["resampled against realisations (of 2 bars)"], cid, q, abs(multi[-1, c] - ll[ROWS - 1 + c]) / abs(ref) / 2.0,
                                existing, max(RN.rel(mll, ref), RN.rel(mmulti, ref)))
            # the "flux" cell on the handle's prior variances: another model than the reduced data set's under marginalised offsets, the
            # same one in both entries; the cell's bar (of its reference's size) serves
            RC.add_pair(worst["resampled against realisations (of 2 bars)"], cid, "cell 1 on the handle's sigma_b",
                        abs(multi[-1, 1] - hl[0]) / abs(bar[1][0]) / 2.0, bar[1][1], bar[1][2] / RC.FACTOR if tier != RC.CONTROL else 0.0)
    assert worst["resampled"].pairs == sum(len(RN.cells(c)) for c in cases) and (worst["realisations"].pairs > 0) == (tier in K_TIERS)
    RC.report(w for w in worst.values() if w.pairs)
