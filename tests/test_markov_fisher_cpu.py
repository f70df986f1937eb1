"""The linear-time Fisher information's numpy mirror (gpcc_amd.markov.loglik_fisher) on the CPU: all six blocks against
the extended-precision Fisher matrix under its own per-block bars times the filter's conditioning factor
(tests/_markov_fisher_cases.py), the NaN contract on OU rows with a cross-band tie, every injected slip rejected, the torch witness,
positive semi-definiteness, independence of the fluxes, `pairs=`, the outputs' contract, and fit.delay_covariance(curvature="fisher")
over the mirror."""
import math
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _hess_highprec as HH
import _markov_cases as MC
import _markov_fisher_cases as FC
import _markov_hess_full_cases as HF
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


@pytest.fixture(scope="module")
def mirror():
    """{case id: loglik_fisher's result} of the 144 cases."""
    return {c[0]: markov.loglik_fisher(c[1], *c[2], c[3], c[4], c[5], c[6]) for c in FC.cases()}


@extended
def test_mirror_against_extended_reference(references, mirror):
    """132 cases within 1 bar in every block; the 12 OU cases with a tie: NaN in every tau entry, info 0, the (alpha, rho) block within
    its bars.  Value, gradient and info are loglik_grad's; the smallest eigenvalue is not below -(the sum of the entries' bars)."""
    cases = FC.cases()
    assert len(cases) == 144
    worst = {(k, b): FC.Worst("mirror Fisher %s %s" % (k, b)) for k in MC.KERNELS for b in HH.BLOCKS}
    tied = 0
    for case in cases:
        cid, k, data, delays, alpha, rho, mb, _ = case
        L = len(alpha)
        ll, g, F, info = mirror[cid]
        gl, gg, ginfo = markov.loglik_grad(k, *data, delays, alpha, rho, mb)
        assert info == 0 == ginfo and ll == gl and np.array_equal(g, gg), cid
        assert F.shape == (2 * L + 1, 2 * L + 1) and np.array_equal(F, F.T, equal_nan=True), cid
        ref = references[cid]
        if FC.ou_tie(case):
            tied += 1
            tau = FC.tau_mask(L)
            assert ref.ties and np.isnan(F[tau]).all() and np.isfinite(F[~tau]).all(), cid
            for b, r in FC.ratios(F, ref, case, blocks=FC.HYPER_BLOCKS).items():
                worst[(k, b)].add(r, cid)
            lo = float(np.linalg.eigvalsh(F[:L + 1, :L + 1]).min())
        else:
            assert np.isfinite(F).all(), cid
            if L == 1:
                assert not F[2, :].any() and not F[:, 2].any(), cid          # exact zeros
            for b, r in FC.ratios(F, ref, case).items():
                worst[(k, b)].add(r, cid)
            lo = float(np.linalg.eigvalsh(F).min())
        assert lo >= -FC.bar_sum(ref, case), (cid, lo)
    assert tied == 12
    for w in worst.values():
        w.report()


@extended
def test_every_slip_misses_the_bar(references, mirror):
    """Each slip over the N = 110 cases it applies to (tau_one_lag: L >= 2 without an OU tie; the others: all 72, the tau entries of OU
    ties left out): it misses a bar in some block on every one of them."""
    for slip in FC.SLIPS:
        cases = [c for c in FC.cases(110) if slip != "tau_one_lag" or (len(c[4]) >= 2 and not FC.ou_tie(c))]
        assert len(cases) == (42 if slip == "tau_one_lag" else 72)
        missed, closest, escaped = 0, math.inf, []
        for case in cases:
            cid, k, data, delays, alpha, rho, mb, _ = case
            F = markov.loglik_fisher(k, *data, delays, alpha, rho, mb, _slip=slip)[2]
            blocks = FC.HYPER_BLOCKS if FC.ou_tie(case) else None
            r = max(FC.ratios(F, references[cid], case, blocks=blocks).values())
            if r > 1.0:
                missed += 1
                closest = min(closest, r)
            else:
                escaped.append((cid, r))
        print("slip %-16s cases missed of %d: %d; closest miss: %.3g bars; not caught: %s" % (slip, len(cases), missed, closest, escaped))
        assert missed == len(cases), (slip, escaped)


@extended
def test_against_the_torch_witness(references, mirror):
    """The mirror against _hess_witness.hessian_and_fisher (autograd through a dense Cholesky) on the N = 110 rows without a cross-band
    tie, within the reference's bars."""
    import _hess_witness as HW
    cases = [c for c in FC.cases(110) if not references[c[0]].ties]
    assert len(cases) >= 36
    worst = FC.Worst("mirror Fisher against the torch witness")
    for case in cases:
        cid, k, data, delays, alpha, rho, mb, _ = case
        Fw = HW.hessian_and_fisher(k, *data, delays, alpha, rho, mb)[3]
        worst.add(max(FC.ratios(mirror[cid][2], references[cid], case, against=Fw).values()), cid)
    worst.report()


def test_no_flux_enters_and_pairs():
    t, y, s, d0 = MC.lightcurves([30, 20], seed=3, kind="plain")
    other = [np.cos(3.0 * np.asarray(a)) * 2.0 + 0.3 for a in t]
    for k in MC.KERNELS:
        F = markov.loglik_fisher(k, t, y, s, d0, [1.0, 1.2], 2.0, marginalise_b=False)[2]
        G = markov.loglik_fisher(k, t, other, s, d0, [1.0, 1.2], 2.0, marginalise_b=False)[2]
        assert np.isfinite(F).all() and np.array_equal(F, G), k
    full = markov.loglik_fisher("matern32", t, y, s, d0, [1.0, 1.2], 2.0)
    pairs = [(2, 2), (0, 4), (4, 1), (4, 4)]
    ll, g, part, info = markov.loglik_fisher("matern32", t, y, s, d0, [1.0, 1.2], 2.0, pairs=pairs)
    listed = np.zeros((5, 5), bool)
    for a, b in pairs:
        listed[a, b] = listed[b, a] = True
    assert info == 0 and ll == full[0] and np.array_equal(g, full[1])
    assert np.array_equal(part[listed], full[2][listed]) and np.isnan(part[~listed]).all()
    with pytest.raises(ValueError):
        markov.loglik_fisher("matern32", t, y, s, d0, [1.0, 1.2], 2.0, pairs=[(0, 5)])


def test_outputs_codes_and_the_objective():
    t, y, s, d0 = MC.lightcurves([30, 20], seed=3, kind="plain")
    with pytest.raises(ValueError):
        markov.loglik_fisher("rbf", t, y, s, d0, [1.0, 1.0], 2.0)
    ll, g, F, info = markov.loglik_fisher("matern32", t, y, s, d0, [1.0, 1.2], 2.0)
    gl, gg, ginfo = markov.loglik_grad("matern32", t, y, s, d0, [1.0, 1.2], 2.0)
    assert info == 0 == ginfo and ll == gl and np.array_equal(g, gg) and F.shape == (5, 5) and np.array_equal(F, F.T)
    assert np.isfinite(F).all() and np.linalg.eigvalsh(F).min() >= -1e-10 * np.max(np.abs(F))
    # a common shift of every delay changes nothing: the tau rows sum to zero (up to rounding of sums of entries of this size)
    assert np.max(np.abs(F[:, 3:].sum(1))) <= 1e-9 * np.max(np.abs(F))
    for args, code in ((([0.0, 1.0], 2.0), -1), (([1.0, 1.0], -1.0), -2)):
        ll, g, F, info = markov.loglik_fisher("OU", t, y, s, d0, *args)
        assert info == code and math.isnan(ll) and np.isnan(g).all() and np.isnan(F).all() and F.shape == (5, 5)
    t1, y1, s1, d1 = MC.lightcurves([40], seed=4, kind="plain")
    F1 = markov.loglik_fisher("OU", t1, y1, s1, d1, [1.1], 2.0)[2]
    assert F1.shape == (3, 3) and np.isfinite(F1).all() and not F1[2, :].any() and not F1[:, 2].any()
    # an OU tie made by hand: the delay equals a difference of two observation times
    tie = np.array([0.0, t[1][3] - t[0][5]])
    assert t[1][3] - tie[1] == t[0][5]
    ll, g, F, info = markov.loglik_fisher("OU", t, y, s, tie, [1.0, 1.2], 2.0)
    assert info == 0 and np.isfinite(ll) and np.isfinite(g).all() and np.isfinite(F[:3, :3]).all()
    assert np.isnan(F[3:, :]).all() and np.isnan(F[:, 3:]).all()
    assert np.isfinite(markov.loglik_fisher("matern32", t, y, s, tie, [1.0, 1.2], 2.0)[2]).all()
    obj = markov.MarkovObjective(t, y, s, "matern32")
    delays, alpha, rho = [d0, d0, d0], [[1.0, 1.2], [0.0, 1.0], [0.9, 1.1]], [2.0, 2.0, 3.0]
    bl, bg, bf, binfo = obj.loglik_fisher_markov_batch(delays, alpha, rho)
    assert list(binfo) == [0, -1, 0] and bf.shape == (3, 5, 5) and bg.shape == (3, 5) and np.isnan(bf[1]).all()
    one = markov.loglik_fisher("matern32", t, y, s, d0, [0.9, 1.1], 3.0)
    assert bl[2] == one[0] and np.array_equal(bg[2], one[1]) and np.array_equal(bf[2], one[2])
    t5, y5, s5, d5 = MC.lightcurves([30, 25, 20, 25, 30], seed=12, kind="ties")
    with pytest.raises(ValueError):
        markov.loglik_fisher("OU", t5, y5, s5, d5, np.linspace(0.6, 1.4, 5), 2.0, True)


@extended
@pytest.mark.parametrize("kernel", ["OU", "matern32"])
def test_delay_covariance_fisher_over_the_mirror(kernel):
    """fit.delay_covariance(curvature="fisher") over MarkovObjective at the README point of _markov_hess_full_cases: (I_ff)^-1 of the
    mirror's Fisher matrix, each entry within 1e-6 of sqrt(cov_ii cov_jj) of the same over the extended-precision F; the default
    curvature is untouched; ok rules and ValueErrors as for the Hessian."""
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    delays = np.array(HF.README_DELAYS)
    a0, r0 = HF.README_MODE[kernel]
    obj = markov.MarkovObjective(t, y, s, kernel)
    cov, ok = fit.delay_covariance(obj, delays, a0, r0, solver="markov", curvature="fisher")
    F = markov.loglik_fisher(kernel, t, y, s, delays, a0, r0)[2]
    want, wok = fit.laplace_covariance(-F, [0, 1, 2, 4])
    assert ok and wok and cov.shape == (4, 4) and np.array_equal(cov, want) and (np.diag(cov) > 0).all()
    ref = HH.evaluate(kernel, t, y, s, delays, np.asarray(a0, float), r0, True)
    exact, eok = fit.laplace_covariance(-np.asarray(ref.F, np.float64), [0, 1, 2, 4])
    sd = np.sqrt(np.diag(exact))
    worst = float(np.max(np.abs(cov - exact) / (sd[:, None] * sd[None, :])))
    print("delay_covariance(curvature='fisher') %s: mirror against extended precision, worst %.3g (bar 1e-6)" % (kernel, worst))
    assert eok and worst <= 1e-6
    hess, hok = fit.delay_covariance(obj, delays, a0, r0, solver="markov")
    assert hok and np.array_equal(hess, fit.delay_covariance(obj, delays, a0, r0, solver="markov", curvature="hessian")[0])
    assert not np.array_equal(hess, cov)
    with pytest.raises(ValueError):
        fit.delay_covariance(obj, delays, a0, r0, solver="markov", curvature="expected")
    with pytest.raises(ValueError):
        fit.delay_covariance(obj, delays, a0, r0, free=[0, 3, 4], solver="markov", curvature="fisher")
    bad, okb = fit.delay_covariance(obj, delays, [0.0, 1.0], r0, solver="markov", curvature="fisher")
    assert not okb and np.isnan(bad).all() and bad.shape == (4, 4)
    # away from a maximum -H need not be positive definite; the Fisher information is
    away = fit.delay_covariance(obj, np.array([0.0, 7.3]), [0.2, 2.5], 6.0, solver="markov", curvature="fisher")
    assert away[1] and (np.diag(away[0]) > 0).all()
