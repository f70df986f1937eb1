"""The linear-time Hessian block's numpy mirror (gpcc_amd.markov.loglik_hess_hyper) on the CPU: the closed forms of d2A/drho2 and
d2Pinf/drho2 against 40-digit mpmath differences, the block against the extended-precision reference (tests/_hess_highprec.py) under the
reference's own per-block bars times the filter's conditioning factor (tests/_markov_hess_cases.py), every injected slip rejected, the
outputs' contract, and the Laplace evidence over the mirror against the dense CPU witness."""
import math
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _hess_highprec as HH
import _hess_witness as HW
import _markov_cases as MC
import _markov_hess_cases as HC
from gpcc_amd import laplace, markov, synthetic
from test_laplace_cpu import WitnessObjective
from test_markov_grad_cpu import _mp_stationary, _mp_transition

extended = pytest.mark.skipif(not HH.EXTENDED, reason=HH.SKIP_REASON)
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


@pytest.fixture(scope="module")
def references(pool):
    """{case id: Reference with its bars} of the 144 cases."""
    cases = HC.cases()
    refs = list(pool.map(HH.reference_job, [HC.job(c) for c in cases]))
    for c, r in zip(cases, refs):
        assert r.info == 0, c[0]
    return dict(zip((c[0] for c in cases), refs))


# ---- closed forms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_second_order_closed_forms_against_mpmath_differences(kernel):
    """d2A/drho2 and d2Pinf/drho2 of the mirror against second central differences of the 40-digit expm and of the stationary covariance
    (h = 1e-10 rho: truncation ~1e-20, rounding ~1e-20 relative): agreement to fp64 rounding of entries whose size is that of A's, in
    the units of the first-order check of tests/test_markov_grad_cpu.py divided by rho once more."""
    mp = pytest.importorskip("mpmath").mp
    mp.dps = 40
    p = markov.order(kernel)
    worst = 0.0
    for rho in (0.1, 3.0, 20.0, 300.0):
        r = mp.mpf(rho)
        h = r * mp.mpf(10) ** -10
        lam = float(markov.rate(kernel, rho))
        d2pinf = (_mp_stationary(mp, kernel, r + h) - 2 * _mp_stationary(mp, kernel, r) + _mp_stationary(mp, kernel, r - h)) / (h * h)
        got_pinf = markov.stationary_d2rho(kernel, rho)
        for d in (0.0, 2.0 ** -10, 0.37, 4.5):
            dd = mp.mpf(d)
            d2a = (_mp_transition(mp, kernel, dd, r + h)[0] - 2 * _mp_transition(mp, kernel, dd, r)[0]
                   + _mp_transition(mp, kernel, dd, r - h)[0]) / (h * h)
            got_a = markov.transition_d2rho(kernel, d, rho)
            for i in range(p):
                for j in range(p):
                    sc = lam ** (i - j)          # the scale of entry (i, j) of A: lambda^(i - j)
                    for got, want, unit in ((got_a[i, j], d2a[i, j], sc / rho ** 2), (got_pinf[i, j], d2pinf[i, j], lam ** (i + j) / rho ** 2)):
                        err = abs(float(mp.mpf(float(got)) - want)) / unit
                        worst = max(worst, err)
                        assert err <= 64 * HH.EPS64, (kernel, rho, d, i, j, float(got), float(want))
    print("%s: second-order closed forms, worst scaled error %.3g" % (kernel, worst))


# ---- the mirror against the extended-precision reference ------------------------------------------------------------------------
@extended
def test_mirror_against_extended_reference(references):
    cases = HC.cases()
    assert len(cases) == 144
    worst = {k: HC.Worst("mirror Hessian block %s" % k) for k in MC.KERNELS}
    for case in cases:
        cid, k, data, delays, alpha, rho, mb, _ = case
        ll, g, H, info = markov.loglik_hess_hyper(k, *data, delays, alpha, rho, mb)
        assert info == 0 and np.array_equal(H, H.T), cid
        worst[k].add(HC.ratio(H, references[cid], case), cid)
    for w in worst.values():
        w.report()


# ---- every slip misses the bar --------------------------------------------------------------------------------------------------
# no_d2pinf cannot show on OU (Pinf = 1 does not depend on rho) nor on Matern-3/2 (Pinf_rhorho has one entry, the variance of f', and
# with it left out of the prior and the step alike D = C_xx - Pinf carries the same second tangent: nothing in the observed row moves,
# as with no_dpinf in the gradient's tests).  Every other slip shows on every kernel.
APPLIES = {"no_d2a": MC.KERNELS, "no_d2pinf": ("matern52",), "no_cross": MC.KERNELS, "no_hahb": MC.KERNELS, "chain_rho": MC.KERNELS}


@extended
def test_every_slip_misses_the_bar(references):
    """Each slip on all 24 cases at N = 110 of every kernel it applies to: measured on the CPU, every one of them misses (the smallest
    miss is printed), which is more than the one case per kernel that is asked for."""
    assert set(APPLIES) == set(HC.SLIPS)
    for slip in HC.SLIPS:
        closest = math.inf
        for case in HC.cases(110):
            cid, k, data, delays, alpha, rho, mb, _ = case
            H = markov.loglik_hess_hyper(k, *data, delays, alpha, rho, mb, _slip=slip)[2]
            r = HC.ratio(H, references[cid], case)
            if k in APPLIES[slip]:
                closest = min(closest, r)
                assert r > 1.0, (slip, cid, r)
            else:
                assert r <= 1.0, (slip, cid, r)       # (where it cannot show it changes nothing that is observed)
        print("slip %-10s closest miss: error / bar %.3g" % (slip, closest))


# ---- the outputs' contract --------------------------------------------------------------------------------------------------------
def test_outputs_codes_and_the_objective():
    t, y, s, d0 = MC.lightcurves([30, 20], seed=3, kind="plain")
    with pytest.raises(ValueError):
        markov.loglik_hess_hyper("rbf", t, y, s, d0, [1.0, 1.0], 2.0)
    ll, g, H, info = markov.loglik_hess_hyper("matern32", t, y, s, d0, [1.0, 1.2], 2.0)
    vl, vinfo = markov.loglik("matern32", t, y, s, d0, [1.0, 1.2], 2.0)
    gl, gg, ginfo = markov.loglik_grad("matern32", t, y, s, d0, [1.0, 1.2], 2.0)
    assert info == 0 == vinfo == ginfo and ll == vl == gl and np.array_equal(g, gg) and H.shape == (3, 3) and np.array_equal(H, H.T)
    for args, code in ((([0.0, 1.0], 2.0), -1), (([1.0, 1.0], -1.0), -2)):
        ll, g, H, info = markov.loglik_hess_hyper("OU", t, y, s, d0, *args)
        assert info == code and math.isnan(ll) and np.isnan(g).all() and np.isnan(H).all()
    obj = markov.MarkovObjective(t, y, s, "matern32")
    delays, alpha, rho = [d0, d0, d0], [[1.0, 1.2], [0.0, 1.0], [0.9, 1.1]], [2.0, 2.0, 3.0]
    bl, bg, bh, binfo = obj.loglik_hess_hyper_markov_batch(delays, alpha, rho)
    assert list(binfo) == [0, -1, 0] and bh.shape == (3, 3, 3) and bg.shape == (3, 5) and np.isnan(bh[1]).all()
    one = markov.loglik_hess_hyper("matern32", t, y, s, d0, [0.9, 1.1], 3.0)
    assert bl[2] == one[0] and np.array_equal(bg[2], one[1]) and np.array_equal(bh[2], one[2])
    al = obj.loglik_hess_hyper_batch(delays, alpha, rho)             # the dense entry's name and shape: no Fisher information
    assert len(al) == 5 and al[3] is None and np.array_equal(al[2], bh, equal_nan=True) and np.array_equal(al[4], binfo)
    # five bands: with marginalised offsets refused, without them fine
    t5, y5, s5, d5 = MC.lightcurves([30, 25, 20, 25, 30], seed=12, kind="ties")
    a5 = np.linspace(0.6, 1.4, 5)
    with pytest.raises(ValueError):
        markov.loglik_hess_hyper("OU", t5, y5, s5, d5, a5, 2.0, True)
    assert markov.loglik_hess_hyper("OU", t5, y5, s5, d5, a5, 2.0, False)[2].shape == (6, 6)


# ---- Laplace over the mirror ------------------------------------------------------------------------------------------------------
def test_laplace_over_the_mirror_against_the_dense_witness():
    """The README-size sweep (N = 110, two bands), five delays: laplace.laplace_evidence over MarkovObjective, through both of its names,
    and over the dense torch witness of tests/test_laplace_cpu.py: the same codes, log_evidence within twice the evidence tests' bar
    max(1e-6, 64 eps cond_1(K) |l^|) (each side gets one allowance)."""
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    data = (t, y, s)
    delays = np.array([[0.0, d] for d in (0.0, 1.0, 2.0, 3.0, 5.0)])
    G = len(delays)
    a0, r0 = synthetic.default_hyperparameters(y)
    kw = dict(rhomin=1e-3, rhomax=1e3, g_tol=1e-7)
    dense = laplace.laplace_evidence(WitnessObjective(data, "OU"), delays, np.tile(a0, (G, 1)), np.full(G, r0), **kw)
    mobj = markov.MarkovObjective(t, y, s, "OU")
    alias = laplace.laplace_evidence(mobj, delays, np.tile(a0, (G, 1)), np.full(G, r0), **kw)
    named = laplace.laplace_evidence(mobj, delays, np.tile(a0, (G, 1)), np.full(G, r0), solver="markov", **kw)
    for x, z in zip(alias, named):
        assert np.array_equal(np.asarray(x), np.asarray(z), equal_nan=True)
    assert np.array_equal(dense[5], alias[5]) and (dense[5] == 0).all(), (dense[5], alias[5])
    band, tt, _, Kn = HW._setup(*data, True)
    worst = 0.0
    for g in range(G):
        u = tt - delays[g][band]
        al, rho = dense[1][g], dense[2][g]
        K = al[band][:, None] * al[band][None, :] * HW.derivatives("OU", u[:, None] - u[None, :], rho)[0] + Kn
        bar = 2 * max(1e-6, 64 * EPS * np.linalg.cond(np.asarray(K, np.float64), 1) * abs(dense[0][g]))
        worst = max(worst, abs(alias[3][g] - dense[3][g]) / bar)
        assert abs(alias[3][g] - dense[3][g]) <= bar, (g, alias[3][g], dense[3][g], bar)
    print("Laplace over the mirror against the dense witness: worst |dlogZ| / (2 bars) %.3g; rounds %s and %s"
          % (worst, list(alias[6]), list(dense[6])))
    with pytest.raises(ValueError):
        laplace.laplace_evidence(mobj, delays, np.tile(a0, (G, 1)), np.full(G, r0), solver="sparse")
