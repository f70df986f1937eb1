"""The linear-time gradient's numpy mirror (gpcc_amd.markov.loglik_grad) on the CPU: its building blocks against 40-digit mpmath
differences, the gradient against the extended-precision reference (tests/_grad_highprec.py) under the dense gradient's own bar and
against the fp64 torch witness at the large shapes, every injected slip rejected, and the refusals."""
import math
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _grad_highprec as H
import _grad_witness as W
import _markov_cases as MC
import _markov_grad_cases as GC
from gpcc_amd import markov

extended = pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


def _references(pool, cases):
    jobs = [(k, *data, delays, alpha, rho, mb) for (_, k, data, delays, alpha, rho, mb, _) in cases]
    refs = list(pool.map(H.evaluate_job, jobs))
    for c, r in zip(cases, refs):
        assert r.info == 0, c[0]
    return refs


# ---- building blocks ------------------------------------------------------------------------------------------------------------
def _mp_transition(mp, kernel, d, rho):
    """A(d) = expm(F d) at the working precision, from the companion matrix."""
    p = markov.order(kernel)
    lam = (mp.mpf(1) if kernel == "OU" else mp.sqrt(3 if kernel == "matern32" else 5)) / rho
    F = mp.zeros(p, p)
    for i in range(p - 1):
        F[i, i + 1] = 1
    for j in range(p):
        F[p - 1, j] = -math.comb(p, j) * lam ** (p - j)
    return mp.expm(F * d), F


def _mp_stationary(mp, kernel, rho):
    lam = (mp.mpf(1) if kernel == "OU" else mp.sqrt(3 if kernel == "matern32" else 5)) / rho
    if kernel == "OU":
        return mp.matrix([[1]])
    if kernel == "matern32":
        return mp.matrix([[1, 0], [0, lam ** 2]])
    kap = lam ** 2 / 3
    return mp.matrix([[1, 0, -kap], [0, kap, 0], [-kap, 0, lam ** 4]])


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_building_blocks_against_mpmath_differences(kernel):
    """dA/dd = F A, dA/drho and dPinf/drho of the mirror against central differences of the 40-digit expm (h = 1e-15: truncation
    ~1e-30, rounding ~1e-25): agreement to fp64 rounding of entries whose size is that of A's."""
    mp = pytest.importorskip("mpmath").mp
    mp.dps = 40
    h = mp.mpf(10) ** -15
    p = markov.order(kernel)
    worst = 0.0
    for rho in (0.1, 3.0, 20.0, 300.0):
        for d in (0.0, 2.0 ** -10, 0.37, 4.5):
            r, dd = mp.mpf(rho), mp.mpf(d)
            A, F = _mp_transition(mp, kernel, dd, r)
            # the mirror's blocks are those of the exact A and F
            got_A, got_F = markov.transition(kernel, d, rho), markov.companion(kernel, rho)
            dlag = (_mp_transition(mp, kernel, dd + h, r)[0] - _mp_transition(mp, kernel, dd - h, r)[0]) / (2 * h)
            drho = (_mp_transition(mp, kernel, dd, r + h)[0] - _mp_transition(mp, kernel, dd, r - h)[0]) / (2 * h)
            dpinf = (_mp_stationary(mp, kernel, r + h) - _mp_stationary(mp, kernel, r - h)) / (2 * h)
            got_lag, got_rho, got_pinf = got_F @ got_A, markov.transition_drho(kernel, d, rho), markov.stationary_drho(kernel, rho)
            for i in range(p):
                for j in range(p):
                    # scale of entry (i, j): lambda^(i - j), the units of d^i/dt^i over d^j/dt^j
                    lam = float(markov.rate(kernel, rho))
                    sc = lam ** (i - j)
                    for got, want, unit in ((got_F[i, j], F[i, j], sc * lam), (got_A[i, j], A[i, j], sc), (got_lag[i, j], dlag[i, j], sc * lam),
                                            (got_rho[i, j], drho[i, j], sc / rho), (got_pinf[i, j], dpinf[i, j], lam ** (i + j) / rho)):
                        err = abs(float(mp.mpf(float(got)) - want)) / unit
                        worst = max(worst, err)
                        assert err <= 64 * H.EPS64, (kernel, rho, d, i, j, float(got), float(want))
    print("%s: building blocks, worst scaled error %.3g" % (kernel, worst))


# ---- the mirror against the extended-precision reference ----------------------------------------------------------------------
@extended
@pytest.mark.parametrize("N", [110, 150, 767])
def test_mirror_against_extended_reference(pool, N):
    cases = GC.cases(N) if N != 767 else GC.subset_767()
    assert len(cases) == (72 if N != 767 else 12)
    refs = _references(pool, cases)
    worst = {k: GC.Worst("mirror %s N = %d" % (k, N)) for k in MC.KERNELS}
    for (cid, k, data, delays, alpha, rho, mb, _), ref in zip(cases, refs):
        ll, g, info = markov.loglik_grad(k, *data, delays, alpha, rho, mb)
        assert info == 0 and ll == markov.loglik(k, *data, delays, alpha, rho, mb)[0], cid
        worst[k].add(H.ratio(g, ref), cid)
    for w in worst.values():
        w.report()


@pytest.mark.parametrize("N", sorted(GC.LARGE))
def test_mirror_against_witness_large(N):
    kernel, data, delays, alpha, rho = GC.large(N, 64)
    g0 = 17   # one row of the grid
    ll, g, info = markov.loglik_grad(kernel, *data, delays[g0], alpha[g0], rho[g0], True)
    lw, gw = W.loglik_and_grad(kernel, *data, delays[g0], alpha[g0], rho[g0], True)
    err, scale = float(np.max(np.abs(g - gw))), float(np.max(np.abs(gw)))
    print("mirror %s N = %d: disagreement with the witness %.3g of max|g| (bar %.0e)" % (kernel, N, err / scale, GC.WITNESS_BAR))
    assert info == 0 and err <= GC.WITNESS_BAR * scale, (g, gw)


# ---- every slip misses the bar ------------------------------------------------------------------------------------------------
@extended
def test_every_slip_misses_the_bar(pool):
    cases = GC.cases(110)
    refs = dict(zip((c[0] for c in cases), _references(pool, cases)))
    by_id = {c[0]: c for c in cases}

    def miss(cid, slip):
        _, k, data, delays, alpha, rho, mb, _ = by_id[cid]
        return H.ratio(markov.loglik_grad(k, *data, delays, alpha, rho, mb, _slip=slip)[1], refs[cid])

    closest = {}
    # "one_sided" on every OU "ties" case with two or more bands
    ties = [c[0] for c in cases if c[1] == "OU" and c[0].endswith("ties") and len(c[4]) >= 2]
    assert len(ties) >= 4
    for cid in ties:
        r = miss(cid, "one_sided")
        closest["one_sided"] = min(closest.get("one_sided", math.inf), r)
        assert r > 1.0, (cid, r)
    # (Matern-3/2's dPinf has no entry in the observed row, dPinf h = 0: leaving it out moves nothing there, so Matern-5/2 is named)
    named = {"no_dpinf": ["matern52-N110-L2-b1-rho3-plain", "matern52-N110-L3-b0-rho3-ties", "matern52-N110-L1-b1-rho300-before"],
             "tau_one_lag": ["OU-N110-L2-b1-rho20-plain", "matern32-N110-L2-b1-rho0.1-plain", "matern52-N110-L3-b1-rho3-plain"],
             "no_dh": ["OU-N110-L1-b1-rho3-before", "matern32-N110-L2-b1-rho3-ties", "matern52-N110-L3-b1-rho20-ties"]}
    for slip, ids in named.items():
        for cid in ids:
            assert cid in by_id, cid
            r = miss(cid, slip)
            closest[slip] = min(closest.get(slip, math.inf), r)
            assert r > 1.0, (slip, cid, r)
    assert set(closest) == set(GC.SLIPS)
    for slip in GC.SLIPS:
        print("slip %-12s closest miss: error / bar %.3g" % (slip, closest[slip]))


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_and_codes():
    t, y, s, d0 = MC.lightcurves([30, 20], seed=3, kind="plain")
    with pytest.raises(ValueError):
        markov.loglik_grad("rbf", t, y, s, d0, [1.0, 1.0], 2.0)
    t5, y5, s5, d5 = MC.lightcurves([30, 25, 20, 25, 30], seed=12, kind="ties")
    a5 = np.linspace(0.6, 1.4, 5)
    with pytest.raises(ValueError):
        markov.loglik_grad("OU", t5, y5, s5, d5, a5, 2.0, True)
    ll, g, info = markov.loglik_grad("OU", t5, y5, s5, d5, a5, 2.0, False)
    assert info == 0 and np.isfinite(g).all() and g.shape == (11,)
    # the codes take precedence, as in markov.loglik
    bad = a5.copy()
    bad[2] = 0.0
    for args, code in (((t5, y5, s5, d5, bad, 2.0, True), -1), ((t5, y5, s5, d5, a5, -1.0, True), -2), ((t, y, s, d0, [1.0, -1.0], 0.0), -1),
                       ((t, y, s, d0, [1.0, 1.0], 0.0), -2)):
        ll, g, info = markov.loglik_grad("OU", *args)
        assert info == code == markov.loglik("OU", *args)[1] and math.isnan(ll) and np.isnan(g).all()
    llb, gb, ib = markov.loglik_grad_batch("matern32", t, y, s, [d0, d0], [[1.0, 1.0], [0.0, 1.0]], [2.0, 2.0])
    one = markov.loglik_grad("matern32", t, y, s, d0, [1.0, 1.0], 2.0)
    assert list(ib) == [0, -1] and np.array_equal(gb[0], one[1]) and llb[0] == one[0] and np.isnan(gb[1]).all()
    assert gb.shape == (2, 5)
