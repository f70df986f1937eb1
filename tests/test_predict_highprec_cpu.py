"""The extended-precision reference of the prediction family and its bars (tests/_predict_highprec.py) check themselves, without a
GPU: the reference against 40-digit mpmath; the bars against every slip that the witnesses and the numpy mirror can inject, on every
case of tests/_markov_predict_cases.py where the slip can act; and the healthy fp64 evaluations inside the bars.

Where a slip can act is decided by the case's construction (CAN_ACT), never by the outcome:
    no_sigma_b_cross, no_b_cross     b is marginalised (Sigma_b is zero otherwise)
    wrong_band, wrong_band_mean      L >= 2 and band 0 (the first band) has a test point: the slip moves that point to the next band
    skip_tile_row                    N > 128 (a second training tile row exists): the N = 150 case added here
    no_flip                          a Matern kernel (OU's state has no derivative to flip)
    tie_both                         a test point ties with a training point in shifted time (every case has such points, by
                                     _markov_predict_cases.test_points (b); the rule checks it on the data)
    every other slip                 every case."""
import numpy as np
import pytest

import _heldout_witness as HW
import _markov_cases as MC
import _markov_predict_cases as PC
import _predict_highprec as PH
import _predict_witness as PW
from gpcc_amd import markov

pytestmark = pytest.mark.skipif(not PH.EXTENDED, reason=PH.SKIP_REASON)

CASES = PC.cpu_cases()
MIN_REJECTION = 10.0


def _n150():
    t, y, s, delays = MC.lightcurves(MC.SHAPES[150][2], seed=2150, kind="ties")
    return ("matern32-N150-L2-b1-rho3-ties", "matern32", (t, y, s), delays, np.array([1.3, 0.7]), 3.0, True, PC.test_points(t, delays, 3150, -1))


EXTRA = _n150()


def _has_tie(case):
    _, _, (t, _, _), delays, _, _, _, tests = case
    train = np.concatenate([np.asarray(a) - delays[l] for l, a in enumerate(t)])
    star = np.concatenate([np.asarray(a) - delays[l] for l, a in enumerate(tests[0])])
    return bool(np.isin(star, train).any())


def _every(case):
    return True


def _mb(case):
    return bool(case[6])


def _band0_point(case):
    return len(case[2][0]) >= 2 and len(case[7][0][0]) > 0


def _second_tile_row(case):
    return sum(len(a) for a in case[2][0]) > PW.TILE


def _matern(case):
    return case[1] in ("matern32", "matern52")


CAN_ACT = {("predict witness", "no_jitter"): _every, ("predict witness", "no_sigma_b_cross"): _mb,
           ("predict witness", "skip_tile_row"): _second_tile_row, ("predict witness", "wrong_band"): _band0_point,
           ("heldout witness", "no_jitter"): _every, ("heldout witness", "sigma_not_squared"): _every,
           ("heldout witness", "no_b_cross"): _mb, ("heldout witness", "wrong_band_mean"): _band0_point,
           ("heldout witness", "padded_row"): _every,
           ("predict mirror", "no_flip"): _matern, ("predict mirror", "tie_both"): _has_tie, ("predict mirror", "no_prior"): _every,
           ("predict mirror", "no_jitter"): _every,
           ("heldout mirror", "no_jitter"): _every, ("heldout mirror", "test_mean"): _every}


def _slipped_ratio(oracle, source, slip, case):
    """error / bar of the slipped evaluation of a case: the larger of mu's and var's, or the held-out value's."""
    cid, k, data, delays, alpha, rho, mb, tests = case
    ref = PH.case_reference(oracle, case)
    if source == "predict witness":
        mu, var, _, _ = PW.predict_row(oracle, k, *data, delays, alpha, rho, tests[0], mb, slip=slip)
    elif source == "predict mirror":
        mu, var, _, _ = markov.predict(k, *data, delays, alpha, rho, tests[0], mb, _slip=slip)
    elif source == "heldout witness":
        return ref.ratio("held", HW.heldout_row(oracle, k, *data, delays, alpha, rho, *tests, mb, slip=slip)[0])
    else:
        return ref.ratio("held", markov.heldout(k, *data, delays, alpha, rho, *tests, mb, _slip=slip)[0])
    return max(ref.ratio("mu", mu), ref.ratio("var", var))


def test_case_rules():
    """The rules select what the issue of this test says they do."""
    assert len(CASES) == 72
    assert all(_has_tie(c) for c in CASES + [EXTRA])
    assert sum(_mb(c) for c in CASES) == 36 and sum(_matern(c) for c in CASES) == 48
    assert not any(_second_tile_row(c) for c in CASES) and _second_tile_row(EXTRA)
    n = sum(_band0_point(c) for c in CASES)
    assert 24 <= n < 48, n                                         # L >= 2: 48 cases, a few of them with band 0 dropped from the test set


@pytest.mark.parametrize("source,slip", sorted(CAN_ACT))
def test_bars_reject_slips(oracle, source, slip):
    rule = CAN_ACT[(source, slip)]
    acts = [c for c in CASES + [EXTRA] if rule(c)]
    assert acts, "the slip acts on no case"
    if (source, slip) != ("predict witness", "skip_tile_row"):
        assert len(acts) >= 36
    if slip == "no_jitter":
        assert len(acts) == len(CASES) + 1
    ratios = [(_slipped_ratio(oracle, source, slip, c), c[0]) for c in acts]
    low = min(ratios)
    print("%s %s: smallest error / bar %.3g (%s) over the %d cases it can act on" % (source, slip, low[0], low[1], len(acts)))
    missed = [(r, cid) for r, cid in ratios if not r >= MIN_REJECTION]
    assert not missed, missed


def test_healthy_paths(oracle):
    """The fp64 evaluations (witness, mirror, blocked) lie within the bar of every quantity of every case (<= 1 / FACTOR of it, by the bar's construction); the
    worst error / bar of each group is printed."""
    worst = {}
    for case in CASES + [EXTRA]:
        ref = PH.case_reference(oracle, case)
        for what, b in ref.bar.items():
            for which, e in (("witness", ref.e_witness[what]), (ref.second, ref.e_second[what]), ("blocked", ref.e_blocked[what])):
                r = e / float(np.min(b))
                assert r <= 1.0 / PH.FACTOR * (1 + 1e-12), (case[0], what, which, r)
                key = "%s %s %s" % (which, what, case[1])
                if r >= worst.get(key, (0.0, None, 0.0))[0]:
                    worst[key] = (r, case[0], e)
    for key in sorted(worst):
        print("%s: worst error / bar %.3g (error %.3g, %s)" % (key, worst[key][0], worst[key][2], worst[key][1]))


def test_old_bar_missed_no_jitter(oracle):
    """The conditioning-scaled bar that the parity tests keep accepts a variance without JITTER wherever b is marginalised (its
    Sigma_b-sized scale puts it above 1e-8); the bar here is below 1e-9 in all of them."""
    for case in CASES:
        cid, k, data, delays, alpha, rho, mb, tests = case
        _, _, _, old = PC.predict_reference(oracle, case)
        new = float(np.max(PH.case_reference(oracle, case).bar["var"]))
        assert (old > 1e-8) == bool(mb), (cid, old)
        assert new < 1e-9, (cid, new)


# -- the reference against mpmath ---------------------------------------------------------------------------------------------------
def _tiny(mb):
    """N = 12 in two bands, T = 5: one test time of the second band equals, in shifted time, a training time of the first; one is beyond
    the data.  sigma* lies in the range of _markov_predict_cases.test_points (0.2 .. 0.25).  (A pivot of S is a difference of alpha^2-sized
    terms, so the held-out value carries longdouble's rounding times alpha^2 / pivot, which its terms do not see: about 40 at this noise,
    more below it -- rbf, which leaves next to no posterior variance at a tie, measured 18 eps of the terms with sigma* = 0.1 there.)"""
    t, y, s, delays = MC.lightcurves([7, 5], seed=77, kind="plain")
    tt = [np.array([12.5, -2.25, 17.75]), np.array([np.sort(t[0])[3] + delays[1], 21.0625])]
    yt = [np.array([0.3, -0.1, 0.25]), np.array([0.7, 0.4])]
    st = [np.array([0.2, 0.25, 0.225]), np.array([0.2125, 0.2375])]
    return (t, y, s), delays, np.array([1.25, 0.75]), 2.5, (tt, yt, st)


def _mp_kernel(mp, kernel, s, rho):
    r = abs(s)
    if kernel == "OU":
        return mp.exp(-r / rho)
    if kernel == "rbf":
        return mp.exp(-s * s / (4 * rho))
    a = mp.sqrt(3 if kernel == "matern32" else 5) * r / rho
    return (1 + a) * mp.exp(-a) if kernel == "matern32" else (1 + a + a * a / 3) * mp.exp(-a)


def _mp_reference(kernel, data, delays, alpha, rho, tests, mb):
    """mu, var, held, postb mean and covariance in 40-digit mpmath, straight from the formulas."""
    import mpmath as mp
    mp.mp.dps = 40
    f = lambda v: mp.mpf(float(v))
    t, y, s = data
    L = len(t)
    band = [l for l, a in enumerate(t) for _ in a]
    bs = [l for l, a in enumerate(tests[0]) for _ in a]
    u = [f(v) - f(delays[l]) for l, a in enumerate(t) for v in a]
    us = [f(v) - f(delays[l]) for l, a in enumerate(tests[0]) for v in a]
    yy = [f(v) for a in y for v in a]
    sd = [f(v) for a in s for v in a]
    yt = [f(v) for a in tests[1] for v in a]
    st = [f(v) for a in tests[2] for v in a]
    al, rho = [f(v) for v in alpha], f(rho)
    mean = [mp.fsum(f(v) for v in a) / len(a) for a in y]
    Sigb = [100 * mp.fsum((f(v) - m) ** 2 for v in a) / (len(a) - 1) for a, m in zip(y, mean)]
    sb = Sigb if mb else [mp.mpf(0)] * L
    N, T = len(u), len(us)
    K0 = mp.matrix(N, N)
    K = mp.matrix(N, N)
    for i in range(N):
        for j in range(N):
            K0[i, j] = al[band[i]] * al[band[j]] * _mp_kernel(mp, kernel, u[i] - u[j], rho) + (sd[i] ** 2 if i == j else 0)
            K[i, j] = K0[i, j] + (sb[band[i]] if band[i] == band[j] else 0)
    kB = mp.matrix(N, T)
    for i in range(N):
        for j in range(T):
            kB[i, j] = al[band[i]] * al[bs[j]] * _mp_kernel(mp, kernel, u[i] - us[j], rho) + (sb[band[i]] if band[i] == bs[j] else 0)
    Ki = mp.inverse(K)
    r = mp.matrix([yy[i] - mean[band[i]] for i in range(N)])
    KikB = Ki * kB
    mu = kB.T * (Ki * r) + mp.matrix([mean[q] for q in bs])
    P = kB.T * KikB
    jit = f(PH.JITTER)
    var = [al[bs[j]] ** 2 + sb[bs[j]] - P[j, j] + jit for j in range(T)]
    S = mp.matrix(T, T)
    for i in range(T):
        for j in range(T):
            S[i, j] = (al[bs[i]] * al[bs[j]] * _mp_kernel(mp, kernel, us[i] - us[j], rho) + (sb[bs[i]] if bs[i] == bs[j] else 0)
                       - (P[i, j] + P[j, i]) / 2 + (st[i] ** 2 + jit if i == j else 0))
    d = mp.matrix(yt) - mu
    held = -(T * mp.log(2 * mp.pi) + mp.log(mp.det(S)) + (d.T * (mp.inverse(S) * d))[0]) / 2
    pmu = pS = None
    if mb:
        Q = mp.matrix(N, L)
        for i in range(N):
            Q[i, band[i]] = 1
        K0i = mp.inverse(K0)
        A = Q.T * K0i * Q
        for l in range(L):
            A[l, l] += 1 / Sigb[l]
        pS = mp.inverse(A)
        pmu = pS * (Q.T * (K0i * mp.matrix(yy)) + mp.matrix([mean[l] / Sigb[l] for l in range(L)]))
    return mu, var, held, pmu, pS


def _ld(x):
    """An mpf as longdouble: its float64 head plus the float64 head of the rest."""
    hi = float(x)
    return PH.LD(hi) + PH.LD(float(x - hi))


@pytest.mark.parametrize("mb", [True, False])
@pytest.mark.parametrize("kernel", ["OU", "rbf", "matern32", "matern52"])
def test_reference_against_mpmath(kernel, mb):
    data, delays, alpha, rho, tests = _tiny(mb)
    m = PH.model(kernel, *data, delays, alpha, rho, tests[0], mb)
    assert len(m.r) == 12 and len(m.bs) == 5
    mu, var, tmu, tvar = PH.predict_from(m)
    held, th = PH.heldout_from(m, tests[1], tests[2])
    xmu, xvar, xheld, xpmu, xpS = _mp_reference(kernel, data, delays, alpha, rho, tests, mb)
    tol = 16 * np.finfo(PH.LD).eps
    got = {"mu": np.max(np.abs(mu - np.array([_ld(v) for v in xmu])) / tmu), "var": np.max(np.abs(var - np.array([_ld(v) for v in xvar])) / tvar),
           "held": abs(held - _ld(xheld)) / th}
    if mb:
        pmu, pS = PH.postb_from(m)
        got["pmu"] = np.max(np.abs(pmu - np.array([_ld(v) for v in xpmu]))) / np.max(np.abs(pmu))
        got["pS"] = np.max(np.abs(pS - np.array([[_ld(xpS[i, j]) for j in range(2)] for i in range(2)]))) / np.max(np.abs(pS))
    print("%s b%d: |extended - mpmath| / terms in units of longdouble's eps: %s"
          % (kernel, mb, ", ".join("%s %.2f" % (k, float(v / np.finfo(PH.LD).eps)) for k, v in got.items())))
    for k, v in got.items():
        assert v <= tol, (k, float(v / np.finfo(PH.LD).eps))
