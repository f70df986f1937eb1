"""The numpy mirror of the linear-time leave-one-out scores (gpcc_amd.markov.loo, loo_mix) against the extended-precision definition,
with bars measured on the reference side only (tests/_loo_highprec.py); every injected mistake must exceed the bar on every case where
it can act; edge cases.  The lines that start with "loo-parity" are kept in profiles/loo/loo_parity.log.

Which cases can catch which slip.  with_self, no_sigma, jitter and arith_mix act on every case.  sorted_order acts on every case too,
because every case hands its last band over unsorted (a case whose bands are all sorted could not see it: the two orders coincide).
tie_both changes the backward walk only among points that tie in shifted time, so it can act only on the cases that hold such a pair
-- the "ties" cases with L >= 2, and whichever others happen to draw the same time twice on the 2^-10 grid; the cases without a tie
give the same bits with and without it, which the test asserts."""
import math

import numpy as np
import pytest

import _loo_highprec as LH
import _markov_cases as MC
from gpcc_amd import markov

extended = pytest.mark.skipif(not LH.EXTENDED, reason=LH.SKIP_REASON)      # the tests that call LH.reference
CASES = LH.cases()


def _mirror(case, rows=(0, 1), slip=None):
    cid, k, data, delays, alpha, rho, mb, N = case
    out = [markov.loo(k, *data, delays[m], alpha[m], rho[m], mb, _slip=slip) for m in rows]
    assert all(o[5] == 0 for o in out), cid
    return {"mu": np.stack([o[0] for o in out]), "var": np.stack([o[1] for o in out]), "lp": np.stack([o[2] for o in out]),
            "loo": np.array([o[3] for o in out]), "loglik": np.array([o[4] for o in out])}


def _has_tie(case):
    cid, k, data, delays, alpha, rho, mb, N = case
    s = np.concatenate([np.asarray(t, np.float64) - delays[0][l] for l, t in enumerate(data[0])])
    return len(np.unique(s)) < len(s)


def test_case_count():
    assert len(CASES) == 2 * 3 * 3 * 2 * len(MC.RHOS) and len(LH.rbf_cases()) == 2 * 2 * len(MC.RHOS)
    assert {c[0].split("-")[-1] for c in CASES} == {"ties", "before", "plain"}
    assert sum(_has_tie(c) for c in CASES) >= 16


@extended
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_mirror_meets_the_bar(kernel):
    worst = {q: LH.Worst("loo-parity mirror %s %s" % (q, kernel)) for q in LH.QUANTITIES}
    for case in CASES:
        cid, k, data, delays, alpha, rho, mb, N = case
        if k != kernel:
            continue
        ref, got = LH.reference(case), _mirror(case)
        assert got["loglik"][0] == markov.loglik(k, *data, delays[0], alpha[0], rho[0], mb)[0], cid   # the taps do not split the chain
        got["mix_lp"], got["mix_loo"] = markov.loo_mix(got["lp"], LH.WEIGHTS)
        for q in LH.QUANTITIES:
            worst[q].add(ref.ratio(q, got[q], markov=True), cid)
    for q in LH.QUANTITIES:
        print(worst[q].line())
    missed = [w.line() for w in worst.values() if not w.worst <= 1.0]
    assert not missed, missed


@extended
@pytest.mark.parametrize("slip", [s for s in markov.LOO_SLIPS if s != "arith_mix"])
def test_every_slip_misses_the_bar(slip):
    """Row 0 of every case with the slip against the extended reference: the quantity the slip moves misses its bar."""
    moved = {"with_self": ("mu", "var", "lp"), "tie_both": ("var", "lp"), "no_sigma": ("var", "lp"), "jitter": ("var",),
             "sorted_order": ("mu", "lp")}[slip]
    acted = 0
    for case in CASES:
        cid = case[0]
        got = _mirror(case, rows=(0,), slip=slip)
        if slip == "tie_both" and not _has_tie(case):
            clean = _mirror(case, rows=(0,))
            assert all(np.array_equal(got[q], clean[q]) for q in ("mu", "var", "lp")), cid
            continue
        acted += 1
        ref = LH.reference(case)
        for q in moved:
            assert ref.ratio(q, got[q], rows=[0], markov=True) > 1.0, (cid, slip, q)
    assert acted >= 16


@extended
def test_arith_mix_misses_the_bar():
    for case in CASES:
        ref = LH.reference(case)
        lp = ref.lp.astype(np.float64)     # the extended rows, rounded once: only the mixture differs
        good, _ = markov.loo_mix(lp, LH.WEIGHTS)
        bad, bad_sum = markov.loo_mix(lp, LH.WEIGHTS, _slip="arith_mix")
        assert ref.ratio("mix_lp", good, markov=True) <= 1.0, case[0]
        assert ref.ratio("mix_lp", bad, markov=True) > 1.0 and ref.ratio("mix_loo", bad_sum, markov=True) > 1.0, case[0]


@extended
def test_extended_value_against_mpmath():
    mp = pytest.importorskip("mpmath")
    case = CASES[0]
    cid, k, data, delays, alpha, rho, mb, N = case
    ref = LH.reference(case)
    mu, var, lp = LH.mpmath_row(k, data, delays[0], alpha[0], rho[0], mb)
    for q, vals in (("mu", mu), ("var", var), ("lp", lp)):
        e = max(abs(float(mp.mpf(float(x)) + mp.mpf(float(x - LH.LD(float(x)))) - v)) for x, v in zip(getattr(ref, q)[0], vals))
        assert e <= 1e-3 * float(np.min(ref.bar[q][0])), (q, e)     # the extended value is exact on the bar's scale


@extended
def test_brute_force_includes_tied_points():
    n = 0
    for case in CASES:
        if case[0].endswith("ties") and len(case[2][0]) >= 2:
            ref = LH.reference(case)
            cid, k, data, delays, alpha, rho, mb, N = case
            s = np.concatenate([np.asarray(t, np.float64) - delays[0][l] for l, t in enumerate(data[0])])
            assert sum(np.sum(s == s[i]) > 1 for i in ref.pts) >= 2 and len(ref.pts) == LH.BRUTE_POINTS, cid
            n += 1
    assert n >= 8


def test_single_point():
    """N = 1 (b not marginalised): nothing to condition on, so var = K_11 = alpha^2 + sigma^2 and mu = bbar = mean(y) = y_1."""
    for k in MC.KERNELS:
        mu, var, lp, loo, ll, info = markov.loo(k, [np.array([1.5])], [np.array([0.7])], [np.array([0.25])], [0.0], [1.5], 2.0, False)
        assert info == 0 and abs(var[0] - (1.5 ** 2 + 0.25 ** 2)) <= 4 * 2.0 ** -52 * var[0] and mu[0] == 0.7
        assert abs(lp[0] - (-0.5 * (markov.LOG2PI + math.log(var[0])))) <= 1e-15 and loo == lp[0] and abs(ll - lp[0]) <= 1e-15


def test_mixture_identities():
    cid, k, data, delays, alpha, rho, mb, N = CASES[7]
    lp = _mirror(CASES[7])["lp"]
    one, one_sum = markov.loo_mix(lp[:1], [3.0])
    assert np.array_equal(one, lp[0])                                   # one row of weight 1: the row's bits
    skip, _ = markov.loo_mix(lp, [2.0, 0.0])
    assert np.array_equal(skip, lp[0])                                  # zero weights are skipped
    twice, _ = markov.loo_mix(np.stack([lp[0], lp[0]]), [1.0, 1.0])
    assert np.max(np.abs(twice - lp[0])) <= 4 * 2.0 ** -52 * np.max(np.abs(lp[0]) + math.log(2.0))   # log(1/2) + x, then + log 2
    harm, _ = markov.loo_mix(lp, LH.WEIGHTS)
    assert np.all(harm <= np.max(lp, axis=0)) and np.all(harm >= np.min(lp, axis=0))
    nan, nan_sum = markov.loo_mix(np.stack([lp[0], np.full(N, math.nan)]), [1.0, 1.0])
    assert np.all(np.isnan(nan)) and math.isnan(nan_sum)


def test_codes_and_objective():
    cid, k, data, delays, alpha, rho, mb, N = CASES[7]
    out = markov.loo(k, *data, delays[0], -alpha[0], rho[0], mb)
    assert out[5] == -1 and np.all(np.isnan(out[0])) and math.isnan(out[3])
    assert markov.loo(k, *data, delays[0], alpha[0], -1.0, mb)[5] == -2
    with pytest.raises(ValueError):
        markov.loo("rbf", *data, delays[0], alpha[0], rho[0], mb)
    obj = markov.MarkovObjective(*data, k, mb)
    res = obj.loo_markov_batch(delays, alpha, rho, weights=LH.WEIGHTS)
    row = markov.loo(k, *data, delays[1], alpha[1], rho[1], mb)
    assert np.array_equal(res.lp[1], row[2]) and res.loo[1] == row[3] and res.info.tolist() == [0, 0]
    assert np.array_equal(res.mix_lp, markov.loo_mix(res.lp, LH.WEIGHTS)[0])
