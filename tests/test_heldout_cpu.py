"""The held-out log-likelihood's witness (tests/_heldout_witness.py) and the cross-validation helpers on the CPU: the witness against
the conditional identity log p(y*|y) = log p([y; y*]) - log p(y), the parity bar against injected slips, the folds of cvindices, the
row-order log-sum-exp of the mixture, and performcv_grid's refusal of a split that starves a band."""
import numpy as np
import pytest

import _heldout_witness as HW
from gpcc_amd import api, fit, synthetic


def _case(Nl, Nt, seed):
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=seed)
    rng = np.random.default_rng(seed)
    span = max(float(np.max(a)) for a in t)
    ttest = [np.sort(rng.random(n) * (span + 10) - 5) for n in Nt]
    ytest = [rng.normal(np.mean(a), np.std(a) + 0.1, n) for a, n in zip(y, Nt)]
    stest = [0.05 + 0.2 * rng.random(n) for n in Nt]
    return t, y, s, ttest, ytest, stest


@pytest.mark.parametrize("kname,mb", [("OU", True), ("rbf", False), ("matern32", True), ("matern52", False)])
def test_witness_conditional_identity(oracle, kname, mb):
    t, y, s, tt, yt, st = _case([60, 50, 40], [30, 0, 41], seed=3)
    delays, alpha, rho = [0.0, 2.0, 4.0], [1.0, 1.4, 0.8], 3.1
    ll, cond = HW.heldout_row(oracle, kname, t, y, s, delays, alpha, rho, tt, yt, st, marginalise_b=mb)
    ref = HW.union_identity(oracle, kname, t, y, s, delays, alpha, rho, tt, yt, st, marginalise_b=mb)
    assert abs(ll - ref) <= HW.bar(cond, ref), (ll, ref, cond)


SLIPS = ["no_jitter", "sigma_not_squared", "no_b_cross", "wrong_band_mean", "padded_row"]


@pytest.mark.parametrize("slip", SLIPS)
def test_bar_rejects_slips(oracle, slip):
    """Each slip lands far above the GPU tests' parity bar max(1e-10, 64 eps cond_1(K_aug)) * max(1, |l|).  (no_jitter: the fixed-b
    model -- the marginalised one's Sigma_b = 100 var(y) lifts cond_1 so far that 1e-8 on the diagonal sits at the bar -- with test
    noise 1e-3, where the 1e-8 matters.)"""
    t, y, s, tt, yt, st = _case([180, 150], [140, 129], seed=11)
    kname, mb = "matern32", True
    if slip == "no_jitter":
        st = [np.full(len(a), 1e-3) for a in st]
        kname, mb = "OU", False
    delays, alpha, rho = [0.0, 2.0], [1.1, 0.8], 2.5
    ll, cond = HW.heldout_row(oracle, kname, t, y, s, delays, alpha, rho, tt, yt, st, marginalise_b=mb)
    l2, _ = HW.heldout_row(oracle, kname, t, y, s, delays, alpha, rho, tt, yt, st, marginalise_b=mb, slip=slip)
    ratio = abs(l2 - ll) / HW.bar(cond, ll)
    print("%s: error / bar %.3g (cond_1(K_aug) %.3g)" % (slip, ratio, cond))
    assert ratio > 10.0, (slip, ratio)


def test_cvindices_partitions():
    Nl, F = [23, 7, 3, 40], 5
    folds = fit.cvindices(Nl, F, seed=1)
    assert len(folds) == len(Nl)
    for n, fb in zip(Nl, folds):
        assert len(fb) == F
        allidx = np.concatenate(fb)
        assert np.array_equal(np.sort(allidx), np.arange(n))          # a partition
        sizes = [len(f) for f in fb]
        assert max(sizes) - min(sizes) <= 1
        assert all(np.array_equal(f, np.sort(f)) for f in fb)
    assert any(len(f) == 0 for f in folds[2])                          # N_l < F: empty test folds arise
    again = fit.cvindices(Nl, F, seed=1)
    assert all(np.array_equal(a, b) for fa, fb in zip(folds, again) for a, b in zip(fa, fb))
    # band b draws from default_rng(seed + b): band 2 of seed 1 is band 1 of seed 2 (same length), and bands differ
    s2 = fit.cvindices([Nl[1], Nl[1]], F, seed=2)
    s1 = fit.cvindices([Nl[1], Nl[1]], F, seed=1)
    assert all(np.array_equal(a, b) for a, b in zip(s1[1], s2[0]))
    assert not all(np.array_equal(a, b) for a, b in zip(s1[0], s1[1]))
    with pytest.raises(ValueError):
        fit.cvindices(Nl, 1, seed=1)


def test_split_with_empty_test_band():
    t, y, s, _, _, _ = _case([20, 4], [1, 1], seed=2)
    folds = fit.cvindices([20, 4], 5, seed=1)
    f = [k for k in range(5) if len(folds[1][k]) == 0][0]
    (ttr, ytr, _), (tte, yte, ste) = fit._split(t, y, s, folds, f)
    assert len(tte[1]) == 0 and len(ttr[1]) == 4 and len(tte[0]) + len(ttr[0]) == 20
    assert np.array_equal(np.sort(np.concatenate([ttr[0], tte[0]])), np.sort(t[0]))


def test_performcv_grid_refuses_a_starved_band():
    t, y, s, _, _, _ = _case([30, 2], [1, 1], seed=4)
    with pytest.raises(ValueError, match="training point"):
        fit.performcv_grid(t, y, s, candidatedelays=[[0.0, 1.0]], kernel="OU", numberoffolds=5)
    with pytest.raises(ValueError, match="training point"):
        fit.performcv(t, y, s, delays=[0.0, 1.0], kernel="OU", numberoffolds=5)


def test_logsumexp_rows():
    rng = np.random.default_rng(2)
    v = rng.normal(-300, 20, 9)
    w = rng.random(9)
    w[[2, 5]] = 0.0
    p = w / w.sum()
    keep = p > 0
    ref = np.log(np.sum(p[keep] * np.exp(v[keep] - v[keep].max()))) + v[keep].max()
    assert abs(api.logsumexp_rows(v, p) - ref) <= 1e-12 * abs(ref)
    one = np.zeros(9)
    one[4] = 1.0
    assert api.logsumexp_rows(v, one) == v[4]                           # its own bits
    v2 = v.copy()
    v2[2] = np.nan
    assert api.logsumexp_rows(v2, p) == api.logsumexp_rows(v, p)        # zero weight: skipped
    v2[3] = np.nan
    assert np.isnan(api.logsumexp_rows(v2, p))
