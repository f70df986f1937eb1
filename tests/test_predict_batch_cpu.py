"""The batched predictive's witness (tests/_predict_witness.py) and its Python layer on the CPU: the witness against the full
_reference_predict of tests/test_gpu_parity.py, the parity bar against the injected slips, and fit.DelayAveragedPredictor over an
injected objective whose predict_batch is the witness."""
import numpy as np
import pytest

import _predict_witness as PW
from gpcc_amd import fit, synthetic
from test_gpu_parity import _reference_predict


def _case(Nl, Nt, seed):
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=seed)
    rng = np.random.default_rng(seed)
    span = max(float(np.max(a)) for a in t)
    ttest = [np.sort(rng.random(n) * (span + 10) - 5) for n in Nt]
    return t, y, s, ttest


@pytest.mark.parametrize("kname", ["OU", "rbf", "matern32", "matern52"])
def test_witness_against_reference_predict(oracle, kname):
    t, y, s, ttest = _case([60, 50, 40], [30, 0, 41], seed=3)
    delays, alpha, rho = [0.0, 2.0, 4.0], [1.0, 1.4, 0.8], 3.1
    mu, var, _, cmax = PW.predict_row(oracle, kname, t, y, s, delays, alpha, rho, ttest)
    mu_ref, Sig_ref = _reference_predict(oracle, kname, t, y, s, delays, alpha, rho, ttest)
    # (var is a difference of two terms of the size of diag(cB): its error is relative to that)
    assert np.max(np.abs(mu - mu_ref)) <= 1e-13 * max(1.0, np.max(np.abs(mu_ref)))
    assert np.max(np.abs(var - np.diag(Sig_ref))) <= 1e-13 * cmax


def test_witness_fixed_b(oracle):
    """The fixed-b variant (gpccfixdelay.jl:244-266): no Sigma_b anywhere, the mean around the band means."""
    t, y, s, ttest = _case([70, 45], [33, 20], seed=5)
    delays, alpha, rho = [0.0, 1.5], [1.2, 0.9], 2.7
    mu, var, _, cmax = PW.predict_row(oracle, "matern52", t, y, s, delays, alpha, rho, ttest, marginalise_b=False)
    K, resid = oracle.model_matrix("matern52", t, y, s, delays, alpha, rho, False)
    bs = np.concatenate([np.full(len(a), l) for l, a in enumerate(ttest)])
    kB = oracle.delayed_covariance("matern52", alpha, delays, rho, t, ttest)
    cB = oracle.delayed_covariance("matern52", alpha, delays, rho, ttest)
    Sref = cB - kB.T @ np.linalg.solve(K, kB) + 1e-8 * np.eye(len(bs))
    mref = kB.T @ np.linalg.solve(K, resid) + np.array([np.mean(a) for a in y])[bs]
    assert np.max(np.abs(mu - mref)) <= 1e-13 * max(1.0, np.max(np.abs(mref)))
    assert np.max(np.abs(var - np.diag(Sref))) <= 1e-13 * cmax


@pytest.mark.parametrize("slip,mb,alpha", [("no_jitter", False, [1.0, 1.0]), ("no_sigma_b_cross", True, [1.1, 0.8]),
                                           ("skip_tile_row", True, [1.1, 0.8]), ("wrong_band", True, [1.1, 0.8])])
def test_bar_rejects_slips(oracle, slip, mb, alpha):
    """Each slip lands above the GPU tests' parity bar max(1e-10, 64 eps cond_1(K)) * scale in mu or in var."""
    t, y, s, ttest = _case([180, 150], [140, 129], seed=11)
    delays, rho = [0.0, 2.0], 2.5
    mu, var, cond, cmax = PW.predict_row(oracle, "matern32", t, y, s, delays, alpha, rho, ttest, marginalise_b=mb)
    mu2, var2, _, _ = PW.predict_row(oracle, "matern32", t, y, s, delays, alpha, rho, ttest, marginalise_b=mb, slip=slip)
    bmu, bvar = PW.bar(cond, max(1.0, np.max(np.abs(mu)))), PW.bar(cond, cmax)
    ratio = max(np.max(np.abs(mu2 - mu)) / bmu, np.max(np.abs(var2 - var)) / bvar)
    print("%s: error / bar %.3g (cond_1(K) %.3g)" % (slip, ratio, cond))
    assert ratio > 10.0, (slip, ratio)


def test_mixture_two_pass():
    rng = np.random.default_rng(2)
    mu, var = rng.normal(10, 1, (5, 7)), rng.random((5, 7))
    w = np.array([0.0, 1.0, 3.0, 0.0, 2.0])
    mm, mv = PW.mixture(mu, var, w)
    p = w / w.sum()
    assert np.allclose(mm, p @ mu, rtol=1e-15, atol=0)
    assert np.allclose(mv, p @ var + p @ (mu ** 2) - (p @ mu) ** 2, rtol=1e-10)
    # the law of total variance: the mixture variance is at least the mean variance
    assert np.all(mv >= p @ var - 1e-12)
    mu[0] = np.nan   # a zero-weight row is skipped
    assert np.array_equal(PW.mixture(mu, var, w)[0], mm)


class _WitnessObjective:
    """An injected objective: predict_batch is the witness (plus the mixture), L and the argument rules of Objective.predict_batch."""

    def __init__(self, oracle, kname, t, y, s, floor_var=None):
        self.oracle, self.kname, self.data, self.L, self.floor_var = oracle, kname, (t, y, s), len(t), floor_var
        self.calls = []

    def predict_batch(self, delays, alpha, rho, ttest, weights=None):
        assert len(ttest) == self.L
        self.calls.append([np.asarray(a) for a in ttest])
        mu, var, _, _ = PW.predict_rows(self.oracle, self.kname, *self.data, delays, alpha, rho, ttest)
        if self.floor_var is not None:
            var = np.full_like(var, self.floor_var)
        ll, info = np.zeros(len(rho)), np.zeros(len(rho), np.int32)
        if weights is None:
            return mu, var, ll, info, None, None
        mm, mv = PW.mixture(mu, var, weights)
        return mu, var, ll, info, mm, mv


def _grid():
    delays = np.array([[0.0, 1.0], [0.0, 2.0], [0.0, 3.0]])
    alpha = np.array([[1.0, 1.3], [1.1, 1.2], [0.9, 1.4]])
    rho = np.array([2.0, 3.0, 4.0])
    w = np.array([0.2, 0.5, 0.3])
    return delays, alpha, rho, w


def test_delay_averaged_predictor_shapes(oracle):
    t, y, s, _ = _case([40, 35], [1, 1], seed=7)
    obj = _WitnessObjective(oracle, "OU", t, y, s)
    delays, alpha, rho, w = _grid()
    pred = fit.DelayAveragedPredictor(obj, delays, alpha, rho, w)
    tt = np.linspace(-2.0, 20.0, 17)
    mus, sigs = pred(tt)                                  # one array: the same times in every band
    assert len(mus) == len(sigs) == 2 and all(len(m) == 17 for m in mus + sigs)
    assert all(np.array_equal(c, tt) for c in obj.calls[-1])
    mu, var, _, _ = PW.predict_rows(oracle, "OU", t, y, s, delays, alpha, rho, [tt, tt])
    mm, mv = PW.mixture(mu, var, w)
    assert np.array_equal(mus[0], mm[:17]) and np.array_equal(mus[1], mm[17:])
    assert np.array_equal(sigs[1], np.sqrt(np.maximum(mv[17:], 1e-6)))
    mus2, sigs2 = pred(range(3))                          # a range counts as one array
    assert [len(m) for m in mus2] == [3, 3]
    per_band = [np.array([0.5, 1.5, 2.5]), np.array([4.0])]  # a list of L arrays: each band its own times
    mus3, sigs3 = pred(per_band)
    assert [len(m) for m in mus3] == [3, 1] and [len(v) for v in sigs3] == [3, 1]


def test_delay_averaged_predictor_floor(oracle):
    t, y, s, _ = _case([40, 35], [1, 1], seed=7)
    delays, alpha, rho, w = _grid()
    pred = fit.DelayAveragedPredictor(_WitnessObjective(oracle, "OU", t, y, s, floor_var=1e-9), delays, alpha, rho, w)
    _, sigs = pred(np.array([1.0, 2.0]))
    # mixture of identical variances 1e-9 plus the spread of the means; the floor lifts it to at least 1e-3
    assert all(np.all(sg >= 1e-3) for sg in sigs)


@pytest.mark.parametrize("bad", [[0.2, -0.1, 0.3], [0.2, np.nan, 0.3], [0.2, np.inf, 0.3], [0.0, 0.0, 0.0], [0.5, 0.5]])
def test_delay_averaged_predictor_weight_rules(oracle, bad):
    t, y, s, _ = _case([40, 35], [1, 1], seed=7)
    delays, alpha, rho, _ = _grid()
    with pytest.raises(ValueError):
        fit.DelayAveragedPredictor(_WitnessObjective(oracle, "OU", t, y, s), delays, alpha, rho, bad)


def test_delay_averaged_predictor_shape_rules(oracle):
    t, y, s, _ = _case([40, 35], [1, 1], seed=7)
    delays, alpha, rho, w = _grid()
    obj = _WitnessObjective(oracle, "OU", t, y, s)
    with pytest.raises(ValueError):
        fit.DelayAveragedPredictor(obj, delays[:, :1], alpha, rho, w)
    with pytest.raises(ValueError):
        fit.DelayAveragedPredictor(obj, delays, alpha[:2], rho, w)
