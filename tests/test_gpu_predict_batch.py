"""gpcc_predict_batch on the device: every row against Objective.predict (the augmented single-delay path) and the numpy witness
(tests/_predict_witness.py) over kernels, b-modes, tile edges of the training and test points; loglik and info against the gradient;
repeatability over batch sizes and slot options; failed rows; the mixture; fp32 handles; N = 4096; and the README sweep end to end.

The bar is max(1e-10, 64 eps cond_1(K)) times max(1, max|mu_ref|) for mu and max diag(cB) for the variance (tests/test_predict_batch_cpu.py
shows that it rejects the injected slips); the worst error / bar of each group is printed."""

import numpy as np
import pytest

import _grad_witness as W
import _predict_witness as PW
import gpcc_amd
from gpcc_amd import _capi, fit, synthetic
from gpcc_amd.api import _d, _dp, _flatten, _ip

pytestmark = pytest.mark.gpu

KERNELS = {"OU": gpcc_amd.OU, "rbf": gpcc_amd.rbf, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}

# N -> (training band lengths, test points per band): band and tile edges of both sides, a band without test points
GEOMETRY = {2: ([2], [3]), 60: ([60], [129]), 127: ([40, 40, 47], [127, 0, 1]), 128: ([16] * 8, [1, 0, 127, 1, 0, 2, 0, 1]),
            129: ([100, 29], [128, 1]), 385: ([129, 127, 129], [300, 0, 129]), 1024: ([512, 512], [128, 129])}


def _tests(t, delays, Nt, seed):
    """Test times per band over the training span; a few of them coincide with shifted training times of another band
    (t*_j - tau_q = t_i - tau_p)."""
    rng = np.random.default_rng(seed)
    L = len(t)
    out = []
    for q, n in enumerate(Nt):
        tq = np.sort(rng.uniform(-3.0, 33.0, n))
        for k in range(min(3, n)):
            p = (q + 1 + k) % L
            i = int(rng.integers(len(t[p])))
            tq[k] = t[p][i] - delays[p] + delays[q]
        out.append(tq)
    return out


class Worst:
    def __init__(self, group):
        self.group, self.worst, self.where = group, 0.0, None

    def add(self, r, where):
        if r >= self.worst:
            self.worst, self.where = r, where
        assert r <= 1.0, (where, r)

    def report(self):
        print("%s: worst error / bar %.3g (%s)" % (self.group, self.worst, self.where))


def _check_rows(oracle, name, data, mb, obj, delays, alpha, rho, ttest, mu, var, worst, label):
    for m in range(len(rho)):
        wm, wv, cond, cmax = PW.predict_row(oracle, name, *data, delays[m], alpha[m], rho[m], ttest, marginalise_b=mb)
        pm, pS = obj.predict(delays[m], alpha[m], rho[m], ttest)
        bmu, bvar = PW.bar(cond, max(1.0, np.max(np.abs(wm)))), PW.bar(cond, cmax)
        for ref_mu, ref_var, what in ((wm, wv, "witness"), (pm, np.diag(pS), "predict")):
            worst.add(max(np.max(np.abs(mu[m] - ref_mu)) / bmu, np.max(np.abs(var[m] - ref_var)) / bvar), (label, m, what))


@pytest.mark.parametrize("N", sorted(GEOMETRY))
def test_parity(oracle, N):
    Nl, Nt = GEOMETRY[N]
    L = len(Nl)
    data = W.ragged_data(Nl, seed=N)
    worst = Worst("parity N = %d, L = %d, T = %d" % (N, L, sum(Nt)))
    for ki, (name, kern) in enumerate(KERNELS.items()):
        for mb in (True, False):
            delays, alpha, rho = W.random_params(L, 2, seed=N + 10 * ki + mb)
            ttest = _tests(data[0], delays[0], Nt, seed=N + ki)
            with gpcc_amd.Objective(*data, kern, marginalise_b=mb) as obj:
                mu, var, ll, info, mm, mv = obj.predict_batch(delays, alpha, rho, ttest)
                gl, _, gi = obj.loglik_grad_batch(delays, alpha, rho)
            assert mm is None and mv is None
            assert (info == 0).all() and np.array_equal(info, gi) and np.array_equal(ll, gl), (name, mb)
            with gpcc_amd.Objective(*data, kern, marginalise_b=mb) as obj:
                _check_rows(oracle, name, data, mb, obj, delays, alpha, rho, ttest, mu, var, worst, (name, mb))
    worst.report()


def _repeat_data():
    data = W.ragged_data([170, 130], seed=300)
    delays, alpha, rho = W.random_params(2, 40, seed=31)
    ttest = _tests(data[0], delays[0], [150, 140], seed=3)
    return data, delays, alpha, rho, ttest


def test_repeatable_across_batches_and_slots():
    data, delays, alpha, rho, ttest = _repeat_data()
    with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
        full = obj.predict_batch(delays, alpha, rho, ttest)
        again = obj.predict_batch(delays, alpha, rho, ttest)
        seven = obj.predict_batch(delays[:7], alpha[:7], rho[:7], ttest)
        ones = [obj.predict_batch(delays[i:i + 1], alpha[i:i + 1], rho[i:i + 1], ttest) for i in (0, 6, 39)]
        gl, _, gi = obj.loglik_grad_batch(delays, alpha, rho)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32, slots_per_stream=8) as obj8:
        eight = obj8.predict_batch(delays, alpha, rho, ttest)
    assert (full[3] == 0).all() and np.array_equal(full[2], gl) and np.array_equal(full[3], gi)
    for k in range(4):
        assert np.array_equal(full[k], again[k]) and np.array_equal(full[k], eight[k]), k
        assert np.array_equal(full[k][:7], seven[k]), k
        for i, one in zip((0, 6, 39), ones):
            assert np.array_equal(full[k][i], one[k][0]), (k, i)


def test_failed_rows():
    from test_gpu_gradient_edges import _failure_data
    data = _failure_data()
    off = [0, 100, 300]
    delays = np.array([[0, 10, 20], [0, 1, 20], [0, 10, 12], [0, -5, 7.5], [0, 10, 3], [0, 10, 14], [0, 6, 17], [0, 3, 5]], float)
    want = [0, off[1] + 10 + 1, off[2] + 20 + 1, 0, off[2] + 150 + 1, off[2] + 212 + 1, 0, -1]
    M = len(delays)
    alpha = np.ones((M, 3))
    alpha[[0, 3, 6]] = [[0.9, 1.2, 1.1], [1.3, 0.7, 1.0], [1.0, 1.0, 0.8]]
    alpha[7] = [1.0, 0.0, 1.0]                  # alpha <= 0: info -1
    rho = np.full(M, 3.0)
    ttest = [np.linspace(0, 30, 50), np.linspace(1, 29, 7), np.linspace(2, 20, 140)]
    with gpcc_amd.Objective(*data, gpcc_amd.OU, marginalise_b=False, slots_per_stream=8) as obj:
        mu, var, ll, info, _, _ = obj.predict_batch(delays, alpha, rho, ttest)
        gl, _, gi = obj.loglik_grad_batch(delays, alpha, rho)
        assert list(info) == want and np.array_equal(info, gi)
        assert np.array_equal(ll, gl, equal_nan=True)
        bad = np.array(want) != 0
        assert np.isnan(mu[bad]).all() and np.isnan(var[bad]).all() and np.isnan(ll[bad]).all()
        assert np.isfinite(mu[~bad]).all() and np.isfinite(var[~bad]).all()
        for i in np.flatnonzero(~bad):
            one = obj.predict_batch(delays[i:i + 1], alpha[i:i + 1], rho[i:i + 1], ttest)
            assert np.array_equal(one[0][0], mu[i]) and np.array_equal(one[1][0], var[i]) and one[2][0] == ll[i], i
        # mixture: zero-weight failed rows do not matter; a positive-weight failed row makes it NaN (and the call still succeeds)
        w = np.where(bad, 0.0, 1.0 + np.arange(M))
        r0 = obj.predict_batch(delays, alpha, rho, ttest, weights=w)
        keep = ~bad
        r1 = obj.predict_batch(delays[keep], alpha[keep], rho[keep], ttest, weights=w[keep])
        assert np.array_equal(r0[4], r1[4]) and np.array_equal(r0[5], r1[5])
        w2 = w.copy()
        w2[1] = 0.5
        r2 = obj.predict_batch(delays, alpha, rho, ttest, weights=w2)
        assert np.isnan(r2[4]).all() and np.isnan(r2[5]).all()


def _mixture_only(obj, delays, alpha, rho, ttest, w):
    """gpcc_predict_batch with mu_out = var_out = NULL."""
    M = len(rho)
    Nt, tt = _flatten(ttest)
    T = int(Nt.sum())
    delays, alpha, rho, w = _d(delays), _d(alpha), _d(rho), _d(w)
    mm, mv, ll = np.empty(T), np.empty(T), np.empty(M)
    info = np.zeros(M, np.int32)
    rc = _capi.load().gpcc_predict_batch(obj._h, M, _dp(delays), _dp(alpha), _dp(rho), _ip(Nt), _dp(tt), _dp(w), None, None, _dp(mm),
                                         _dp(mv), _dp(ll), _ip(info))
    return rc, mm, mv, ll, info


def test_mixture():
    data, delays, alpha, rho, ttest = _repeat_data()
    w = np.random.default_rng(5).random(40) ** 3
    w[[3, 17]] = 0.0
    with gpcc_amd.Objective(*data, gpcc_amd.matern52) as obj:
        mu, var, ll, info, mm, mv = obj.predict_batch(delays, alpha, rho, ttest, weights=w)
        assert (info == 0).all()
        wm, wv = PW.mixture(mu, var, w)
        assert np.max(np.abs(mm - wm) / np.abs(wm)) <= 1e-13 and np.max(np.abs(mv - wv) / np.abs(wv)) <= 1e-13
        # mixture only: the same bits; the grouping (slots_per_stream) does not change them either
        rc, m2, v2, l2, i2 = _mixture_only(obj, delays, alpha, rho, ttest, w)
        assert rc == 0 and np.array_equal(m2, mm) and np.array_equal(v2, mv) and np.array_equal(l2, ll)
        for k in (0, 11, 39):   # one row of weight 1 reproduces it bitwise
            e = np.zeros(40)
            e[k] = 1.0
            r = obj.predict_batch(delays, alpha, rho, ttest, weights=e)
            assert np.array_equal(r[4], mu[k]) and np.array_equal(r[5], var[k]), k
        # the law of total variance
        p = w / w.sum()
        assert np.all(mv >= p @ var - 1e-12 * np.max(np.abs(var)))
        for bad in ([-1.0] + [1.0] * 39, [np.nan] + [1.0] * 39, [np.inf] + [1.0] * 39, [0.0] * 40):
            with pytest.raises(gpcc_amd.GpccError) as ei:
                obj.predict_batch(delays, alpha, rho, ttest, weights=np.array(bad))
            assert ei.value.code == -1
    with gpcc_amd.Objective(*data, gpcc_amd.matern52, slots_per_stream=3, streams=2) as obj3:
        r3 = obj3.predict_batch(delays, alpha, rho, ttest, weights=w)
    assert np.array_equal(r3[4], mm) and np.array_equal(r3[5], mv) and np.array_equal(r3[0], mu)


def test_argument_errors():
    data, delays, alpha, rho, ttest = _repeat_data()
    with gpcc_amd.Objective(*data, gpcc_amd.OU) as obj:
        with pytest.raises(AssertionError):
            obj.predict_batch(delays, alpha, rho, ttest[:1])
        with pytest.raises(gpcc_amd.GpccError):
            obj.predict_batch(delays, alpha, rho, [np.zeros(0), np.zeros(0)])
        with pytest.raises(gpcc_amd.GpccError):
            obj.predict_batch(delays, alpha, rho, [np.zeros(20000), np.zeros(13000)])
        with pytest.raises(ValueError):
            obj.predict_batch(delays, alpha, rho, ttest, weights=np.ones(3))


def test_fp32_handle_runs_the_fp64_twin():
    data, delays, alpha, rho, ttest = _repeat_data()
    w = np.linspace(1.0, 2.0, 40)
    with gpcc_amd.Objective(*data, gpcc_amd.rbf) as o64:
        r64 = o64.predict_batch(delays, alpha, rho, ttest, weights=w)
    with gpcc_amd.Objective(*data, gpcc_amd.rbf, precision="fp32") as o32:
        r32 = o32.predict_batch(delays, alpha, rho, ttest, weights=w)
    with gpcc_amd.Objective(*data, gpcc_amd.rbf, devices=[0, 0]) as om:
        rm = om.predict_batch(delays, alpha, rho, ttest, weights=w)
    for other in (r32, rm):
        for a, b in zip(r64, other):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("N", [4095, 4096])
def test_large(oracle, N):
    Nl = [N // 2, N - N // 2]
    data = W.ragged_data(Nl, seed=N)
    delays, alpha, rho = W.random_params(2, 4, seed=N)
    ttest = _tests(data[0], delays[0], [256, 256], seed=N)
    worst = Worst("N = %d, M = 4, T = 512" % N)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
        mu, var, ll, info, _, _ = obj.predict_batch(delays, alpha, rho, ttest)
        assert (info == 0).all()
        for m in range(4):
            K, _ = oracle.model_matrix("matern32", *data, delays[m], alpha[m], rho[m], True)
            cond = np.linalg.norm(K, 1) * np.linalg.norm(np.linalg.inv(K), 1)
            pm, pS = obj.predict(delays[m], alpha[m], rho[m], ttest)
            cmax = np.max(alpha[m] ** 2 + 100 * np.array([np.var(a, ddof=1) for a in data[1]]))
            worst.add(max(np.max(np.abs(mu[m] - pm)) / PW.bar(cond, max(1.0, np.max(np.abs(pm)))),
                          np.max(np.abs(var[m] - np.diag(pS))) / PW.bar(cond, cmax)), m)
    worst.report()


def test_readme_sweep_end_to_end(oracle):
    """The README's two-band sweep (N = 110, 101 delays): gpcc_grid with the Laplace evidence, then DelayAveragedPredictor."""
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    grid = np.arange(0.0, 20.01, 0.2)
    cand = np.stack([np.zeros_like(grid), grid], 1)
    res = fit.gpcc_grid(t, y, s, kernel=gpcc_amd.OU, candidatedelays=cand, iterations=1000, evidence="laplace")
    ok = np.isfinite(res.log_evidence)
    assert ok.sum() >= len(grid) // 2
    w = gpcc_amd.getprobabilities(np.where(ok, res.log_evidence, -np.inf))
    tt = np.linspace(-1.0, 21.0, 201)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        pred = fit.DelayAveragedPredictor(obj, cand, res.alpha, res.rho, w)
        mus, sigs = pred(tt)
        mu, var, _, info, mm, mv = obj.predict_batch(cand, res.alpha, res.rho, [tt, tt], weights=w)
    pos = w > 0
    assert (info[pos] == 0).all()
    wmu, wvar, conds, cmaxs = PW.predict_rows(oracle, "OU", t, y, s, cand[pos], res.alpha[pos], res.rho[pos], [tt, tt])
    xm, xv = PW.mixture(wmu, wvar, w[pos])
    cond, cmax = np.max(conds), np.max(cmaxs)
    got_mu, got_sig = np.concatenate(mus), np.concatenate(sigs)
    assert np.max(np.abs(got_mu - xm)) <= PW.bar(cond, max(1.0, np.max(np.abs(xm))))
    assert np.max(np.abs(got_sig ** 2 - np.maximum(xv, 1e-6))) <= PW.bar(cond, cmax)
    # the law of total variance, and the mean inside the range of the positive-weight rows' means
    p = w / w.sum()
    assert np.all(mv >= p @ np.where(pos[:, None], var, 0.0) - 1e-12 * np.max(np.abs(var[pos])))
    lo, hi = np.min(mu[pos], axis=0), np.max(mu[pos], axis=0)
    eps = 1e-12 * max(1.0, np.max(np.abs(mu[pos])))
    assert np.all(mm >= lo - eps) and np.all(mm <= hi + eps)
    print("README sweep: %d delays with weight > 0, max sigma %.3g, min %.3g" % (pos.sum(), np.max(got_sig), np.min(got_sig)))
