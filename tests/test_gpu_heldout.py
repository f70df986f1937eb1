"""gpcc_heldout_loglik_batch on the device: every row against the numpy witness (tests/_heldout_witness.py) and against the single-row
Predictor(ttest, ytest, sigmatest) over kernels, b-modes, tile edges of the training and test points; loglik and info against the
gradient; repeatability over batch sizes and slot options; training and test-block failures and the Python fallback; the mixture; fp32
handles; N = 4096; and cross-validation at the README size against the loop of gpcc fits it replaces.

The bar is max(1e-10, 64 eps cond_1(K_aug)) * max(1, |l_ref|) (tests/test_heldout_cpu.py shows that it rejects the injected slips); the
worst error / bar of each group is printed."""

import numpy as np
import pytest

import _grad_witness as W
import _heldout_witness as HW
import gpcc_amd
from gpcc_amd import _capi, api, fit, synthetic
from gpcc_amd.api import _d, _dp, _flatten, _ip

pytestmark = pytest.mark.gpu

KERNELS = {"OU": gpcc_amd.OU, "rbf": gpcc_amd.rbf, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}

# N -> (training band lengths, test points per band): T = 1, 127, 128, 129, 300 -- test blocks that start and end on and off tile
# edges --, L = 1 .. 8, bands without test points
GEOMETRY = {2: ([2], [1]), 60: ([60], [127]), 127: ([40, 40, 47], [127, 0, 1]), 128: ([16] * 8, [1, 0, 127, 1, 0, 0, 0, 0]),
            129: ([100, 29], [300, 0]), 385: ([129, 127, 129], [100, 0, 200]), 1024: ([512, 512], [64, 65])}


def _testset(t, y, delays, Nt, seed):
    """Test times per band over the training span -- a few of them equal to shifted training times of another band (t*_j - tau_q =
    t_i - tau_p) --, fluxes around the band's training mean and noise levels."""
    rng = np.random.default_rng(seed)
    L = len(t)
    tt, yt, st = [], [], []
    for q, n in enumerate(Nt):
        tq = np.sort(rng.uniform(-3.0, 33.0, n))
        for k in range(min(3, n)):
            p = (q + 1 + k) % L
            i = int(rng.integers(len(t[p])))
            tq[k] = t[p][i] - delays[p] + delays[q]
        tt.append(tq)
        yt.append(rng.normal(np.mean(y[q]), np.std(y[q]) + 0.1, n))
        st.append(0.05 + 0.2 * rng.random(n))
    return tt, yt, st


class Worst:
    def __init__(self, group):
        self.group, self.worst, self.where = group, 0.0, None

    def add(self, r, where):
        if r >= self.worst:
            self.worst, self.where = r, where
        assert r <= 1.0, (where, r)

    def report(self):
        print("%s: worst error / bar %.3g (%s)" % (self.group, self.worst, self.where))


@pytest.mark.parametrize("N", sorted(GEOMETRY))
def test_parity(oracle, N):
    Nl, Nt = GEOMETRY[N]
    L = len(Nl)
    data = W.ragged_data(Nl, seed=N)
    worst = Worst("parity N = %d, L = %d, T = %d" % (N, L, sum(Nt)))
    for ki, (name, kern) in enumerate(KERNELS.items()):
        for mb in (True, False):
            delays, alpha, rho = W.random_params(L, 2, seed=N + 10 * ki + mb)
            tt, yt, st = _testset(data[0], data[1], delays[0], Nt, seed=N + ki)
            with gpcc_amd.Objective(*data, kern, marginalise_b=mb) as obj:
                held, ll, info, mix, refit = obj.heldout_loglik_batch(delays, alpha, rho, tt, yt, st)
                gl, _, gi = obj.loglik_grad_batch(delays, alpha, rho)
                assert mix is None and not refit.any()
                assert (info == 0).all() and np.array_equal(info, gi) and np.array_equal(ll, gl), (name, mb)   # bitwise the gradient's
                for m in range(2):
                    ref, cond = HW.heldout_row(oracle, name, *data, delays[m], alpha[m], rho[m], tt, yt, st, marginalise_b=mb)
                    pr = fit.Predictor(obj, delays[m], alpha[m], rho[m])(tt, yt, st)
                    worst.add(abs(held[m] - ref) / HW.bar(cond, ref), ((name, mb), m, "witness"))
                    worst.add(abs(held[m] - pr) / HW.bar(cond, pr), ((name, mb), m, "Predictor"))
    worst.report()


def _repeat_data():
    data = W.ragged_data([170, 130], seed=300)
    delays, alpha, rho = W.random_params(2, 40, seed=31)
    tt, yt, st = _testset(data[0], data[1], delays[0], [150, 140], seed=3)
    return data, delays, alpha, rho, (tt, yt, st)


def test_repeatable_across_batches_slots_and_precision():
    data, delays, alpha, rho, ts = _repeat_data()
    with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
        full = obj.heldout_loglik_batch(delays, alpha, rho, *ts)
        again = obj.heldout_loglik_batch(delays, alpha, rho, *ts)
        seven = obj.heldout_loglik_batch(delays[:7], alpha[:7], rho[:7], *ts)
        ones = [obj.heldout_loglik_batch(delays[i:i + 1], alpha[i:i + 1], rho[i:i + 1], *ts) for i in (0, 6, 39)]
        gl, _, gi = obj.loglik_grad_batch(delays, alpha, rho)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32, slots_per_stream=8) as obj8:
        eight = obj8.heldout_loglik_batch(delays, alpha, rho, *ts)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32, slots_per_stream=3, streams=2) as obj3:
        three = obj3.heldout_loglik_batch(delays, alpha, rho, *ts)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32, precision="fp32") as o32:
        f32 = o32.heldout_loglik_batch(delays, alpha, rho, *ts)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32, devices=[0, 0]) as om:
        multi = om.heldout_loglik_batch(delays, alpha, rho, *ts)
    assert (full[2] == 0).all() and np.array_equal(full[1], gl) and np.array_equal(full[2], gi)
    for k in range(3):
        for other in (again, eight, three, f32, multi):
            assert np.array_equal(full[k], other[k]), k
        assert np.array_equal(full[k][:7], seven[k]), k
        for i, one in zip((0, 6, 39), ones):
            assert np.array_equal(full[k][i], one[k][0]), (k, i)


@pytest.mark.parametrize("N", [4095, 4096])
def test_large(oracle, N):
    Nl = [N // 2, N - N // 2]
    data = W.ragged_data(Nl, seed=N)
    delays, alpha, rho = W.random_params(2, 4, seed=N)
    tt, yt, st = _testset(data[0], data[1], delays[0], [410, 410], seed=N)
    worst = Worst("N = %d, M = 4, T = 820" % N)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
        held, ll, info, _, _ = obj.heldout_loglik_batch(delays, alpha, rho, tt, yt, st)
        assert (info == 0).all()
        for m in range(4):
            ref, cond = HW.heldout_row(oracle, "matern32", *data, delays[m], alpha[m], rho[m], tt, yt, st)
            worst.add(abs(held[m] - ref) / HW.bar(cond, ref), m)
    worst.report()


def test_training_failure_rows():
    from test_gpu_gradient_edges import _failure_data
    data = _failure_data()
    N = sum(len(a) for a in data[0])
    delays = np.array([[0, 10, 20], [0, 1, 20], [0, 10, 12], [0, -5, 7.5], [0, 10, 3], [0, 6, 17]], float)
    M = len(delays)
    alpha = np.ones((M, 3))
    alpha[[0, 3, 5]] = [[0.9, 1.2, 1.1], [1.3, 0.7, 1.0], [1.0, 1.0, 0.8]]
    rho = np.full(M, 3.0)
    rng = np.random.default_rng(1)
    tt = [np.linspace(0, 30, 50), np.linspace(1, 29, 7), np.linspace(2, 20, 140)]
    yt = [rng.normal(0, 1, len(a)) for a in tt]
    st = [np.full(len(a), 0.1) for a in tt]
    with gpcc_amd.Objective(*data, gpcc_amd.OU, marginalise_b=False, slots_per_stream=8) as obj:
        held, ll, info, _, _ = obj.heldout_loglik_batch(delays, alpha, rho, tt, yt, st)
        gl, _, gi = obj.loglik_grad_batch(delays, alpha, rho)
        bad = info != 0
        assert bad.sum() >= 2 and np.all((info[bad] >= 1) & (info[bad] <= N)), info
        assert np.array_equal(info, gi) and np.array_equal(ll, gl, equal_nan=True)
        assert np.isnan(held[bad]).all() and np.isfinite(held[~bad]).all()
        for i in np.flatnonzero(~bad):
            one = obj.heldout_loglik_batch(delays[i:i + 1], alpha[i:i + 1], rho[i:i + 1], tt, yt, st)
            assert one[0][0] == held[i] and one[1][0] == ll[i], i
        # mixture: zero-weight failed rows are skipped; a positive-weight failed row makes it NaN (the call still succeeds)
        w = np.where(bad, 0.0, 1.0 + np.arange(M))
        r0 = obj.heldout_loglik_batch(delays, alpha, rho, tt, yt, st, weights=w)
        r1 = obj.heldout_loglik_batch(delays[~bad], alpha[~bad], rho[~bad], tt, yt, st, weights=w[~bad])
        assert r0[3] == r1[3] and np.isfinite(r0[3])
        w[np.flatnonzero(bad)[0]] = 0.5
        assert np.isnan(obj.heldout_loglik_batch(delays, alpha, rho, tt, yt, st, weights=w)[3])


def test_test_block_failure_and_fallback():
    """Two identical test times in one band, sigmatest = 0 and a large alpha: the 2 x 2 block of Sigma_pred + 1e-8 I is singular in
    fp64, and the device must report it as N + j with a valid training loglik.  The fallback then equals Predictor's nearestposdef
    result."""
    data = W.ragged_data([90, 70], seed=7)
    N = 160
    tt = [np.array([5.0, 12.5, 12.5, 20.0]), np.array([3.0, 17.0])]
    yt = [np.array([0.1, 0.2, 0.2, -0.1]), np.array([0.0, 0.3])]
    st = [np.zeros(4), np.zeros(2)]
    delays, rho = np.array([[0.0, 2.0]]), np.array([2.0])
    seen = None
    with gpcc_amd.Objective(*data, gpcc_amd.matern52, marginalise_b=False) as obj:
        for a in (1e1, 1e2, 1e3, 1e4, 1e5, 1e6):
            alpha = np.array([[a, 1.0]])
            held, ll, info, _, refit = obj.heldout_loglik_batch(delays, alpha, rho, tt, yt, st, fallback=False)
            if info[0] > N:
                seen = (a, alpha, held, ll, info)
                break
        assert seen is not None, "no test-block failure reported up to alpha = 1e6"
        a, alpha, held, ll, info = seen
        assert N < info[0] <= N + 6 and np.isnan(held[0]) and not refit[0]
        gl, _, gi = obj.loglik_grad_batch(delays, alpha, rho)
        assert gi[0] == 0 and ll[0] == gl[0]
        h2, l2, i2, _, r2 = obj.heldout_loglik_batch(delays, alpha, rho, tt, yt, st)
        try:
            ref = fit.Predictor(obj, delays[0], alpha[0], rho[0])(tt, yt, st)
        except gpcc_amd.PosDefException:
            ref = None
        if ref is None:
            assert np.isnan(h2[0]) and not r2[0]
        else:
            assert r2[0] and h2[0] == ref
        # the mixture is recomputed on the host from the final rows when such a row has weight
        d3 = np.concatenate([delays, [[0.0, 2.5]]])
        a3 = np.concatenate([alpha, [[1.0, 1.0]]])
        r3 = np.array([2.0, 2.0])
        h3, _, i3, mx, f3 = obj.heldout_loglik_batch(d3, a3, r3, tt, yt, st, weights=[1.0, 3.0])
        if f3[0]:
            assert mx == api.logsumexp_rows(h3, np.array([0.25, 0.75]))
    print("test-block failure at alpha = %g: info = N + %d" % (a, info[0] - N))


def _mixture_only(obj, delays, alpha, rho, ts, w):
    """gpcc_heldout_loglik_batch with heldout = NULL."""
    M = len(rho)
    Nt, tt = _flatten(ts[0])
    _, yt = _flatten(ts[1])
    _, st = _flatten(ts[2])
    delays, alpha, rho, w = _d(delays), _d(alpha), _d(rho), _d(w)
    mix, ll = np.empty(1), np.empty(M)
    info = np.zeros(M, np.int32)
    rc = _capi.load().gpcc_heldout_loglik_batch(obj._h, M, _dp(delays), _dp(alpha), _dp(rho), _ip(Nt), _dp(tt), _dp(yt), _dp(st),
                                                _dp(w), None, _dp(mix), _dp(ll), _ip(info))
    return rc, float(mix[0]), ll, info


def test_mixture():
    data, delays, alpha, rho, ts = _repeat_data()
    w = np.random.default_rng(5).random(40) ** 3
    w[[3, 17]] = 0.0
    with gpcc_amd.Objective(*data, gpcc_amd.matern52) as obj:
        held, ll, info, mix, _ = obj.heldout_loglik_batch(delays, alpha, rho, *ts, weights=w)
        assert (info == 0).all()
        p = w / w.sum()
        keep = p > 0
        mx = np.max(np.log(p[keep]) + held[keep])
        ref = mx + np.log(np.sum(np.exp(np.log(p[keep]) + held[keep] - mx)))
        assert abs(mix - ref) <= 1e-13 * abs(ref)
        assert mix == api.logsumexp_rows(held, p) or abs(mix - api.logsumexp_rows(held, p)) <= 1e-14 * abs(mix)
        rc, m2, l2, _ = _mixture_only(obj, delays, alpha, rho, ts, w)
        assert rc == 0 and m2 == mix and np.array_equal(l2, ll)
        for k in (0, 11, 39):   # one row of weight 1 returns its own bits
            e = np.zeros(40)
            e[k] = 1.0
            assert obj.heldout_loglik_batch(delays, alpha, rho, *ts, weights=e)[3] == held[k], k
        for bad in ([-1.0] + [1.0] * 39, [np.nan] + [1.0] * 39, [np.inf] + [1.0] * 39, [0.0] * 40):
            with pytest.raises(gpcc_amd.GpccError) as ei:
                obj.heldout_loglik_batch(delays, alpha, rho, *ts, weights=np.array(bad))
            assert ei.value.code == -1
    with gpcc_amd.Objective(*data, gpcc_amd.matern52, slots_per_stream=3, streams=2) as obj3:
        r3 = obj3.heldout_loglik_batch(delays, alpha, rho, *ts, weights=w)
    assert r3[3] == mix and np.array_equal(r3[0], held)


def test_argument_errors():
    data, delays, alpha, rho, (tt, yt, st) = _repeat_data()
    with gpcc_amd.Objective(*data, gpcc_amd.OU) as obj:
        with pytest.raises(AssertionError):
            obj.heldout_loglik_batch(delays, alpha, rho, tt[:1], yt[:1], st[:1])
        with pytest.raises(gpcc_amd.GpccError):
            obj.heldout_loglik_batch(delays, alpha, rho, [np.zeros(0)] * 2, [np.zeros(0)] * 2, [np.zeros(0)] * 2)
        with pytest.raises(ValueError):
            obj.heldout_loglik_batch(delays, alpha, rho, tt, [yt[0], yt[1][:3]], st)
        with pytest.raises(ValueError):
            obj.heldout_loglik_batch(delays, alpha, rho, tt, yt, st, weights=np.ones(3))


def _readme():
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    grid = np.arange(0.0, 20.01, 0.2)
    return t, y, s, np.stack([np.zeros_like(grid), grid], 1)


def test_cross_validation_readme_size(oracle):
    """performcv_grid at the README size (N = 110, 101 delays, 5 folds) against the loop it replaces: fit.gpcc on each split and
    delay, then Predictor(ttest, ytest, stest); performcv at one delay against its column; DelayAveragedPredictor.loglik against the
    fold's mixture."""
    t, y, s, cand = _readme()
    it = 40
    cv = fit.performcv_grid(t, y, s, candidatedelays=cand, kernel=gpcc_amd.OU, iterations=it)
    F, G = cv.heldout.shape
    assert (F, G) == (5, 101) and np.array_equal(cv.cv_score, cv.heldout.sum(0))
    assert np.isfinite(cv.mix).all() and abs(cv.probabilities.sum() - 1.0) < 1e-12
    folds = fit.cvindices([60, 50], 5, 1)
    worst = Worst("README CV: performcv_grid vs loop of gpcc + Predictor")
    for f in range(F):
        (ttr, ytr, str_), (tte, yte, ste) = fit._split(t, y, s, folds, f)
        for g in range(G):
            _, pred, _ = fit.gpcc(ttr, ytr, str_, kernel=gpcc_amd.OU, delays=cand[g], iterations=it, initialrandom=1, seed=1,
                                  rhomin=0.1, rhomax=20.0)
            ref = pred(tte, yte, ste)
            pred.obj.close()
            if g % 25 == 0:
                _, cond = HW.heldout_row(oracle, "OU", ttr, ytr, str_, cand[g], pred.alpha, pred.rho, tte, yte, ste)
                b = HW.bar(cond, ref)
            worst.add(abs(cv.heldout[f, g] - ref) / b, (f, g))
        with gpcc_amd.Objective(ttr, ytr, str_, gpcc_amd.OU) as obj:
            dap = fit.DelayAveragedPredictor(obj, cand, cv.fits[f].alpha, cv.fits[f].rho, cv.weights[f])
            assert dap.loglik(tte, yte, ste) == cv.mix[f]
    worst.report()
    g = 10
    pcv = fit.performcv(t, y, s, delays=cand[g], kernel=gpcc_amd.OU, iterations=it)
    assert np.max(np.abs(pcv - cv.heldout[:, g]) / np.maximum(1.0, np.abs(pcv))) <= 1e-9, (pcv, cv.heldout[:, g])
    lap = fit.performcv_grid(t, y, s, candidatedelays=cand, kernel=gpcc_amd.OU, iterations=it, evidence="laplace")
    assert np.array_equal(lap.heldout, cv.heldout) and np.isfinite(lap.mix).all()
    print("README CV: mix per fold %s, cv mode at delay %.1f" % (np.round(cv.mix, 3), cand[int(np.argmax(cv.probabilities)), 1]))
