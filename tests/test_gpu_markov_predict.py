"""gpcc_predict_markov_batch, gpcc_heldout_loglik_markov_batch and gpcc_posterior_offsets_markov_batch on the device: parity with the
dense witnesses over the CPU cases of tests/_markov_predict_cases.py and at N = 2048, 4095 and 4096 (the dense entries' own bars,
measured on the reference side; the worst error / bar of each group is printed); the numpy mirror within twice the bar; loglik and
info bitwise gpcc_loglik_markov_batch's; bitwise invariance over batch sizes, row order, chunking and handle flavours; the mixtures;
refusals and failed rows (argument-level only); the predictors and the cross-validation with solver="markov"; memory."""
import numpy as np
import pytest

import _heldout_witness as HW
import _markov_cases as MC
import _markov_predict_cases as PC
import _predict_witness as PW
import gpcc_amd
from gpcc_amd import fit, markov, synthetic

pytestmark = pytest.mark.gpu

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
UNSUPPORTED, ARGUMENT = -3, -1


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_parity_cpu_cases(oracle, kernel):
    wm, wv, wh = (MC.Worst("device %s %s" % (what, kernel)) for what in ("mu", "var", "held-out"))
    n = 0
    for case in PC.cpu_cases():
        cid, k, data, delays, alpha, rho, mb, tests = case
        if k != kernel:
            continue
        n += 1
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll0, info0 = obj.loglik_markov_batch(delays[None, :], alpha[None, :], [rho])
            mu, var, ll, info, _, _ = obj.predict_markov_batch(delays[None, :], alpha[None, :], [rho], tests[0])
            held, llh, infoh, _ = obj.heldout_loglik_markov_batch(delays[None, :], alpha[None, :], [rho], *tests)
            if mb:
                pmu, pS, llp, infop = obj.posterior_offsets_markov_batch(delays[None, :], alpha[None, :], [rho])
        assert info0[0] == 0 and info[0] == 0 and infoh[0] == 0, cid
        assert np.array_equal(ll, ll0) and np.array_equal(llh, ll0), cid
        rmu, rvar, bmu, bvar = PC.predict_reference(oracle, case)
        wm.add(float(np.max(np.abs(mu[0] - rmu))), bmu, cid)
        wv.add(float(np.max(np.abs(var[0] - rvar))), bvar, cid)
        ref, bh = PC.heldout_reference(oracle, case)
        wh.add(abs(held[0] - ref), bh, cid)
        hmu, hvar, _, _ = markov.predict(k, *data, delays, alpha, rho, tests[0], mb)      # the numpy mirror: another rounding order
        assert np.max(np.abs(mu[0] - hmu)) <= 2 * bmu and np.max(np.abs(var[0] - hvar)) <= 2 * bvar, cid
        assert abs(held[0] - markov.heldout(k, *data, delays, alpha, rho, *tests, mb)[0]) <= 2 * bh, cid
        if mb:
            assert infop[0] == 0 and np.array_equal(llp, ll0), cid
            PC.assert_postb(pmu[0], pS[0], *PC.postb_reference(oracle, k, *data, delays, alpha, rho))
    assert n == 3 * 2 * len(MC.RHOS)
    for w in (wm, wv, wh):
        w.report()


LARGE = {2048: ("OU", [1024, 1024]), 4095: ("matern32", [1500, 1300, 1295]), 4096: ("matern52", [2048, 2048])}


def _large(N, G=16, T=256):
    kernel, Nl = LARGE[N]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=N)
    L = len(Nl)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    delays = np.zeros((G, L))
    delays[:, 1:] = np.linspace(0.0, 12.6, G)[:, None] * (1.0 + 0.5 * np.arange(L - 1))[None, :]
    rg = np.random.default_rng(N)
    lo, hi = min(np.min(a) for a in t), max(np.max(a) for a in t)
    tt = [rg.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), T) for _ in range(L)]      # unsorted, beyond the data on both sides
    yt = [np.mean(y[l]) + np.std(y[l]) * rg.standard_normal(T) for l in range(L)]
    st = [np.mean(s[l]) * (0.5 + rg.random(T)) for l in range(L)]
    return kernel, (t, y, s), delays, np.tile(alpha0, (G, 1)), np.full(G, rho0), (tt, yt, st)


@pytest.mark.parametrize("N", sorted(LARGE))
def test_parity_large(oracle, N):
    """16 delays, T = 256 per band, against the dense witnesses row by row."""
    kernel, data, delays, alpha, rho, tests = _large(N)
    with gpcc_amd.Objective(*data, KERN[kernel]) as obj:
        ll0, info0 = obj.loglik_markov_batch(delays, alpha, rho)
        mu, var, ll, info, _, _ = obj.predict_markov_batch(delays, alpha, rho, tests[0])
        held, llh, infoh, _ = obj.heldout_loglik_markov_batch(delays, alpha, rho, *tests)
        pmu, pS, llp, infop = obj.posterior_offsets_markov_batch(delays, alpha, rho)
    assert (info0 == 0).all() and (info == 0).all() and (infoh == 0).all() and (infop == 0).all()
    assert np.array_equal(ll, ll0) and np.array_equal(llh, ll0) and np.array_equal(llp, ll0)
    wm, wv, wh = (MC.Worst("device %s %s N = %d, 16 delays, T = %d" % (what, kernel, N, mu.shape[1])) for what in ("mu", "var", "held-out"))
    for g in range(len(rho)):
        rmu, rvar, cond, cmax = PW.predict_row(oracle, kernel, *data, delays[g], alpha[g], rho[g], tests[0], True)
        wm.add(float(np.max(np.abs(mu[g] - rmu))), PW.bar(cond, max(1.0, float(np.max(np.abs(rmu))))), g)
        wv.add(float(np.max(np.abs(var[g] - rvar))), PW.bar(cond, cmax), g)
        ref, conda = HW.heldout_row(oracle, kernel, *data, delays[g], alpha[g], rho[g], *tests, True)
        wh.add(abs(held[g] - ref), HW.bar(conda, ref), g)
    for w in (wm, wv, wh):
        w.report()
    PC.assert_postb(pmu[0], pS[0], *PC.postb_reference(oracle, kernel, *data, delays[0], alpha[0], rho[0]))


def _batch(L, M, seed):
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 45.0, (M, L - 1)))], 1)
    return delays, rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))


def _all_three(obj, delays, alpha, rho, tests, mb):
    mu, var, ll, info, _, _ = obj.predict_markov_batch(delays, alpha, rho, tests[0])
    held, llh, infoh, _ = obj.heldout_loglik_markov_batch(delays, alpha, rho, *tests)
    out = [mu, var, ll, info, held, llh, infoh]
    if mb:
        out += list(obj.posterior_offsets_markov_batch(delays, alpha, rho))
    return out


def _same(got, full, rows):
    return all(np.array_equal(a, b[rows], equal_nan=True) for a, b in zip(got, full))


@pytest.mark.parametrize("kernel,Nl,mb", [("matern52", [300, 200, 267], True), ("OU", [60, 50], False), ("matern32", [2048, 2048], True)])
def test_bitwise_invariance(kernel, Nl, mb):
    t, y, s, d0 = MC.lightcurves(Nl, seed=7, kind="ties")
    L = len(Nl)
    tests = PC.test_points(t, d0, 8, -1)
    delays, alpha, rho = _batch(L, 257, seed=L)
    delays[0] = d0                                               # (a row whose test points tie with training points)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        full = _all_three(obj, delays, alpha, rho, tests, mb)
        ll0, info0 = obj.loglik_markov_batch(delays, alpha, rho)
        assert (full[3] == 0).all() and (full[6] == 0).all() and np.isfinite(full[0]).all() and np.isfinite(full[4]).all()
        assert np.array_equal(full[2], ll0) and np.array_equal(full[5], ll0) and np.array_equal(full[3], info0)
        for M in (1, 63, 64, 65):
            assert _same(_all_three(obj, delays[:M], alpha[:M], rho[:M], tests, mb), full, slice(0, M)), M
        perm = np.random.default_rng(1).permutation(257)
        assert _same(_all_three(obj, delays[perm], alpha[perm], rho[perm], tests, mb), full, perm)
        for chunk in (7, 64, 100):
            obj.set_option("markov_chunk_rows", chunk)
            assert _same(_all_three(obj, delays, alpha, rho, tests, mb), full, slice(None)), chunk
        obj.set_option("markov_chunk_rows", 0)
        # sorted test times give the unsorted call's values at the sorted positions
        order = [np.argsort(a, kind="stable") for a in tests[0]]
        mu_s = obj.predict_markov_batch(delays[:5], alpha[:5], rho[:5], [a[o] for a, o in zip(tests[0], order)])[0]
        off = np.concatenate([[0], np.cumsum([len(a) for a in tests[0]])])
        flat = np.concatenate([off[l] + order[l] for l in range(L)])
        assert np.array_equal(mu_s, full[0][:5][:, flat])
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, precision="fp32") as o32:
        assert _same(_all_three(o32, delays[:65], alpha[:65], rho[:65], tests, mb), full, slice(0, 65))
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, devices=[0, 0]) as om:
        assert _same(_all_three(om, delays[:65], alpha[:65], rho[:65], tests, mb), full, slice(0, 65))


def test_mixtures():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=9, kind="ties")
    tests = PC.test_points(t, d0, 10, -1)
    delays, alpha, rho = _batch(2, 130, seed=4)
    w = np.random.default_rng(2).uniform(0.0, 1.0, 130)
    w[[3, 64, 129]] = 0.0
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        mu, var, _, info, mm, mv = obj.predict_markov_batch(delays, alpha, rho, tests[0], weights=w)
        held, _, infoh, mix = obj.heldout_loglik_markov_batch(delays, alpha, rho, *tests, weights=w)
        assert (info == 0).all() and (infoh == 0).all()
        rm, rv = PW.mixture(mu, var, w)
        np.testing.assert_allclose(mm, rm, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(mv, rv, rtol=1e-11, atol=1e-13)
        p = w / w.sum()
        x = np.log(p[p > 0]) + held[p > 0]
        assert abs(mix - (x.max() + np.log(np.sum(np.exp(x - x.max()))))) <= 1e-12 * abs(mix)
        obj.set_option("markov_chunk_rows", 50)                  # the running mixture across chunks: the same bits
        _, _, _, _, mm2, mv2 = obj.predict_markov_batch(delays, alpha, rho, tests[0], weights=w)
        assert np.array_equal(mm2, mm) and np.array_equal(mv2, mv)
        obj.set_option("markov_chunk_rows", 0)
        one = np.zeros(130)
        one[17] = 2.5                                            # one row of weight: its own bits
        _, _, _, _, mm1, mv1 = obj.predict_markov_batch(delays, alpha, rho, tests[0], weights=one)
        assert np.array_equal(mm1, mu[17]) and np.array_equal(mv1, var[17])
        assert obj.heldout_loglik_markov_batch(delays, alpha, rho, *tests, weights=one)[3] == held[17]
        a2 = alpha.copy()
        a2[3, 0] = -1.0                                          # a failed row of weight zero is skipped
        mu3, _, _, info3, mm3, mv3 = obj.predict_markov_batch(delays, a2, rho, tests[0], weights=w)
        held3, _, infoh3, mix3 = obj.heldout_loglik_markov_batch(delays, a2, rho, *tests, weights=w)
        assert info3[3] == -1 and infoh3[3] == -1 and np.isnan(mu3[3]).all() and np.isnan(held3[3])
        assert np.array_equal(mm3, mm) and np.array_equal(mv3, mv) and mix3 == mix
        a2[5, 1] = 0.0                                           # one with weight makes the mixture NaN; the call still returns
        _, _, _, info4, mm4, mv4 = obj.predict_markov_batch(delays, a2, rho, tests[0], weights=w)
        mix4 = obj.heldout_loglik_markov_batch(delays, a2, rho, *tests, weights=w)[3]
        assert info4[5] == -1 and np.isnan(mm4).all() and np.isnan(mv4).all() and np.isnan(mix4)
        # mixture only: no rows asked for
        import ctypes
        from gpcc_amd import _capi
        Nt = np.array([len(a) for a in tests[0]], dtype=np.int32)
        tt = np.concatenate(tests[0])
        T = len(tt)
        omu, ovar, oll, oinfo = np.empty(T), np.empty(T), np.empty(130), np.zeros(130, dtype=np.int32)
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        rc = _capi.load().gpcc_predict_markov_batch(obj._h, 130, dp(delays), dp(alpha), dp(rho), Nt.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                    dp(tt), dp(w), None, None, dp(omu), dp(ovar), dp(oll), oinfo.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        assert rc == 0 and np.array_equal(omu, mm) and np.array_equal(ovar, mv)


def test_refusals_and_failed_rows():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    tests = PC.test_points(t, d0, 12, -1)
    N = 110
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        for call in (lambda: obj.predict_markov_batch([d0], [[1.0, 1.0]], [2.0], tests[0]),
                     lambda: obj.heldout_loglik_markov_batch([d0], [[1.0, 1.0]], [2.0], *tests),
                     lambda: obj.posterior_offsets_markov_batch([d0], [[1.0, 1.0]], [2.0])):
            with pytest.raises(gpcc_amd.GpccError) as ei:
                call()
            assert ei.value.code == UNSUPPORTED and "rbf" in ei.value.message
    t5, y5, s5, d5 = MC.lightcurves([30, 25, 20, 25, 30], seed=12, kind="ties")
    a5 = np.linspace(0.6, 1.4, 5)
    tt5 = [np.array([1.0, 40.0])] * 5
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=True) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.predict_markov_batch([d5], [a5], [2.0], tt5)
        assert ei.value.code == UNSUPPORTED
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=False) as obj:      # five bands without offsets are fine
        mu, var, _, info, _, _ = obj.predict_markov_batch([d5], [a5], [2.0], tt5)
        hmu, hvar, _, _ = markov.predict("OU", t5, y5, s5, d5, a5, 2.0, tt5, False)
        assert info[0] == 0 and np.max(np.abs(mu[0] - hmu)) <= 2e-10 and np.max(np.abs(var[0] - hvar)) <= 2e-10 * np.max(a5) ** 2
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.posterior_offsets_markov_batch([d5], [a5], [2.0])
        assert ei.value.code == ARGUMENT
    delays, alpha, rho = _batch(2, 8, seed=5)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        for bad in ([1.0] * 7 + [-1.0], [0.0] * 8, [1.0] * 7 + [np.nan]):
            with pytest.raises(gpcc_amd.GpccError) as ei:
                obj.predict_markov_batch(delays, alpha, rho, tests[0], weights=bad)
            assert ei.value.code == ARGUMENT
            with pytest.raises(gpcc_amd.GpccError) as ei:
                obj.heldout_loglik_markov_batch(delays, alpha, rho, *tests, weights=bad)
            assert ei.value.code == ARGUMENT
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.predict_markov_batch(delays, alpha, rho, [np.zeros(0), np.zeros(0)])      # T = 0
        assert ei.value.code == ARGUMENT
        good = _all_three(obj, delays, alpha, rho, tests, True)
        a2, r2 = alpha.copy(), rho.copy()
        a2[1, 0] = 0.0
        a2[2, 1] = -1.0
        r2[3] = 0.0
        got = _all_three(obj, delays, a2, r2, tests, True)
        ll0, info0 = obj.loglik_markov_batch(delays, a2, r2)
        for infos in (got[3], got[6], got[10]):
            assert np.array_equal(infos, info0) and list(infos[[1, 2, 3]]) == [-1, -1, -2]
        for arr in (got[0], got[1], got[4], got[7], got[8]):
            assert np.isnan(arr[[1, 2, 3]]).all()
        keep = [0, 4, 5, 6, 7]
        assert _same([g[keep] for g in got], good, keep)                                 # the neighbours are untouched
        # a non-finite sigma*: the predictive variance of that test point (the caller's order) fails in every row; loglik stays valid
        st = [a.copy() for a in tests[2]]
        st[1][4] = np.inf
        held, ll, info, _ = obj.heldout_loglik_markov_batch(delays, alpha, rho, tests[0], tests[1], st)
        assert (info == N + len(st[0]) + 4 + 1).all() and np.isnan(held).all() and np.array_equal(ll, good[2])


def _cond(oracle, kernel, t, y, s, delays, alpha, rho):
    K, _ = oracle.model_matrix(kernel, t, y, s, delays, alpha, rho, True)
    return np.linalg.norm(K, 1) * np.linalg.norm(np.linalg.inv(K), 1)


def test_predictors_against_their_dense_selves(oracle):
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    grid = np.arange(0.0, 4.01, 0.5)
    cand = np.stack([np.zeros_like(grid), grid], 1)
    G = len(grid)
    alpha, rho = np.tile(alpha0, (G, 1)), np.full(G, rho0)
    tt = np.linspace(-2.0, 24.0, 41)
    tests = PC.test_points(t, cand[4], 13, -1)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        ll, _ = obj.loglik_markov_batch(cand, alpha, rho)
        w = gpcc_amd.getprobabilities(ll)
        dense, lin = fit.Predictor(obj, cand[4], alpha0, rho0), fit.Predictor(obj, cand[4], alpha0, rho0, solver="markov")
        cond = _cond(oracle, "matern32", t, y, s, cand[4], alpha0, rho0)
        (dm, ds), (lm, ls) = dense(tt), lin(tt)
        cmax = float(np.max(alpha0) ** 2 + 100 * max(np.var(a, ddof=1) for a in y))
        for l in range(2):
            assert np.max(np.abs(dm[l] - lm[l])) <= 2 * PW.bar(cond, max(1.0, float(np.max(np.abs(dm[l])))))
            assert np.max(np.abs(ds[l] ** 2 - ls[l] ** 2)) <= 2 * PW.bar(cond, cmax)
        hd, hl = dense(*tests), lin(*tests)
        _, conda = HW.heldout_row(oracle, "matern32", t, y, s, cand[4], alpha0, rho0, *tests, True)
        assert abs(hd - hl) <= 2 * HW.bar(conda, hd)
        with pytest.raises(Exception):
            fit.Predictor(obj, cand[4], alpha0, rho0, solver="other")
        jm, jS = lin([tt, tt])                                                       # the joint form stays dense
        assert jS.shape == (82, 82)
        da, la = fit.DelayAveragedPredictor(obj, cand, alpha, rho, w), fit.DelayAveragedPredictor(obj, cand, alpha, rho, w, solver="markov")
        (dm, ds), (lm, ls) = da(tt), la(tt)
        conds = max(_cond(oracle, "matern32", t, y, s, cand[g], alpha0, rho0) for g in range(G))
        # every row of either path lies within its bar of the truth, so the rows differ by 2 bmu and 2 bvar; the mixture's mean then by
        # 2 bmu, and its variance sum p (var + (mu - mix)^2) by 2 bvar + 2 |mu - mix| 4 bmu + (4 bmu)^2 with |mu - mix| <= 2 max|mu|
        for l in range(2):
            top = float(np.max(np.abs(dm[l])))
            bmu, bvar = PW.bar(conds, max(1.0, top)), PW.bar(conds, cmax)
            assert np.max(np.abs(dm[l] - lm[l])) <= 2 * bmu
            assert np.max(np.abs(ds[l] ** 2 - ls[l] ** 2)) <= 2 * bvar + 16 * top * bmu + 16 * bmu ** 2
        assert abs(da.loglik(*tests) - la.loglik(*tests)) <= 2 * HW.bar(conda, da.loglik(*tests))
    # gpcc(..., solver="markov"): a Markov predictor and a linear-time postb, against the dense entries at the same fitted parameters
    llk, pred, (a_fit, postb, r_fit) = fit.gpcc(t, y, s, kernel=gpcc_amd.OU, delays=[0.0, 2.0], iterations=50, rhomax=20.0, solver="markov")
    assert pred.solver == "markov" and np.isfinite(llk)
    PC.assert_postb(postb[0], postb[1], *PC.postb_reference(oracle, "OU", t, y, s, [0.0, 2.0], a_fit, r_fit))
    mu_d, Sig_d = pred.obj.posterior_offsets([0.0, 2.0], a_fit, r_fit)
    np.testing.assert_allclose(postb[0], mu_d, rtol=1e-7)
    np.testing.assert_allclose(postb[1], Sig_d, rtol=1e-7, atol=1e-12)
    pred.obj.close()


def test_performcv_grid_markov_scores(oracle):
    """The folds scored by the linear-time entry, against the dense entry and the witness at the SAME fitted parameters (two fits with
    different likelihood roundings need not take the same optimiser path, so the scores are compared at the Markov run's parameters)."""
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    grid = np.arange(0.0, 4.01, 1.0)
    cand = np.stack([np.zeros_like(grid), grid], 1)
    cv = fit.performcv_grid(t, y, s, candidatedelays=cand, kernel=gpcc_amd.OU, iterations=20, numberoffolds=3, solver="markov")
    assert cv.heldout.shape == (3, len(grid)) and (cv.info == 0).all() and not cv.refit.any()
    folds = fit.cvindices([len(a) for a in t], 3, 1)
    for f in range(3):
        (ttr, ytr, str_), (tte, yte, ste) = fit._split(t, y, s, folds, f)
        res = cv.fits[f]
        with gpcc_amd.Objective(ttr, ytr, str_, gpcc_amd.OU) as obj:
            held, _, info, mix, _ = obj.heldout_loglik_batch(cand, res.alpha, res.rho, tte, yte, ste, weights=cv.weights[f])
        assert (info == 0).all()
        for g in (0, len(grid) - 1):
            ref, conda = HW.heldout_row(oracle, "OU", ttr, ytr, str_, cand[g], res.alpha[g], res.rho[g], tte, yte, ste, True)
            b = HW.bar(conda, ref)
            assert abs(cv.heldout[f, g] - ref) <= b and abs(cv.heldout[f, g] - held[g]) <= 2 * b
        assert abs(cv.mix[f] - mix) <= 2 * b


def test_memory_and_the_global_memory_path():
    """N = 16384, Matern-5/2, T = 2 x 512, 64 delays: the handle grows by the documented buffers (the tap scratch 16 T (n + n (n + 1) / 2)
    bytes per row with n = 5, mu and var 16 T per row, the light curves and the staging) and none of the N^2 workspace.  There is no
    dense fp64 reference of this size on the device (the dense path takes fp32 tiles there), so the result is held against the numpy
    mirror, within twice the floor of the witnesses' bar (1e-10 x scale: the bar is never below it)."""
    import torch
    Nl = [8192, 8192]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=3)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    delays = np.stack([np.zeros(64), np.linspace(0.0, 12.6, 64)], 1)
    alpha, rho = np.tile(alpha0, (64, 1)), np.full(64, rho0)
    rg = np.random.default_rng(5)
    hi = max(np.max(a) for a in t)
    tt = [rg.uniform(-0.02 * hi, 1.02 * hi, 512) for _ in range(2)]
    yt = [np.mean(y[l]) + np.std(y[l]) * rg.standard_normal(512) for l in range(2)]
    st = [np.full(512, float(np.mean(s[l]))) for l in range(2)]
    T, nrec = 1024, 5 + 15
    torch.cuda.synchronize()
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        free0, _ = torch.cuda.mem_get_info(0)
        mu, var, ll, info, _, _ = obj.predict_markov_batch(delays, alpha, rho, tt)
        held, _, infoh, _ = obj.heldout_loglik_markov_batch(delays, alpha, rho, tt, yt, st)
        pmu, pS, _, infop = obj.posterior_offsets_markov_batch(delays, alpha, rho)
        free1, _ = torch.cuda.mem_get_info(0)
        assert obj.get_option("workspace_slots") == obj.get_option("slots_per_stream")     # (never built)
        assert obj.get_option("markov_tap_bytes") == 16 * T * nrec * 64
        ll0, _ = obj.loglik_markov_batch(delays, alpha, rho)
    documented = 16 * T * nrec * 64 + 16 * T * 64
    print("N = 16384 linear-time predictions: %.2f MiB of growth (tap scratch, mu and var: %.2f MiB)"
          % ((free0 - free1) / 2.0 ** 20, documented / 2.0 ** 20))
    assert free0 - free1 < documented + 4 * 2 ** 20
    assert (info == 0).all() and (infoh == 0).all() and (infop == 0).all() and np.array_equal(ll, ll0)
    for g in (0, 63):
        hmu, hvar, _, hinfo = markov.predict("matern52", t, y, s, delays[g], alpha[g], rho[g], tt, True)
        assert hinfo == 0
        cmax = float(np.max(alpha0) ** 2 + 100 * max(np.var(a, ddof=1) for a in y))
        assert np.max(np.abs(mu[g] - hmu)) <= 2e-10 * max(1.0, float(np.max(np.abs(hmu))))
        assert np.max(np.abs(var[g] - hvar)) <= 2e-10 * cmax
    hheld = markov.heldout("matern52", t, y, s, delays[63], alpha[63], rho[63], tt, yt, st, True)[0]
    assert abs(held[63] - hheld) <= 2e-10 * max(1.0, abs(hheld))
    hp = markov.posterior_offsets("matern52", t, y, s, delays[63], alpha[63], rho[63])
    PC.assert_postb(pmu[63], pS[63], hp[0], hp[1])
