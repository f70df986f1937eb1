"""gpcc_sample_markov_batch on the device: every draw against the numpy mirror (gpcc_amd.markov.sample, the same seed)
and against the dense-algebra Matheron draw on the oracle's matrices (tests/_markov_sample_cases.py), both at the dense draws' own bar
max(1e-10, 64 eps cond_1(K_aug)) max(1, max |f*|) (tests/test_markov_sample_cpu.py shows that it rejects the injected slips); loglik,
info and the mixture's rows bitwise against the entries they are defined by; bitwise invariance over batch sizes, row order, chunking,
fp32 and multi-device handles and prefixes in S; refusals and failed rows; the statistics of the draws at test_gpu_sample.py's
acceptance limit of 5 standard errors; memory at N = 16384."""
import numpy as np
import pytest

import _markov_cases as MC
import _markov_predict_cases as PC
import _markov_sample_cases as SC
import _sample_witness as SW
import gpcc_amd
from gpcc_amd import fit, markov, rng

pytestmark = pytest.mark.gpu

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
UNSUPPORTED, ARGUMENT, NOT_DRAWN = -3, -1, -14
CASES = SC.cpu_cases()


def _check_case(oracle, case, S, seed, wm, ww, weights=False):
    """S draws of one row on the device against the mirror and the dense-algebra witness."""
    cid, k, data, delays, alpha, rho, mb, tests = case
    tt, st = tests[0], tests[2]
    with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
        kw = dict(weights=[1.0]) if weights else {}
        dr, rows, ll, info = obj.sample_markov_batch(delays[None, :], alpha[None, :], [rho], tt, S, seed, sigmatest=st, **kw)
        _, _, pl, pi, _, _ = obj.predict_markov_batch(delays[None, :], alpha[None, :], [rho], tt)
    T = sum(len(a) for a in tt)
    assert dr.shape == (S, T) and info[0] == 0 and np.array_equal(ll, pl) and np.array_equal(info, pi), cid
    _, _, _, cond, _ = SC.witness(oracle, case)
    word = rng.MIXROW if weights else 0
    for s in range(S):
        mir, mll, minfo = markov.sample(k, *data, delays, alpha, rho, tt, st, mb, seed=seed, s=s, m=word)
        assert minfo == 0, cid
        wm.add(float(np.max(np.abs(dr[s] - mir))), SW.bar(cond, mir), cid)
        rt, gt, noise = markov.prior_draw(k, *data, delays, alpha, rho, tt, st, mb, seed=seed, s=s, m=word)
        ref, b = SC.matheron(oracle, case, rt, gt, noise)
        ww.add(float(np.max(np.abs(dr[s] - ref))), b, cid)


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_parity_cpu_cases(oracle, kernel, L):
    wm, ww = MC.Worst("device draw vs mirror %s L=%d" % (kernel, L)), MC.Worst("device draw vs dense Matheron %s L=%d" % (kernel, L))
    n = 0
    for idx, case in enumerate(CASES):
        if case[1] != kernel or len(case[2][0]) != L:
            continue
        _check_case(oracle, case, 3, 500 + idx, wm, ww, weights=bool(idx % 2))
        n += 1
    assert n == 8
    wm.report()
    ww.report()


def _tiny(kernel, Nl, Nt, mb, seed):
    """A case of SC.witness's form with Nl training and Nt test points per band."""
    rg = np.random.default_rng(seed)
    L = len(Nl)
    delays = np.concatenate([[0.0], MC.snap(rg.uniform(-1.0, 2.0, L - 1))])
    t = [MC.snap(rg.uniform(0.0, 6.0, n)) for n in Nl]
    y = [np.sin(t[l] - delays[l]) + 0.3 * l + 0.1 * rg.standard_normal(Nl[l]) for l in range(L)]
    s = [0.15 + 0.05 * rg.random(n) for n in Nl]
    tt = [MC.snap(rg.uniform(-1.0, 7.0, n)) for n in Nt]
    st = [0.1 + 0.1 * rg.random(n) for n in Nt]
    return ("tiny-%s-%s-%s-b%d" % (kernel, Nl, Nt, mb), kernel, (t, y, s), delays, rg.uniform(0.5, 1.5, L), 1.5, mb, (tt, None, st))


@pytest.mark.parametrize("kernel,Nl,Nt,mb", [("matern32", [1, 1], [1, 0], False),          # N = 2, one point per band; T = 1
                                             ("OU", [7, 5], [0, 4], True),                  # one band without test points
                                             ("matern52", [5, 4, 6, 3], [2, 1, 2, 1], True),       # L = 4 with offsets
                                             ("matern52", [3, 4, 2, 3, 4, 2, 3, 2], [1, 0, 1, 1, 0, 1, 1, 1], False)])   # L = 8 without
def test_parity_edge_shapes(oracle, kernel, Nl, Nt, mb):
    case = _tiny(kernel, Nl, Nt, mb, seed=sum(Nl) + len(Nl))
    wm, ww = MC.Worst("device draw vs mirror %s" % case[0]), MC.Worst("device draw vs dense Matheron %s" % case[0])
    _check_case(oracle, case, 3, 41, wm, ww)
    wm.report()
    ww.report()


def _batch(L, M, seed):
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 45.0, (M, L - 1)))], 1)
    return delays, rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))


def _eq(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_bitwise_properties():
    Nl, mb, kernel = [60, 50], True, "matern32"
    t, y, s, d0 = MC.lightcurves(Nl, seed=7, kind="ties")
    tt, _, st = PC.test_points(t, d0, 8, -1)
    delays, alpha, rho = _batch(2, 65, seed=3)
    S, seed = 4, 99
    w = np.random.default_rng(5).random(65) ** 2
    w[[2, 40]] = 0.0
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        full = obj.sample_markov_batch(delays, alpha, rho, tt, S, seed, sigmatest=st)
        assert _eq(full, obj.sample_markov_batch(delays, alpha, rho, tt, S, seed, sigmatest=st))
        pred = obj.predict_markov_batch(delays, alpha, rho, tt)
        assert (full[3] == 0).all() and np.isfinite(full[0]).all()
        assert np.array_equal(full[2], pred[2]) and np.array_equal(full[3], pred[3])            # loglik and info: the predictions'
        assert np.array_equal(full[1], np.repeat(np.arange(65), S))
        for M in (1, 63, 64):                                                                   # M = 1 / 63 / 64 / 65
            part = obj.sample_markov_batch(delays[:M], alpha[:M], rho[:M], tt, S, seed, sigmatest=st)
            assert np.array_equal(part[0], full[0][:M * S]) and np.array_equal(part[2], full[2][:M]), M
        short = obj.sample_markov_batch(delays, alpha, rho, tt, 3, seed, sigmatest=st)           # prefixes in S
        assert np.array_equal(full[0].reshape(65, S, -1)[:, :3].reshape(65 * 3, -1), short[0])
        mix = obj.sample_markov_batch(delays, alpha, rho, tt, 300, seed, weights=w, sigmatest=st)
        dense = obj.sample_batch(delays, alpha, rho, tt, 300, seed, weights=w, sigmatest=st)
        assert np.array_equal(mix[1], dense[1]) and np.array_equal(mix[1], rng.pick_rows(seed, 300, w))     # the dense entry's rows
        mix_short = obj.sample_markov_batch(delays, alpha, rho, tt, 200, seed, weights=w, sigmatest=st)
        assert np.array_equal(mix[0][:200], mix_short[0]) and np.array_equal(mix[1][:200], mix_short[1])
        drawn = np.zeros(65, bool)
        drawn[mix[1]] = True
        assert not drawn[[2, 40]].any() and np.all(mix[3][~drawn] == NOT_DRAWN) and np.isnan(mix[2][~drawn]).all()
        assert np.array_equal(mix[2][drawn], pred[2][drawn]) and np.array_equal(mix[3][drawn], pred[3][drawn])
        perm = np.random.default_rng(6).permutation(65)                  # permuted rows (mixture mode: no row word in the counters)
        w1 = np.zeros(65)
        w1[17] = 1.0
        one = obj.sample_markov_batch(delays, alpha, rho, tt, 70, seed, weights=w1, sigmatest=st)
        pm = obj.sample_markov_batch(delays[perm], alpha[perm], rho[perm], tt, 70, seed, weights=w1[perm], sigmatest=st)
        assert (one[1] == 17).all() and (perm[pm[1]] == 17).all() and np.array_equal(one[0], pm[0])
        for rows_opt, draws_opt in ((7, 0), (64, 0), (0, 64), (0, 100), (7, 100)):
            obj.set_option("markov_chunk_rows", rows_opt)
            obj.set_option("markov_sample_chunk_draws", draws_opt)
            assert _eq(full, obj.sample_markov_batch(delays, alpha, rho, tt, S, seed, sigmatest=st)), (rows_opt, draws_opt)
            assert _eq(mix, obj.sample_markov_batch(delays, alpha, rho, tt, 300, seed, weights=w, sigmatest=st)), (rows_opt, draws_opt)
        obj.set_option("markov_chunk_rows", 0)
        obj.set_option("markov_sample_chunk_draws", 0)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, precision="fp32") as o32:
        assert _eq(full, o32.sample_markov_batch(delays, alpha, rho, tt, S, seed, sigmatest=st))
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, devices=[0, 0]) as om:
        assert _eq(full, om.sample_markov_batch(delays, alpha, rho, tt, S, seed, sigmatest=st))


def test_refusals_and_failed_rows():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    tt, _, st = PC.test_points(t, d0, 12, -1)
    delays, alpha, rho = _batch(2, 5, seed=2)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.sample_markov_batch(delays, alpha, rho, tt, 2, 1)
        assert ei.value.code == UNSUPPORTED
    t5, y5, s5, d5 = MC.lightcurves([30, 25, 20, 20, 15], seed=12, kind="plain")
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=True) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.sample_markov_batch(d5[None, :], np.ones((1, 5)), [1.0], [np.array([1.0])] * 5, 2, 1)
        assert ei.value.code == UNSUPPORTED
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.sample_markov_batch(delays, alpha, rho, tt, 0, 1)
        assert ei.value.code == ARGUMENT
        for bad in ([-1.0] + [1.0] * 4, [np.nan] + [1.0] * 4, [0.0] * 5):
            with pytest.raises(gpcc_amd.GpccError) as ei:
                obj.sample_markov_batch(delays, alpha, rho, tt, 2, 1, weights=np.array(bad))
            assert ei.value.code == ARGUMENT
        good = obj.sample_markov_batch(delays, alpha, rho, tt, 3, 8, sigmatest=st)
        a2 = alpha.copy()
        a2[2, 1] = -0.5
        dr, rows, ll, info = obj.sample_markov_batch(delays, a2, rho, tt, 3, 8, sigmatest=st)
        assert list(info) == [0, 0, -1, 0, 0] and np.isnan(ll[2]) and np.isnan(dr[6:9]).all()
        keep = np.r_[0:6, 9:15]
        assert np.array_equal(dr[keep], good[0][keep]) and np.array_equal(ll[[0, 1, 3, 4]], good[2][[0, 1, 3, 4]])   # neighbours untouched
        w = np.array([1.0, 0.0, 0.0, 2.0, 0.0])
        dr, rows, ll, info = obj.sample_markov_batch(delays, a2, rho, tt, 50, 8, weights=w)
        assert set(rows) == {0, 3} and list(info) == [0, NOT_DRAWN, NOT_DRAWN, 0, NOT_DRAWN] and np.isfinite(dr).all()


def test_statistics_one_row(oracle):
    """20 000 draws of one row: the mean against predict_markov_batch's and the covariance against the dense Sigma_pred + JITTER (the
    oracle's matrices), within test_gpu_sample.py's 5 standard errors."""
    t, y, s, d0 = MC.lightcurves([60, 50], seed=5, kind="plain")
    delays, alpha, rho = np.array([0.0, 2.0]), np.array([1.2, 0.9]), 3.0
    tt = [np.linspace(0, 20, 5), np.linspace(3, 18, 3)]
    S = 20000
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        dr, _, _, info = obj.sample_markov_batch(delays[None, :], alpha[None, :], [rho], tt, S, seed=2024)
        mu, var, _, _, _, _ = obj.predict_markov_batch(delays[None, :], alpha[None, :], [rho], tt)
    assert info[0] == 0
    _, Sig, _, _, _ = SC.witness(oracle, ("stat-one", "matern32", (t, y, s), delays, alpha, rho, True, (tt, None, None)))
    m, C = dr.mean(0), np.cov(dr.T, bias=False)
    d2 = np.diag(Sig)
    se_m, se_c = np.sqrt(d2 / S), np.sqrt((np.outer(d2, d2) + Sig ** 2) / S)
    print("linear-time draws, one row: mean %.2f SE, covariance %.2f SE (limit 5)"
          % (np.max(np.abs(m - mu[0]) / se_m), np.max(np.abs(C - Sig) / se_c)))
    assert np.all(np.abs(m - mu[0]) <= 5 * se_m)
    assert np.all(np.abs(C - Sig) <= 5 * se_c)


def test_mixture_statistics():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=8, kind="plain")
    G = 12
    grid = np.linspace(0.0, 6.0, G)
    delays = np.stack([np.zeros(G), grid], 1)
    alpha, rho = np.tile([1.1, 0.9], (G, 1)), np.full(G, 2.5)
    w = np.exp(-0.5 * (grid - 3.0) ** 2)
    w[[0, 5]] = 0.0
    tt = [np.linspace(0, 25, 10), np.linspace(2, 22, 10)]
    S = 20000
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        dr, rows, ll, info = obj.sample_markov_batch(delays, alpha, rho, tt, S, seed=11, weights=w)
        _, _, _, _, mix_mu, mix_var = obj.predict_markov_batch(delays, alpha, rho, tt, weights=w)
    assert np.array_equal(rows, rng.pick_rows(11, S, w)) and np.all(info[[0, 5]] == NOT_DRAWN)
    m, v = dr.mean(0), dr.var(0, ddof=1)
    m4 = np.mean((dr - m) ** 4, 0)
    se_m, se_v = np.sqrt(mix_var / S), np.sqrt(np.maximum(m4 - v ** 2, 0) / S)
    print("linear-time draws, mixture: mean %.2f SE, variance %.2f SE (limit 5)"
          % (np.max(np.abs(m - mix_mu) / se_m), np.max(np.abs(v - mix_var) / se_v)))
    assert np.all(np.abs(m - mix_mu) <= 5 * se_m)
    assert np.all(np.abs(v - mix_var) <= 5 * se_v)


def test_predictors_sample_with_the_markov_solver():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=13, kind="plain")
    cand = np.stack([np.zeros(3), d0[1] + np.array([-0.5, 0.0, 0.5])], 1)
    alpha, rho, w = np.tile([1.0, 0.8], (3, 1)), np.array([2.0, 3.0, 4.0]), np.array([0.2, 0.5, 0.3])
    grid = np.linspace(-1.0, 31.0, 9)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        pred = fit.Predictor(obj, cand[1], alpha[1], rho[1], solver="markov")
        bands = pred.sample(grid, 4, 11, solver="markov")
        raw = obj.sample_markov_batch(cand[1][None, :], alpha[1][None, :], [rho[1]], [grid, grid], 4, 11)[0]
        assert [b.shape for b in bands] == [(4, 9), (4, 9)] and np.array_equal(np.concatenate(bands, 1), raw)
        assert np.array_equal(np.concatenate(pred.sample(grid, 4, 11), 1), obj.sample_batch(cand[1][None, :], alpha[1][None, :], [rho[1]],
                                                                                              [grid, grid], 4, 11)[0])      # None: dense
        avg = fit.DelayAveragedPredictor(obj, cand, alpha, rho, w, solver="markov")
        mb, rows = avg.sample(grid, 50, 12, solver="markov")
        db, drows = avg.sample(grid, 50, 12)
        assert np.array_equal(rows, drows) and all(np.isfinite(b).all() and b.shape == (50, 9) for b in mb)
        assert not np.array_equal(mb[0], db[0])


def test_memory_at_16384():
    """N = 16384, Matern-5/2, T = 2 x 64, S = 64 draws of one row: the handle grows by the documented buffers and none of the N^2
    workspace -- the tap scratch 16 T (n + n (n + 1) / 2) and the weights 16 T n bytes per row (n = 5), mu and var 16 T per row, the
    scratch 8 (N + T) x 256 lanes, the draws 8 S T, the lists 4 (N + 3 S + 1), the light curves 24 N and the staging."""
    import torch
    rg = np.random.default_rng(16384)
    Nl = [8192, 8192]
    t = [np.sort(MC.snap(rg.uniform(0.0, 2000.0, n))) for n in Nl]
    y = [np.sin(0.05 * a) + 0.1 * rg.standard_normal(len(a)) for a in t]
    s = [0.1 + 0.05 * rg.random(len(a)) for a in t]
    tt = [MC.snap(rg.uniform(0.0, 2000.0, 64)) for _ in range(2)]
    N, T, S, n = 16384, 128, 64, 5
    torch.cuda.synchronize()
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        free0, _ = torch.cuda.mem_get_info(0)
        dr, _, ll, info = obj.sample_markov_batch([[0.0, 3.0]], [[1.0, 0.9]], [20.0], tt, S, 7)
        free1, _ = torch.cuda.mem_get_info(0)
        assert obj.get_option("workspace_slots") == obj.get_option("slots_per_stream")     # (never built)
        ints = 4 * (N + 3 * S + 1)
        assert obj.get_option("markov_sample_bytes") == 16 * T * n + 8 * (N + T) * 256 + ints
        pll = obj.predict_markov_batch([[0.0, 3.0]], [[1.0, 0.9]], [20.0], tt)[2]
    documented = 16 * T * (n + n * (n + 1) // 2) + 16 * T * n + 16 * T + 8 * (N + T) * 256 + 8 * S * T + ints + 24 * N
    print("N = 16384 linear-time draws: %.2f MiB of growth (documented buffers %.2f MiB)" % ((free0 - free1) / 2.0 ** 20,
                                                                                           documented / 2.0 ** 20))
    assert info[0] == 0 and np.isfinite(dr).all() and dr.shape == (S, T) and ll[0] == pll[0]
    assert free0 - free1 < documented + 4 * 2 ** 20       # (test_gpu_markov_predict.py's allowance for the allocator and the staging)
