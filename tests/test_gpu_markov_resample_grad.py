"""gpcc_loglik_grad_markov_resampled_batch on the device: the "flux + subset" cell of every case of
tests/_markov_resample_grad_cases.py at N = 110, and one L = 3 case per kernel at N = 150 and N = 767, against the extended-precision
dense gradient of the reduced fresh data set under that gradient's own bar (tests/_grad_highprec.bar; the worst error / bar of each
group is printed); value and info bitwise the value entry's; the handle's own data bitwise gpcc_loglik_grad_markov_batch; the bitwise
invariances of a row; an OU tie among kept points across a dropped one; the unstaged path; codes, NaN fluxes, refusals;
fit.realisation_refits with the BFGS optimiser and fit.realisation_peaks end to end."""
import ctypes

import numpy as np
import pytest

import _grad_highprec as H
import _markov_cases as MC
import _markov_resample_cases as SC
import _markov_resample_grad_cases as GC
import gpcc_amd
from gpcc_amd import _capi, fit, markov, synthetic

pytestmark = pytest.mark.gpu

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
ARGUMENT, UNSUPPORTED = -1, -3


@pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_parity_110(kernel):
    picked = [c for c in GC.cases((110,)) if c[1] == kernel]
    assert len(picked) == 3 * 2 * 3
    worst = GC.Worst("device gradient %s N = 110, flux + subset" % kernel)
    for case in picked:
        cid, k, data, delays, alpha, rho, mb, N = case
        Y, counts = SC.realisations(case)
        d, a, rh, real = SC.rows(case)
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll, grad, info = obj.loglik_grad_markov_resampled(Y, d, a, rh, real, counts=counts)
        assert grad.shape == (SC.R, 2 * len(delays) + 1) and (info == 0).all(), cid
        ref = GC.reference(case, GC.BOTH)
        err = np.abs(grad[GC.BOTH] - ref.grad) / H.bar(ref)
        assert (err <= 1.0).all(), (cid, err)                           # each of the 2L + 1 entries
        worst.add(float(err.max()), cid)
    worst.report()


@pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)
@pytest.mark.parametrize("N", [150, 767])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_parity_larger(kernel, N):
    """One L = 3 case per kernel.  At N = 767 M = 70 rows cycle through the 4 realisations in a scrambled order: more than one
    workgroup, lanes beyond M."""
    case = next(c for c in GC.cases((N,)) if c[1] == kernel and len(c[3]) == 3 and c[6] and c[5] == 3.0)
    cid, k, data, delays, alpha, rho, mb, _ = case
    Y, counts = SC.realisations(case)
    M = 70 if N == 767 else SC.R
    real = (np.random.default_rng(N).permutation(M) * 3 + 1) % SC.R
    assert set(real) == set(range(SC.R))
    with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
        ll, grad, info = obj.loglik_grad_markov_resampled(Y, np.tile(delays, (M, 1)), np.tile(alpha, (M, 1)), np.full(M, rho), real,
                                                          counts=counts)
    assert (info == 0).all()
    worst = GC.Worst("device gradient %s N = %d, L = 3" % (kernel, N))
    for m in range(M):
        worst.add(H.ratio(grad[m], GC.reference(case, int(real[m]))), (cid, m, int(real[m])))
    worst.report()


def _batch(L, M, seed):
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), rg.uniform(-3.0, 45.0, (M, L - 1))], 1)
    return delays, rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))


def _raw(obj, M, delays, alpha, rho, real, R, Y, count=None, mean=None, sigma_b=None, with_grad=True, L=None):
    """The C entry itself: NULL arguments, and the arguments the Python wrapper refuses first."""
    dp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
    i = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
    W = 2 * (obj.L if L is None else L) + 1
    ll, info, grad = np.full(max(M, 1), -7.0), np.full(max(M, 1), 99, np.int32), np.full((max(M, 1), W), -5.0)
    keep = [f(delays), f(alpha), f(rho), i(real), f(Y), i(count), f(mean), f(sigma_b)]
    rc = _capi.load().gpcc_loglik_grad_markov_resampled_batch(obj._h, M, dp(keep[0]), dp(keep[1]), dp(keep[2]), ip(keep[3]), R, dp(keep[4]),
                                                              ip(keep[5]), dp(keep[6]), dp(keep[7]), dp(ll), dp(grad) if with_grad else None,
                                                              ip(info))
    return rc, ll, grad, info


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_value_and_info_are_the_value_entrys_bitwise(kernel):
    """Mixed rows, failing ones among them: loglik and info bitwise loglik_markov_resampled's, NaN gradients exactly on the failing rows,
    the neighbours' gradients bitwise those of the call without failing rows."""
    t, y, s, _ = MC.lightcurves([60, 50, 40], seed=11, kind="ties")
    R, M = 4, 140
    Y, counts = synthetic.resample(y, s, R, seed=2)
    delays, alpha, rho = _batch(3, M, seed=5)
    real = np.arange(M) % R
    with gpcc_amd.Objective(t, y, s, KERN[kernel]) as obj:
        count = obj.get_option("markov_count")
        gl, good, ginfo = obj.loglik_grad_markov_resampled(Y, delays, alpha, rho, real, counts=counts)
        assert obj.get_option("markov_count") == count + M
        vl, vinfo = obj.loglik_markov_resampled(Y, delays, alpha, rho, real, counts=counts)
        assert (ginfo == 0).all() and np.isfinite(good).all() and np.array_equal(gl, vl) and np.array_equal(ginfo, vinfo)
        a2, r2 = alpha.copy(), rho.copy()
        a2[1, 0], a2[70, 2], r2[3], r2[131] = 0.0, -1.0, 0.0, -2.0
        ll, grad, info = obj.loglik_grad_markov_resampled(Y, delays, a2, r2, real, counts=counts)
        vl, vinfo = obj.loglik_markov_resampled(Y, delays, a2, r2, real, counts=counts)
    bad = np.array([1, 70, 3, 131])
    assert list(info[bad]) == [-1, -1, -2, -2] and np.array_equal(ll, vl, equal_nan=True) and np.array_equal(info, vinfo)
    rest = np.setdiff1d(np.arange(M), bad)
    assert np.isnan(grad[bad]).all() and np.isnan(ll[bad]).all()
    assert (info[rest] == 0).all() and np.array_equal(grad[rest], good[rest]) and np.array_equal(ll[rest], gl[rest])


@pytest.mark.parametrize("mb", [True, False])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_the_handles_own_data_is_loglik_grad_markov_batch_bitwise(kernel, mb):
    """real pointing to the handle's own y, count, mean and sigma_b NULL: gpcc_loglik_grad_markov_batch's gradient, value and info, bit
    for bit (one walk, the step functions shared unedited) -- on light curves with ties, also for failing rows, and with the own y at
    another position among other fluxes."""
    Nl = [40, 41, 30]
    t, y, s, _ = MC.lightcurves(Nl, seed=9, kind="ties")
    M = 130
    delays, alpha, rho = _batch(3, M, seed=8)
    alpha[5, 1] = -1.0
    rho[7] = 0.0
    Y = np.concatenate(synthetic.flux_randomise(y, s, 3, seed=1), axis=1)
    Y[1] = np.concatenate(y)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        pl, plain, pinfo = obj.loglik_grad_markov_batch(delays, alpha, rho)
        rc, ll, grad, info = _raw(obj, M, delays, alpha, rho, np.ones(M), 3, Y)
        assert rc == 0
        assert np.array_equal(grad, plain, equal_nan=True) and np.array_equal(ll, pl, equal_nan=True) and np.array_equal(info, pinfo)
        assert list(pinfo[[5, 7]]) == [-1, -2] and np.isfinite(plain[pinfo == 0]).all()
        rc, one, g1, oinfo = _raw(obj, M, delays, alpha, rho, np.zeros(M), 1, np.concatenate(y), count=np.ones(sum(Nl)))
        assert rc == 0 and np.array_equal(g1, plain, equal_nan=True) and np.array_equal(one, pl, equal_nan=True) and np.array_equal(oinfo, pinfo)


@pytest.mark.parametrize("kernel,Nl,mb", [("matern52", [300, 200, 267], True), ("OU", [60, 50], False), ("matern32", [40, 41], True)])
def test_bitwise_invariance_of_a_rows_gradient(kernel, Nl, mb):
    """A row's gradient does not depend on M, on the row order, on R, on the position of its realisation in Y or on the handle's
    flavour (the shapes of test_gpu_markov_resample.test_bitwise_invariance_of_a_row)."""
    t, y, s, _ = MC.lightcurves(Nl, seed=7, kind="ties")
    L, N, M, R = len(Nl), sum(Nl), 257, 7
    delays, alpha, rho = _batch(L, M, seed=L)
    Y, counts = synthetic.resample(y, s, R, seed=5)
    Y, counts = np.concatenate(Y, axis=1), np.concatenate(counts, axis=1)
    real = np.random.default_rng(4).integers(0, R, M)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        fl, full, info = obj.loglik_grad_markov_resampled(Y, delays, alpha, rho, real, counts=counts)
        assert full.shape == (M, 2 * L + 1) and (info == 0).all() and np.isfinite(full).all()
        for Ms in (1, 63, 64, 65):
            ll, g, inf = obj.loglik_grad_markov_resampled(Y, delays[:Ms], alpha[:Ms], rho[:Ms], real[:Ms], counts=counts)
            assert np.array_equal(g, full[:Ms]) and np.array_equal(ll, fl[:Ms]) and (inf == 0).all(), Ms
        rows = np.random.default_rng(2).permutation(M)
        ll, g, _ = obj.loglik_grad_markov_resampled(Y, delays[rows], alpha[rows], rho[rows], real[rows], counts=counts)
        assert np.array_equal(g, full[rows]) and np.array_equal(ll, fl[rows])
        order = np.argsort(real, kind="stable")                                 # realisation-major, as the fit orders its rows
        ll, g, _ = obj.loglik_grad_markov_resampled(Y, delays[order], alpha[order], rho[order], real[order], counts=counts)
        assert np.array_equal(g, full[order])
        perm = np.random.default_rng(1).permutation(R)                           # the realisations at other positions of Y
        inv = np.argsort(perm)
        ll, g, _ = obj.loglik_grad_markov_resampled(Y[perm], delays, alpha, rho, inv[real], counts=counts[perm])
        assert np.array_equal(g, full)
        sel = real < 3                                                           # a smaller R
        ll, g, _ = obj.loglik_grad_markov_resampled(Y[:3], delays[sel], alpha[sel], rho[sel], real[sel], counts=counts[:3])
        assert np.array_equal(g, full[sel])
        before = obj.get_option("markov_resample_bytes_max")
        obj.set_option("markov_resample_bytes_max", 16 * N * 2 + 5)              # R split across calls of 2 realisations
        ll, g, inf = obj.loglik_grad_markov_resampled(Y, delays, alpha, rho, real, counts=counts)
        assert np.array_equal(g, full) and np.array_equal(ll, fl) and (inf == 0).all()
        obj.set_option("markov_resample_bytes_max", before)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, precision="fp32") as o32:
        ll, g, inf = o32.loglik_grad_markov_resampled(Y, delays[:65], alpha[:65], rho[:65], real[:65], counts=counts)
        assert np.array_equal(g, full[:65]) and np.array_equal(ll, fl[:65]) and (inf == 0).all()
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, devices=[0, 0]) as om:
        ll, g, inf = om.loglik_grad_markov_resampled(Y, delays[:65], alpha[:65], rho[:65], real[:65], counts=counts)
        assert np.array_equal(g, full[:65]) and np.array_equal(ll, fl[:65]) and (inf == 0).all()


def test_ou_tie_among_kept_points_across_a_dropped_point():
    """Two kept points of different bands tie in shifted time, a dropped point between them in the handle's merged order: the tau
    entries are the mean of the two one-sided mirror tangents, and the whole gradient is the reduced fresh handle's
    loglik_grad_markov_batch within WITNESS_BAR max|g|."""
    t, y, s, d0, Y, counts, _ = GC.tie_case()
    alpha, rho, L = np.array([1.0, 0.8]), 2.0, 2
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU, marginalise_b=False) as obj:
        ll, grad, info = obj.loglik_grad_markov_resampled(Y, [d0], [alpha], [rho], [0], counts=counts)
    red = SC.reduced((t, y, s), Y, counts, 0)
    with gpcc_amd.Objective(*red, gpcc_amd.OU, marginalise_b=False) as fresh:
        fl, fgrad, finfo = fresh.loglik_grad_markov_batch([d0], [alpha], [rho])
    assert info[0] == 0 and finfo[0] == 0
    scale = float(np.max(np.abs(fgrad[0])))
    assert np.max(np.abs(grad[0] - fgrad[0])) <= GC.WITNESS_BAR * scale
    # the two one-sided tangents of the mirror: band l first / last among the tied kept points
    mean, vb = markov.resample_constants(t, Y, counts, False)
    name, _, dl, al, rh, _, v, _, p, n, points = markov._resampled_setup("OU", t, y, s, Y, counts, [0], d0, alpha, rho, False, mean, vb)
    train = [(tt - d0[l], l, i, res, s2) for (l, i, tt, res, s2) in points(0)]
    sides = np.array([[markov._grad_pass("OU", train, alpha, rho, p, n, v[0], "tau", l, rank=rk) for rk in (-1, L)] for l in range(L)])
    assert (sides[:, 0] != sides[:, 1]).all()                                     # a kink: the one-sided derivatives differ
    assert np.max(np.abs(grad[0, L + 1:] - sides.mean(axis=1))) <= GC.WITNESS_BAR * scale
    assert np.min(np.abs(grad[0, L + 1:] - sides.T)) > 100 * GC.WITNESS_BAR * scale   # and it is neither of the two


def test_unstaged_path():
    """N = 7000 does not fit the LDS: the times come through the caches too.  4 rows x 3 realisations (one with RSS) against 3 fresh
    handles' loglik_grad_markov_batch on the reduced data, within WITNESS_BAR max|g| (device against device: the dense reference is
    too slow here)."""
    Nl = [3500, 3500]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=4)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    G, R, N = 4, 3, sum(Nl)
    delays = np.stack([np.zeros(G), np.linspace(0.0, 12.6, G)], 1)
    alpha, rho = np.tile(alpha0, (G, 1)), np.full(G, rho0)
    Y, counts = synthetic.resample(y, s, R, seed=6, subset=False)
    _, rss = synthetic.resample(y, s, 1, seed=7, flux=False)
    for l in range(2):
        counts[l][2] = rss[l][0]
    g, r = np.tile(np.arange(G), R), np.repeat(np.arange(R), G)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        ll, grad, info = obj.loglik_grad_markov_resampled(Y, delays[g], alpha[g], rho[g], r, counts=counts)
        vl, vinfo = obj.loglik_markov_resampled(Y, delays[g], alpha[g], rho[g], r, counts=counts)
    assert (info == 0).all() and np.isfinite(grad).all() and np.array_equal(ll, vl) and np.array_equal(info, vinfo)
    worst = 0.0
    for k in range(R):
        red = SC.reduced((t, y, s), Y, counts, k)
        with gpcc_amd.Objective(*red, gpcc_amd.matern32) as fresh:
            one, fgrad, finfo = fresh.loglik_grad_markov_batch(delays, alpha, rho)
        assert (finfo == 0).all()
        rel = np.max(np.abs(grad[r == k] - fgrad), axis=1) / np.max(np.abs(fgrad), axis=1)
        worst = max(worst, float(rel.max()) / GC.WITNESS_BAR)
        assert (rel <= GC.WITNESS_BAR).all(), (k, rel)
    assert sum(len(a) for a in SC.reduced((t, y, s), Y, counts, 2)[0]) < N
    print("unstaged N = 7000 gradient: worst disagreement with the fresh handles / (WITNESS_BAR max|g|) %.3g" % worst)


def test_codes_nan_fluxes_and_empty_realisations():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    R, M = 4, 12
    Y, counts = synthetic.resample(y, s, R, seed=2)
    Y, counts = np.concatenate(Y, axis=1), np.concatenate(counts, axis=1)
    delays, alpha, rho = _batch(2, M, seed=5)
    real = np.arange(M) % R
    zero = dict(counts=counts, center=np.zeros((R, 2)), sigma_b="handle")
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        bl, base, binfo = obj.loglik_grad_markov_resampled(Y, delays, alpha, rho, real, **zero)
        assert (binfo == 0).all() and np.isfinite(base).all()
        # a flux that is not finite at a kept point poisons exactly the rows of that realisation; at a dropped point none
        kept, dropped = int(np.flatnonzero(counts[1] > 0)[3]), int(np.flatnonzero(counts[1] == 0)[2])
        for bad in (np.nan, np.inf):
            Yb = Y.copy()
            Yb[1, kept] = bad
            ll, grad, info = obj.loglik_grad_markov_resampled(Yb, delays, alpha, rho, real, **zero)
            assert (info == 0).all() and np.isnan(ll[real == 1]).all() and np.isnan(grad[real == 1]).all()
            assert np.array_equal(grad[real != 1], base[real != 1]) and np.array_equal(ll[real != 1], bl[real != 1])
            Yb = Y.copy()
            Yb[1, dropped] = bad
            ll, grad, info = obj.loglik_grad_markov_resampled(Yb, delays, alpha, rho, real, **zero)
            assert (info == 0).all() and np.array_equal(grad, base) and np.array_equal(ll, bl)
        # a realisation that keeps nothing: 0.0, a zero gradient, info 0; its neighbours untouched
        c0 = counts.copy()
        c0[2] = 0
        hl, hbase, _ = obj.loglik_grad_markov_resampled(Y, delays, alpha, rho, real, counts=counts, center="handle", sigma_b="handle")
        ll, grad, info = obj.loglik_grad_markov_resampled(Y, delays, alpha, rho, real, counts=c0, center="handle", sigma_b="handle")
        assert (info == 0).all() and (ll[real == 2] == 0.0).all() and (grad[real == 2] == 0.0).all()
        assert np.array_equal(grad[real != 2], hbase[real != 2]) and np.array_equal(ll[real != 2], hl[real != 2])


def test_refusals():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    N, R = 110, 3
    Y, counts = synthetic.resample(y, s, R, seed=2)
    Yf, cf = np.concatenate(Y, axis=1), np.concatenate(counts, axis=1)
    delays, alpha, rho = _batch(2, 8, seed=5)
    real = np.arange(8) % R
    untouched = lambda ll, grad, info: (ll == -7.0).all() and (grad == -5.0).all() and (info == 99).all()
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loglik_grad_markov_resampled(Y, delays, alpha, rho, real, counts=counts)
        assert ei.value.code == UNSUPPORTED and "rbf" in ei.value.message and "gpcc_loglik_grad_markov_resampled_batch" in ei.value.message
        assert obj.loglik_batch([d0], [[1.0, 1.0]], [2.0])[1][0] == 0            # the handle still serves its other entries
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        # everything below is refused on the host, before any device work: the handle has not even sorted its light curves
        for bad in ([0, 1, 2, 3, 0, 1, 2, 0], [0, -1, 2, 0, 0, 1, 2, 0]):
            rc, ll, grad, info = _raw(obj, 8, delays, alpha, rho, bad, R, Yf, count=cf)
            assert rc == ARGUMENT and untouched(ll, grad, info)
        cb = cf.copy()
        cb[2, 17] = -1
        for kw in (dict(R=R, Y=Yf, count=cb), dict(R=0, Y=Yf), dict(R=R, Y=None), dict(R=R, Y=Yf, real=None),
                   dict(R=R, Y=Yf, with_grad=False)):
            rc, ll, grad, info = _raw(obj, 8, delays, alpha, rho, kw.pop("real", real), kw.pop("R"), kw.pop("Y"), **kw)
            assert rc == ARGUMENT and untouched(ll, grad, info), kw
        obj.set_option("markov_resample_bytes_max", 16 * N * R - 1)
        rc, ll, grad, info = _raw(obj, 8, delays, alpha, rho, real, R, Yf)
        assert rc == UNSUPPORTED and "markov_resample_bytes_max" in _capi.last_error(obj._h) and untouched(ll, grad, info)
        obj.set_option("markov_resample_bytes_max", 16 * N * R)
        assert obj.get_option("markov_resample_bytes") == 0 and obj.get_option("markov_count") == 0
        rc, ll, grad, info = _raw(obj, 0, delays, alpha, rho, real, R, Yf)
        assert rc == 0 and untouched(ll, grad, info)                             # M = 0 returns 0 and touches nothing
        rc, out, grad, info = _raw(obj, 8, delays, alpha, rho, real, R, Yf, count=cf)    # NULL mean and sigma_b: the handle's
        ll, g, linfo = obj.loglik_grad_markov_resampled(Y, delays, alpha, rho, real, counts=counts, center="handle", sigma_b="handle")
        assert rc == 0 and np.array_equal(out, ll) and np.array_equal(grad, g) and np.array_equal(info, linfo) and (linfo == 0).all()
        _, own, _ = obj.loglik_grad_markov_resampled(Y, delays, alpha, rho, real, counts=counts)
        assert not np.array_equal(own, g)
        with pytest.raises(ValueError):
            obj.loglik_grad_markov_resampled(Y, delays, alpha, rho, [0, 1, 2, 3, 0, 1, 2, 0], counts=counts)
        with pytest.raises(ValueError):
            obj.loglik_grad_markov_resampled(Y, delays, alpha, rho, real, counts=[c * -1 for c in counts])
        with pytest.raises(ValueError):
            obj.loglik_grad_markov_resampled(Yf[:, :-1], delays, alpha, rho, real)
    # five bands: with marginalised offsets unsupported, without them fine
    t5, y5, s5, d5 = MC.lightcurves([30, 25, 20, 25, 30], seed=12, kind="ties")
    a5 = np.linspace(0.6, 1.4, 5)
    Y5, c5 = synthetic.resample(y5, s5, 2, seed=1)
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=True) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loglik_grad_markov_resampled(Y5, [d5] * 2, [a5] * 2, [2.0] * 2, [0, 1], counts=c5)
        assert ei.value.code == UNSUPPORTED
        assert obj.loglik_batch([d5], [a5], [2.0])[1][0] == 0
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=False) as obj:
        ll, grad, info = obj.loglik_grad_markov_resampled(Y5, [d5] * 2, [a5] * 2, [2.0] * 2, [0, 1], counts=c5)
        assert (info == 0).all() and grad.shape == (2, 11)
        if H.EXTENDED:
            for r in range(2):
                assert H.ratio(grad[r], H.evaluate("OU", *SC.reduced((t5, y5, s5), Y5, c5, r), d5, a5, 2.0, False)) <= 1.0


@pytest.fixture(scope="module")
def readme_fits():
    """README size, R = 3, G = 5, 30 iterations from the original data's fit, per kernel: (data, grid, resampled data, the original
    fit, the refits by both optimisers) -- computed once, shared by the two end-to-end tests."""
    out = {}

    def get(kernel):
        if kernel not in out:
            t, y, s, _ = synthetic.simulate_lightcurves((55, 55))
            grid = np.array([0.0, 1.0, 2.0, 3.0, 8.0])
            cand = np.stack([np.zeros_like(grid), grid], 1)
            Y, counts = synthetic.resample(y, s, 3, seed=3)
            with gpcc_amd.Objective(t, y, s, KERN[kernel]) as obj:
                res = fit.gpcc_grid(t, y, s, kernel=KERN[kernel], candidatedelays=cand, iterations=30, seed=1, objective=obj, solver="markov")
                refit = {o: fit.realisation_refits(obj, cand, Y, counts, iterations=30, start=(res.alpha, res.rho), optimiser=o)
                         for o in ("bfgs", "neldermead")}
            out[kernel] = ((t, y, s), cand, Y, counts, res, refit)
        return out[kernel]

    return get


@pytest.mark.parametrize("kernel", ["OU", "matern32"])
def test_refit_bfgs_end_to_end(readme_fits, kernel):
    """Every returned (alpha, rho) re-evaluated on a fresh handle of that realisation's reduced data reproduces the returned loglikel
    under the bar (F N_kept 2^-53: device against device); every cell is >= its start value; for the converged cells the fresh
    handle's gradient, taken to the optimiser's coordinates, is within g_tol + bar of zero."""
    (t, y, s), cand, Y, counts, res, refit = readme_fits(kernel)
    out, R, G, g_tol = refit["bfgs"], 3, 5, 1e-6
    assert out.loglikel.shape == (R, G) and out.alpha.shape == (R, G, 2) and out.rho.shape == (R, G)
    assert np.isfinite(out.loglikel).all() and (out.loglikel >= out.start_loglikel).all()
    worst, worst_g = 0.0, 0.0
    for r in range(R):
        red = SC.reduced((t, y, s), Y, counts, r)
        n = sum(len(a) for a in red[0])
        with gpcc_amd.Objective(*red, KERN[kernel]) as fresh:
            one, grad, finfo = fresh.loglik_grad_markov_batch(cand, out.alpha[r], out.rho[r])
        assert (finfo == 0).all()
        tol = np.array([MC.bar(0.0, n, MC.factor(out.alpha[r, k], red[2])) for k in range(G)])
        rel = np.abs(out.loglikel[r] - one) / np.abs(one)
        worst = max(worst, float(np.max(rel / tol)))
        assert (rel <= tol).all(), (r, rel, tol)
        gx = np.abs(fit.unpack_grad(out.x[r], grad[:, :3], 2, 0.1, 20.0)).max(axis=1)      # (out.x: the optimiser's own coordinates)
        gbar = GC.WITNESS_BAR * np.max(np.abs(grad[:, :3]), axis=1).clip(1.0)    # the fresh handle's gradient against the entry's
        conv = out.converged[r]
        worst_g = max(worst_g, float(np.max(gx[conv], initial=0.0)))
        assert (gx[conv] <= g_tol + gbar[conv]).all(), (r, gx, conv)
    nm = refit["neldermead"]
    print("refit end to end %s: bfgs %d rounds, %d f_calls, mean loglikel %.6f, %d of %d cells converged (worst fresh gradient %.3g); "
          "neldermead %d rounds, %d f_calls, mean loglikel %.6f; worst |bfgs - fresh handle| / (F N 2^-53) %.3g"
          % (kernel, out.rounds, out.f_calls, float(out.loglikel.mean()), int(out.converged.sum()), R * G, worst_g, nm.rounds, nm.f_calls,
             float(nm.loglikel.mean()), worst))


def test_peaks_end_to_end(readme_fits):
    """realisation_peaks from the BFGS refit (matern32): each realisation's loglikel is >= its start cell's, the delays lie inside
    the grid's range, band 1's delay is unchanged, and a fresh handle at the returned (tau, alpha, rho) reproduces loglikel."""
    (t, y, s), cand, Y, counts, res, refit = readme_fits("matern32")
    R = 3
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        pk = fit.realisation_peaks(obj, cand, Y, counts, start=refit["bfgs"], iterations=30)
    cell = refit["bfgs"].delays.map_index
    assert pk.delays.shape == (R, 2) and (pk.delays[:, 0] == cand[cell, 0]).all()
    assert (pk.delays[:, 1] >= cand[:, 1].min()).all() and (pk.delays[:, 1] <= cand[:, 1].max()).all()
    assert np.isfinite(pk.loglikel).all() and (pk.loglikel >= pk.start_loglikel).all()
    for r in range(R):
        red = SC.reduced((t, y, s), Y, counts, r)
        n = sum(len(a) for a in red[0])
        with gpcc_amd.Objective(*red, gpcc_amd.matern32) as fresh:
            one, finfo = fresh.loglik_markov_batch(pk.delays[r:r + 1], pk.alpha[r:r + 1], pk.rho[r:r + 1])
        tol = MC.bar(0.0, n, MC.factor(pk.alpha[r], red[2]))
        assert finfo[0] == 0 and abs(pk.loglikel[r] - one[0]) <= tol * abs(one[0]), (r, pk.loglikel[r], one[0])
        # >= the refit's value at the start cell (the round trip through the transforms: under the bar)
        assert pk.loglikel[r] >= refit["bfgs"].loglikel[r, cell[r]] - tol * abs(one[0])
    print("peaks end to end: delays %s from cells %s, gain %s, converged %s, %d rounds, %d f_calls"
          % (pk.delays[:, 1], cand[cell, 1], pk.loglikel - pk.start_loglikel, pk.converged, pk.rounds, pk.f_calls))
