"""gpcc_loglik_markov_resampled_batch on the device: every cell of tests/_markov_resample_cases.py at N = 110, and one L = 3 case
per kernel at N = 150 and N = 767, against the extended-precision dense value of the reduced fresh data set under the family's bar
(measured on the reference side; the worst error / bar of each group is printed); the bitwise invariances of a row and its bitwise
identity with gpcc_loglik_markov_batch on the handle's own data; agreement with gpcc_loglik_markov_multi_batch; the unstaged path;
codes, NaN fluxes, refusals; memory; fit.realisation_refits end to end."""
import ctypes

import numpy as np
import pytest

import _markov_cases as MC
import _markov_resample_cases as SC
import gpcc_amd
from gpcc_amd import _capi, fit, markov, synthetic

pytestmark = pytest.mark.gpu

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
ARGUMENT, UNSUPPORTED = -1, -3


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_parity_110(oracle, kernel):
    picked = [c for c in SC.cases((110,)) if c[1] == kernel]
    assert len(picked) == 3 * 2 * 3
    worst = {k: MC.Worst("device %s N = 110, %s" % (kernel, k)) for k in SC.KINDS}
    for case in picked:
        cid, k, data, delays, alpha, rho, mb, N = case
        Y, counts = SC.realisations(case)
        d, a, rh, real = SC.rows(case)
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll, info = obj.loglik_markov_resampled(Y, d, a, rh, real, counts=counts)
        assert ll.shape == (SC.R,) and (info == 0).all(), cid
        for r in range(SC.R):
            ref, b, _ = SC.reference(oracle, case, r)
            worst[SC.KINDS[r]].add(abs(ll[r] - ref) / abs(ref), b, (cid, r))
    for w in worst.values():
        assert w.where is not None
        w.report()


@pytest.mark.parametrize("N", [150, 767])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_parity_larger(oracle, kernel, N):
    """One L = 3 case per kernel.  At N = 767 M = 70 rows cycle through the 4 realisations in a scrambled order: more than one
    workgroup, lanes beyond M."""
    case = next(c for c in SC.cases((N,)) if c[1] == kernel and len(c[3]) == 3 and c[6] and c[5] == 3.0)
    cid, k, data, delays, alpha, rho, mb, _ = case
    Y, counts = SC.realisations(case)
    M = 70 if N == 767 else SC.R
    real = (np.random.default_rng(N).permutation(M) * 3 + 1) % SC.R
    assert set(real) == set(range(SC.R))
    with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
        ll, info = obj.loglik_markov_resampled(Y, np.tile(delays, (M, 1)), np.tile(alpha, (M, 1)), np.full(M, rho), real, counts=counts)
    assert (info == 0).all()
    worst = MC.Worst("device %s N = %d, L = 3" % (kernel, N))
    for m in range(M):
        ref, b, _ = SC.reference(oracle, case, int(real[m]))
        worst.add(abs(ll[m] - ref) / abs(ref), b, (cid, m, int(real[m])))
    worst.report()


def _batch(L, M, seed):
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), rg.uniform(-3.0, 45.0, (M, L - 1))], 1)
    return delays, rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))


@pytest.mark.parametrize("kernel,Nl,mb", [("matern52", [300, 200, 267], True), ("OU", [60, 50], False), ("matern32", [40, 41], True)])
def test_bitwise_invariance_of_a_row(kernel, Nl, mb):
    """A row's value does not depend on M, on the row order, on R, on the position of its realisation in Y, on the handle's flavour or
    on a split of R across calls."""
    t, y, s, _ = MC.lightcurves(Nl, seed=7, kind="ties")
    L, N, M, R = len(Nl), sum(Nl), 257, 7
    delays, alpha, rho = _batch(L, M, seed=L)
    Y, counts = synthetic.resample(y, s, R, seed=5)
    Y, counts = np.concatenate(Y, axis=1), np.concatenate(counts, axis=1)
    real = np.random.default_rng(4).integers(0, R, M)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        count = obj.get_option("markov_count")
        full, info = obj.loglik_markov_resampled(Y, delays, alpha, rho, real, counts=counts)
        assert obj.get_option("markov_count") == count + M
        assert full.shape == (M,) and (info == 0).all() and np.isfinite(full).all()
        for Ms in (1, 63, 64, 65):
            ll, inf = obj.loglik_markov_resampled(Y, delays[:Ms], alpha[:Ms], rho[:Ms], real[:Ms], counts=counts)
            assert np.array_equal(ll, full[:Ms]) and (inf == 0).all(), Ms
        rows = np.random.default_rng(2).permutation(M)
        ll, _ = obj.loglik_markov_resampled(Y, delays[rows], alpha[rows], rho[rows], real[rows], counts=counts)
        assert np.array_equal(ll, full[rows])
        order = np.argsort(real, kind="stable")                                 # realisation-major, as the fit orders its rows
        ll, _ = obj.loglik_markov_resampled(Y, delays[order], alpha[order], rho[order], real[order], counts=counts)
        assert np.array_equal(ll, full[order])
        perm = np.random.default_rng(1).permutation(R)                           # the realisations at other positions of Y
        inv = np.argsort(perm)
        ll, _ = obj.loglik_markov_resampled(Y[perm], delays, alpha, rho, inv[real], counts=counts[perm])
        assert np.array_equal(ll, full)
        sel = real < 3                                                           # a smaller R
        ll, _ = obj.loglik_markov_resampled(Y[:3], delays[sel], alpha[sel], rho[sel], real[sel], counts=counts[:3])
        assert np.array_equal(ll, full[sel])
        before = obj.get_option("markov_resample_bytes_max")
        assert before == 512 << 20
        for per in (1, 2, 3):                                                    # R split across calls of `per` realisations
            obj.set_option("markov_resample_bytes_max", 16 * N * per + 5)
            ll, inf = obj.loglik_markov_resampled(Y, delays, alpha, rho, real, counts=counts)
            assert np.array_equal(ll, full) and (inf == 0).all(), per
        obj.set_option("markov_resample_bytes_max", before)
        with pytest.raises(gpcc_amd.GpccError):
            obj.set_option("markov_resample_bytes_max", -1)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, precision="fp32") as o32:
        ll, inf = o32.loglik_markov_resampled(Y, delays[:65], alpha[:65], rho[:65], real[:65], counts=counts)
        assert np.array_equal(ll, full[:65]) and (inf == 0).all()
        assert o32.get_option("markov_resample_bytes") == 16 * N * R
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, devices=[0, 0]) as om:
        ll, inf = om.loglik_markov_resampled(Y, delays[:65], alpha[:65], rho[:65], real[:65], counts=counts)
        assert np.array_equal(ll, full[:65]) and (inf == 0).all()


def _raw(obj, M, delays, alpha, rho, real, R, Y, count=None, mean=None, sigma_b=None):
    """The C entry itself: NULL arguments, and the arguments the Python wrapper refuses first."""
    dp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
    i = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
    ll, info = np.full(max(M, 1), -7.0), np.full(max(M, 1), 99, np.int32)
    keep = [f(delays), f(alpha), f(rho), i(real), f(Y), i(count), f(mean), f(sigma_b)]
    rc = _capi.load().gpcc_loglik_markov_resampled_batch(obj._h, M, dp(keep[0]), dp(keep[1]), dp(keep[2]), ip(keep[3]), R, dp(keep[4]),
                                                         ip(keep[5]), dp(keep[6]), dp(keep[7]), dp(ll), ip(info))
    return rc, ll, info


@pytest.mark.parametrize("mb", [True, False])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_the_handles_own_data_is_loglik_markov_batch_bitwise(kernel, mb):
    """real pointing to the handle's own y, counts, mean and sigma_b NULL: gpcc_loglik_markov_batch's value and info, bit for bit
    (the step functions are shared unedited) -- also for failing rows, and with the own y at another position among other fluxes."""
    Nl = [40, 41, 30]
    t, y, s, _ = MC.lightcurves(Nl, seed=9, kind="ties")
    M = 130
    delays, alpha, rho = _batch(3, M, seed=8)
    alpha[5, 1] = -1.0
    rho[7] = 0.0
    Y = np.concatenate(synthetic.flux_randomise(y, s, 3, seed=1), axis=1)
    Y[1] = np.concatenate(y)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        single, sinfo = obj.loglik_markov_batch(delays, alpha, rho)
        rc, ll, info = _raw(obj, M, delays, alpha, rho, np.ones(M), 3, Y)
        assert rc == 0
        assert np.array_equal(ll, single, equal_nan=True) and np.array_equal(info, sinfo)
        assert list(sinfo[[5, 7]]) == [-1, -2] and np.isfinite(single[sinfo == 0]).all()
        rc, one, oinfo = _raw(obj, M, delays, alpha, rho, np.zeros(M), 1, np.concatenate(y), count=np.ones(sum(Nl)))
        assert rc == 0 and np.array_equal(one, single, equal_nan=True) and np.array_equal(oinfo, sinfo)


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_agreement_with_the_many_realisations_entry(kernel):
    """Counts of 1, the handle's means and Sigma_b, several rows sharing (tau, alpha, rho): gpcc_loglik_markov_multi_batch's cell
    within twice the bar (the two entries order their statements differently; the bar without a dense error, F N 2^-53)."""
    Nl = [60, 50]
    t, y, s, _ = MC.lightcurves(Nl, seed=21, kind="plain")
    G, R = 6, 5
    delays, alpha, rho = _batch(2, G, seed=3)
    Y = np.concatenate(synthetic.flux_randomise(y, s, R, seed=2), axis=1)
    with gpcc_amd.Objective(t, y, s, KERN[kernel]) as obj:
        multi, minfo = obj.loglik_markov_realisations(Y, delays, alpha, rho, center="handle")
        g, r = np.repeat(np.arange(G), R), np.tile(np.arange(R), G)
        ll, info = obj.loglik_markov_resampled(Y, delays[g], alpha[g], rho[g], r, center="handle", sigma_b="handle")
    assert (minfo == 0).all() and (info == 0).all()
    tol = 2 * np.array([MC.bar(0.0, sum(Nl), MC.factor(alpha[k], s)) for k in g])
    rel = np.abs(ll - multi.reshape(-1)) / np.abs(multi.reshape(-1))
    print("resampled against multi, %s: worst disagreement / (2 F N 2^-53) %.3g" % (kernel, float(np.max(rel / tol))))
    assert (rel <= tol).all()


def test_unstaged_path():
    """N = 7000 does not fit the LDS: the times come through the caches too.  8 rows x 3 realisations (one with RSS) against 3 fresh
    handles' loglik_markov_batch on the reduced data, within 2 F N 2^-53 of the value (device against device: the dense reference is
    too slow here)."""
    Nl = [3500, 3500]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=4)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    G, R, N = 8, 3, sum(Nl)
    delays = np.stack([np.zeros(G), np.linspace(0.0, 12.6, G)], 1)
    alpha, rho = np.tile(alpha0, (G, 1)), np.full(G, rho0)
    Y, counts = synthetic.resample(y, s, R, seed=6, subset=False)
    _, rss = synthetic.resample(y, s, 1, seed=7, flux=False)
    for l in range(2):
        counts[l][2] = rss[l][0]
    g, r = np.tile(np.arange(G), R), np.repeat(np.arange(R), G)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        ll, info = obj.loglik_markov_resampled(Y, delays[g], alpha[g], rho[g], r, counts=counts)
    assert (info == 0).all() and np.isfinite(ll).all()
    tol = 2 * MC.factor(alpha0, s) * N * 2.0 ** -53
    worst = 0.0
    for k in range(R):
        red = SC.reduced((t, y, s), Y, counts, k)
        with gpcc_amd.Objective(*red, gpcc_amd.matern32) as fresh:
            one, finfo = fresh.loglik_markov_batch(delays, alpha, rho)
        assert (finfo == 0).all()
        rel = np.max(np.abs(ll[r == k] - one) / np.abs(one))
        worst = max(worst, rel / tol)
        assert rel <= tol, (k, rel, tol)
    assert sum(len(a) for a in SC.reduced((t, y, s), Y, counts, 2)[0]) < N
    print("unstaged N = 7000: worst disagreement / (2 F N 2^-53) %.3g" % worst)


def test_codes_nan_fluxes_and_empty_realisations():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    R, M = 4, 12
    Y, counts = synthetic.resample(y, s, R, seed=2)
    Y, counts = np.concatenate(Y, axis=1), np.concatenate(counts, axis=1)
    delays, alpha, rho = _batch(2, M, seed=5)
    real = np.arange(M) % R
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        good, ginfo = obj.loglik_markov_resampled(Y, delays, alpha, rho, real, counts=counts)
        assert (ginfo == 0).all() and np.isfinite(good).all()
        # failing rows: loglik_markov_batch's codes, NaN; the neighbours bitwise untouched
        a2, r2 = alpha.copy(), rho.copy()
        a2[1, 0] = 0.0
        a2[2, 1] = -1.0
        r2[3] = 0.0
        r2[4] = -2.0
        ll, info = obj.loglik_markov_resampled(Y, delays, a2, r2, real, counts=counts)
        assert list(info[[1, 2, 3, 4]]) == [-1, -1, -2, -2] and np.isnan(ll[1:5]).all()
        rest = [0] + list(range(5, M))
        assert (info[rest] == 0).all() and np.array_equal(ll[rest], good[rest])
        # a flux that is not finite at a kept point poisons exactly the rows of that realisation; at a dropped point none
        kept, dropped = int(np.flatnonzero(counts[1] > 0)[3]), int(np.flatnonzero(counts[1] == 0)[2])
        for bad in (np.nan, np.inf, -np.inf):
            Yb = Y.copy()
            Yb[1, kept] = bad
            ll, info = obj.loglik_markov_resampled(Yb, delays, alpha, rho, real, counts=counts, center=np.zeros((R, 2)), sigma_b="handle")
            base, _ = obj.loglik_markov_resampled(Y, delays, alpha, rho, real, counts=counts, center=np.zeros((R, 2)), sigma_b="handle")
            assert (info == 0).all() and np.isnan(ll[real == 1]).all() and np.array_equal(ll[real != 1], base[real != 1])
            Yb = Y.copy()
            Yb[1, dropped] = bad
            ll, info = obj.loglik_markov_resampled(Yb, delays, alpha, rho, real, counts=counts, center=np.zeros((R, 2)), sigma_b="handle")
            assert (info == 0).all() and np.array_equal(ll, base)
        # a realisation that keeps nothing: 0.0 with info 0, its neighbours untouched
        c0 = counts.copy()
        c0[2] = 0
        ll, info = obj.loglik_markov_resampled(Y, delays, alpha, rho, real, counts=c0, center="handle", sigma_b="handle")
        base, _ = obj.loglik_markov_resampled(Y, delays, alpha, rho, real, counts=counts, center="handle", sigma_b="handle")
        assert (info == 0).all() and (ll[real == 2] == 0.0).all() and np.array_equal(ll[real != 2], base[real != 2])
    # info counts the kept points: sigma = 0 at two kept points that coincide in shifted time, dropped points ahead of them
    t, y, s, d0 = MC.lightcurves([30, 20], seed=5, kind="ties")
    ts = markov.prepare(t, y, s)[0]
    seq = markov.merge_order(ts, d0)
    sh = [ts[b][i] - d0[b] for b, i in seq]
    single = lambda q: np.count_nonzero(t[seq[q][0]] == ts[seq[q][0]][seq[q][1]]) == 1
    j = next(j for j in range(3, len(seq)) if seq[j][0] != seq[j - 1][0] and sh[j] == sh[j - 1] and single(j) and single(j - 1)
             and (j + 1 == len(seq) or sh[j + 1] != sh[j]) and sh[j - 2] != sh[j])
    for b, i in (seq[j - 1], seq[j]):
        s[b][np.where(t[b] == ts[b][i])[0]] = 0.0
    cz = [np.ones((2, len(x)), dtype=np.int64) for x in t]
    for b, i in seq[:2]:
        cz[b][1, np.where(t[b] == ts[b][i])[0][0]] = 0
    dropped = sum(int((x[1] == 0).sum()) for x in cz)
    Yz = [np.tile(np.asarray(x), (2, 1)) for x in y]
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU, marginalise_b=False) as obj:
        ll, info = obj.loglik_markov_resampled(Yz, [d0, d0, d0 + [0.0, 0.37]], [[1.0, 1.0]] * 3, [2.0] * 3, [0, 1, 1], counts=cz)
        host, hinfo = markov.MarkovObjective(t, y, s, "OU", marginalise_b=False).loglik_markov_resampled(
            Yz, [d0, d0, d0 + [0.0, 0.37]], [[1.0, 1.0]] * 3, [2.0] * 3, [0, 1, 1], counts=cz)
    assert dropped >= 1 and list(info[:2]) == [j + 1, j + 1 - dropped] and np.isnan(ll[:2]).all()
    assert info[2] == 0 and np.isfinite(ll[2]) and np.array_equal(info, hinfo)


def test_refusals():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    N, R = 110, 3
    Y, counts = synthetic.resample(y, s, R, seed=2)
    Yf, cf = np.concatenate(Y, axis=1), np.concatenate(counts, axis=1)
    delays, alpha, rho = _batch(2, 8, seed=5)
    real = np.arange(8) % R
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loglik_markov_resampled(Y, delays, alpha, rho, real, counts=counts)
        assert ei.value.code == UNSUPPORTED and "rbf" in ei.value.message
        assert obj.loglik_batch([d0], [[1.0, 1.0]], [2.0])[1][0] == 0            # the handle still serves its other entries
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        # everything below is refused on the host, before any device work: the handle has not even sorted its light curves
        for bad in ([0, 1, 2, 3, 0, 1, 2, 0], [0, -1, 2, 0, 0, 1, 2, 0]):
            rc, ll, info = _raw(obj, 8, delays, alpha, rho, bad, R, Yf, count=cf)
            assert rc == ARGUMENT and (ll == -7.0).all() and (info == 99).all()
        cb = cf.copy()
        cb[2, 17] = -1
        assert _raw(obj, 8, delays, alpha, rho, real, R, Yf, count=cb)[0] == ARGUMENT
        assert _raw(obj, 8, delays, alpha, rho, real, 0, Yf)[0] == ARGUMENT
        assert _raw(obj, 8, delays, alpha, rho, real, R, None)[0] == ARGUMENT
        assert _raw(obj, 8, delays, alpha, rho, None, R, Yf)[0] == ARGUMENT
        obj.set_option("markov_resample_bytes_max", 16 * N * R - 1)
        rc, ll, info = _raw(obj, 8, delays, alpha, rho, real, R, Yf)
        assert rc == UNSUPPORTED and "markov_resample_bytes_max" in _capi.last_error(obj._h) and (ll == -7.0).all()
        obj.set_option("markov_resample_bytes_max", 16 * N * R)
        assert obj.get_option("markov_resample_bytes") == 0 and obj.get_option("markov_count") == 0
        rc, out, info = _raw(obj, 0, delays, alpha, rho, real, R, Yf)
        assert rc == 0 and (out == -7.0).all()                                   # M = 0 returns 0 and touches nothing
        rc, out, info = _raw(obj, 8, delays, alpha, rho, real, R, Yf, count=cf)  # NULL mean and sigma_b: the handle's
        ll, linfo = obj.loglik_markov_resampled(Y, delays, alpha, rho, real, counts=counts, center="handle", sigma_b="handle")
        assert rc == 0 and np.array_equal(out, ll) and np.array_equal(info, linfo) and (linfo == 0).all()
        own, _ = obj.loglik_markov_resampled(Y, delays, alpha, rho, real, counts=counts)
        assert not np.array_equal(own, ll)
        with pytest.raises(ValueError):
            obj.loglik_markov_resampled(Y, delays, alpha, rho, [0, 1, 2, 3, 0, 1, 2, 0], counts=counts)
        with pytest.raises(ValueError):
            obj.loglik_markov_resampled(Y, delays, alpha, rho, real, counts=[c * -1 for c in counts])
        with pytest.raises(ValueError):
            obj.loglik_markov_resampled(Yf[:, :-1], delays, alpha, rho, real)
        one = [c.copy() for c in counts]
        one[0][1, :] = 0
        one[0][1, 5] = 60
        with pytest.raises(ValueError):
            obj.loglik_markov_resampled(Y, delays, alpha, rho, real, counts=one)
    # five bands: with marginalised offsets unsupported, without them fine
    t5, y5, s5, d5 = MC.lightcurves([30, 25, 20, 25, 30], seed=12, kind="ties")
    a5 = np.linspace(0.6, 1.4, 5)
    Y5, c5 = synthetic.resample(y5, s5, 2, seed=1)
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=True) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loglik_markov_resampled(Y5, [d5] * 2, [a5] * 2, [2.0] * 2, [0, 1], counts=c5)
        assert ei.value.code == UNSUPPORTED
        assert obj.loglik_batch([d5], [a5], [2.0])[1][0] == 0
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=False) as obj:
        ll, info = obj.loglik_markov_resampled(Y5, [d5] * 2, [a5] * 2, [2.0] * 2, [0, 1], counts=c5)
        host, hinfo = markov.MarkovObjective(t5, y5, s5, "OU", marginalise_b=False).loglik_markov_resampled(
            Y5, [d5] * 2, [a5] * 2, [2.0] * 2, [0, 1], counts=c5)
        assert (info == 0).all() and (hinfo == 0).all()
        assert np.all(np.abs(ll - host) <= 2 * MC.bar(0.0, 130, MC.factor(a5, s5)) * np.abs(host))


def test_memory_of_a_resampling_only_handle():
    """N = 16384: the handle allocates the sorted light curves, the staging and this entry's scratch, none of the N^2 workspace;
    markov_resample_bytes reports the packed data, 16 N R bytes."""
    import torch
    Nl = [8192, 8192]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=3)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    G, R, N = 16, 4, sum(Nl)
    delays = np.stack([np.zeros(G), np.linspace(0.0, 12.6, G)], 1)
    alpha, rho = np.tile(alpha0, (G, 1)), np.full(G, rho0)
    Y, counts = synthetic.resample(y, s, R, seed=2)
    g, r = np.tile(np.arange(G), R), np.repeat(np.arange(R), G)
    torch.cuda.synchronize()
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        assert obj.get_option("markov_resample_bytes") == 0 and obj.get_option("markov_resample_upload_bytes") == 0
        free0, _ = torch.cuda.mem_get_info(0)
        ll, info = obj.loglik_markov_resampled(Y, delays[g], alpha[g], rho[g], r, counts=counts)
        ll2, _ = obj.loglik_markov_resampled([a[:2] for a in Y], delays[:3], alpha[:3], rho[:3], [1, 1, 0], counts=[c[:2] for c in counts])
        free1, _ = torch.cuda.mem_get_info(0)
        assert obj.get_option("workspace_slots") == obj.get_option("slots_per_stream")     # (never built)
        scratch, upload = obj.get_option("markov_resample_bytes"), obj.get_option("markov_resample_upload_bytes")
    assert scratch == 16 * N * R
    assert upload == 12 * N * R + 16 * 2 * R + 4 * G * R + 4 * N
    print("N = 16384 resampling-only handle: %.2f MiB of growth, %.2f MiB of it packed data, %.2f MiB uploads"
          % ((free0 - free1) / 2.0 ** 20, scratch / 2.0 ** 20, upload / 2.0 ** 20))
    assert free0 - free1 < scratch + upload + 8 * 2 ** 20                    # (the N^2 workspace would be gigabytes)
    assert (info == 0).all() and np.isfinite(ll).all()
    assert np.array_equal(ll2, ll[[G, G + 1, 2]])
    red = SC.reduced((t, y, s), Y, counts, 3)
    with gpcc_amd.Objective(*red, gpcc_amd.matern52) as fresh:
        one, finfo = fresh.loglik_markov_batch(delays, alpha, rho)
    assert (finfo == 0).all() and np.all(np.abs(ll[3 * G:] - one) <= 2 * MC.bar(0.0, N, MC.factor(alpha0, s)) * np.abs(one))


def test_refit_end_to_end(oracle):
    """README size, realisation_refits on the device: R = 3, G = 5, 30 iterations from the original data's fit.  Every returned
    (alpha, rho) re-evaluated on a fresh handle of that realisation's reduced data reproduces the returned loglikel under the bar
    (F N_kept 2^-53: device against device); every cell is >= its start value."""
    t, y, s, _ = synthetic.simulate_lightcurves((55, 55))
    grid = np.array([0.0, 1.0, 2.0, 3.0, 8.0])
    cand = np.stack([np.zeros_like(grid), grid], 1)
    R, G = 3, 5
    Y, counts = synthetic.resample(y, s, R, seed=3)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        res = fit.gpcc_grid(t, y, s, kernel=gpcc_amd.OU, candidatedelays=cand, iterations=30, seed=1, objective=obj, solver="markov")
        out = fit.realisation_refits(obj, cand, Y, counts, iterations=30, start=(res.alpha, res.rho))
        real = np.repeat(np.arange(R), G)
        start, sinfo = obj.loglik_markov_resampled(Y, np.tile(cand, (R, 1)), np.tile(res.alpha, (R, 1)), np.tile(res.rho, R), real,
                                                   counts=counts)
    assert out.loglikel.shape == (R, G) and out.alpha.shape == (R, G, 2) and out.rho.shape == (R, G) and (sinfo == 0).all()
    assert np.isfinite(out.loglikel).all() and (out.loglikel >= out.start_loglikel).all()
    worst = 0.0
    for r in range(R):
        red = SC.reduced((t, y, s), Y, counts, r)
        n = sum(len(a) for a in red[0])
        with gpcc_amd.Objective(*red, gpcc_amd.OU) as fresh:
            one, finfo = fresh.loglik_markov_batch(cand, out.alpha[r], out.rho[r])
            at, ainfo = fresh.loglik_markov_batch(cand, res.alpha, res.rho)
        assert (finfo == 0).all() and (ainfo == 0).all()
        tol = np.array([MC.bar(0.0, n, MC.factor(out.alpha[r, k], red[2])) for k in range(G)])
        rel = np.abs(out.loglikel[r] - one) / np.abs(one)
        worst = max(worst, float(np.max(rel / tol)))
        assert (rel <= tol).all(), (r, rel, tol)
        # >= the start as given (the optimiser holds it after a round trip through its transforms: the bar covers that)
        tol0 = np.array([MC.bar(0.0, n, MC.factor(res.alpha[k], red[2])) for k in range(G)])
        assert (out.loglikel[r] >= at - tol0 * np.abs(at)).all() and (out.loglikel[r] >= start[r * G:(r + 1) * G] - tol0 * np.abs(at)).all()
    assert np.all(np.abs(out.delays.prob.sum(axis=1) - 1.0) <= 1e-12) and out.delays.mean_delay.shape == (R, 2)
    print("refit end to end: worst |refit - fresh handle| / (F N 2^-53) %.3g; mean gain over the start %.3g"
          % (worst, float(np.mean(out.loglikel - out.start_loglikel))))
