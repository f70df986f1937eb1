"""gpcc_loglik_hess_noise_markov_batch on the device: the Hessian over [alpha, rho, kappa, nu] against the
extended-precision reference on the effective error bars and against the numpy mirror (tests/_markov_noise_hess_cases.py); value, info
and gradient bitwise the noise gradient entry's; every shipped <P, NOFF> and the refused one; rows that do not depend on M, the row
order, the launch shape, options and handle flavours; the unstaged path; one large shape against the dense entry on effective_std and
central differences of the gradient entry; fit.noise_evidence on the device and on the mirror.  The references are computed in a pool
of CPU processes that never touch the GPU; the worst error / bar of each group is printed."""
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _hess_highprec as HH
import _hess_witness as HW
import _markov_cases as MC
import _markov_grad_cases as GC
import _markov_noise_cases as NC
import _markov_noise_hess_cases as NH
import gpcc_amd
from gpcc_amd import _capi, fit, markov, synthetic
from gpcc_amd.api import _dp, _ip

pytestmark = pytest.mark.gpu

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
UNSUPPORTED = -3
EPS = np.finfo(float).eps
LARGE_BAR = 2e-7          # per block, of max|H_dense|: what tests/test_gpu_markov_hess.py accepts for the plain block against the dense entry


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


# ---- parity over the CPU cases -----------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not HH.EXTENDED, reason=HH.SKIP_REASON)
@pytest.mark.parametrize("N", NH.SIZES)
def test_parity_cpu_cases(pool, N):
    cases = NH.cases(N)
    assert len(cases) == 72
    refs = pool.map(NH.reference_job, [NH.job(c) for c in cases])
    mirrors = pool.map(NH.mirror_job, cases)
    worst = {b: GC.Worst("device noise Hessian N = %d block %s" % (N, b)) for b in NH.BLOCKS}
    mirror = GC.Worst("device against mirror N = %d (of 2 bars)" % N)
    print("build: %s" % gpcc_amd.build_info())
    for case, ref, (ml, mg, mh, minfo) in zip(cases, refs, mirrors):
        cid, k, data, delays, alpha, rho, mb, _, kappa, nu = case
        L = len(alpha)
        assert ref.info == 0 and minfo == 0, cid
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll, grad, hess, info = obj.loglik_hess_markov_noise_batch(delays[None, :], alpha[None, :], [rho], kappa, nu)
            gl, gg, ginfo = obj.loglik_grad_markov_noise_batch(delays[None, :], alpha[None, :], [rho], kappa, nu)
        assert info[0] == 0 and hess.shape == (1, 3 * L + 1, 3 * L + 1) and np.array_equal(hess[0], hess[0].T), cid
        assert np.array_equal(ll, gl) and np.array_equal(grad, gg) and np.array_equal(info, ginfo), cid
        for b, r in NH.ratios(hess[0], ref, case).items():
            worst[b].add(r, cid)
        mirror.add(NH.worst(NH.ratios(hess[0], ref, case, against=mh)) / 2.0, cid)
    for w in worst.values():
        w.report()
    mirror.report()


def test_null_hess_is_the_gradient_entry():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    M, L = 5, 2
    rg = np.random.default_rng(3)
    d = np.ascontiguousarray(np.tile(d0, (M, 1)))
    a, r = rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.5), np.log(30.0), M))
    kappa, nu = rg.uniform(0.5, 2.0, (M, L)), rg.uniform(0.0, 0.05, (M, L))
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        gl, gg, ginfo = obj.loglik_grad_markov_noise_batch(d, a, r, kappa, nu)
        before = obj.get_option("markov_count")
        ll, grad, info = np.empty(M), np.empty((M, 4 * L + 1)), np.zeros(M, np.int32)
        rc = _capi.load().gpcc_loglik_hess_noise_markov_batch(obj._h, M, _dp(d), _dp(a), _dp(r), _dp(kappa), _dp(nu), _dp(ll), _dp(grad), None,
                                                              _ip(info))
        assert rc == 0 and obj.get_option("markov_count") - before == M
        assert np.array_equal(ll, gl) and np.array_equal(grad, gg) and np.array_equal(info, ginfo)
        # kappa = nu = NULL: kappa = 1, nu = 0
        h0 = obj.loglik_hess_markov_noise_batch(d, a, r)
        h1 = obj.loglik_hess_markov_noise_batch(d, a, r, np.ones((M, L)), np.zeros((M, L)))
        for x, z in zip(h0, h1):
            assert np.array_equal(x, z)
        assert _capi.load().gpcc_loglik_hess_noise_markov_batch(obj._h, 0, None, None, None, None, None, None, None, None, None) == 0


# ---- every shipped instantiation ---------------------------------------------------------------------------------------------------
SIZES110 = {0: [60, 50], 1: [110], 2: [60, 50], 3: [40, 40, 30], 4: [30, 30, 25, 25]}


def _unit_case(kernel, noff, row):
    Nl = SIZES110[noff]
    L = len(Nl)
    t, y, s, d0 = MC.lightcurves(Nl, seed=50 + noff, kind="ties" if L > 1 else "plain")
    rg = np.random.default_rng(1000 * noff + row)
    alpha, rho = rg.uniform(0.5, 1.8, L), float(np.exp(rg.uniform(np.log(0.5), np.log(30.0))))
    kappa, nu = rg.uniform(0.5, 2.0, L), rg.uniform(0.0, 0.05, L)
    if row == 2:
        kappa[0], nu[0] = 0.0, 0.01
    return ("%s-noff%d-row%d" % (kernel, noff, row), kernel, (t, y, s), np.asarray(d0, np.float64), alpha, rho, noff > 0, 110, kappa, nu)


@pytest.mark.skipif(not HH.EXTENDED, reason=HH.SKIP_REASON)
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_every_shipped_instantiation_and_the_refused_one(pool, kernel):
    """<P, NOFF> for NOFF = 0..4 (NOFF = 0: two bands without marginalised offsets), N = 110, 3 rows each with their own (alpha, rho,
    kappa, nu), against the mirror within 2 bars of the row's reference and against the reference within its bars.  <3, 4> does not
    ship: GPCC_ERR_UNSUPPORTED before any device work."""
    p = markov.order(kernel)
    shipped = [noff for noff in range(5) if not (p == 3 and noff == 4)]
    cases = [_unit_case(kernel, noff, row) for noff in shipped for row in range(3)]
    refs = list(pool.map(NH.reference_job, [NH.job(c) for c in cases]))
    mirrors = list(pool.map(NH.mirror_job, cases))
    for noff in range(5):
        rows = [_unit_case(kernel, noff, row) for row in range(3)]
        data, mb = rows[0][2], rows[0][6]
        d, a, r = np.stack([c[3] for c in rows]), np.stack([c[4] for c in rows]), np.array([c[5] for c in rows])
        kap, exc = np.stack([c[8] for c in rows]), np.stack([c[9] for c in rows])
        with gpcc_amd.Objective(*data, KERN[kernel], marginalise_b=mb) as obj:
            before = obj.get_option("markov_count")
            if noff not in shipped:
                with pytest.raises(gpcc_amd.GpccError) as ei:
                    obj.loglik_hess_markov_noise_batch(d, a, r, kap, exc)
                assert ei.value.code == UNSUPPORTED and "effective_std" in ei.value.message and "gpcc_loglik_hess_hyper_batch" in ei.value.message
                assert obj.get_option("markov_count") == before
                assert obj.loglik_grad_markov_noise_batch(d, a, r, kap, exc)[2].tolist() == [0, 0, 0]      # the handle still serves the gradient
                continue
            ll, grad, hess, info = obj.loglik_hess_markov_noise_batch(d, a, r, kap, exc)
            assert obj.get_option("markov_count") - before == 3 and (info == 0).all()
        worst = GC.Worst("<%d, %d> against the reference" % (p, noff))
        mirror = GC.Worst("<%d, %d> against the mirror (of 2 bars)" % (p, noff))
        for row in range(3):
            i = shipped.index(noff) * 3 + row
            assert refs[i].info == 0 and mirrors[i][3] == 0
            worst.add(NH.worst(NH.ratios(hess[row], refs[i], cases[i])), cases[i][0])
            mirror.add(NH.worst(NH.ratios(hess[row], refs[i], cases[i], against=mirrors[i][2])) / 2.0, cases[i][0])
        worst.report()
        mirror.report()


# ---- row independence --------------------------------------------------------------------------------------------------------------
PROBLEMS = {"matern32-b": ("matern32", [7, 5], True), "OU-fixed": ("OU", [6, 5, 4], False)}     # test_gpu_markov_noise.py's


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _batch_rows(C, ny, waves_per_workgroup):
    """test_gpu_markov_noise.py's: M with a ragged last workgroup of one row."""
    if waves_per_workgroup == 4:
        return 128 * C + 1
    blocks = (3 * C // 2) // ny
    blocks -= 1 - blocks % 2
    return 64 * (blocks - 1) + 1


@pytest.mark.parametrize("wpw", [4, 2])
@pytest.mark.parametrize("problem", list(PROBLEMS))
def test_rows_do_not_depend_on_the_launch_shape(problem, wpw):
    kernel, Nl, mb = PROBLEMS[problem]
    L, C = len(Nl), _cus()
    ny = (3 * L + 1) * (3 * L + 2) // 2                                  # the pair slots: the grid's y
    M = _batch_rows(C, ny, wpw)
    waves = (M + 63) // 64 * ny
    assert waves > 2 * C if wpw == 4 else C < waves <= 2 * C, (M, ny, C)
    t, y, s, _ = MC.lightcurves(Nl, seed=31 + L, kind="plain")
    rg = np.random.default_rng(M + ny)
    delays = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 8.0, (M, L - 1)))], 1)
    alpha, rho = rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))
    kappa, nu = rg.uniform(0.0, 2.0, (M, L)), rg.uniform(0.001, 0.05, (M, L))
    good = kappa[M - 1, L - 1]
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        call = lambda sl: obj.loglik_hess_markov_noise_batch(delays[sl], alpha[sl], rho[sl], kappa[sl], nu[sl])
        clean = call(slice(0, M))
        assert (clean[3] == 0).all() and np.isfinite(clean[2]).all()
        kappa[M - 1, L - 1] = -0.5                                       # the last row fails (-3), alone in the last workgroup
        ll, grad, hess, info = call(slice(0, M))
        assert info[M - 1] == -3 and (info[:M - 1] == 0).all()
        assert np.isnan(ll[M - 1]) and np.isnan(grad[M - 1]).all() and np.isnan(hess[M - 1]).all()
        for x, z in zip((ll, grad, hess), clean[:3]):                    # ... and leaves every other row's bits unchanged
            assert np.array_equal(x[:M - 1], z[:M - 1])
        assert np.array_equal(hess[:M - 1], np.swapaxes(hess[:M - 1], 1, 2))
        gl, gg, ginfo = obj.loglik_grad_markov_noise_batch(delays, alpha, rho, kappa, nu)
        assert np.array_equal(ll, gl, equal_nan=True) and np.array_equal(grad, gg, equal_nan=True) and np.array_equal(info, ginfo)

        def same(got, sl):
            return all(np.array_equal(x, z[sl], equal_nan=True) for x, z in zip(got, (ll, grad, hess, info)))

        rpw = 64 * wpw
        nb = (M + rpw - 1) // rpw
        windows = [(0, 1), (0, 63), (0, 64), (0, 65), (M - 65, 64), (M - 1, 1)] + [(k * rpw - 32, 64) for k in sorted({1, nb // 2, nb - 2}) if k >= 1]
        for r0, n in windows:                                            # calls of <= 65 rows
            assert 0 <= r0 and r0 + n <= M
            assert same(call(slice(r0, r0 + n)), slice(r0, r0 + n)), (problem, M, r0, n)
        perm = np.random.default_rng(1).permutation(M)                   # the row order
        assert same(call(perm), perm)
        obj.set_option("markov_chunk_rows", 64)                          # ... and the option
        try:
            assert same(call(slice(0, M)), slice(0, M))
        finally:
            obj.set_option("markov_chunk_rows", 0)
    kappa[M - 1, L - 1] = good
    for kw in ({"precision": "fp32"}, {"devices": [0, 0]}):              # an fp32 handle (on its fp64 twin), a two-device handle
        with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, **kw) as o:
            sl = slice(M - 65, M)
            got = o.loglik_hess_markov_noise_batch(delays[sl], alpha[sl], rho[sl], kappa[sl], nu[sl])
            assert all(np.array_equal(x, z[sl]) for x, z in zip(got, clean)), kw


# ---- the unstaged path -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [6600, 110])
def test_unstaged_and_staged_against_the_mirror(pool, N):
    """One band, Matern-5/2, three rows that differ in (kappa, nu) alone, kappa = 0 among them (test_gpu_markov_noise.py's data).
    N = 6600: the light curves do not fit the LDS beside the lanes' part and come through the caches; N = 110: staged.  Against the
    numpy mirror under the CPU test's formula FACTOR max(e_dense, floor) factor / 16 per block with e_dense at its floor (the dense
    reference is out of reach at N = 6600) and the floor's size |T1| + |T2| + |T3| replaced by its lower bound max|H| of the block from
    the mirror -- a smaller bar, never a wider one."""
    rg = np.random.default_rng(N)
    t = [np.sort(MC.snap(rg.uniform(0.0, 30.0 * N / 110, N)))]
    y = [np.sin(0.4 * t[0]) + 0.2 * rg.standard_normal(N)]
    s = [0.2 + 0.05 * rg.random(N)]
    alpha0, rho0 = 1.3, 2.5
    kappa, nu = np.array([[0.6], [1.7], [0.0]]), np.array([[0.004], [0.03], [0.05]])
    d, a, r = np.zeros((3, 1)), np.full((3, 1), alpha0), np.full(3, rho0)
    host = pool.map(NH.hess_noise_job, [("matern52", t, y, s, d[m], a[m], r[m], kappa[m], nu[m], True) for m in range(3)])
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        ll, grad, hess, info = obj.loglik_hess_markov_noise_batch(d, a, r, kappa, nu)
        gl, gg, ginfo = obj.loglik_grad_markov_noise_batch(d, a, r, kappa, nu)
    assert (info == 0).all() and np.array_equal(ll, gl) and np.array_equal(grad, gg) and np.array_equal(hess, np.swapaxes(hess, 1, 2))
    masks = NH.block_masks(1)
    for m, (hl, hg, hh, hinfo) in enumerate(host):
        assert hinfo == 0
        factor = MC.factor([alpha0], NC.effective(s, kappa[m], nu[m]))
        for b, mask in masks.items():
            bar = MC.FACTOR * N * 2.0 ** -53 * float(np.max(np.abs(hh[mask]))) * factor / MC.FACTOR
            err = float(np.max(np.abs(hess[m][mask] - hh[mask])))
            print("N = %d row %d block %s: %.3g of its bar" % (N, m, b, err / bar if bar > 0 else err))
            assert err <= bar, (N, m, b, err, bar)


# ---- one large shape ---------------------------------------------------------------------------------------------------------------
def test_large_shape_against_dense_and_central_differences():
    """Matern-3/2, three ragged bands, N = 4095, 4 rows with their own kappa and nu.  Leading block: a fresh handle's dense
    loglik_hess_hyper_batch on effective_std, per block within LARGE_BAR of max|H_dense| (what the plain block is held to).  Noise rows
    and columns: five-point central differences of loglik_grad_markov_noise_batch in kappa and nu with relative step h / 2, h = 2e-3; the
    tolerance is the difference scheme's own error estimate, twice the largest change of the scheme's result over the row from step h to
    step h / 2 (the truncation of the coarser step, 16 times the finer one's, and the rounding of both); nothing of it comes from the
    entry under test.  Measured on an MI355X: the entry within 1.1e-11 of max|H| of the scheme, the tolerance 3e-11 to 2e-10 of it; the
    leading block within 3.1e-8 of max|H| of the dense entry."""
    G, N, L = 4, 4095, 3
    kernel, (t, y, s), delays, alpha, rho = GC.large(N, G)
    rg = np.random.default_rng(12)
    kappa, nu = rg.uniform(0.5, 2.0, (G, L)), rg.uniform(0.2, 1.0, (G, L)) * np.array([np.mean(a ** 2) for a in s])
    n = 3 * L + 1
    idx = list(range(L + 1)) + list(range(2 * L + 1, 4 * L + 1))          # theta's entries of a gradient row
    with gpcc_amd.Objective(t, y, s, KERN[kernel]) as obj:
        ll, grad, hess, info = obj.loglik_hess_markov_noise_batch(delays, alpha, rho, kappa, nu)
        assert (info == 0).all() and np.array_equal(hess, np.swapaxes(hess, 1, 2))

        def scheme(h):
            fd = np.empty((G, n, 2 * L))
            for c in range(2 * L):
                e = np.zeros((G, 2 * L))
                e[:, c] = h * np.concatenate([kappa, nu], 1)[:, c]
                f = [obj.loglik_grad_markov_noise_batch(delays, alpha, rho, kappa + q * e[:, :L], nu + q * e[:, L:])[1][:, idx] for q in (1, -1, 2, -2)]
                fd[:, :, c] = (8 * (f[0] - f[1]) - (f[2] - f[3])) / (12 * e[:, c])[:, None]
            return fd

        coarse, fine = scheme(2e-3), scheme(1e-3)
    worst_d, worst_n = 0.0, 0.0
    for g in range(G):
        eff = fit.effective_std(s, kappa[g], nu[g])
        with gpcc_amd.Objective(t, y, eff, KERN[kernel]) as fresh:
            dl, dgrad, dh, _, dinfo = fresh.loglik_hess_hyper_batch(delays[g:g + 1], alpha[g:g + 1], rho[g:g + 1])
        assert dinfo[0] == 0
        for name, m in HH.block_masks(L, L + 1).items():
            rr = float(np.max(np.abs(hess[g][:L + 1, :L + 1][m] - dh[0][m]))) / float(np.max(np.abs(dh[0][m])))
            worst_d = max(worst_d, rr)
            assert rr <= LARGE_BAR, (g, name, rr)
        got = hess[g][:, L + 1:]
        size = float(np.max(np.abs(fine[g])))
        tol = 2.0 * float(np.max(np.abs(coarse[g] - fine[g])))
        err = float(np.max(np.abs(got - fine[g])))
        worst_n = max(worst_n, err / size)
        print("row %d: noise rows against central differences %.3g of max|H| (tolerance %.3g)" % (g, err / size, tol / size))
        assert err <= tol, (g, err, tol)
    print("N = %d %s: leading block against the dense entry on effective_std %.3g of max|H| (bar %.0e); noise rows against central "
          "differences %.3g of max|H|" % (N, kernel, worst_d, LARGE_BAR, worst_n))


# ---- the evidence ------------------------------------------------------------------------------------------------------------------
def test_noise_evidence_on_the_device_and_on_the_mirror():
    """README-size data, 5 delays, the same NoiseGridFit as the warm start of fit.noise_evidence on Objective and on MarkovObjective: the
    same info codes, pinned sets and Newton rounds, and |dlogZ| within the two-bar allowance of tests/test_gpu_laplace.py for solver
    "markov" against "dense", 2 max(1e-6, 64 eps cond_1(K) |l^|), K on the effective error bars at the mode.  The noise model is an
    excess variance per band (the data's error bars are one number per band, so kappa and nu together are degenerate there); on this
    data w of band 1 ends pinned at its lower bound at every delay and w of band 2 at one.  Nearly all of the test's time is the numpy
    mirror's (some 25 rows of 28 pairs each)."""
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    cand = np.stack([np.zeros(5), np.array([1.0, 1.5, 2.0, 2.5, 3.0])], 1)
    a0, r0 = synthetic.default_hyperparameters(y)
    kw = dict(noise="excess", shared=False, rhomin=1e-3, rhomax=1e3)
    mobj = markov.MarkovObjective(t, y, s, "OU")
    start = fit.gpcc_grid_noise(mobj, cand, iterations=250, start=(np.tile(a0, (5, 1)), np.full(5, min(r0, 19.0))), **kw)
    host = fit.noise_evidence(mobj, cand, start, g_tol=1e-6, **kw)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        before = obj.get_option("markov_count")
        dev = fit.noise_evidence(obj, cand, start, g_tol=1e-6, **kw)
        assert obj.get_option("markov_count") - before == int(dev.rounds.sum())
    assert np.array_equal(dev.info, host.info) and np.array_equal(dev.pinned, host.pinned) and np.array_equal(dev.rounds, host.rounds), (dev, host)
    assert (dev.info == 0).any()
    band, tt, _, _ = HW._setup(t, y, s, True)
    worst = 0.0
    for g in np.flatnonzero(dev.info == 0):
        eff = fit.effective_std(s, dev.kappa[g], dev.nu[g])
        Kn = HW._setup(t, y, eff, True)[3]
        u = tt - cand[g][band]
        al = dev.alpha[g]
        K = al[band][:, None] * al[band][None, :] * HW.derivatives("OU", u[:, None] - u[None, :], dev.rho[g])[0] + Kn
        bar = 2 * max(1e-6, 64 * EPS * np.linalg.cond(np.asarray(K, np.float64), 1) * abs(dev.loglik[g]))
        worst = max(worst, abs(dev.log_evidence[g] - host.log_evidence[g]) / bar)
        assert abs(dev.log_evidence[g] - host.log_evidence[g]) <= bar, (g, dev.log_evidence[g], host.log_evidence[g], bar)
    print("noise evidence, device against mirror: info %s, rounds %s, pinned %s, worst |dlogZ| / (2 bars) %.3g"
          % (dev.info.tolist(), dev.rounds.tolist(), dev.pinned.astype(int).tolist(), worst))
