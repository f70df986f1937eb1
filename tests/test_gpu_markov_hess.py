"""gpcc_loglik_hess_hyper_markov_batch on the device: the (alpha, rho) block of the Hessian in linear time against the
extended-precision reference over the 144 cases of tests/_markov_hess_cases.py under the reference's own per-block bars and against the
numpy mirror; value, info and gradient bitwise gpcc_loglik_grad_markov_batch's; bitwise symmetry and invariance over batch sizes, row
order and handle flavours; refusal rows and refused requests; the large shapes against the dense device entry; N = 16384 against central
differences of the linear-time gradient; and the Laplace evidence with solver="markov" against solver="dense".  The references are
computed in a pool of CPU processes that never touch the GPU; the worst error / bar of each group is printed."""
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _hess_highprec as HH
import _hess_witness as HW
import _markov_cases as MC
import _markov_grad_cases as GC
import _markov_hess_cases as HC
import gpcc_amd
from gpcc_amd import fit, markov, synthetic

pytestmark = pytest.mark.gpu

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
UNSUPPORTED = -3
EPS = np.finfo(float).eps
LARGE_BAR = 2e-7          # per block, of max|H_dense|: tests/test_gpu_hessian.py's BAR = 1e-7 for the dense entry, and as much for this one


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


@pytest.mark.skipif(not HH.EXTENDED, reason=HH.SKIP_REASON)
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_parity_cpu_cases(pool, kernel):
    cases = [c for c in HC.cases() if c[1] == kernel]
    assert len(cases) == 2 * 3 * 2 * len(MC.RHOS)
    refs = pool.map(HH.reference_job, [HC.job(c) for c in cases])
    worst = HC.Worst("device Hessian block %s" % kernel)
    mirror = HC.Worst("device against mirror %s (of 2 bars)" % kernel)
    print("build: %s" % gpcc_amd.build_info())
    for case, ref in zip(cases, refs):
        cid, k, data, delays, alpha, rho, mb, N = case
        assert ref.info == 0, cid
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll, grad, hess, info = obj.loglik_hess_hyper_markov_batch(delays[None, :], alpha[None, :], [rho])
        assert info[0] == 0, cid
        worst.add(HC.ratio(hess[0], ref, case), cid)
        ml, mg, mh, minfo = markov.loglik_hess_hyper(k, *data, delays, alpha, rho, mb)     # the same algorithm, another rounding order
        assert minfo == 0
        mirror.add(HC.ratio(hess[0], ref, case, against=mh) / 2.0, cid)
    worst.report()
    mirror.report()


def _batch(L, M, seed):
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), rg.uniform(-3.0, 45.0, (M, L - 1))], 1)
    return delays, rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))


@pytest.mark.parametrize("kernel,Nl,mb", [("matern52", [300, 200, 267], True), ("OU", [60, 50], False), ("matern32", [2048, 2048], True)])
def test_bitwise_properties(kernel, Nl, mb):
    t, y, s, _ = MC.lightcurves(Nl, seed=7, kind="ties")
    L = len(Nl)
    delays, alpha, rho = _batch(L, 1024, seed=len(Nl))
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        gl, gg, ginfo = obj.loglik_grad_markov_batch(delays, alpha, rho)
        fl, fg, full, info = obj.loglik_hess_hyper_markov_batch(delays, alpha, rho)
        assert (info == 0).all() and np.isfinite(full).all() and full.shape == (1024, L + 1, L + 1)
        assert np.array_equal(fl, gl) and np.array_equal(fg, gg) and np.array_equal(info, ginfo)
        assert np.array_equal(full, np.swapaxes(full, 1, 2))
        for M in (1, 63, 64, 65):
            ll, g, hs, inf = obj.loglik_hess_hyper_markov_batch(delays[:M], alpha[:M], rho[:M])
            assert np.array_equal(hs, full[:M]) and np.array_equal(g, fg[:M]) and np.array_equal(ll, fl[:M]) and (inf == 0).all(), M
        perm = np.random.default_rng(1).permutation(1024)
        ll, g, hs, _ = obj.loglik_hess_hyper_markov_batch(delays[perm], alpha[perm], rho[perm])
        assert np.array_equal(hs, full[perm]) and np.array_equal(g, fg[perm]) and np.array_equal(ll, fl[perm])
    for kw in ({"precision": "fp32"}, {"devices": [0, 0]}):
        with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, **kw) as o:
            ll, g, hs, inf = o.loglik_hess_hyper_markov_batch(delays[:65], alpha[:65], rho[:65])
            assert np.array_equal(hs, full[:65]) and np.array_equal(g, fg[:65]) and np.array_equal(ll, fl[:65]) and (inf == 0).all(), kw


def test_refusal_rows_leave_their_neighbours_alone():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    delays, alpha, rho = _batch(2, 8, seed=5)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        gl, gg, good, ginfo = obj.loglik_hess_hyper_markov_batch(delays, alpha, rho)
        assert (ginfo == 0).all()
        a2, r2 = alpha.copy(), rho.copy()
        a2[1, 0] = 0.0
        a2[2, 1] = -1.0
        r2[3] = 0.0
        r2[4] = -2.0
        ll, grad, hess, info = obj.loglik_hess_hyper_markov_batch(delays, a2, r2)
        bad = [1, 2, 3, 4]
        assert list(info[bad]) == [-1, -1, -2, -2]
        assert np.isnan(ll[bad]).all() and np.isnan(grad[bad]).all() and np.isnan(hess[bad]).all()
        keep = [0, 5, 6, 7]
        assert np.array_equal(hess[keep], good[keep]) and np.array_equal(grad[keep], gg[keep]) and np.array_equal(ll[keep], gl[keep])
        assert (info[keep] == 0).all()


def test_refused_requests_and_every_shipped_combination():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loglik_hess_hyper_markov_batch([d0], [[1.0, 1.0]], [2.0])
        assert ei.value.code == UNSUPPORTED and "rbf" in ei.value.message and "gpcc_loglik_hess_hyper_batch" in ei.value.message
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.set_option("laplace_markov", 1)
        assert ei.value.code == UNSUPPORTED
        assert obj.get_option("laplace_markov") == 0
    sizes = [30, 25, 20, 25, 30, 20, 25, 30]
    ran = 0
    for kernel in MC.KERNELS:
        for mb in (True, False):
            for L in range(1, 9):
                tl, yl, sl, dl = MC.lightcurves(sizes[:L], seed=12 + L, kind="ties")
                al = np.linspace(0.6, 1.4, L)
                with gpcc_amd.Objective(tl, yl, sl, KERN[kernel], marginalise_b=mb) as obj:
                    shipped = not (mb and L > 4) and not (kernel == "matern52" and mb and L == 4)   # <3, 4> needs scratch memory
                    if shipped:
                        ll, grad, hess, info = obj.loglik_hess_hyper_markov_batch([dl], [al], [2.0])
                        assert info[0] == 0 and np.isfinite(hess).all() and hess.shape == (1, L + 1, L + 1), (kernel, mb, L)
                        dll, dgrad, dh, _, dinfo = obj.loglik_hess_hyper_batch([dl], [al], [2.0])
                        assert np.max(np.abs(hess - dh)) <= LARGE_BAR * np.max(np.abs(dh)), (kernel, mb, L)
                        ran += 1
                    else:
                        with pytest.raises(gpcc_amd.GpccError) as ei:
                            obj.loglik_hess_hyper_markov_batch([dl], [al], [2.0])
                        assert ei.value.code == UNSUPPORTED and "gpcc_loglik_hess_hyper_batch" in ei.value.message, (kernel, mb, L)
                        assert obj.loglik_hess_hyper_batch([dl], [al], [2.0])[4][0] == 0           # the handle still serves the dense path
    assert ran == 3 * 12 - 1


@pytest.mark.parametrize("N", sorted(GC.LARGE))
def test_large_shapes_against_the_dense_entry(N):
    G = 4
    kernel, data, delays, alpha, rho = GC.large(N, 64)
    rows = [3, 17, 40, 63]
    delays, alpha, rho = delays[rows], alpha[rows], rho[rows]
    with gpcc_amd.Objective(*data, KERN[kernel]) as obj:
        ll, grad, hess, info = obj.loglik_hess_hyper_markov_batch(delays, alpha, rho)
        dl, dgrad, dh, _, dinfo = obj.loglik_hess_hyper_batch(delays, alpha, rho)
    assert (info == 0).all() and (dinfo == 0).all()
    L = len(data[0])
    worst = 0.0
    for g in range(G):
        for name, m in HH.block_masks(L, L + 1).items():
            r = float(np.max(np.abs(hess[g][m] - dh[g][m]))) / float(np.max(np.abs(dh[g][m])))
            worst = max(worst, r)
    print("device Hessian block %s N = %d, %d rows: worst per-block disagreement with loglik_hess_hyper_batch %.3g of max|H| (bar %.0e)"
          % (kernel, N, G, worst, LARGE_BAR))
    assert worst <= LARGE_BAR


def test_n16384_against_central_differences_of_the_gradient():
    """N = 16384, Matern-5/2, 2 rows (no dense fp64 Hessian fits here): every column of the block against central differences of
    loglik_grad_markov_batch with relative steps 1e-5 in alpha and rho, within 1e-5 max|H| -- the step and the bar of the dense
    Hessian's N = 4096 central-difference test; the N^2 workspace is never built."""
    Nl = [8192, 8192]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=3)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    L = 2
    delays = np.array([[0.0, 2.0], [0.0, 6.2]])
    alpha, rho = np.tile(alpha0, (2, 1)), np.full(2, rho0)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        ll, grad, hess, info = obj.loglik_hess_hyper_markov_batch(delays, alpha, rho)
        assert (info == 0).all()
        worst = 0.0
        for g in range(2):
            x0 = np.concatenate([alpha[g], [rho[g]]])
            X = np.repeat(x0[None, :], 2 * (L + 1), 0)
            for i in range(L + 1):
                X[2 * i, i] += 1e-5 * abs(x0[i])
                X[2 * i + 1, i] -= 1e-5 * abs(x0[i])
            _, gf, finfo = obj.loglik_grad_markov_batch(np.tile(delays[g], (len(X), 1)), X[:, :L], X[:, L])
            assert (finfo == 0).all()
            fd = np.stack([(gf[2 * i, :L + 1] - gf[2 * i + 1, :L + 1]) / (X[2 * i, i] - X[2 * i + 1, i]) for i in range(L + 1)], 1)
            err = float(np.max(np.abs(hess[g] - fd))) / float(np.max(np.abs(hess[g])))
            worst = max(worst, err)
            assert err <= 1e-5, (g, hess[g], fd)
        assert obj.get_option("workspace_slots") == obj.get_option("slots_per_stream")     # (never built)
    print("N = 16384 matern52: Hessian block against central differences of the gradient: %.3g of max|H| (bar 1e-5)" % worst)


# ---- the evidence ---------------------------------------------------------------------------------------------------------------
def _tv(a, b):
    return 0.5 * float(np.abs(gpcc_amd.getprobabilities(a) - gpcc_amd.getprobabilities(b)).sum())


def _projected(obj, cand, alpha, rho, rhomin, rhomax):
    """|grad_u l|_inf at (alpha, rho) per delay, the rho component dropped where rho sits on the box and the gradient points out of it"""
    _, grad, _, _, info = obj.loglik_hess_hyper_batch(cand, alpha, rho)
    L = cand.shape[1]
    gu = np.concatenate([alpha, rho[:, None]], 1) * grad[:, :L + 1]
    out = ((rho <= rhomin * (1 + 1e-12)) & (gu[:, L] < 0)) | ((rho >= rhomax * (1 - 1e-12)) & (gu[:, L] > 0))
    gu[out, L] = 0.0
    return np.where(info == 0, np.max(np.abs(gu), 1), np.nan)


def _cond1(kernel, data, delay, alpha, rho):
    band, t, _, Kn = HW._setup(*data, True)
    u = t - delay[band]
    K = alpha[band][:, None] * alpha[band][None, :] * HW.derivatives(kernel, u[:, None] - u[None, :], rho)[0] + Kn
    return float(np.linalg.cond(np.asarray(K, np.float64), 1))


@pytest.mark.parametrize("shape", ["readme", "n1024"])
def test_evidence_markov_against_dense(shape):
    g_tol, rhomin, rhomax = 1e-6, 0.1, 20.0
    if shape == "readme":
        t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
        grid = np.arange(0.0, 20.01, 0.2)
        kernel, iterations = "OU", 1000
    else:
        t, y, s, _ = synthetic.simulate_lightcurves([512, 512], seed=5)
        grid = np.linspace(0.0, 6.0, 16)
        kernel, iterations = "matern32", 200
    cand = np.stack([np.zeros_like(grid), grid], 1)
    G = len(cand)
    with gpcc_amd.Objective(t, y, s, KERN[kernel]) as obj:
        ll0, a0, r0, finfo, _, _ = obj.grid_loglik(cand, iterations, rhomin=rhomin, rhomax=rhomax)
        assert (finfo == 0).all()
        first = obj.laplace_evidence(cand, a0, r0, rhomin=rhomin, rhomax=rhomax, g_tol=g_tol)      # before the option is ever touched
        perm = np.random.default_rng(2).permutation(G)
        again = obj.laplace_evidence(cand[perm], a0[perm], r0[perm], rhomin=rhomin, rhomax=rhomax, g_tol=g_tol)
        assert np.array_equal(again[5], first[5][perm])                 # the dense path decides every delay the same way twice
        mk = obj.laplace_evidence(cand, a0, r0, rhomin=rhomin, rhomax=rhomax, g_tol=g_tol, solver="markov")
        assert obj.get_option("laplace_markov") == 0                    # restored
        after = obj.laplace_evidence(cand, a0, r0, rhomin=rhomin, rhomax=rhomax, g_tol=g_tol)
        for x, z in zip(first[:7], after[:7]):
            assert np.array_equal(np.asarray(x), np.asarray(z), equal_nan=True)     # laplace_markov = 0: the bits of before
        dl, da, dr, dz, dcov, dinfo, drounds, _ = first
        ml, ma, mr, mz, mcov, minfo, mrounds, _ = mk
        differ = np.flatnonzero(dinfo != minfo)
        if len(differ):
            pd, pm = _projected(obj, cand[differ], da[differ], dr[differ], rhomin, rhomax), _projected(obj, cand[differ], ma[differ], mr[differ],
                                                                                                       rhomin, rhomax)
            near = ((pd >= g_tol / 10) & (pd <= 10 * g_tol)) | ((pm >= g_tol / 10) & (pm <= 10 * g_tol))
            assert near.all(), (differ, dinfo[differ], minfo[differ], pd, pm)
        assert len(differ) <= 0.05 * G, (differ, dinfo[differ], minfo[differ])
    both = np.flatnonzero((dinfo == 0) & (minfo == 0))
    assert len(both) >= G // 2
    worst = 0.0
    for g in both:
        bar = 2 * max(1e-6, 64 * EPS * _cond1(kernel, (t, y, s), cand[g], da[g], dr[g]) * abs(dl[g]))
        worst = max(worst, abs(mz[g] - dz[g]) / bar)
        assert abs(mz[g] - dz[g]) <= bar, (g, mz[g], dz[g], bar)
    keep = np.zeros(G, bool)
    keep[both] = True
    tv = _tv(np.where(keep, dz, -np.inf), np.where(keep, mz, -np.inf))
    print("evidence %s (%s, %d delays): %d decided differently, worst |dlogZ| / (2 bars) %.3g, TV of the delay posteriors %.3g (bar 1e-6); "
          "Newton rounds per delay dense %.2f, markov %.2f" % (shape, kernel, G, len(differ), worst, tv, drounds.mean(), mrounds.mean()))
    assert tv <= 1e-6


def test_gpcc_grid_with_the_markov_evidence():
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    cand = np.stack([np.zeros(8), np.linspace(1.0, 4.5, 8)], 1)
    kw = dict(kernel=gpcc_amd.matern32, candidatedelays=cand, iterations=300, evidence="laplace", solver="markov")
    dense = fit.gpcc_grid(t, y, s, **kw)
    none = fit.gpcc_grid(t, y, s, evidence_solver=None, **kw)
    mk = fit.gpcc_grid(t, y, s, evidence_solver="markov", **kw)
    assert np.array_equal(dense.log_evidence, none.log_evidence, equal_nan=True)       # None: as before
    assert np.array_equal(mk.laplace_info, dense.laplace_info) and np.allclose(mk.log_evidence, dense.log_evidence, rtol=0, atol=1e-6,
                                                                               equal_nan=True)
    with pytest.raises(ValueError):
        fit.gpcc_grid(t, y, s, evidence_solver="sparse", **kw)
