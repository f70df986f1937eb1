"""gpcc_loglik_hess_full_noise_markov_batch on the device: the full Hessian over [alpha, rho, tau, kappa, nu] against the
extended-precision reference on the effective error bars and against the numpy mirror (tests/_markov_noise_hess_full_cases.py); the NaN
contract on the OU rows with a cross-band tie; value, info, gradient and the [alpha, rho, kappa, nu] sub-block bitwise the sibling
entries'; every shipped <P, NOFF> and the refused one; rows that do not depend on M, the row order, the launch shape, options and handle
flavours; the unstaged path; one large shape against the dense entry on effective_std and central differences of the gradient entry;
fit.delay_covariance with a noise model on the device and on the mirror.  The references are computed in a pool of CPU processes that
never touch the GPU; the worst error / bar of each group is printed."""
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _hess_highprec as HH
import _markov_cases as MC
import _markov_grad_cases as GC
import _markov_hess_full_cases as FC
import _markov_noise_cases as NC
import _markov_noise_hess_full_cases as NF
import gpcc_amd
from gpcc_amd import _capi, fit, markov, synthetic
from gpcc_amd.api import _dp, _ip
from test_gpu_markov_hess import KERN, LARGE_BAR, UNSUPPORTED
from test_gpu_markov_noise_hess import PROBLEMS, _batch_rows, _cus, _unit_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(12, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


def _slots(L):
    """(the new kernel's pair slots, the block's of the same call)."""
    return 3 * L * L + L + L * (L + 1) // 2, (3 * L + 1) * (3 * L + 2) // 2


def _siblings_bitwise(obj, args, ll, grad, hess, info, L):
    """loglik, grad and info are bitwise loglik_grad_markov_noise_batch's; the sub-block on {0..L, 2L+1..4L} is bitwise
    loglik_hess_markov_noise_batch's."""
    gl, gg, ginfo = obj.loglik_grad_markov_noise_batch(*args)
    assert np.array_equal(ll, gl, equal_nan=True) and np.array_equal(grad, gg, equal_nan=True) and np.array_equal(info, ginfo)
    nl, ng, nh, ninfo = obj.loglik_hess_markov_noise_batch(*args)
    ix = NF.noise_index(L)
    assert np.array_equal(hess[:, ix][:, :, ix], nh, equal_nan=True) and np.array_equal(ng, grad, equal_nan=True) and np.array_equal(ninfo, info)
    assert np.array_equal(hess, np.swapaxes(hess, 1, 2), equal_nan=True)


# ---- parity over the CPU cases -----------------------------------------------------------------------------------------------------
def _batch65(case):
    """65 rows with the case's delays, the case itself the last one: alone in the second wave of its workgroup."""
    cid, k, data, delays, alpha, rho, mb, _, kappa, nu = case
    L = len(alpha)
    rg = np.random.default_rng(len(cid) + L)
    d = np.ascontiguousarray(np.tile(delays, (65, 1)))
    a, r = alpha * rg.uniform(0.8, 1.25, (65, L)), rho * rg.uniform(0.8, 1.25, 65)
    kap, exc = rg.uniform(0.5, 2.0, (65, L)), rg.uniform(0.0, 0.05, (65, L))
    a[64], r[64], kap[64], exc[64] = alpha, rho, kappa, nu
    return d, a, r, kap, exc


@pytest.mark.skipif(not HH.EXTENDED, reason=HH.SKIP_REASON)
@pytest.mark.parametrize("N", NF.SIZES)
def test_parity_cpu_cases(pool, N):
    cases = NF.cases(N)
    ties = [c for c in cases if NF.is_tie(c)]
    held = [c for c in cases if not NF.is_tie(c)]
    assert len(cases) == 72 and len(ties) == 6 and all(c[0].endswith("-ties") and c[1] == "OU" for c in ties)
    refs = dict(zip((c[0] for c in held), pool.map(NF.reference_job, [NF.job(c) for c in held])))
    mirrors = dict(zip((c[0] for c in held), pool.map(NF.mirror_job, held)))
    worst = {b: GC.Worst("device full noise Hessian N = %d block %s (of the case's allowance)" % (N, b)) for b in NF.BLOCKS}
    mirror = GC.Worst("device against mirror N = %d (of 2 bars)" % N)
    print("build: %s" % gpcc_amd.build_info())
    for case in cases:
        cid, k, data, delays, alpha, rho, mb, _, kappa, nu = case
        L = len(alpha)
        args = _batch65(case)
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll, grad, hess, info = obj.loglik_hess_full_markov_noise_batch(*args)
            assert (info == 0).all() and hess.shape == (65, 4 * L + 1, 4 * L + 1), cid
            _siblings_bitwise(obj, args, ll, grad, hess, info, L)
        H = hess[64]
        if NF.is_tie(case):           # the NaN contract: value, gradient and the [alpha, rho, kappa, nu] sub-block finite (and bitwise, above)
            tau = NF.tau_mask(L)
            assert np.isnan(hess[:, tau]).all() and np.isfinite(hess[:, ~tau]).all() and np.isfinite(ll).all() and np.isfinite(grad).all(), cid
            continue
        ref, (ml, mg, mh, minfo) = refs[cid], mirrors[cid]
        assert ref.info == 0 and minfo == 0 and np.isfinite(H).all(), cid
        limit = FC.device_limit(case)
        for b, r in NF.ratios(H, ref, case).items():
            worst[b].add(r / limit, cid)
        mirror.add(NF.worst(NF.ratios(H, ref, case, against=mh)) / 2.0, cid)
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
        rc = _capi.load().gpcc_loglik_hess_full_noise_markov_batch(obj._h, M, _dp(d), _dp(a), _dp(r), _dp(kappa), _dp(nu), _dp(ll), _dp(grad),
                                                                   None, _ip(info))
        assert rc == 0 and obj.get_option("markov_count") - before == M
        assert np.array_equal(ll, gl) and np.array_equal(grad, gg) and np.array_equal(info, ginfo)
        # kappa = nu = NULL: kappa = 1, nu = 0
        h0 = obj.loglik_hess_full_markov_noise_batch(d, a, r)
        h1 = obj.loglik_hess_full_markov_noise_batch(d, a, r, np.ones((M, L)), np.zeros((M, L)))
        for x, z in zip(h0, h1):
            assert np.array_equal(x, z)
        assert _capi.load().gpcc_loglik_hess_full_noise_markov_batch(obj._h, 0, None, None, None, None, None, None, None, None, None) == 0


def test_common_sub_block_and_the_gradient_are_the_siblings_bitwise():
    """Three bands, Matern-5/2 with marginalised offsets (<3, 3>, the largest instantiation) and OU without, 130 rows."""
    for kernel, mb in (("matern52", True), ("OU", False)):
        t, y, s, d0 = MC.lightcurves([40, 40, 30], seed=21, kind="plain")
        M, L = 130, 3
        rg = np.random.default_rng(5)
        d = np.concatenate([np.zeros((M, 1)), rg.uniform(-3.0, 8.0, (M, L - 1))], 1)
        a, r = rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.5), np.log(30.0), M))
        kappa, nu = rg.uniform(0.0, 2.0, (M, L)), rg.uniform(0.001, 0.05, (M, L))
        with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
            before = obj.get_option("markov_count")
            ll, grad, hess, info = obj.loglik_hess_full_markov_noise_batch(d, a, r, kappa, nu)
            assert obj.get_option("markov_count") - before == M and (info == 0).all() and np.isfinite(hess).all()
            _siblings_bitwise(obj, (d, a, r, kappa, nu), ll, grad, hess, info, L)


# ---- every shipped instantiation ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not HH.EXTENDED, reason=HH.SKIP_REASON)
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_every_shipped_instantiation_and_the_refused_one(pool, kernel):
    """<P, NOFF> for NOFF = 0..4 (NOFF = 0: two bands without marginalised offsets), N = 110, 3 rows each with their own (alpha, rho,
    kappa, nu) (test_gpu_markov_noise_hess.py's _unit_case), against the mirror within 2 bars of the row's reference and against the
    reference within its bars; an OU problem whose delays tie keeps the NaN contract in its tau entries and its other blocks are held
    to the bars.  <3, 4> does not ship: GPCC_ERR_UNSUPPORTED before any device work.  The resource table refuses no other
    instantiation (profiles/markov/kernel_resources_noise_hess_tau.log)."""
    p = markov.order(kernel)
    shipped = [noff for noff in range(5) if not (p == 3 and noff == 4)]
    cases = [_unit_case(kernel, noff, row) for noff in shipped for row in range(3)]
    refs = list(pool.map(NF.reference_job, [NF.job(c) for c in cases]))
    mirrors = list(pool.map(NF.mirror_job, cases))
    for noff in range(5):
        rows = [_unit_case(kernel, noff, row) for row in range(3)]
        data, mb = rows[0][2], rows[0][6]
        L = len(rows[0][4])
        d, a, r = np.stack([c[3] for c in rows]), np.stack([c[4] for c in rows]), np.array([c[5] for c in rows])
        kap, exc = np.stack([c[8] for c in rows]), np.stack([c[9] for c in rows])
        with gpcc_amd.Objective(*data, KERN[kernel], marginalise_b=mb) as obj:
            before = obj.get_option("markov_count")
            if noff not in shipped:
                with pytest.raises(gpcc_amd.GpccError) as ei:
                    obj.loglik_hess_full_markov_noise_batch(d, a, r, kap, exc)
                assert ei.value.code == UNSUPPORTED and "effective_std" in ei.value.message and "gpcc_loglik_hess_batch" in ei.value.message
                assert obj.get_option("markov_count") == before
                assert obj.loglik_grad_markov_noise_batch(d, a, r, kap, exc)[2].tolist() == [0, 0, 0]      # the handle still serves the gradient
                continue
            ll, grad, hess, info = obj.loglik_hess_full_markov_noise_batch(d, a, r, kap, exc)
            assert obj.get_option("markov_count") - before == 3 and (info == 0).all()
        worst = GC.Worst("<%d, %d> against the reference" % (p, noff))
        mirror = GC.Worst("<%d, %d> against the mirror (of 2 bars)" % (p, noff))
        for row in range(3):
            i = shipped.index(noff) * 3 + row
            assert refs[i].info == 0 and mirrors[i][3] == 0
            blocks = NF.BLOCKS
            if NF.is_tie(cases[i]):
                tau = NF.tau_mask(L)
                assert np.isnan(hess[row][tau]).all() and np.isnan(mirrors[i][2][tau]).all() and np.isfinite(hess[row][~tau]).all()
                blocks = tuple(b for b in NF.BLOCKS if b not in NF.TAU_BLOCKS)
            else:
                assert np.isfinite(hess[row]).all()
            mh = np.where(np.isnan(mirrors[i][2]), 0.0, mirrors[i][2])
            got = np.where(np.isnan(hess[row]), 0.0, hess[row])
            worst.add(NF.worst(NF.ratios(got, refs[i], cases[i], blocks=blocks)), cases[i][0])
            mirror.add(NF.worst(NF.ratios(got, refs[i], cases[i], against=mh, blocks=blocks)) / 2.0, cases[i][0])
        worst.report()
        mirror.report()


# ---- row independence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,wpw,grid", [(p, w, g) for p in PROBLEMS for (w, g) in ((4, "both"), (2, "both"), (2, "new"))])
def test_rows_do_not_depend_on_the_launch_shape(problem, wpw, grid):
    """grid "both": M chosen for the new slot count plus the block's as the grid's y; "new": for the new kernel's own launch, so that
    it, too, runs with two waves per workgroup (with M chosen for the sum its grid is below one wave per CU)."""
    kernel, Nl, mb = PROBLEMS[problem]
    L, C = len(Nl), _cus()
    ny = sum(_slots(L)) if grid == "both" else _slots(L)[0]
    M = _batch_rows(C, ny, wpw)
    waves = (M + 63) // 64 * ny
    assert waves > 2 * C if wpw == 4 else C < waves <= 2 * C, (M, ny, C)
    t, y, s, _ = MC.lightcurves(Nl, seed=31 + L, kind="plain")
    rg = np.random.default_rng(M + ny)
    delays = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 8.0, (M, L - 1)))], 1)
    alpha, rho = rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))
    kappa, nu = rg.uniform(0.0, 2.0, (M, L)), rg.uniform(0.001, 0.05, (M, L))
    good = kappa[M - 1, L - 1]
    if kernel == "OU":                                                   # tie rows among the M whatever M: a point of band 2 on one of band 1
        for row, (i, j) in ((1, (0, 2)), (M // 2, (3, 1)), (M - 2, (4, 4))):
            delays[row, 1] = t[1][i] - t[0][j]                           # (exact: the times are on the 2^-10 grid)
    tied = FC.tie_rows(t, delays) if kernel == "OU" else np.zeros(M, bool)
    assert tied.sum() >= (3 if kernel == "OU" else 0) and not tied.all() and not tied[M - 1]
    tau = NF.tau_mask(L)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        call = lambda sl: obj.loglik_hess_full_markov_noise_batch(delays[sl], alpha[sl], rho[sl], kappa[sl], nu[sl])
        clean = call(slice(0, M))
        assert (clean[3] == 0).all() and np.isfinite(clean[0]).all() and np.isfinite(clean[1]).all()
        assert np.isfinite(clean[2][~tied]).all() and np.isnan(clean[2][tied][:, tau]).all() and np.isfinite(clean[2][tied][:, ~tau]).all()
        kappa[M - 1, L - 1] = -0.5                                       # the last row fails (-3), alone in the last workgroup
        ll, grad, hess, info = call(slice(0, M))
        assert info[M - 1] == -3 and (info[:M - 1] == 0).all()
        assert np.isnan(ll[M - 1]) and np.isnan(grad[M - 1]).all() and np.isnan(hess[M - 1]).all()
        for x, z in zip((ll, grad, hess), clean[:3]):                    # ... and leaves every other row's bits unchanged
            assert np.array_equal(x[:M - 1], z[:M - 1], equal_nan=True)
        _siblings_bitwise(obj, (delays, alpha, rho, kappa, nu), ll, grad, hess, info, L)

        def same(got, sl):
            return all(np.array_equal(x, z[sl], equal_nan=True) for x, z in zip(got, (ll, grad, hess, info)))

        rpw = 64 * wpw
        nb = (M + rpw - 1) // rpw
        windows = [(0, 1), (0, 63), (0, 64), (0, 65), (M - 65, 64), (M - 1, 1)]
        windows += [(k * rpw - 32, min(64, M - (k * rpw - 32))) for k in sorted({1, nb // 2, nb - 2}) if k >= 1]   # across workgroups' borders
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
            got = o.loglik_hess_full_markov_noise_batch(delays[sl], alpha[sl], rho[sl], kappa[sl], nu[sl])
            assert all(np.array_equal(x, z[sl], equal_nan=True) for x, z in zip(got, clean)), kw


# ---- the unstaged path -------------------------------------------------------------------------------------------------------------
# one pair of each kind present at L = 2, in the order [alpha_1, alpha_2, rho, tau_1, tau_2, kappa_1, kappa_2, nu_1, nu_2]
UNSTAGED_PAIRS = {"at": (0, 4), "rt": (2, 4), "tt diagonal": (4, 4), "tt off": (3, 4), "tau kappa own band": (4, 6), "tau kappa other band": (4, 5),
                  "tau nu": (3, 7)}


@pytest.mark.parametrize("N", [6600, 110])
def test_unstaged_and_staged_against_the_mirror(pool, N):
    """Two bands of N / 2 points, Matern-5/2, two rows that differ in (kappa, nu) alone.  N = 6600: the light curves do not fit the LDS
    beside the lanes' part and come through the caches; N = 110: staged.  Against the numpy mirror restricted (pairs=) to one pair of
    each kind, under test_gpu_markov_noise_hess.py's bar of the same name: the CPU test's formula FACTOR max(e_dense, floor) factor / 16
    with e_dense at its floor and the floor's size |T1| + |T2| + |T3| replaced by its lower bound |H| of the entry from the mirror."""
    rg = np.random.default_rng(N)
    n = N // 2
    t = [np.sort(MC.snap(rg.uniform(0.0, 30.0 * N / 110, n))) for _ in range(2)]
    y = [np.sin(0.4 * tl) + 0.2 * rg.standard_normal(n) for tl in t]
    s = [0.2 + 0.05 * rg.random(n) for _ in range(2)]
    alpha0, rho0, d0 = np.array([1.3, 0.9]), 2.5, np.array([0.0, 1.0 + 1.0 / 3.0])
    kappa, nu = np.array([[0.6, 1.4], [1.7, 0.0]]), np.array([[0.004, 0.02], [0.03, 0.05]])
    d, a, r = np.tile(d0, (2, 1)), np.tile(alpha0, (2, 1)), np.full(2, rho0)
    jobs = [(("row%d" % m, "matern52", (t, y, s), d[m], a[m], r[m], True, N, kappa[m], nu[m]), None, [pair]) for m in range(2)
            for pair in UNSTAGED_PAIRS.values()]
    host = list(pool.map(NF.slip_job, jobs))
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        ll, grad, hess, info = obj.loglik_hess_full_markov_noise_batch(d, a, r, kappa, nu)
        _siblings_bitwise(obj, (d, a, r, kappa, nu), ll, grad, hess, info, 2)
    assert (info == 0).all() and np.isfinite(hess).all()
    k = 0
    for m in range(2):
        factor = MC.factor(alpha0, NC.effective(s, kappa[m], nu[m]))
        for name, (i, j) in UNSTAGED_PAIRS.items():
            hl, hg, hh, hinfo = host[k]
            k += 1
            assert hinfo == 0 and np.isfinite(hh[i, j])
            bar = MC.FACTOR * N * 2.0 ** -53 * abs(hh[i, j]) * factor / MC.FACTOR
            err = abs(hess[m][i, j] - hh[i, j])
            print("N = %d row %d pair %s: %.3g of its bar" % (N, m, name, err / bar if bar > 0 else err))
            assert err <= bar, (N, m, name, err, bar)


# ---- one large shape ---------------------------------------------------------------------------------------------------------------
def test_large_shape_against_dense_and_central_differences():
    """Matern-3/2, three ragged bands, N = 4095, 4 rows with their own kappa and nu.  The [alpha, rho, tau] block: a fresh handle's dense
    loglik_hess_batch on effective_std, per block within LARGE_BAR of max|H_dense|, what tests/test_gpu_markov_hess_full.py holds the
    plain rows to at this shape.  The (tau, kappa) and (tau, nu) entries: five-point central differences of
    loglik_grad_markov_noise_batch's tau entries in kappa and nu with relative steps 2e-3 and 1e-3; the tolerance is twice the largest
    change of the scheme's result over the row between the two steps (the truncation of the coarser step, 16 times the finer one's, and
    the rounding of both); nothing of it comes from the entry under test."""
    G, N, L = 4, 4095, 3
    kernel, (t, y, s), delays, alpha, rho = GC.large(N, G)
    rg = np.random.default_rng(12)
    kappa, nu = rg.uniform(0.5, 2.0, (G, L)), rg.uniform(0.2, 1.0, (G, L)) * np.array([np.mean(a ** 2) for a in s])
    W = 2 * L + 1
    with gpcc_amd.Objective(t, y, s, KERN[kernel]) as obj:
        ll, grad, hess, info = obj.loglik_hess_full_markov_noise_batch(delays, alpha, rho, kappa, nu)
        assert (info == 0).all() and np.array_equal(hess, np.swapaxes(hess, 1, 2)) and np.isfinite(hess).all()

        def scheme(h):
            fd = np.empty((G, L, 2 * L))
            for c in range(2 * L):
                e = np.zeros((G, 2 * L))
                e[:, c] = h * np.concatenate([kappa, nu], 1)[:, c]
                f = [obj.loglik_grad_markov_noise_batch(delays, alpha, rho, kappa + q * e[:, :L], nu + q * e[:, L:])[1][:, L + 1:W] for q in (1, -1, 2, -2)]
                fd[:, :, c] = (8 * (f[0] - f[1]) - (f[2] - f[3])) / (12 * e[:, c])[:, None]
            return fd

        coarse, fine = scheme(2e-3), scheme(1e-3)
    worst_d, worst_n = 0.0, 0.0
    for g in range(G):
        eff = fit.effective_std(s, kappa[g], nu[g])
        with gpcc_amd.Objective(t, y, eff, KERN[kernel]) as fresh:
            dl, dgrad, dh, _, dinfo = fresh.loglik_hess_batch(delays[g:g + 1], alpha[g:g + 1], rho[g:g + 1])
        assert dinfo[0] == 0
        for name, m in HH.block_masks(L).items():
            rr = float(np.max(np.abs(hess[g][:W, :W][m] - dh[0][m]))) / float(np.max(np.abs(dh[0][m])))
            worst_d = max(worst_d, rr)
            print("row %d block %s against the dense entry on effective_std: %.3g of max|H|" % (g, name, rr))
            assert rr <= LARGE_BAR, (g, name, rr)
        got = hess[g][L + 1:W, W:]
        size = float(np.max(np.abs(fine[g])))
        tol = 2.0 * float(np.max(np.abs(coarse[g] - fine[g])))
        err = float(np.max(np.abs(got - fine[g])))
        worst_n = max(worst_n, err / size)
        print("row %d: (tau, noise) entries against central differences %.3g of max|H_tn| (tolerance %.3g)" % (g, err / size, tol / size))
        assert err <= tol, (g, err, tol)
    print("N = %d %s: [alpha, rho, tau] block against the dense entry on effective_std %.3g of max|H| (bar %.0e); (tau, noise) entries "
          "against central differences %.3g of max|H_tn|" % (N, kernel, worst_d, LARGE_BAR, worst_n))


# ---- the delay's covariance --------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not HH.EXTENDED, reason=HH.SKIP_REASON)
def test_delay_covariance_with_a_noise_model_on_the_device():
    """README-size data at (README_DELAYS, README_MODE["matern32"]), kappa = 1.2 free, nu = 0.01 fixed: fit.delay_covariance on Objective
    against the same call on MarkovObjective.  PROPAGATION: device (allowance 1 bar at this rho) and mirror (1 bar) are each within
    their bars of the reference per block, so their Hessians differ entrywise by at most E = 2 bar_B / scale, B the entry's block (tt
    and tn among them); cov = (-H_ff)^-1 then differs entrywise by at most inverse_bound(cov, E) = 2 |cov| E |cov|."""
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    alpha, rho = NF.README_MODE["matern32"]
    delays, alpha = np.array(NF.README_DELAYS), np.array(alpha)
    kappa, nu = np.array([1.2, 1.2]), np.array([0.01, 0.01])
    case = ("readme-matern32", "matern32", (t, y, s), delays, alpha, rho, True, 110, kappa, nu)
    ref = NF.reference_job(NF.job(case))
    assert ref.info == 0 and FC.device_limit(case) == 1.0
    kw = dict(solver="markov", kappa=kappa, nu=nu, noise_free=[True, True, False, False])
    host, hok = fit.delay_covariance(markov.MarkovObjective(t, y, s, "matern32"), delays, alpha, rho, **kw)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        before = obj.get_option("markov_count")
        dev, dok = fit.delay_covariance(obj, delays, alpha, rho, **kw)
        assert obj.get_option("markov_count") - before == 1
        fixed, fok = fit.delay_covariance(obj, delays, alpha, rho, solver="markov", kappa=kappa, nu=nu, noise_free=[False] * 4)
        with pytest.raises(ValueError):
            fit.delay_covariance(obj, delays, alpha, rho, solver="dense", kappa=kappa, nu=nu)
    assert hok and dok and fok and dev.shape == (6, 6) == host.shape
    free = [0, 1, 2, 4, 5, 6]
    bound = NF.inverse_bound(host, NF.entry_bars(ref, case, 2.0)[np.ix_(free, free)])
    print("delay_covariance with kappa free, device against mirror: largest |dcov| / bound %.3g; sd(tau_2) %.6g (noise fixed: %.6g)"
          % (float(np.max(np.abs(dev - host) / bound)), np.sqrt(dev[3, 3]), np.sqrt(fixed[3, 3])))
    assert np.all(np.abs(dev - host) <= bound)
    assert dev[3, 3] >= fixed[3, 3] * (1.0 - 64 * 2.0 ** -53 * np.linalg.cond(dev))
