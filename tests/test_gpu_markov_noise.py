"""gpcc_loglik_noise_markov_batch and gpcc_loglik_grad_noise_markov_batch on the device: value and all 4L+1 gradient
entries against the extended-precision reference on the effective error bars (tests/_markov_noise_cases.py); the contract -- a row's
value is a fresh handle's on effective_std; bitwise gpcc_loglik_markov_batch at kappa = 1, nu = 0 in every shipped <P, NOFF>; rows that
do not depend on the launch shape, M, the row order and options; the unstaged path; codes, refusals and edges; one large shape against
the dense entries and central differences; fit.gpcc_grid_noise.  The references are computed in a pool of CPU processes that never
touch the GPU; the worst error / bar of each group is printed."""
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _grad_highprec as H
import _markov_cases as MC
import _markov_grad_cases as GC
import _markov_noise_cases as NC
import gpcc_amd
from gpcc_amd import fit, markov

pytestmark = pytest.mark.gpu

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
UNSUPPORTED = -3


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


# ---- 6. parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)
@pytest.mark.parametrize("N", [110, 150, 767])
def test_parity_cpu_cases(oracle, pool, N):
    cases = NC.cases(N)
    assert len(cases) == (72 if N != 767 else 12)
    refs = pool.map(NC.reference_job, [NC.job(c) for c in cases])
    worst = {g: GC.Worst("device %s N = %d" % (g, N)) for g in ("value", "alpha rho tau", "kappa nu")}
    print("build: %s" % gpcc_amd.build_info())
    for case, reference in zip(cases, refs):
        cid, k, data, delays, alpha, rho, mb, _, kappa, nu = case
        assert reference[0].info == 0, cid
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll, grad, info = obj.loglik_grad_markov_noise_batch(delays[None, :], alpha[None, :], [rho], kappa, nu)
            vl, vinfo = obj.loglik_markov_noise_batch(delays[None, :], alpha[None, :], [rho], kappa[None, :], nu[None, :])
        assert info[0] == 0 and vinfo[0] == 0 and vl[0] == ll[0] and grad.shape == (1, 4 * len(alpha) + 1), cid
        rv, rg, rn = NC.ratios(ll[0], grad[0], oracle, case, reference)
        worst["value"].add(rv, cid)
        worst["alpha rho tau"].add(rg, cid)
        worst["kappa nu"].add(rn, cid)
    for w in worst.values():
        w.report()


# ---- 7. the contract -----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_value_is_a_fresh_handles_on_effective_std(oracle, pool, kernel):
    cases = [c for c in NC.cases(110) if c[1] == kernel][1::9][:3]
    assert len(cases) == 3
    refs = pool.map(NC.reference_job, [NC.job(c) for c in cases])
    for case, (ref, _, _) in zip(cases, refs):
        cid, k, (t, y, s), delays, alpha, rho, mb, N, kappa, nu = case
        b, e = NC.value_bar(oracle, case, ref)
        with gpcc_amd.Objective(t, y, s, KERN[k], marginalise_b=mb) as obj:
            ll, info = obj.loglik_markov_noise_batch([delays], [alpha], [rho], kappa, nu)
        with gpcc_amd.Objective(t, y, fit.effective_std(s, kappa, nu), KERN[k], marginalise_b=mb) as fresh:
            fl, finfo = fresh.loglik_markov_batch([delays], [alpha], [rho])
            dl, dinfo = fresh.loglik_batch([delays], [alpha], [rho])
        assert info[0] == 0 and finfo[0] == 0 and dinfo[0] == 0, cid
        print("%s: against the fresh handle's filter %.3g, its dense value %.3g (bar %.3g, e_dense %.3g)"
              % (cid, abs(ll[0] - fl[0]) / abs(ref.loglik), abs(ll[0] - dl[0]) / abs(ref.loglik), b, e))
        assert abs(ll[0] - fl[0]) <= b * abs(ref.loglik), cid
        assert abs(ll[0] - dl[0]) <= (b + e) * abs(ref.loglik), cid


# ---- 8. bitwise at kappa = 1, nu = 0 ---------------------------------------------------------------------------------------------
def _batch(L, M, seed):
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 45.0, (M, L - 1)))], 1)
    return delays, rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))


def _unit_problem(kernel, noff):
    """<P, NOFF> = <order of the kernel, noff>: noff bands with marginalised offsets, or two bands without; 130 rows, refused and
    failing ones among them.  -> (data, delays, alpha, rho, loglik_markov_batch's, loglik_grad_markov_batch's, the noise value entry's
    three ways, the noise gradient entry's with None and with explicit arrays)."""
    Nl = [13, 11, 9, 8][:noff] if noff else [13, 11]
    L, M = len(Nl), 130
    t, y, s, _ = MC.lightcurves(Nl, seed=40 + noff, kind="ties" if L > 1 else "plain")
    delays, alpha, rho = _batch(L, M, seed=noff)
    alpha[5, L - 1] = 0.0
    rho[70] = -1.0
    rho[99] = np.nan
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=noff > 0) as obj:
        plain = obj.loglik_markov_batch(delays, alpha, rho)
        pgrad = obj.loglik_grad_markov_batch(delays, alpha, rho)
        values = [obj.loglik_markov_noise_batch(delays, alpha, rho, np.ones((M, L)), np.zeros((M, L))),
                  obj.loglik_markov_noise_batch(delays, alpha, rho), obj.loglik_markov_noise_batch(delays, alpha, rho, np.ones(L), None)]
        grads = [obj.loglik_grad_markov_noise_batch(delays, alpha, rho),
                 obj.loglik_grad_markov_noise_batch(delays, alpha, rho, np.ones((M, L)), np.zeros((M, L)))]
    return (t, y, s), delays, alpha, rho, plain, pgrad, values, grads


@pytest.mark.parametrize("noff", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_unit_noise_is_bitwise_the_plain_entry(kernel, noff):
    """Value and info at kappa = 1, nu = 0, explicit arrays and None: np.array_equal to loglik_markov_batch's."""
    _, delays, alpha, rho, (pl, pinfo), _, values, grads = _unit_problem(kernel, noff)
    M, L = alpha.shape
    assert list(pinfo[[5, 70]]) == [-1, -2] and pinfo[99] != 0 and (np.delete(pinfo, [5, 70, 99]) == 0).all()
    for ll, info in values + [(gl, ginfo) for gl, _, ginfo in grads]:
        assert np.array_equal(ll, pl, equal_nan=True) and np.array_equal(info, pinfo)
    g, g2 = grads[0][1], grads[1][1]
    assert np.array_equal(g, g2, equal_nan=True) and g.shape == (M, 4 * L + 1)
    bad = pinfo != 0
    assert np.isnan(g[bad]).all() and np.isfinite(g[~bad]).all()


@pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)
@pytest.mark.parametrize("noff", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_unit_noise_gradient_is_the_plain_gradient(pool, kernel, noff):
    """The first 2L+1 gradient entries at kappa = 1, nu = 0 against loglik_grad_markov_batch's (gpcc_markov_grad's walk on the same
    variance): within _grad_highprec.bar of the row's extended-precision reference on every row that did not fail; whether they
    are bitwise is printed."""
    data, delays, alpha, rho, (pl, pinfo), (_, pg, _), _, grads = _unit_problem(kernel, noff)
    L = alpha.shape[1]
    g = grads[0][1][:, :2 * L + 1]
    good = np.flatnonzero(pinfo == 0)
    assert len(good) == 127
    refs = list(pool.map(H.evaluate_job, [(kernel, *data, delays[m], alpha[m], rho[m], noff > 0) for m in good]))
    worst = GC.Worst("<%d, %d>: noise gradient against the plain gradient" % (markov.order(kernel), noff))
    for m, ref in zip(good, refs):
        assert ref.info == 0, m
        worst.add(float(np.max(np.abs(g[m] - pg[m]))) / H.bar(ref), int(m))
    worst.report()
    print("<%d, %d>: the first 2L+1 gradient entries at kappa = 1, nu = 0 are %sbitwise gpcc_loglik_grad_markov_batch's"
          % (markov.order(kernel), noff, "" if np.array_equal(g, pg, equal_nan=True) else "NOT "))


# ---- 9. launch shapes ------------------------------------------------------------------------------------------------------------
PROBLEMS = {"matern32-b": ("matern32", [7, 5], True), "OU-fixed": ("OU", [6, 5, 4], False)}     # test_gpu_markov_launch_shapes.py's


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _batch_rows(C, ny, waves_per_workgroup):
    """M with a ragged last workgroup of one row: four waves per workgroup: 128 C + 1; two: ceil(M / 64) ny between C and 2 C."""
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
    ny = 2 * L + 1 + (2 * L if kernel == "OU" else L) + L                # the gradient kernel's slots: its grid's y
    M = _batch_rows(C, ny, wpw)
    waves = (M + 63) // 64 * ny
    assert waves > 2 * C if wpw == 4 else C < waves <= 2 * C, (M, ny, C)
    t, y, s, _ = MC.lightcurves(Nl, seed=31 + L, kind="plain")
    rg = np.random.default_rng(M + ny)
    delays = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 8.0, (M, L - 1)))], 1)
    alpha, rho = rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))
    kappa, nu = rg.uniform(0.0, 2.0, (M, L)), rg.uniform(0.001, 0.05, (M, L))
    kappa[M - 1, L - 1] = -0.5                                           # the last row fails (-3), alone in the last workgroup
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        call = lambda sl: obj.loglik_grad_markov_noise_batch(delays[sl], alpha[sl], rho[sl], kappa[sl], nu[sl])
        ll, grad, info = call(slice(0, M))
        vl, vinfo = obj.loglik_markov_noise_batch(delays, alpha, rho, kappa, nu)
        assert info[M - 1] == -3 and (info[:M - 1] == 0).all() and np.array_equal(info, vinfo) and np.array_equal(ll, vl, equal_nan=True)
        assert np.isnan(ll[M - 1]) and np.isnan(grad[M - 1]).all() and np.isfinite(grad[:M - 1]).all()
        rpw = 64 * wpw
        nb = (M + rpw - 1) // rpw
        windows = [(0, 64), (M - 65, 64), (M - 1, 1)] + [(k * rpw - 32, 64) for k in sorted({1, nb // 2, nb - 2})]
        assert all(0 <= r0 and r0 + n <= M for r0, n in windows) and M % rpw == 1
        for r0, n in windows:                                            # calls of <= 64 rows: one wave, one workgroup along x
            sl = slice(r0, r0 + n)
            sll, sg, sinfo = call(sl)
            svl, svinfo = obj.loglik_markov_noise_batch(delays[sl], alpha[sl], rho[sl], kappa[sl], nu[sl])
            assert np.array_equal(sll, ll[sl], equal_nan=True) and np.array_equal(sg, grad[sl], equal_nan=True), (problem, M, r0)
            assert np.array_equal(sinfo, info[sl]) and np.array_equal(svl, ll[sl], equal_nan=True) and np.array_equal(svinfo, info[sl])
        perm = np.random.default_rng(1).permutation(M)                   # the row order
        pll, pg, pinfo = call(perm)
        assert np.array_equal(pll, ll[perm], equal_nan=True) and np.array_equal(pg, grad[perm], equal_nan=True) and np.array_equal(pinfo, info[perm])
        obj.set_option("markov_chunk_rows", 64)                          # ... and the option
        try:
            cll, cg, cinfo = call(slice(0, M))
        finally:
            obj.set_option("markov_chunk_rows", 0)
        assert np.array_equal(cll, ll, equal_nan=True) and np.array_equal(cg, grad, equal_nan=True) and np.array_equal(cinfo, info)


# ---- 10. the unstaged path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [6600, 110])
def test_unstaged_and_staged_against_the_mirror(N):
    """One band, Matern-5/2, three rows that differ in (kappa, nu) alone.  N = 6600: 24 N + 44 x 64 bytes exceed the 156 KiB a
    workgroup may take, so the light curves come through the caches (the plain entry's 24 N + 28 x 64 exceed it too); N = 110: staged.
    Against the numpy mirror -- the same algorithm in another rounding order -- at the value's bar with e_dense at its floor,
    F N 2^-53 (the dense reference is too slow at N = 6600), and at the gradient's bar max(1e-11, 64 eps cond_1(K)) max(1, max|g|)
    with cond_1 of the fp64 K of the row with the smallest variances (K = A + D, A fixed and D >= 0 diagonal: the smallest D has the
    largest |K^-1|)."""
    rg = np.random.default_rng(N)
    t = [np.sort(MC.snap(rg.uniform(0.0, 30.0 * N / 110, N)))]
    y = [np.sin(0.4 * t[0]) + 0.2 * rg.standard_normal(N)]
    s = [0.2 + 0.05 * rg.random(N)]
    alpha0, rho0 = 1.3, 2.5
    kappa, nu = np.array([[0.6], [1.7], [0.0]]), np.array([[0.004], [0.03], [0.05]])
    d, a, r = np.zeros((3, 1)), np.full((3, 1), alpha0), np.full(3, rho0)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        ll, grad, info = obj.loglik_grad_markov_noise_batch(d, a, r, kappa, nu)
        vl, vinfo = obj.loglik_markov_noise_batch(d, a, r, kappa, nu)
    assert (info == 0).all() and np.array_equal(vl, ll) and np.array_equal(vinfo, info)
    hl, hg, hinfo = markov.loglik_grad_noise_batch("matern52", t, y, s, d, a, r, kappa, nu)
    assert (hinfo == 0).all()
    x = np.sqrt(5.0) * np.abs(t[0][:, None] - t[0][None, :]) / rho0
    K = alpha0 ** 2 * (1.0 + x + x * x / 3.0) * np.exp(-x) + 100.0 * np.var(y[0], ddof=1)
    K[np.diag_indices(N)] += 0.6 ** 2 * s[0] ** 2 + 0.004
    cond = float(np.linalg.cond(K, 1))
    for m in range(3):
        vbar = MC.bar(0.0, N, MC.factor([alpha0], NC.effective(s, kappa[m], nu[m])))
        gbar = max(1e-11, 64 * H.EPS64 * cond) * max(1.0, float(np.max(np.abs(hg[m]))))
        ev, eg = abs(ll[m] - hl[m]) / abs(hl[m]), float(np.max(np.abs(grad[m] - hg[m])))
        print("N = %d row %d: value %.3g of its bar, gradient %.3g of its bar (cond_1 %.3g)" % (N, m, ev / vbar, eg / gbar, cond))
        assert ev <= vbar and eg <= gbar, (N, m, ev, vbar, eg, gbar)


# ---- 11. edges -------------------------------------------------------------------------------------------------------------------
def test_codes_refusals_and_edges():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    M = 9
    rg = np.random.default_rng(5)
    d, a, r = np.tile(d0, (M, 1)), rg.uniform(0.4, 2.0, (M, 2)), np.exp(rg.uniform(np.log(0.5), np.log(30.0), M))
    kappa, nu = rg.uniform(0.5, 2.0, (M, 2)), rg.uniform(0.0, 0.05, (M, 2))
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        for call in (obj.loglik_markov_noise_batch, obj.loglik_grad_markov_noise_batch):
            with pytest.raises(gpcc_amd.GpccError) as ei:
                call(d, a, r, kappa, nu)
            assert ei.value.code == UNSUPPORTED and "rbf" in ei.value.message
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        good, gg, ginfo = obj.loglik_grad_markov_noise_batch(d, a, r, kappa, nu)
        assert (ginfo == 0).all() and np.isfinite(gg).all()
        a2, r2, k2, v2 = a.copy(), r.copy(), kappa.copy(), nu.copy()
        a2[1, 0] = 0.0          # -1
        k2[1, 1] = -1.0         # ... before -3
        r2[2] = 0.0             # -2
        v2[2, 0] = -0.5         # ... before -3
        k2[3, 0] = -1e-300      # -3
        v2[4, 1] = -1e-300      # -3
        k2[5, 1] = np.nan       # -3
        v2[6, 0] = np.inf       # -3
        k2[7, 0] = np.inf       # -3
        ll, g, info = obj.loglik_grad_markov_noise_batch(d, a2, r2, k2, v2)
        vl, vinfo = obj.loglik_markov_noise_batch(d, a2, r2, k2, v2)
        hl, hinfo = markov.loglik_noise_batch("matern32", t, y, s, d, a2, r2, k2, v2)
        assert list(info) == [0, -1, -2, -3, -3, -3, -3, -3, 0] and np.array_equal(info, vinfo) and np.array_equal(info, hinfo)
        assert np.isnan(ll[1:8]).all() and np.isnan(g[1:8]).all() and np.isnan(vl[1:8]).all()
        for m in (0, 8):        # the neighbouring rows are untouched
            assert ll[m] == good[m] == vl[m] and np.array_equal(g[m], gg[m])
        with pytest.raises(ValueError):
            obj.loglik_markov_noise_batch(d, a, r, np.ones((M, 3)), None)
        pl, pinfo = obj.loglik_markov_batch(d, a, r)                     # the handle still serves the plain entry
        assert (pinfo == 0).all() and np.array_equal(pl, obj.loglik_markov_noise_batch(d, a, r)[0])
    # five bands: with marginalised offsets unsupported, without them the entry works
    t5, y5, s5, d5 = MC.lightcurves([30, 25, 20, 25, 30], seed=12, kind="ties")
    a5, k5, v5 = np.linspace(0.6, 1.4, 5), np.linspace(0.5, 1.5, 5), np.linspace(0.0, 0.02, 5)
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=True) as obj:
        for call in (obj.loglik_markov_noise_batch, obj.loglik_grad_markov_noise_batch):
            with pytest.raises(gpcc_amd.GpccError) as ei:
                call([d5], [a5], [2.0], k5, v5)
            assert ei.value.code == UNSUPPORTED
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=False) as obj:
        ll, g, info = obj.loglik_grad_markov_noise_batch([d5], [a5], [2.0], k5, v5)
        hl, hg, hinfo = markov.loglik_grad_noise("OU", t5, y5, s5, d5, a5, 2.0, k5, v5, False)
        assert info[0] == 0 and hinfo == 0 and g.shape == (1, 21)
        assert abs(ll[0] - hl) <= MC.bar(0.0, 130, MC.factor(a5, NC.effective(s5, k5, v5))) * abs(hl)
        if H.EXTENDED:
            ref, gk, gv = NC.reference_job(("OU", t5, y5, NC.effective(s5, k5, v5), d5, a5, 2.0, False, s5, k5))
            assert H.ratio(g[0, :11], ref) <= 1.0
            assert float(np.max(np.abs(g[0, 11:] - np.concatenate([gk, gv])))) <= NC.noise_bar(ref, gk, gv)
    # kappa = 0, nu = 0: no noise at all; two observations that tie in shifted time: the second one's predictive variance is 0
    # (tests/test_gpu_markov.py's construction with sigma = 0; here every point is noiseless, so the data holds exactly one tie, a
    # sixteenth after the point before it: the variance left by the first of the pair, at most 2^-52 (1 - exp(-1/16)), vanishes
    # against Pinf = 1 in the propagation over the zero lag)
    t, y, s, d0 = MC.lightcurves([30, 20], seed=5, kind="plain")
    t[0][10] = t[0][9] + 2.0 ** -4
    t[1][np.argsort(t[1])[7]] = t[0][10] + d0[1]
    ts = markov.prepare(t, y, s)[0]
    seq = markov.merge_order(ts, d0)
    sh = [ts[b][i] - d0[b] for b, i in seq]
    tied = [j for j in range(1, len(seq)) if sh[j] == sh[j - 1]]
    assert len(tied) == 1 and sh[tied[0] - 1] - sh[tied[0] - 2] == 2.0 ** -4 and seq[tied[0]][0] == 1
    j = tied[0]
    host = markov.loglik_noise("OU", t, y, s, d0, [1.0, 1.0], 2.0, [0.0, 0.0], [0.0, 0.0], False)
    assert host[1] == j + 1
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU, marginalise_b=False) as obj:
        ll, g, info = obj.loglik_grad_markov_noise_batch([d0, d0], [[1.0, 1.0]] * 2, [2.0, 2.0], [[0.0, 0.0], [0.0, 1.0]], [[0.0, 0.0], [0.01, 0.0]])
        assert info[0] == j + 1 and np.isnan(ll[0]) and np.isnan(g[0]).all()
        assert info[1] == 0 and np.isfinite(ll[1]) and np.isfinite(g[1]).all()      # its neighbour, with noise, is fine


# ---- 12. one large shape ---------------------------------------------------------------------------------------------------------
def test_large_shape_against_dense_and_central_differences():
    """Matern-3/2, three ragged bands, N = 4095, three rows with their own kappa and nu.  Value: a fresh handle's dense loglik_batch per
    row, under the value's bar, e_dense being the disagreement of that value with oracle/lapack_baseline.py's
    (as tests/test_gpu_markov.py::test_parity_large measures it).  First 2L+1 gradient entries: that handle's dense loglik_grad_batch within
    WITNESS_BAR of max|g|.  Noise entries: five-point central differences of the new value entry, relative step 1e-4."""
    G, N = 3, 4095
    kernel, (t, y, s), delays, alpha, rho = GC.large(N, G)
    L = 3
    rg = np.random.default_rng(12)
    kappa, nu = rg.uniform(0.5, 2.0, (G, L)), rg.uniform(0.2, 1.0, (G, L)) * np.array([np.mean(a ** 2) for a in s])
    h = 1e-4
    with gpcc_amd.Objective(t, y, s, KERN[kernel]) as obj:
        ll, grad, info = obj.loglik_grad_markov_noise_batch(delays, alpha, rho, kappa, nu)
        assert (info == 0).all()
        fd = np.empty((G, 2 * L))
        for c in range(2 * L):
            e = np.zeros((G, 2 * L))
            e[:, c] = h * np.concatenate([kappa, nu], 1)[:, c]
            f = [obj.loglik_markov_noise_batch(delays, alpha, rho, kappa + q * e[:, :L], nu + q * e[:, L:])[0] for q in (1, -1, 2, -2)]
            fd[:, c] = (8 * (f[0] - f[1]) - (f[2] - f[3])) / (12 * e[:, c])
    worst = MC.Worst("device value %s N = %d against a fresh handle's dense value" % (kernel, N))
    for g in range(G):
        eff = fit.effective_std(s, kappa[g], nu[g])
        with gpcc_amd.Objective(t, y, eff, KERN[kernel]) as fresh:
            dl, dg, dinfo = fresh.loglik_grad_batch(delays[g:g + 1], alpha[g:g + 1], rho[g:g + 1])
        assert dinfo[0] == 0
        e = MC.dense_pair_error(kernel, (t, y, eff), delays[g], alpha[g], rho[g], True, dl[0])
        worst.add(abs(ll[g] - dl[0]) / abs(dl[0]), MC.bar(e, N, MC.factor(alpha[g], eff)), g)
        scale = float(np.max(np.abs(dg[0])))
        err = float(np.max(np.abs(grad[g, :2 * L + 1] - dg[0]))) / scale
        nscale = float(np.max(np.abs(grad[g, 2 * L + 1:])))
        nerr = float(np.max(np.abs(grad[g, 2 * L + 1:] - fd[g]))) / nscale
        print("row %d: alpha, rho, tau against the dense gradient %.3g of max|g| (bar %.0e); kappa, nu against central differences %.3g of "
              "max|g_noise| (bar 1e-6)" % (g, err, GC.WITNESS_BAR, nerr))
        assert err <= GC.WITNESS_BAR and nerr <= 1e-6, (g, grad[g], dg[0], fd[g])
    worst.report()


# ---- 13. the fit -----------------------------------------------------------------------------------------------------------------
def test_grid_noise_on_the_device_and_on_the_mirror(oracle):
    """README-size data, 5 delays, 30 iterations, warm start, on Objective and on MarkovObjective.  The criterion is that of
    tests/test_gpu_markov.py::test_fit_with_markov_solver: the fit's value against a reference value AT THE FITTED POINT under the
    value's bar plus e_dense (two optimiser trajectories in two rounding orders are not compared point by point), and the same most
    probable delay."""
    from gpcc_amd import synthetic
    t, y, s, _ = synthetic.simulate_lightcurves((55, 55))
    cand = np.stack([np.zeros(5), np.array([1.0, 1.6, 2.0, 2.4, 3.0])], 1)
    a0, r0 = synthetic.default_hyperparameters(y)
    kw = dict(iterations=30, noise="scale", shared=True, start=(np.tile(a0, (5, 1)), np.full(5, min(r0, 19.0))))
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        before = obj.get_option("markov_count")
        dev = fit.gpcc_grid_noise(obj, cand, **kw)
        assert obj.get_option("markov_count") - before == dev.f_calls + 5
    host = fit.gpcc_grid_noise(markov.MarkovObjective(t, y, s, "OU"), cand, **kw)
    assert (dev.loglikel >= dev.start_loglikel).all() and (host.loglikel >= host.start_loglikel).all()
    worst = MC.Worst("noise fit: reference value at the device's fitted point")
    for g in range(5):
        eff = fit.effective_std(s, dev.kappa[g], dev.nu[g])
        d, dinfo = oracle.loglik_batch("OU", t, y, eff, cand[g][None, :], dev.alpha[g][None, :], [dev.rho[g]], True)
        assert dinfo[0] == 0
        if H.EXTENDED:
            ref = H.evaluate("OU", t, y, eff, cand[g], dev.alpha[g], dev.rho[g], True, value_only=True).loglik
            e = abs(d[0] - ref) / abs(ref)
        else:
            e = MC.dense_pair_error("OU", (t, y, eff), cand[g], dev.alpha[g], dev.rho[g], True, d[0])
        worst.add(abs(dev.loglikel[g] - d[0]) / abs(d[0]), MC.bar(e, 110, MC.factor(dev.alpha[g], eff)) + e, g)
    worst.report()
    print("fitted kappa: device %s, mirror %s; loglikel device %s, mirror %s" % (np.round(dev.kappa[:, 0], 4), np.round(host.kappa[:, 0], 4),
                                                                                np.round(dev.loglikel, 4), np.round(host.loglikel, 4)))
    assert int(np.argmax(dev.loglikel)) == int(np.argmax(host.loglikel))
    assert np.allclose(dev.kappa, host.kappa, rtol=1e-2, atol=0.0)       # coarse: the two trajectories run in two rounding orders
