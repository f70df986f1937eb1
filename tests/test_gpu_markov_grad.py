"""gpcc_loglik_grad_markov_batch on the device: the gradient against the extended-precision reference over the CPU cases of
tests/_markov_cases.py under the dense gradient's own bar (tests/_grad_highprec.bar) and against the numpy mirror, against the fp64 torch
witness at N = 2048, 4095 and 4096; value and info bitwise gpcc_loglik_markov_batch's; bitwise invariance over batch sizes, row order,
options and handle flavours; refusals and failures; the memory of a handle that only calls this entry; N = 16384 against central
differences; value_and_grad(solver="markov"); the quasi-Newton fit.  The references are computed in a pool of CPU processes that never
touch the GPU; the worst error / bar of each group is printed."""
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _grad_highprec as H
import _grad_witness as W
import _markov_cases as MC
import _markov_grad_cases as GC
import gpcc_amd
from gpcc_amd import fit, markov, synthetic

pytestmark = pytest.mark.gpu

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
UNSUPPORTED = -3


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


@pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_parity_cpu_cases(pool, kernel):
    cases = [c for c in GC.cases() if c[1] == kernel]
    assert len(cases) == 3 * 3 * 2 * len(MC.RHOS)
    refs = pool.map(H.evaluate_job, [(k, *data, delays, alpha, rho, mb) for (_, k, data, delays, alpha, rho, mb, _) in cases])
    worst = {N: GC.Worst("device gradient %s N = %d" % (kernel, N)) for N in MC.SHAPES}
    mirror = {N: GC.Worst("device against mirror %s N = %d (of 2 bars)" % (kernel, N)) for N in MC.SHAPES}
    print("build: %s" % gpcc_amd.build_info())
    for (cid, k, data, delays, alpha, rho, mb, N), ref in zip(cases, refs):
        assert ref.info == 0, cid
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll, grad, info = obj.loglik_grad_markov_batch(delays[None, :], alpha[None, :], [rho])
        assert info[0] == 0, cid
        worst[N].add(H.ratio(grad[0], ref), cid)
        hl, hg, hinfo = markov.loglik_grad(k, *data, delays, alpha, rho, mb)     # the same algorithm, another rounding order
        assert hinfo == 0
        mirror[N].add(float(np.max(np.abs(grad[0] - hg))) / (2 * H.bar(ref)), cid)
    for w in list(worst.values()) + list(mirror.values()):
        w.report()


@pytest.mark.parametrize("N", sorted(GC.LARGE))
def test_parity_large_against_witness(N):
    G = 16
    kernel, data, delays, alpha, rho = GC.large(N, G)
    with gpcc_amd.Objective(*data, KERN[kernel]) as obj:
        ll, grad, info = obj.loglik_grad_markov_batch(delays, alpha, rho)
        dl, dgrad, dinfo = obj.loglik_grad_batch(delays, alpha, rho)
    assert (info == 0).all() and (dinfo == 0).all()
    worst, dense = 0.0, 0.0
    for g in range(G):
        lw, gw = W.loglik_and_grad(kernel, *data, delays[g], alpha[g], rho[g], True)
        scale = float(np.max(np.abs(gw)))
        err = float(np.max(np.abs(grad[g] - gw))) / scale
        worst = max(worst, err)
        dense = max(dense, float(np.max(np.abs(grad[g] - dgrad[g]))) / scale)      # a record, not an assertion
        assert err <= GC.WITNESS_BAR, (g, grad[g], gw)
    print("device gradient %s N = %d, %d delays: worst disagreement with the witness %.3g of max|g| (bar %.0e); with loglik_grad_batch %.3g"
          % (kernel, N, G, worst, GC.WITNESS_BAR, dense))


def _batch(L, M, seed):
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), rg.uniform(-3.0, 45.0, (M, L - 1))], 1)
    return delays, rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))


@pytest.mark.parametrize("mb", [True, False])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_value_and_info_are_the_value_entrys(kernel, mb):
    """1024 mixed rows, refused and failing ones among them: loglik and info bitwise loglik_markov_batch's."""
    t, y, s, _ = MC.lightcurves([300, 200, 267], seed=7, kind="ties")
    delays, alpha, rho = _batch(3, 1024, seed=3)
    alpha[5, 1] = 0.0
    alpha[70, 2] = -1.0
    rho[131] = 0.0
    rho[200] = -3.0
    rho[333] = np.nan
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        vl, vinfo = obj.loglik_markov_batch(delays, alpha, rho)
        ll, grad, info = obj.loglik_grad_markov_batch(delays, alpha, rho)
    assert np.array_equal(info, vinfo) and np.array_equal(ll, vl, equal_nan=True)
    assert list(info[[5, 70, 131, 200]]) == [-1, -1, -2, -2] and info[333] != 0
    bad = info != 0
    assert bad.sum() == 5 and np.isnan(grad[bad]).all() and np.isfinite(grad[~bad]).all() and np.isfinite(ll[~bad]).all()


@pytest.mark.parametrize("kernel,Nl,mb", [("matern52", [300, 200, 267], True), ("OU", [60, 50], False), ("matern32", [2048, 2048], True)])
def test_bitwise_invariance(kernel, Nl, mb):
    t, y, s, _ = MC.lightcurves(Nl, seed=7, kind="ties")
    L = len(Nl)
    delays, alpha, rho = _batch(L, 1024, seed=len(Nl))
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        fl, full, info = obj.loglik_grad_markov_batch(delays, alpha, rho)
        assert (info == 0).all() and np.isfinite(full).all()
        for M in (1, 63, 64, 65):
            ll, g, inf = obj.loglik_grad_markov_batch(delays[:M], alpha[:M], rho[:M])
            assert np.array_equal(g, full[:M]) and np.array_equal(ll, fl[:M]) and (inf == 0).all(), M
        perm = np.random.default_rng(1).permutation(1024)
        ll, g, _ = obj.loglik_grad_markov_batch(delays[perm], alpha[perm], rho[perm])
        assert np.array_equal(g, full[perm]) and np.array_equal(ll, fl[perm])
        for key, val in (("streams", 1), ("slots_per_stream", 8), ("small_n", 0), ("chain_max", 0)):
            obj.set_option(key, val)
        ll, g, _ = obj.loglik_grad_markov_batch(delays[:65], alpha[:65], rho[:65])
        assert np.array_equal(g, full[:65])
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, precision="fp32") as o32:
        ll, g, inf = o32.loglik_grad_markov_batch(delays[:65], alpha[:65], rho[:65])
        assert np.array_equal(g, full[:65]) and np.array_equal(ll, fl[:65]) and (inf == 0).all()
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, devices=[0, 0]) as om:
        ll, g, inf = om.loglik_grad_markov_batch(delays[:65], alpha[:65], rho[:65])
        assert np.array_equal(g, full[:65]) and np.array_equal(ll, fl[:65]) and (inf == 0).all()


def test_refusals_and_failures():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loglik_grad_markov_batch([d0], [[1.0, 1.0]], [2.0])
        assert ei.value.code == UNSUPPORTED and "rbf" in ei.value.message and "gpcc_loglik_grad_batch" in ei.value.message
    delays, alpha, rho = _batch(2, 8, seed=5)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        gl, good, ginfo = obj.loglik_grad_markov_batch(delays, alpha, rho)
        assert (ginfo == 0).all()
        a2, r2, d2 = alpha.copy(), rho.copy(), delays.copy()
        a2[1, 0] = 0.0
        a2[2, 1] = -1.0
        r2[3] = 0.0
        r2[4] = -2.0
        a2[5, 1] = np.nan
        r2[6] = np.nan
        ll, grad, info = obj.loglik_grad_markov_batch(d2, a2, r2)
        vl, vinfo = obj.loglik_markov_batch(d2, a2, r2)
        bad = [1, 2, 3, 4, 5, 6]
        assert list(info[[1, 2, 3, 4, 5]]) == [-1, -1, -2, -2, -1] and np.array_equal(info, vinfo) and info[6] != 0
        assert np.isnan(ll[bad]).all() and np.isnan(grad[bad]).all()
        assert np.array_equal(grad[[0, 7]], good[[0, 7]]) and np.array_equal(ll[[0, 7]], gl[[0, 7]]) and (info[[0, 7]] == 0).all()
    # five bands: with marginalised offsets unsupported, without them fine
    t5, y5, s5, d5 = MC.lightcurves([30, 25, 20, 25, 30], seed=12, kind="ties")
    a5 = np.linspace(0.6, 1.4, 5)
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=True) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loglik_grad_markov_batch([d5], [a5], [2.0])
        assert ei.value.code == UNSUPPORTED and "gpcc_loglik_grad_batch" in ei.value.message
        assert obj.loglik_grad_batch([d5], [a5], [2.0])[2][0] == 0      # the handle still serves the dense path
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=False) as obj:
        ll, grad, info = obj.loglik_grad_markov_batch([d5], [a5], [2.0])
        assert info[0] == 0
        if H.EXTENDED:
            assert H.ratio(grad[0], H.evaluate("OU", t5, y5, s5, d5, a5, 2.0, False)) <= 1.0
    # sigma = 0 at two observations that coincide in shifted time: the second one's predictive variance is 0
    t, y, s, d0 = MC.lightcurves([30, 20], seed=5, kind="ties")
    ts = markov.prepare(t, y, s)[0]
    seq = markov.merge_order(ts, d0)
    sh = [ts[b][i] - d0[b] for b, i in seq]
    single = lambda q: np.count_nonzero(t[seq[q][0]] == ts[seq[q][0]][seq[q][1]]) == 1     # (a time that is not repeated inside its band)
    j = next(j for j in range(1, len(seq)) if seq[j][0] != seq[j - 1][0] and sh[j] == sh[j - 1] and single(j) and single(j - 1)
             and (j + 1 == len(seq) or sh[j + 1] != sh[j]) and (j < 2 or sh[j - 2] != sh[j]))
    for b, i in (seq[j - 1], seq[j]):
        s[b][np.where(t[b] == ts[b][i])[0]] = 0.0
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU, marginalise_b=False) as obj:
        ll, grad, info = obj.loglik_grad_markov_batch([d0, d0 + [0.0, 0.37]], [[1.0, 1.0]] * 2, [2.0, 2.0])
        assert info[0] == j + 1 and np.isnan(ll[0]) and np.isnan(grad[0]).all()
        assert info[1] == 0 and np.isfinite(ll[1]) and np.isfinite(grad[1]).all()      # no tie at the other delay: its neighbour is fine


def test_memory_and_large_n_against_central_differences():
    """N = 16384 (Matern-5/2: no dense fp64 counterpart fits a slot here): the handle allocates the sorted light curves, the staging and
    the gradient's slots, none of the N^2 workspace; one row against central differences of loglik_markov_batch -- relative steps 1e-5 in
    alpha and rho, 2^-10 in tau (exact in the shifted times; the data has no ties, so the merged order does not change inside the
    step... where it does, the Matern-5/2 likelihood is still C^1) -- within 1e-5 max|g|, the bar of the dense gradient's N = 4096
    central-difference test."""
    import torch
    Nl = [8192, 8192]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=3)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    L = 2
    delays = np.stack([np.zeros(64), np.linspace(0.0, 12.6, 64)], 1)
    alpha, rho = np.tile(alpha0, (64, 1)), np.full(64, rho0)
    torch.cuda.synchronize()
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        free0, _ = torch.cuda.mem_get_info(0)
        ll, grad, info = obj.loglik_grad_markov_batch(delays, alpha, rho)
        ll2, grad2, _ = obj.loglik_grad_markov_batch(delays[:3], alpha[:3], rho[:3])
        free1, _ = torch.cuda.mem_get_info(0)
        assert obj.get_option("workspace_slots") == obj.get_option("slots_per_stream")     # (never built)
        print("N = 16384 gradient-only markov handle: %.2f MiB of growth" % ((free0 - free1) / 2.0 ** 20))
        assert free0 - free1 < 4 * 2 ** 20
        assert (info == 0).all() and np.array_equal(ll2, ll[:3]) and np.array_equal(grad2, grad[:3])
        g0 = 31
        x0 = np.concatenate([alpha[g0], [rho[g0]], delays[g0]])
        step = np.concatenate([1e-5 * np.abs(x0[:L + 1]), np.full(L, 2.0 ** -10)])
        X = np.repeat(x0[None, :], 2 * len(x0), 0)
        for i in range(len(x0)):
            X[2 * i, i] += step[i]
            X[2 * i + 1, i] -= step[i]
        lf, finfo = obj.loglik_markov_batch(X[:, L + 1:], X[:, :L], X[:, L])
    assert (finfo == 0).all()
    fd = ((lf[0::2] - lf[1::2]) / (X[0::2] - X[1::2])[np.arange(len(x0)), np.arange(len(x0))])
    g = grad[g0]
    print("N = 16384 matern52: gradient against central differences: %.3g of max|g| (bar 1e-5)" % (np.max(np.abs(g - fd)) / np.max(np.abs(g))))
    assert np.max(np.abs(g - fd)) <= 1e-5 * np.max(np.abs(g)), (g, fd)


def test_value_and_grad_with_the_markov_solver():
    data = W.ragged_data([300, 213], seed=8)
    delays, alpha, rho = W.random_params(2, 4, seed=5)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
        ll, grad, info = obj.loglik_grad_markov_batch(delays, alpha, rho)
        assert (info == 0).all()
        v, g = obj.value_and_grad(alpha[2], rho[2], delays[2], solver="markov")
        assert v == ll[2] and np.array_equal(g["alpha"], grad[2, :2]) and g["rho"] == grad[2, 2] and np.array_equal(g["delays"], grad[2, 3:])
        dv, dg = obj.value_and_grad(alpha[2], rho[2], delays[2])                 # the default is the dense entry
        dl, dgrad, _ = obj.loglik_grad_batch(delays[2:3], alpha[2:3], rho[2:3])
        assert dv == dl[0] and np.array_equal(dg["delays"], dgrad[0, 3:])
        with pytest.raises(AssertionError):
            obj.value_and_grad([0.0, 1.0], rho[0], delays[0], solver="markov")
        with pytest.raises(ValueError):
            obj.value_and_grad(alpha[0], -1.0, delays[0], solver="markov")
        with pytest.raises(ValueError):
            obj.value_and_grad(alpha[0], rho[0], delays[0], solver="sparse")


def test_lbfgs_fit_with_the_markov_gradient_reaches_the_dense_optimum():
    """The README-size L-BFGS-B fit of tests/test_gpu_gradient.py run on both gradients: the linear-time run reaches the dense run's
    optimum within that test's 1e-6."""
    minimize = pytest.importorskip("scipy.optimize").minimize
    t, y, s, true_delays = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    L, rhomin, rhomax, seed = 2, 0.1, 20.0, 1
    delays = np.asarray(true_delays, dtype=np.float64)
    rg = np.random.default_rng(seed)
    rho0 = rg.uniform(rhomin + 1e-3, rhomax - 1e-3, 1)
    vary = np.array([np.var(v, ddof=1) for v in y])
    cands = np.array([np.concatenate([fit.invmakepositive(vary * (rg.random(L) * 0.4 + 0.8)),
                                      [fit.invtransformbetween(rho0[0], rhomin, rhomax)]]) for _ in range(5)])
    best, calls = {}, {}
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        a0 = fit.makepositive(cands[:, :L]) + 1e-8
        r0 = fit.transformbetween(cands[:, L], rhomin, rhomax)
        l0, _ = obj.loglik_batch(np.tile(delays, (5, 1)), a0, r0)
        x0 = cands[int(np.nanargmax(l0))]
        for solver in ("dense", "markov"):
            calls[solver] = 0
            entry = obj.loglik_grad_markov_batch if solver == "markov" else obj.loglik_grad_batch

            def f(x):
                calls[solver] += 1
                a = fit.makepositive(x[:L]) + 1e-8
                r = float(fit.transformbetween(x[L], rhomin, rhomax))
                ll, grad, info = entry(delays[None, :], a[None, :], [r])
                if info[0] != 0:
                    return np.inf, np.zeros(L + 1)
                return -ll[0], -fit.unpack_grad(x, grad[0, :L + 1], L, rhomin, rhomax)

            best[solver] = -minimize(f, x0, jac=True, method="L-BFGS-B").fun
    print("L-BFGS-B: dense gradient %.10f in %d evaluations, linear-time gradient %.10f in %d"
          % (best["dense"], calls["dense"], best["markov"], calls["markov"]))
    assert best["markov"] >= best["dense"] - 1e-6 * abs(best["dense"]), best
