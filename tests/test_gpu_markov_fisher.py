"""gpcc_loglik_fisher_markov_batch on the device: the Fisher information in linear time against the extended-precision
Fisher matrix over the N = 110 cases of tests/_markov_fisher_cases.py under the reference's own per-block bars and against the numpy
mirror; the NaN contract on OU rows with a cross-band tie; value, info and gradient bitwise gpcc_loglik_grad_markov_batch's; bitwise
symmetry and invariance over batch sizes, row order and handle flavours; refusal rows and refused requests; every shipped combination
and the large shapes against the dense device entry's Fisher matrix; N = 16384 against the mirror; fit.delay_covariance(curvature=
"fisher") with solver="markov" against solver="dense".  The references are computed in a pool of CPU processes that never touch the GPU."""
import multiprocessing
import os
import re
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _hess_highprec as HH
import _markov_cases as MC
import _markov_fisher_cases as FC
import _markov_grad_cases as GC
import _markov_hess_full_cases as HF
import gpcc_amd
from gpcc_amd import fit, markov, synthetic
from test_gpu_markov_hess import KERN, LARGE_BAR, UNSUPPORTED, _batch

pytestmark = pytest.mark.gpu

ORDER = {"OU": 1, "matern32": 2, "matern52": 3}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shipped_table():
    """{(P, NOFF)} of the instantiations of gpcc_markov_fisher in the committed resource table that use no scratch memory."""
    out = set()
    with open(os.path.join(ROOT, "profiles", "markov", "kernel_resources_fisher.log")) as f:
        for line in f:
            m = re.search(r"gpcc_markov_fisher<(\d), (\d)>.*scratch\s+(\d+) B", line)
            if m and int(m.group(3)) == 0:
                out.add((int(m.group(1)), int(m.group(2))))
    return out


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


@pytest.mark.skipif(not HH.EXTENDED, reason=HH.SKIP_REASON)
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_parity_cpu_cases(pool, kernel):
    cases = [c for c in FC.cases(110) if c[1] == kernel]
    assert len(cases) == 3 * 2 * len(MC.RHOS)
    refs = pool.map(FC.reference_job, [FC.job(c) for c in cases])
    worst = {b: FC.Worst("device Fisher %s %s (of the case's allowance)" % (kernel, b)) for b in HH.BLOCKS}
    mirror = FC.Worst("device against mirror %s (of 2 bars)" % kernel)
    print("build: %s" % gpcc_amd.build_info())
    tied = 0
    for case, ref in zip(cases, refs):
        cid, k, data, delays, alpha, rho, mb, N = case
        L = len(alpha)
        assert ref.info == 0, cid
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll, grad, fisher, info = obj.loglik_fisher_markov_batch(delays[None, :], alpha[None, :], [rho])
            gl, gg, ginfo = obj.loglik_grad_markov_batch(delays[None, :], alpha[None, :], [rho])
        assert info[0] == 0 and fisher.shape == (1, 2 * L + 1, 2 * L + 1), cid
        assert np.array_equal(ll, gl) and np.array_equal(grad, gg) and np.array_equal(info, ginfo), cid
        F = fisher[0]
        assert np.array_equal(F, F.T, equal_nan=True), cid
        mf = markov.loglik_fisher(k, *data, delays, alpha, rho, mb)[2]       # the same algorithm, another rounding order
        limit = FC.device_limit(case)
        blocks = None
        if FC.ou_tie(case):
            tied += 1
            tau = FC.tau_mask(L)
            assert ref.ties and np.isnan(F[tau]).all() and np.isfinite(F[~tau]).all(), cid
            blocks = FC.HYPER_BLOCKS
            F, mf = np.where(tau, 0.0, F), np.where(tau, 0.0, mf)
        elif L == 1:
            assert not F[2, :].any() and not F[:, 2].any(), cid
        for b, r in FC.ratios(F, ref, case, blocks=blocks).items():
            worst[b].add(r / limit, cid)
        mirror.add(max(FC.ratios(F, ref, case, against=mf, blocks=blocks).values()) / 2.0, cid)
    assert tied == (6 if kernel == "OU" else 0)
    for w in worst.values():
        w.report()
    mirror.report()


@pytest.mark.parametrize("kernel,Nl,mb", [("matern52", [300, 200, 267], True), ("OU", [60, 50], False), ("matern32", [700, 600], True)])
def test_bitwise_properties(kernel, Nl, mb):
    t, y, s, _ = MC.lightcurves(Nl, seed=7, kind="ties")
    L = len(Nl)
    W = 2 * L + 1
    delays, alpha, rho = _batch(L, 1024, seed=len(Nl))
    tied = FC.tie_rows(t, delays) if kernel == "OU" else np.zeros(1024, bool)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        gl, gg, ginfo = obj.loglik_grad_markov_batch(delays, alpha, rho)
        fl, fg, full, info = obj.loglik_fisher_markov_batch(delays, alpha, rho)
        assert (info == 0).all() and full.shape == (1024, W, W)
        assert np.array_equal(fl, gl) and np.array_equal(fg, gg) and np.array_equal(info, ginfo)
        assert np.array_equal(full, np.swapaxes(full, 1, 2), equal_nan=True)
        assert np.isfinite(full[~tied]).all() and np.isfinite(full[:, :L + 1, :L + 1]).all()
        assert np.isnan(full[tied][:, FC.tau_mask(L)]).all()
        for M in (1, 63, 64, 65):
            ll, g, fs, inf = obj.loglik_fisher_markov_batch(delays[:M], alpha[:M], rho[:M])
            assert np.array_equal(fs, full[:M], equal_nan=True) and np.array_equal(g, fg[:M]) and np.array_equal(ll, fl[:M]), M
            assert (inf == 0).all(), M
        perm = np.random.default_rng(1).permutation(1024)
        ll, g, fs, _ = obj.loglik_fisher_markov_batch(delays[perm], alpha[perm], rho[perm])
        assert np.array_equal(fs, full[perm], equal_nan=True) and np.array_equal(g, fg[perm]) and np.array_equal(ll, fl[perm])
    for kw in ({"precision": "fp32"}, {"devices": [0, 0]}):
        with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, **kw) as o:
            ll, g, fs, inf = o.loglik_fisher_markov_batch(delays[:65], alpha[:65], rho[:65])
            assert np.array_equal(fs, full[:65], equal_nan=True) and np.array_equal(g, fg[:65]) and np.array_equal(ll, fl[:65]), kw
            assert (inf == 0).all(), kw


def test_no_flux_enters():
    """Without marginalise_b the Fisher matrix is bitwise the same for other fluxes on the same times and error bars."""
    t, y, s, _ = MC.lightcurves([60, 50], seed=11, kind="plain")
    other = [np.cos(3.0 * np.asarray(a)) * 2.0 + 0.3 for a in t]
    delays, alpha, rho = _batch(2, 8, seed=5)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32, marginalise_b=False) as obj:
        F = obj.loglik_fisher_markov_batch(delays, alpha, rho)[2]
    with gpcc_amd.Objective(t, other, s, gpcc_amd.matern32, marginalise_b=False) as obj:
        G = obj.loglik_fisher_markov_batch(delays, alpha, rho)[2]
    assert np.isfinite(F).all() and np.array_equal(F, G)


def test_refusal_rows_leave_their_neighbours_alone():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    delays, alpha, rho = _batch(2, 8, seed=5)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        gl, gg, good, ginfo = obj.loglik_fisher_markov_batch(delays, alpha, rho)
        assert (ginfo == 0).all()
        a2, r2 = alpha.copy(), rho.copy()
        a2[1, 0] = 0.0
        a2[2, 1] = -1.0
        r2[3] = 0.0
        r2[4] = -2.0
        ll, grad, fisher, info = obj.loglik_fisher_markov_batch(delays, a2, r2)
        bad = [1, 2, 3, 4]
        assert list(info[bad]) == [-1, -1, -2, -2]
        assert np.isnan(ll[bad]).all() and np.isnan(grad[bad]).all() and np.isnan(fisher[bad]).all()
        keep = [0, 5, 6, 7]
        assert np.array_equal(fisher[keep], good[keep]) and np.array_equal(grad[keep], gg[keep]) and np.array_equal(ll[keep], gl[keep])
        assert (info[keep] == 0).all()


def _block_disagreement(fisher, dense, L):
    return max(float(np.max(np.abs(fisher[m] - dense[m]))) / float(np.max(np.abs(dense[m]))) for m in HH.block_masks(L).values()
               if np.max(np.abs(dense[m])) > 0 or np.max(np.abs(fisher[m])) > 0)


def test_refused_requests_and_every_shipped_combination():
    table = shipped_table()
    must = {(p, noff) for p in (1, 2, 3) for noff in range(5) if noff == 0 or p + noff <= 5}
    assert must <= table and (3, 4) not in table
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loglik_fisher_markov_batch([d0], [[1.0, 1.0]], [2.0])
        assert ei.value.code == UNSUPPORTED and "rbf" in ei.value.message and "gpcc_loglik_hess_batch" in ei.value.message
    sizes = [30, 25, 20, 25, 30, 20, 25, 30]
    ran = want = 0
    for kernel in MC.KERNELS:
        for mb in (True, False):
            for L in range(1, 9):
                tl, yl, sl, dl = MC.lightcurves(sizes[:L], seed=12 + L, kind="plain")
                dl = dl + 0.000123 * np.arange(L)              # off the times' 2^-10 grid: a row without ties
                assert not FC.tie_rows(tl, dl).any()
                al = np.linspace(0.6, 1.4, L)
                shipped = not (mb and L > 4) and (ORDER[kernel], L if mb else 0) in table
                want += shipped
                with gpcc_amd.Objective(tl, yl, sl, KERN[kernel], marginalise_b=mb) as obj:
                    if shipped:
                        ll, grad, fisher, info = obj.loglik_fisher_markov_batch([dl], [al], [2.0])
                        assert info[0] == 0 and np.isfinite(fisher).all() and fisher.shape == (1, 2 * L + 1, 2 * L + 1), (kernel, mb, L)
                        dll, dgrad, dh, df, dinfo = obj.loglik_hess_batch([dl], [al], [2.0])
                        assert dinfo[0] == 0 and _block_disagreement(fisher[0], df[0], L) <= LARGE_BAR, (kernel, mb, L)
                        if L == 1:
                            assert not fisher[0][2, :].any() and not fisher[0][:, 2].any()
                        ran += 1
                    else:
                        with pytest.raises(gpcc_amd.GpccError) as ei:
                            obj.loglik_fisher_markov_batch([dl], [al], [2.0])
                        assert ei.value.code == UNSUPPORTED and "gpcc_loglik_hess_batch" in ei.value.message, (kernel, mb, L)
                        assert obj.loglik_hess_batch([dl], [al], [2.0])[4][0] == 0           # the handle still serves the dense path
    assert ran == want == len([1 for (p, noff) in table for _ in ([0] if noff else range(8))])


@pytest.mark.parametrize("N", sorted(GC.LARGE))
def test_large_shapes_against_the_dense_entry(N):
    G = 4
    kernel, data, delays, alpha, rho = GC.large(N, 64)
    free = np.flatnonzero(~FC.tie_rows(data[0], delays)) if kernel == "OU" else np.arange(64)
    rows = free[np.linspace(0, len(free) - 1, G).astype(int)]
    assert len(set(rows)) == G
    delays, alpha, rho = delays[rows], alpha[rows], rho[rows]
    L = len(data[0])
    with gpcc_amd.Objective(*data, KERN[kernel]) as obj:
        ll, grad, fisher, info = obj.loglik_fisher_markov_batch(delays, alpha, rho)
        dl, dgrad, dh, df, dinfo = obj.loglik_hess_batch(delays, alpha, rho)
    assert (info == 0).all() and (dinfo == 0).all() and np.isfinite(fisher).all()
    worst = max(_block_disagreement(fisher[g], df[g], L) for g in range(G))
    print("device Fisher %s N = %d, %d rows: worst per-block disagreement with loglik_hess_batch's %.3g of max|F| (bar %.0e)"
          % (kernel, N, G, worst, LARGE_BAR))
    assert worst <= LARGE_BAR


def test_n16384_against_the_mirror(pool):
    """N = 16384, Matern-5/2, one row, the light curves in global memory (no dense fp64 Fisher matrix fits here): the entries (rho, rho),
    (alpha_1, tau_2) and (tau_2, tau_2) against the numpy mirror's, each within LARGE_BAR of its block's max|F|; the N^2 workspace is
    never built."""
    Nl = [8192, 8192]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=3)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    delays = np.array([0.0, 2.0])
    pairs = [(2, 2), (0, 4), (4, 4)]
    jobs = pool.map(FC.pair_job, [("matern52", t, y, s, delays, alpha0, rho0, True, a, b) for a, b in pairs])
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        ll, grad, fisher, info = obj.loglik_fisher_markov_batch([delays], [alpha0], [rho0])
        assert info[0] == 0 and np.isfinite(fisher).all()
        assert obj.get_option("workspace_slots") == obj.get_option("slots_per_stream")     # (never built)
    masks = HH.block_masks(2)
    worst = 0.0
    for (a, b), want in zip(pairs, jobs):
        size = max(float(np.max(np.abs(fisher[0][m]))) for m in masks.values() if m[a, b])      # the entry's block
        worst = max(worst, abs(fisher[0][a, b] - want) / size)
    print("N = 16384 matern52: Fisher entries %s against the mirror: %.3g of their blocks' max|F| (bar %.0e)" % (pairs, worst, LARGE_BAR))
    assert worst <= LARGE_BAR


@pytest.mark.parametrize("kernel", ["OU", "matern32"])
def test_delay_covariance_fisher_markov_against_dense(kernel):
    """The README size (N = 110, two bands): fit.delay_covariance(curvature="fisher") with solver="markov" against "dense", each entry
    within 1e-6 of sqrt(cov_ii cov_jj); the default curvature's results are untouched."""
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    delays = np.array(HF.README_DELAYS)
    a0, r0 = HF.README_MODE[kernel]
    assert not FC.tie_rows(t, delays).any()
    with gpcc_amd.Objective(t, y, s, KERN[kernel]) as obj:
        dense, dok = fit.delay_covariance(obj, delays, a0, r0, curvature="fisher")
        mk, mok = fit.delay_covariance(obj, delays, a0, r0, solver="markov", curvature="fisher")
        assert dok and mok and dense.shape == mk.shape == (4, 4)
        sd = np.sqrt(np.diag(dense))
        worst = float(np.max(np.abs(mk - dense) / (sd[:, None] * sd[None, :])))
        print("delay_covariance(curvature='fisher') %s: markov against dense, worst |dcov_ij| / sqrt(cov_ii cov_jj) %.3g (bar 1e-6)"
              % (kernel, worst))
        assert worst <= 1e-6
        hess, hok = fit.delay_covariance(obj, delays, a0, r0, solver="markov")
        assert hok and np.array_equal(hess, fit.delay_covariance(obj, delays, a0, r0, solver="markov", curvature="hessian")[0])
        # away from a maximum the Fisher information still gives error bars
        away, aok = fit.delay_covariance(obj, np.array([0.0, 7.3]), [0.2, 2.5], 6.0, solver="markov", curvature="fisher")
        assert aok and (np.diag(away) > 0).all()
        with pytest.raises(ValueError):
            fit.delay_covariance(obj, delays, a0, r0, solver="markov", curvature="expected")
        bad, okb = fit.delay_covariance(obj, delays, [0.0, 1.0], r0, solver="markov", curvature="fisher")
        assert not okb and np.isnan(bad).all()
