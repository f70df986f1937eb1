"""gpcc_loglik_hess_markov_batch on the device: the full Hessian -- the rows of tau -- in linear time against the
extended-precision reference over the N = 110 cases of tests/_markov_hess_full_cases.py under the reference's own per-block bars and
against the numpy mirror; the NaN contract on OU rows with a cross-band tie; value, info and gradient bitwise
gpcc_loglik_grad_markov_batch's and the leading block bitwise gpcc_loglik_hess_hyper_markov_batch's; bitwise symmetry and invariance over
batch sizes, row order and handle flavours; refusal rows and refused requests; every shipped combination and the large shapes against
the dense device entry; N = 16384 against central differences of the linear-time gradient; fit.delay_covariance with solver="markov"
against solver="dense".  The references are computed in a pool of CPU processes that never touch the GPU."""
import multiprocessing
import os
import re
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _hess_highprec as HH
import _markov_cases as MC
import _markov_grad_cases as GC
import _markov_hess_full_cases as FC
import gpcc_amd
from gpcc_amd import fit, markov, synthetic
from test_gpu_markov_hess import KERN, LARGE_BAR, UNSUPPORTED, _batch

pytestmark = pytest.mark.gpu

ORDER = {"OU": 1, "matern32": 2, "matern52": 3}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shipped_table():
    """{(P, NOFF)} of the instantiations of gpcc_markov_hess_tau in the committed resource table that use no scratch memory."""
    out = set()
    with open(os.path.join(ROOT, "profiles", "markov", "kernel_resources_hess_tau.log")) as f:
        for line in f:
            m = re.search(r"gpcc_markov_hess_tau<(\d), (\d)>.*scratch\s+(\d+) B", line)
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
    worst = {b: FC.Worst("device Hessian %s %s (of the case's allowance)" % (kernel, b)) for b in HH.BLOCKS}
    mirror = FC.Worst("device against mirror %s (of 2 bars)" % kernel)
    print("build: %s" % gpcc_amd.build_info())
    tied = 0
    for case, ref in zip(cases, refs):
        cid, k, data, delays, alpha, rho, mb, N = case
        L = len(alpha)
        assert ref.info == 0, cid
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll, grad, hess, info = obj.loglik_hess_markov_batch(delays[None, :], alpha[None, :], [rho])
            hl, hg, hyper, hinfo = obj.loglik_hess_hyper_markov_batch(delays[None, :], alpha[None, :], [rho])
        assert info[0] == 0 and hess.shape == (1, 2 * L + 1, 2 * L + 1), cid
        assert np.array_equal(hess[0, :L + 1, :L + 1], hyper[0]) and np.array_equal(grad, hg) and np.array_equal(ll, hl), cid
        if FC.ou_tie(case):
            tied += 1
            tau = FC.tau_mask(L)
            assert ref.ties and np.isnan(hess[0][tau]).all() and np.isfinite(hess[0][~tau]).all(), cid
            continue
        limit = FC.device_limit(case)
        for b, r in FC.ratios(hess[0], ref, case).items():
            worst[b].add(r / limit, cid)
        mh = markov.loglik_hess(k, *data, delays, alpha, rho, mb)[2]       # the same algorithm, another rounding order
        mirror.add(max(FC.ratios(hess[0], ref, case, against=mh).values()) / 2.0, cid)
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
        hl, hg, hyper, hinfo = obj.loglik_hess_hyper_markov_batch(delays, alpha, rho)
        fl, fg, full, info = obj.loglik_hess_markov_batch(delays, alpha, rho)
        assert (info == 0).all() and full.shape == (1024, W, W)
        assert np.array_equal(fl, gl) and np.array_equal(fg, gg) and np.array_equal(info, ginfo)
        assert np.array_equal(full[:, :L + 1, :L + 1], hyper)
        assert np.array_equal(full, np.swapaxes(full, 1, 2), equal_nan=True)
        assert np.isfinite(full[~tied]).all() and np.isfinite(full[:, :L + 1, :L + 1]).all()
        assert np.isnan(full[tied][:, FC.tau_mask(L)]).all()
        for M in (1, 63, 64, 65):
            ll, g, hs, inf = obj.loglik_hess_markov_batch(delays[:M], alpha[:M], rho[:M])
            assert np.array_equal(hs, full[:M], equal_nan=True) and np.array_equal(g, fg[:M]) and np.array_equal(ll, fl[:M]), M
            assert (inf == 0).all(), M
        perm = np.random.default_rng(1).permutation(1024)
        ll, g, hs, _ = obj.loglik_hess_markov_batch(delays[perm], alpha[perm], rho[perm])
        assert np.array_equal(hs, full[perm], equal_nan=True) and np.array_equal(g, fg[perm]) and np.array_equal(ll, fl[perm])
    for kw in ({"precision": "fp32"}, {"devices": [0, 0]}):
        with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, **kw) as o:
            ll, g, hs, inf = o.loglik_hess_markov_batch(delays[:65], alpha[:65], rho[:65])
            assert np.array_equal(hs, full[:65], equal_nan=True) and np.array_equal(g, fg[:65]) and np.array_equal(ll, fl[:65]), kw
            assert (inf == 0).all(), kw


def test_ou_rows_with_a_tie_are_nan_in_the_tau_entries_only():
    """An OU batch in which rows 1, 4 and 6 have a delay equal to a difference of two observation times: NaN exactly in the tau entries of
    those rows, info 0, everything else finite; the other rows' bits are those of the batch without ties; Matern-3/2 on the same batch is
    finite everywhere."""
    t, y, s, _ = MC.lightcurves([60, 50], seed=11, kind="plain")
    ts = [np.sort(a) for a in t]
    delays, alpha, rho = _batch(2, 8, seed=5)
    assert not FC.tie_rows(t, delays).any()
    hand = delays.copy()
    for row, (i, k) in zip((1, 4, 6), ((3, 5), (20, 31), (49, 0))):
        hand[row, 1] = ts[1][i] - ts[0][k]
        assert ts[1][i] - hand[row, 1] == ts[0][k]              # (times on the 2^-10 grid: the difference is exact)
    tied = FC.tie_rows(t, hand)
    assert list(np.flatnonzero(tied)) == [1, 4, 6]
    tau = FC.tau_mask(2)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        gl, gg, good, ginfo = obj.loglik_hess_markov_batch(delays, alpha, rho)
        ll, grad, hess, info = obj.loglik_hess_markov_batch(hand, alpha, rho)
        hl, hg, hyper, hinfo = obj.loglik_hess_hyper_markov_batch(hand, alpha, rho)
    assert (ginfo == 0).all() and np.isfinite(good).all() and (info == 0).all()
    assert np.isfinite(ll).all() and np.isfinite(grad).all() and np.array_equal(grad, hg) and np.array_equal(hess[:, :3, :3], hyper)
    assert np.array_equal(np.isnan(hess), tied[:, None, None] & tau[None, :, :])
    assert np.array_equal(hess[~tied], good[~tied]) and np.array_equal(grad[~tied], gg[~tied]) and np.array_equal(ll[~tied], gl[~tied])
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        assert np.isfinite(obj.loglik_hess_markov_batch(hand, alpha, rho)[2]).all()


def test_refusal_rows_leave_their_neighbours_alone():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    delays, alpha, rho = _batch(2, 8, seed=5)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        gl, gg, good, ginfo = obj.loglik_hess_markov_batch(delays, alpha, rho)
        assert (ginfo == 0).all()
        a2, r2 = alpha.copy(), rho.copy()
        a2[1, 0] = 0.0
        a2[2, 1] = -1.0
        r2[3] = 0.0
        r2[4] = -2.0
        ll, grad, hess, info = obj.loglik_hess_markov_batch(delays, a2, r2)
        bad = [1, 2, 3, 4]
        assert list(info[bad]) == [-1, -1, -2, -2]
        assert np.isnan(ll[bad]).all() and np.isnan(grad[bad]).all() and np.isnan(hess[bad]).all()
        keep = [0, 5, 6, 7]
        assert np.array_equal(hess[keep], good[keep]) and np.array_equal(grad[keep], gg[keep]) and np.array_equal(ll[keep], gl[keep])
        assert (info[keep] == 0).all()


def _block_disagreement(hess, dense, L):
    return max(float(np.max(np.abs(hess[m] - dense[m]))) / float(np.max(np.abs(dense[m]))) for m in HH.block_masks(L).values()
               if np.max(np.abs(dense[m])) > 0 or np.max(np.abs(hess[m])) > 0)


def test_refused_requests_and_every_shipped_combination():
    table = shipped_table()
    assert (3, 4) not in table and (1, 0) in table
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loglik_hess_markov_batch([d0], [[1.0, 1.0]], [2.0])
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
                        ll, grad, hess, info = obj.loglik_hess_markov_batch([dl], [al], [2.0])
                        assert info[0] == 0 and np.isfinite(hess).all() and hess.shape == (1, 2 * L + 1, 2 * L + 1), (kernel, mb, L)
                        dll, dgrad, dh, _, dinfo = obj.loglik_hess_batch([dl], [al], [2.0])
                        assert dinfo[0] == 0 and _block_disagreement(hess[0], dh[0], L) <= LARGE_BAR, (kernel, mb, L)
                        if L == 1:
                            assert not hess[0][2, :].any() and not hess[0][:, 2].any()
                        ran += 1
                    else:
                        with pytest.raises(gpcc_amd.GpccError) as ei:
                            obj.loglik_hess_markov_batch([dl], [al], [2.0])
                        assert ei.value.code == UNSUPPORTED and "gpcc_loglik_hess_batch" in ei.value.message, (kernel, mb, L)
                        assert obj.loglik_hess_batch([dl], [al], [2.0])[4][0] == 0           # the handle still serves the dense path
    assert ran == want == 3 * 12 - 1          # (everything but <3, 4>)


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
        ll, grad, hess, info = obj.loglik_hess_markov_batch(delays, alpha, rho)
        dl, dgrad, dh, _, dinfo = obj.loglik_hess_batch(delays, alpha, rho)
    assert (info == 0).all() and (dinfo == 0).all() and np.isfinite(hess).all()
    worst = max(_block_disagreement(hess[g], dh[g], L) for g in range(G))
    print("device Hessian %s N = %d, %d rows: worst per-block disagreement with loglik_hess_batch %.3g of max|H| (bar %.0e)"
          % (kernel, N, G, worst, LARGE_BAR))
    assert worst <= LARGE_BAR


def test_n16384_against_central_differences_of_the_gradient():
    """N = 16384, Matern-5/2, 2 rows, the light curves in global memory (no dense fp64 Hessian fits here): every column of the full
    Hessian against central differences of loglik_grad_markov_batch with relative steps 1e-5 in alpha and rho and steps 1e-5 rho in tau,
    within 1e-5 max|H|; the N^2 workspace is never built."""
    Nl = [8192, 8192]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=3)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    L, W = 2, 5
    delays = np.array([[0.0, 2.0], [0.0, 6.2]])
    alpha, rho = np.tile(alpha0, (2, 1)), np.full(2, rho0)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        ll, grad, hess, info = obj.loglik_hess_markov_batch(delays, alpha, rho)
        assert (info == 0).all() and np.isfinite(hess).all()
        worst = 0.0
        for g in range(2):
            x0 = np.concatenate([alpha[g], [rho[g]], delays[g]])
            step = np.concatenate([1e-5 * np.abs(x0[:L + 1]), np.full(L, 1e-5 * rho[g])])
            X = np.repeat(x0[None, :], 2 * W, 0)
            for i in range(W):
                X[2 * i, i] += step[i]
                X[2 * i + 1, i] -= step[i]
            _, gf, finfo = obj.loglik_grad_markov_batch(X[:, L + 1:], X[:, :L], X[:, L])
            assert (finfo == 0).all()
            fd = np.stack([(gf[2 * i] - gf[2 * i + 1]) / (X[2 * i, i] - X[2 * i + 1, i]) for i in range(W)], 1)
            err = float(np.max(np.abs(hess[g] - fd))) / float(np.max(np.abs(hess[g])))
            worst = max(worst, err)
            assert err <= 1e-5, (g, hess[g], fd)
        assert obj.get_option("workspace_slots") == obj.get_option("slots_per_stream")     # (never built)
    print("N = 16384 matern52: full Hessian against central differences of the gradient: %.3g of max|H| (bar 1e-5)" % worst)


@pytest.mark.parametrize("kernel", ["OU", "matern32"])
def test_delay_covariance_markov_against_dense(kernel):
    """The README size (N = 110, two bands): fit.delay_covariance with solver="markov" against "dense", each entry within 1e-6 of
    sqrt(cov_ii cov_jj) (DESIGN.md 4.21 has the margin against the extended-precision Hessian); ok = False as documented."""
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    delays = np.array(FC.README_DELAYS)
    a0, r0 = FC.README_MODE[kernel]
    assert not FC.tie_rows(t, delays).any()
    with gpcc_amd.Objective(t, y, s, KERN[kernel]) as obj:
        dense, dok = fit.delay_covariance(obj, delays, a0, r0)
        mk, mok = fit.delay_covariance(obj, delays, a0, r0, solver="markov")
        assert dok and mok and dense.shape == mk.shape == (4, 4)
        sd = np.sqrt(np.diag(dense))
        worst = float(np.max(np.abs(mk - dense) / (sd[:, None] * sd[None, :])))
        print("delay_covariance %s: markov against dense, worst |dcov_ij| / sqrt(cov_ii cov_jj) %.3g (bar 1e-6)" % (kernel, worst))
        assert worst <= 1e-6
        one, ok1 = fit.delay_covariance(obj, delays, a0, r0, free=[4], solver="markov")
        den, okd = fit.delay_covariance(obj, delays, a0, r0, free=[4])
        assert ok1 and okd and abs(one[0, 0] - den[0, 0]) <= 1e-6 * den[0, 0]
        with pytest.raises(ValueError):
            fit.delay_covariance(obj, delays, a0, r0, free=[3, 4], solver="markov")
        bad, okb = fit.delay_covariance(obj, delays, [0.0, 1.0], r0, solver="markov")
        assert not okb and np.isnan(bad).all()
        if kernel == "OU":
            ts = [np.sort(np.asarray(a, np.float64)) for a in t]
            tie = np.array([0.0, ts[1][7] - ts[0][9]])
            assert FC.tie_rows(t, tie)[0]
            nan, okt = fit.delay_covariance(obj, tie, a0, r0, solver="markov")
            assert not okt and np.isnan(nan).all()
            assert fit.delay_covariance(obj, tie, a0, r0)[0].shape == (4, 4)        # the dense entry has its convention there
