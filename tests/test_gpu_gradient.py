"""gpcc_loglik_grad_batch on the device: against the torch-autograd witness (tests/_grad_witness.py), against central differences
of the device's own values at N = 4096, and its contracts (repeatability, contained failures, other handles, no cost to handles
that never ask for it), and one quasi-Newton fit end to end."""
import numpy as np
import pytest

import _grad_witness as W
import gpcc_amd
from gpcc_amd import fit, synthetic

pytestmark = pytest.mark.gpu

KERNELS = {"OU": gpcc_amd.OU, "rbf": gpcc_amd.rbf, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
SIZES = {60: [35, 25], 110: [40, 35, 35], 150: [80, 70], 513: [300, 213], 1024: [600, 424]}


def _check_rows(name, data, mb, delays, alpha, rho, ll, grad, info):
    assert (info == 0).all(), info
    for i in range(len(rho)):
        lw, gw = W.loglik_and_grad(name, *data, delays[i], alpha[i], rho[i], mb)
        tol = 1e-8 * max(1.0, np.max(np.abs(gw)))
        assert np.max(np.abs(grad[i] - gw)) <= tol, (i, grad[i], gw)
        L = len(alpha[i])
        if L > 1:
            gt = grad[i, L + 1:]
            assert abs(gt.sum()) <= 1e-9 * np.linalg.norm(gt), gt


@pytest.mark.parametrize("N", sorted(SIZES))
@pytest.mark.parametrize("mb", [True, False])
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_device_gradient_matches_witness(oracle, name, mb, N):
    data = W.ragged_data(SIZES[N], seed=N)
    L = len(SIZES[N])
    with gpcc_amd.Objective(*data, KERNELS[name], marginalise_b=mb) as obj:
        for M in (1, 7, 40):
            delays, alpha, rho = W.random_params(L, M, seed=M + N)
            ll, grad, info = obj.loglik_grad_batch(delays, alpha, rho)
            assert grad.shape == (M, 2 * L + 1)
            ref, rinfo = obj.loglik_batch(delays, alpha, rho)
            assert (rinfo == 0).all()
            assert np.max(np.abs(ll - ref) / np.abs(ref)) <= 1e-11
            # (the CPU references' time: every row up to N = 150, a spread of rows above)
            rows = list(range(M)) if N <= 150 else sorted({0, M // 2, M - 1})
            orc, oinfo = oracle.loglik_batch(name, *data, delays[rows], alpha[rows], rho[rows], mb, nthreads=8)
            assert (oinfo == 0).all() and np.max(np.abs(ll[rows] - orc) / np.abs(orc)) <= 1e-8
            _check_rows(name, data, mb, delays[rows], alpha[rows], rho[rows], ll[rows], grad[rows], info[rows])


@pytest.mark.parametrize("case", ["matern32_4096", "matern52_4095"])
def test_large_n_against_finite_differences(case):
    if case == "matern32_4096":
        name, Nl = "matern32", [2048, 2048]
    else:
        name, Nl = "matern52", [1500, 1300, 1295]
    data = W.ragged_data(Nl, seed=len(Nl))
    L = len(Nl)
    delays, alpha, rho = W.random_params(L, 1, seed=3)
    with gpcc_amd.Objective(*data, KERNELS[name]) as obj:
        ll, grad, info = obj.loglik_grad_batch(delays, alpha, rho)
        assert info[0] == 0
        ref, _ = obj.loglik_batch(delays, alpha, rho)
        assert abs(ll[0] - ref[0]) <= 1e-11 * abs(ref[0])
        x0 = np.concatenate([alpha[0], rho, delays[0]])
        H = 1e-5 * np.maximum(np.abs(x0), 1.0)
        X = np.repeat(x0[None, :], 2 * len(x0), 0)
        for i in range(len(x0)):
            X[2 * i, i] += H[i]
            X[2 * i + 1, i] -= H[i]
        lf, finfo = obj.loglik_batch(X[:, L + 1:], X[:, :L], X[:, L])
        assert (finfo == 0).all()
        fd = (lf[0::2] - lf[1::2]) / (2 * H)
        g = grad[0]
        assert np.max(np.abs(g - fd)) <= 1e-5 * np.linalg.norm(g), (g, fd)
        assert abs(g[L + 1:].sum()) <= 1e-9 * np.linalg.norm(g[L + 1:])


def test_bitwise_repeatable_across_calls_and_batch_sizes():
    data = W.ragged_data([300, 213], seed=7)
    delays, alpha, rho = W.random_params(2, 40, seed=11)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
        a = obj.loglik_grad_batch(delays, alpha, rho)
        b = obj.loglik_grad_batch(delays, alpha, rho)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        for i in (0, 13, 39):
            one = obj.loglik_grad_batch(delays[i:i + 1], alpha[i:i + 1], rho[i:i + 1])
            assert np.array_equal(one[0][0], a[0][i]) and np.array_equal(one[1][0], a[1][i])
        seven = obj.loglik_grad_batch(delays[10:17], alpha[10:17], rho[10:17])
        assert np.array_equal(seven[1], a[1][10:17]) and np.array_equal(seven[0], a[0][10:17])


def test_failures_stay_contained():
    data = W.ragged_data([300, 213], seed=8)
    delays, alpha, rho = W.random_params(2, 6, seed=5)
    alpha[1, 1] = 0.0                       # alpha <= 0
    rho[3] = -1.0                           # rho <= 0
    alpha[4] = [1e10, 1e10]                 # rbf: K numerically singular -> non-positive pivot
    rho[4] = 1e4
    good = [0, 2, 5]
    with gpcc_amd.Objective(*data, gpcc_amd.rbf) as obj:
        ll, grad, info = obj.loglik_grad_batch(delays, alpha, rho)
        assert info[1] == -1 and info[3] == -2 and info[4] > 0, info
        assert (info[good] == 0).all()
        assert np.isnan(ll[[1, 3, 4]]).all() and np.isnan(grad[[1, 3, 4]]).all()
        ll_g, grad_g, info_g = obj.loglik_grad_batch(delays[good], alpha[good], rho[good])
        assert np.array_equal(ll[good], ll_g) and np.array_equal(grad[good], grad_g)
        lw, gw = W.loglik_and_grad("rbf", *data, delays[0], alpha[0], rho[0])
        assert np.max(np.abs(grad[0] - gw)) <= 1e-8 * max(1.0, np.max(np.abs(gw)))
        with pytest.raises(AssertionError):
            obj.value_and_grad(alpha[1], rho[1], delays[1])
        with pytest.raises(ValueError):
            obj.value_and_grad(alpha[3], rho[3], delays[3])
        with pytest.raises(gpcc_amd.PosDefException):
            obj.value_and_grad(alpha[4], rho[4], delays[4])
        v, g = obj.value_and_grad(alpha[0], rho[0], delays[0])
        assert v == ll[0] and np.array_equal(g["alpha"], grad[0, :2]) and g["rho"] == grad[0, 2]
        assert np.array_equal(g["delays"], grad[0, 3:])


def test_fp32_and_multi_device_handles_return_the_fp64_numbers():
    data = W.ragged_data([600, 424], seed=9)
    delays, alpha, rho = W.random_params(2, 7, seed=2)
    with gpcc_amd.Objective(*data, gpcc_amd.matern52) as o64:
        ref = o64.loglik_grad_batch(delays, alpha, rho)
    with gpcc_amd.Objective(*data, gpcc_amd.matern52, precision="fp32") as o32:
        got = o32.loglik_grad_batch(delays, alpha, rho)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y)
    with gpcc_amd.Objective(*data, gpcc_amd.matern52, devices=[0, 0]) as om:
        got = om.loglik_grad_batch(delays, alpha, rho)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y)


def test_handle_without_gradient_is_unchanged():
    data = W.ragged_data([300, 213], seed=12)
    delays, alpha, rho = W.random_params(2, 16, seed=4)
    with gpcc_amd.Objective(*data, gpcc_amd.OU) as a, gpcc_amd.Objective(*data, gpcc_amd.OU) as b:
        before = a.loglik_batch(delays, alpha, rho)
        b.loglik_batch(delays, alpha, rho)
        keys = ("bytes_per_slot", "workspace_slots", "workspace_streams")
        ref = [a.get_option(k) for k in keys]
        b.loglik_grad_batch(delays, alpha, rho)
        assert [b.get_option(k) for k in keys] == ref
        after = a.loglik_batch(delays, alpha, rho)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        again = b.loglik_batch(delays, alpha, rho)   # the handle that did ask still computes the same values
        assert np.array_equal(again[0], after[0])


def test_lbfgs_fit_reaches_the_nelder_mead_optimum():
    from scipy.optimize import minimize
    t, y, s, true_delays = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    L, rhomin, rhomax, seed = 2, 0.1, 20.0, 1
    delays = np.asarray(true_delays, dtype=np.float64)
    ll_nm, _, (alpha_nm, _, rho_nm) = gpcc_amd.gpcc(t, y, s, kernel=gpcc_amd.OU, delays=delays, iterations=1000, rhomin=rhomin,
                                                    rhomax=rhomax, seed=seed)
    # the native fit's start: the best of its random candidates (fit.gpcc_grid's draw, numberofrestarts = 1, initialrandom = 5)
    rg = np.random.default_rng(seed)
    rho0 = rg.uniform(rhomin + 1e-3, rhomax - 1e-3, 1)
    vary = np.array([np.var(v, ddof=1) for v in y])
    cands = np.array([np.concatenate([fit.invmakepositive(vary * (rg.random(L) * 0.4 + 0.8)),
                                      [fit.invtransformbetween(rho0[0], rhomin, rhomax)]]) for _ in range(5)])
    calls = [0]
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        a0 = fit.makepositive(cands[:, :L]) + 1e-8
        r0 = fit.transformbetween(cands[:, L], rhomin, rhomax)
        l0, _ = obj.loglik_batch(np.tile(delays, (5, 1)), a0, r0)
        x0 = cands[int(np.nanargmax(l0))]

        def f(x):
            calls[0] += 1
            a = fit.makepositive(x[:L]) + 1e-8
            r = float(fit.transformbetween(x[L], rhomin, rhomax))
            ll, grad, info = obj.loglik_grad_batch(delays[None, :], a[None, :], [r])
            if info[0] != 0:
                return np.inf, np.zeros(L + 1)
            return -ll[0], -fit.unpack_grad(x, grad[0, :L + 1], L, rhomin, rhomax)

        res = minimize(f, x0, jac=True, method="L-BFGS-B")
    ll_bfgs = -res.fun
    print("L-BFGS-B: loglik %.10f in %d value+gradient evaluations; Nelder-Mead (iterations = 1000): %.10f"
          % (ll_bfgs, calls[0], ll_nm))
    assert ll_bfgs >= ll_nm - 1e-6 * abs(ll_nm), (ll_bfgs, ll_nm)
