"""gpcc_loglik_hess_batch on the device: against the torch witness and the term-by-term formula (tests/_hess_witness.py), a bar that
rejects injected slips, tile and band edges, exact properties, central differences of the device's own gradient at N = 4096, the
contracts of the gradient path (repeatability, contained failures, other handles, no cost to handles that never ask), and a
second-order fit end to end."""
import numpy as np
import pytest

import _grad_witness as GW
import _hess_witness as HW
import gpcc_amd
from gpcc_amd import fit, synthetic

pytestmark = pytest.mark.gpu

KERNELS = {"OU": gpcc_amd.OU, "rbf": gpcc_amd.rbf, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
SIZES = {60: [35, 25], 110: [40, 35, 35], 150: [80, 70], 513: [300, 213], 1024: [600, 424]}
# relative to max |H_ref| (and max |F_ref| for F).  Calibrated on the first run from 1e-8: the worst rows, Matern-3/2 and -5/2 at
# N = 1024 without b, came to 1.4 and 2.0 x 1e-8 (K well conditioned, cond_1 ~ 4e4: H is the small difference of T1, T2 and T3); every
# other kernel, size and b-mode stayed below 0.41 x 1e-8.
BAR = 1e-7


def ratio(H, ref, cond=0.0):
    """error / bar, bar = max(BAR, 64 eps64 cond_1(K)) max|ref| (the fp64 witness is itself only good to ~eps cond(K))"""
    return np.max(np.abs(H - ref)) / (max(BAR, 64 * np.finfo(float).eps * cond) * np.max(np.abs(ref)))


def cond1(name, data, delays, alpha, rho, mb):
    band, t, _, Kn = HW._setup(*data, mb)
    u = t - np.asarray(delays, float)[band]
    S = u[:, None] - u[None, :]
    a = np.asarray(alpha, float)[band]
    return np.linalg.cond(a[:, None] * a[None, :] * HW.derivatives(name, S, float(rho))[0] + Kn, 1)


def _exact(L, ll, grad, hess, fisher, info, gl, gg, ginfo):
    """bitwise symmetry, the gradient path's bits, translation invariance, F positive semi-definite to rounding"""
    assert np.array_equal(info, ginfo) and np.array_equal(ll, gl) and np.array_equal(grad, gg)
    assert np.array_equal(hess, np.swapaxes(hess, 1, 2)) and np.array_equal(fisher, np.swapaxes(fisher, 1, 2))
    for i in np.flatnonzero(info == 0):
        sc = np.max(np.abs(hess[i]))
        if L > 1:
            assert np.max(np.abs(hess[i][:, L + 1:].sum(1))) <= 1e-9 * sc, hess[i]
            assert np.max(np.abs(fisher[i][:, L + 1:].sum(1))) <= 1e-9 * sc, fisher[i]
        assert np.linalg.eigvalsh(fisher[i]).min() >= -1e-9 * np.max(np.abs(fisher[i]))


def _run(obj, delays, alpha, rho):
    out = obj.loglik_hess_batch(delays, alpha, rho)
    g = obj.loglik_grad_batch(delays, alpha, rho)
    _exact(obj.L, *out, *g)
    return out


@pytest.mark.parametrize("N", sorted(SIZES))
@pytest.mark.parametrize("mb", [True, False])
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_device_hessian_matches_witness(name, mb, N):
    data = GW.ragged_data(SIZES[N], seed=N)
    L = len(SIZES[N])
    worst = 0.0
    with gpcc_amd.Objective(*data, KERNELS[name], marginalise_b=mb) as obj:
        for M in (1, 7, 40):
            delays, alpha, rho = GW.random_params(L, M, seed=M + N)
            ll, grad, hess, fisher, info = _run(obj, delays, alpha, rho)
            assert hess.shape == (M, 2 * L + 1, 2 * L + 1) and (info == 0).all(), info
            rows = list(range(M)) if N <= 150 else sorted({M // 2})
            for i in rows:
                _, _, Hr, Fr = HW.hessian_and_fisher(name, *data, delays[i], alpha[i], rho[i], mb)
                c = cond1(name, data, delays[i], alpha[i], rho[i], mb)
                r = max(ratio(hess[i], Hr, c), ratio(fisher[i], Fr, c))
                assert r <= 1.0, (i, r, c, hess[i], Hr)
                worst = max(worst, r)
    print("%s mb=%s N=%d: worst error / bar %.3g" % (name, mb, N, worst))   # (bar: max(1e-8, 64 eps cond_1(K)) max|H_ref|)


def test_bar_rejects_injected_slips():
    # (one band of 300 points, alpha = rho = 1: an entry in rho is not small against max |H| there, so a relative slip of k_rr shows)
    data = GW.ragged_data([300], seed=300)
    delays, alpha, rho = np.zeros((1, 1)), np.ones((1, 1)), np.ones(1)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
        _, _, hess, _, info = obj.loglik_hess_batch(delays, alpha, rho)
    assert info[0] == 0
    args = (data[0], data[1], data[2], delays[0], alpha[0], rho[0], True)
    ref, _ = HW.formula("matern32", *args)
    r0 = ratio(hess[0], ref)
    assert r0 <= 1.0, r0
    closest = np.inf
    for slip in ("no_t2", "t3_tile_once", "krr"):
        bad, _ = HW.formula("matern32", *args, slip=slip)
        r = ratio(hess[0], bad)
        assert r > 1.0, (slip, r)
        closest = min(closest, r)
        print("slip %s: error / bar %.3g" % (slip, r))
    print("device against the formula: %.3g of the bar; closest slip at %.3g x the bar" % (r0, closest))


def test_ou_convention_at_coinciding_shifted_times():
    data = HW.ou_coincident_data()
    alpha, rho = np.array([[1.1, 0.9]]), np.array([2.0])
    delays = np.array([[0.0, 1.5]])
    for mb in (False, True):
        with gpcc_amd.Objective(*data, gpcc_amd.OU, marginalise_b=mb) as obj:
            _, _, hess, fisher, info = obj.loglik_hess_batch(delays, alpha, rho)
        assert info[0] == 0
        H, F = HW.formula("OU", *data, delays[0], alpha[0], rho[0], mb)
        assert ratio(hess[0], H) <= 1.0 and ratio(fisher[0], F) <= 1.0, (hess[0], H)


# N -> band lengths: band boundaries at, before and after tile edges
EDGES = {1: [1], 2: [2], 127: [60, 67], 128: [100, 28], 129: [127, 2], 257: [128, 129], 385: [129, 127, 129], 641: [128, 384, 129]}


def test_tile_and_band_edges():
    worst = 0.0
    for N, Nl in EDGES.items():
        data = GW.ragged_data(Nl, seed=N)
        L = len(Nl)
        delays, alpha, rho = GW.random_params(L, 3, seed=N + 1)
        for ki, name in enumerate(KERNELS):
            mb = min(Nl) >= 2 and ki % 2 == 0
            with gpcc_amd.Objective(*data, KERNELS[name], marginalise_b=mb, slots_per_stream=8) as obj:
                ll, grad, hess, fisher, info = _run(obj, delays, alpha, rho)
            assert (info == 0).all(), (N, name, info)
            for i in ([0, 1, 2] if N < 600 else [ki % 3]):
                _, _, Hr, Fr = HW.hessian_and_fisher(name, *data, delays[i], alpha[i], rho[i], mb)
                c = cond1(name, data, delays[i], alpha[i], rho[i], mb)
                r = max(ratio(hess[i], Hr, c), ratio(fisher[i], Fr, c))
                assert r <= 1.0, (N, name, i, r, c)
                worst = max(worst, r)
    # eight bands spanning tiles
    Nl = [20, 100, 30, 140, 9, 60, 130, 50]
    data = GW.ragged_data(Nl, seed=8)
    delays, alpha, rho = GW.random_params(8, 3, seed=88)
    with gpcc_amd.Objective(*data, gpcc_amd.matern52) as obj:
        ll, grad, hess, fisher, info = _run(obj, delays, alpha, rho)
    assert hess.shape == (3, 17, 17) and (info == 0).all()
    _, _, Hr, Fr = HW.hessian_and_fisher("matern52", *data, delays[1], alpha[1], rho[1], True)
    c = cond1("matern52", data, delays[1], alpha[1], rho[1], True)
    r = max(ratio(hess[1], Hr, c), ratio(fisher[1], Fr, c))
    assert r <= 1.0, (r, c)
    print("edges: worst error / bar %.3g (eight bands %.3g)" % (max(worst, r), r))


@pytest.mark.parametrize("case", ["matern32_4096", "matern52_4095"])
def test_large_n_against_differences_of_the_gradient(case):
    if case == "matern32_4096":
        name, Nl = "matern32", [2048, 2048]
    else:
        name, Nl = "matern52", [1500, 1300, 1295]
    data = GW.ragged_data(Nl, seed=len(Nl))
    L = len(Nl)
    delays, alpha, rho = GW.random_params(L, 1, seed=3)
    with gpcc_amd.Objective(*data, KERNELS[name]) as obj:
        ll, grad, hess, fisher, info = _run(obj, delays, alpha, rho)
        assert info[0] == 0
        x0 = np.concatenate([alpha[0], rho, delays[0]])
        h = 1e-4 * np.maximum(np.abs(x0), 1.0)
        X = np.repeat(x0[None, :], 2 * len(x0), 0)
        for i in range(len(x0)):
            X[2 * i, i] += h[i]
            X[2 * i + 1, i] -= h[i]
        _, gf, finfo = obj.loglik_grad_batch(X[:, L + 1:], X[:, :L], X[:, L])
        assert (finfo == 0).all()
    fd = ((gf[0::2] - gf[1::2]) / (2 * h[:, None])).T   # column j: d grad / d x_j
    err = np.max(np.abs(hess[0] - fd)) / np.max(np.abs(hess[0]))
    print("%s: max |H - differences of the gradient| / max |H| = %.3g" % (case, err))
    assert err <= 1e-5, (hess[0], fd)


def test_bitwise_repeatable_across_calls_and_batch_sizes():
    data = GW.ragged_data([300, 213], seed=7)
    delays, alpha, rho = GW.random_params(2, 40, seed=11)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
        a = obj.loglik_hess_batch(delays, alpha, rho)
        b = obj.loglik_hess_batch(delays, alpha, rho)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        for lo, hi in ((0, 1), (13, 14), (39, 40), (10, 17)):
            part = obj.loglik_hess_batch(delays[lo:hi], alpha[lo:hi], rho[lo:hi])
            for x, y in zip(part, a):
                assert np.array_equal(x, y[lo:hi])


def test_failures_stay_contained():
    data = GW.ragged_data([300, 213], seed=8)
    delays, alpha, rho = GW.random_params(2, 6, seed=5)
    alpha[1, 1] = 0.0
    rho[3] = -1.0
    alpha[4] = [1e10, 1e10]
    rho[4] = 1e4
    good = [0, 2, 5]
    with gpcc_amd.Objective(*data, gpcc_amd.rbf) as obj:
        ll, grad, hess, fisher, info = obj.loglik_hess_batch(delays, alpha, rho)
        assert info[1] == -1 and info[3] == -2 and info[4] > 0, info
        assert (info[good] == 0).all()
        bad = [1, 3, 4]
        assert np.isnan(ll[bad]).all() and np.isnan(grad[bad]).all() and np.isnan(hess[bad]).all() and np.isnan(fisher[bad]).all()
        sub = obj.loglik_hess_batch(delays[good], alpha[good], rho[good])
        for x, y in zip(sub, (ll, grad, hess, fisher, info)):
            assert np.array_equal(x, y[good])
    _, _, Hr, _ = HW.hessian_and_fisher("rbf", *data, delays[0], alpha[0], rho[0])
    assert ratio(hess[0], Hr) <= 1.0


def test_fp32_and_multi_device_handles_return_the_fp64_numbers():
    data = GW.ragged_data([600, 424], seed=9)
    delays, alpha, rho = GW.random_params(2, 7, seed=2)
    with gpcc_amd.Objective(*data, gpcc_amd.matern52) as o64:
        ref = o64.loglik_hess_batch(delays, alpha, rho)
    with gpcc_amd.Objective(*data, gpcc_amd.matern52, precision="fp32") as o32:
        got = o32.loglik_hess_batch(delays, alpha, rho)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y)
    with gpcc_amd.Objective(*data, gpcc_amd.matern52, devices=[0, 0]) as om:
        got = om.loglik_hess_batch(delays, alpha, rho)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y)


def test_handle_without_hessian_is_unchanged():
    data = GW.ragged_data([300, 213], seed=12)
    delays, alpha, rho = GW.random_params(2, 16, seed=4)
    with gpcc_amd.Objective(*data, gpcc_amd.OU) as a, gpcc_amd.Objective(*data, gpcc_amd.OU) as b:
        v0 = a.loglik_batch(delays, alpha, rho)
        g0 = a.loglik_grad_batch(delays, alpha, rho)
        b.loglik_batch(delays, alpha, rho)
        b.loglik_grad_batch(delays, alpha, rho)
        keys = ("bytes_per_slot", "workspace_slots", "workspace_streams")
        ref = [a.get_option(k) for k in keys]
        assert a.get_option("hess_slots") == 0 and a.get_option("hess_bytes_per_slot") > 0
        b.loglik_hess_batch(delays, alpha, rho)
        assert [b.get_option(k) for k in keys] == ref and [a.get_option(k) for k in keys] == ref
        assert 1 <= b.get_option("hess_slots") <= ref[1] * ref[2]
        for obj in (a, b):   # values and gradients of both handles after the Hessian call: the same bits
            v1 = obj.loglik_batch(delays, alpha, rho)
            g1 = obj.loglik_grad_batch(delays, alpha, rho)
            assert np.array_equal(v0[0], v1[0]) and np.array_equal(v0[1], v1[1])
            for x, y in zip(g0, g1):
                assert np.array_equal(x, y)


def test_trust_region_fit_reaches_the_nelder_mead_optimum():
    from scipy.optimize import minimize
    t, y, s, true_delays = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    L, rhomin, rhomax, seed = 2, 0.1, 20.0, 1
    delays = np.asarray(true_delays, dtype=np.float64)
    ll_nm, _, (alpha_nm, _, rho_nm) = gpcc_amd.gpcc(t, y, s, kernel=gpcc_amd.OU, delays=delays, iterations=1000, rhomin=rhomin,
                                                    rhomax=rhomax, seed=seed)
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
        cache = {}

        def ev(x):
            key = x.tobytes()
            if key not in cache:
                calls[0] += 1
                a = fit.makepositive(x[:L]) + 1e-8
                r = float(fit.transformbetween(x[L], rhomin, rhomax))
                ll, grad, hess, _, info = obj.loglik_hess_batch(delays[None, :], a[None, :], [r])
                assert info[0] == 0
                gx = fit.unpack_grad(x, grad[0, :L + 1], L, rhomin, rhomax)
                hx = fit.unpack_hessian(x, grad[0, :L + 1], hess[0, :L + 1, :L + 1], L, rhomin, rhomax)
                cache[key] = (-ll[0], -gx, -hx)
            return cache[key]

        res = minimize(lambda x: ev(x)[0], x0, jac=lambda x: ev(x)[1], hess=lambda x: ev(x)[2], method="trust-exact")
        ll_tr = -res.fun
        print("trust-exact: loglik %.10f in %d value+gradient+Hessian evaluations; Nelder-Mead (iterations = 1000): %.10f"
              % (ll_tr, calls[0], ll_nm))
        assert ll_tr >= ll_nm - 1e-6 * abs(ll_nm), (ll_tr, ll_nm)
        # curvature at the optimum: -diag(H) over (alpha, rho) against second differences of the device's values
        a = fit.makepositive(res.x[:L]) + 1e-8
        r = float(fit.transformbetween(res.x[L], rhomin, rhomax))
        _, _, hess, _, info = obj.loglik_hess_batch(delays[None, :], a[None, :], [r])
        x0c = np.concatenate([a, [r], delays])
        h = 1e-3 * np.maximum(np.abs(x0c[:L + 1]), 1.0)
        X = np.repeat(x0c[None, :], 2 * (L + 1) + 1, 0)
        for j in range(L + 1):
            X[2 * j + 1, j] += h[j]
            X[2 * j + 2, j] -= h[j]
        lv, linfo = obj.loglik_batch(X[:, L + 1:], X[:, :L], X[:, L])
        assert (linfo == 0).all()
        d2 = np.array([(lv[2 * j + 1] - 2 * lv[0] + lv[2 * j + 2]) / h[j] ** 2 for j in range(L + 1)])
        dh = np.diag(hess[0])[:L + 1]
        assert np.max(np.abs(dh - d2) / np.abs(dh)) <= 1e-4, (dh, d2)
        cov, ok = fit.laplace_covariance(hess[0], list(range(L + 1)))
        assert ok and np.linalg.eigvalsh(cov).min() > 0
        print("standard errors of (alpha, rho) at the optimum: %s" % np.sqrt(np.diag(cov)))
