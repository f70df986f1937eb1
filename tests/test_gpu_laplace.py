"""gpcc_loglik_hess_hyper_batch and gpcc_laplace_evidence on the device: the hyper-parameter block bitwise against the
full Hessian, the Laplace evidence against an independent torch-autograd witness and against a quadrature through the value path,
the per-delay failure codes, and the other handle kinds."""
import math

import numpy as np
import pytest

import _grad_witness as GW
import _hess_witness as HW
import gpcc_amd
from gpcc_amd import laplace, synthetic

pytestmark = pytest.mark.gpu

KERNELS = [gpcc_amd.OU, gpcc_amd.rbf, gpcc_amd.matern32, gpcc_amd.matern52]
EPS = np.finfo(float).eps


def _bands(N, L):
    return [N // L + (1 if l < N % L else 0) for l in range(L)]


def _check_block(obj, delays, alpha, rho):
    """the block and everything else bitwise the full Hessian's leading block; returns the block call's outputs"""
    L = obj.L
    n = L + 1
    full = obj.loglik_hess_batch(delays, alpha, rho)
    blk = obj.loglik_hess_hyper_batch(delays, alpha, rho)
    assert np.array_equal(blk[0], full[0], equal_nan=True) and np.array_equal(blk[4], full[4])
    assert np.array_equal(blk[1], full[1], equal_nan=True)
    assert np.array_equal(blk[2], full[2][:, :n, :n], equal_nan=True)
    assert np.array_equal(blk[3], full[3][:, :n, :n], equal_nan=True)
    assert np.array_equal(blk[2], np.swapaxes(blk[2], 1, 2), equal_nan=True)
    return blk


# (a handle needs at least two points per band: N = 2 stands in for N = 1)
CASES = [(N, L) for N in (2, 60, 127, 129, 385, 1024) for L in (1, 2, 3, 8) if N >= 2 * L]


@pytest.mark.parametrize("N,L", CASES)
def test_block_is_bitwise_the_leading_block_of_the_full_hessian(N, L):
    i = CASES.index((N, L))
    kernel, mb = KERNELS[i % 4], (i // 4) % 2 == 0      # every kernel and both b-modes over the grid
    data = GW.ragged_data(_bands(N, L), seed=N + L)
    delays, alpha, rho = GW.random_params(L, 40, seed=i)
    with gpcc_amd.Objective(*data, kernel, marginalise_b=mb) as obj:
        blk = _check_block(obj, delays, alpha, rho)
        for M in (1, 7):                                # bitwise repeatable across batch sizes
            sub = _check_block(obj, delays[:M], alpha[:M], rho[:M])
            for x, y in zip(sub, blk):
                assert np.array_equal(x, y[:M], equal_nan=True)


def test_block_kernel_and_b_mode_matrix():
    """all four kernels in both b-modes at one size with two tiles"""
    data = GW.ragged_data([140, 120], seed=3)
    delays, alpha, rho = GW.random_params(2, 7, seed=4)
    for kernel in KERNELS:
        for mb in (True, False):
            with gpcc_amd.Objective(*data, kernel, marginalise_b=mb) as obj:
                _check_block(obj, delays, alpha, rho)


def test_block_nan_for_failed_rows():
    data = GW.ragged_data([300, 213], seed=8)
    delays, alpha, rho = GW.random_params(2, 6, seed=5)
    alpha[1, 1] = 0.0
    alpha[4] = [1e10, 1e10]
    rho[4] = 1e4
    good = [0, 2, 3, 5]
    with gpcc_amd.Objective(*data, gpcc_amd.rbf) as obj:
        ll, grad, hess, fisher, info = _check_block(obj, delays, alpha, rho)
        assert info[1] == -1 and info[4] > 0, info
        assert np.isnan(hess[[1, 4]]).all() and np.isnan(fisher[[1, 4]]).all() and np.isfinite(hess[good]).all()
        sub = obj.loglik_hess_hyper_batch(delays[good], alpha[good], rho[good])
        for x, y in zip(sub, (ll, grad, hess, fisher, info)):
            assert np.array_equal(x, y[good])


def test_block_at_n4096():
    data = synthetic.simulate_lightcurves([2048, 2048], seed=1)[:3]
    delays, alpha, rho = GW.random_params(2, 3, seed=6)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
        _check_block(obj, delays, alpha, rho)


def test_fp32_and_multi_device_handles_return_the_fp64_numbers():
    data = GW.ragged_data([200, 180], seed=9)
    delays, alpha, rho = GW.random_params(2, 5, seed=2)
    G = 4
    cand = np.array([[0.0, d] for d in (0.0, 1.0, 2.0, 3.0)])
    with gpcc_amd.Objective(*data, gpcc_amd.matern52) as o64:
        ref = o64.loglik_hess_hyper_batch(delays, alpha, rho)
        ref_ev = o64.laplace_evidence(cand, np.ones((G, 2)), np.full(G, 2.0))
    for kw in ({"precision": "fp32"}, {"devices": [0, 0]}):
        with gpcc_amd.Objective(*data, gpcc_amd.matern52, **kw) as o:
            got = o.loglik_hess_hyper_batch(delays, alpha, rho)
            for x, y in zip(ref, got):
                assert np.array_equal(x, y)
            got_ev = o.laplace_evidence(cand, np.ones((G, 2)), np.full(G, 2.0))
            for x, y in zip(ref_ev, got_ev):
                assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


# --- the evidence ---------------------------------------------------------------------------------------------------------
def _curve(N, seed):
    t, y, s, true = synthetic.simulate_lightcurves([N // 2, N - N // 2], seed=seed, sigma=0.3)
    return (t, y, s), float(true[1])


def _fit(obj, cand, rhomin=0.1, rhomax=20.0):
    ll, alpha, rho, info, its, _ = obj.grid_loglik(cand, 1000, rhomin=rhomin, rhomax=rhomax)
    assert np.all(info == 0)
    return ll, alpha, rho


def test_laplace_against_torch_witness():
    data, true = _curve(160, seed=4)
    cand = np.array([[0.0, true + d] for d in (-1.0, -0.4, 0.0, 0.3, 0.8)])
    with gpcc_amd.Objective(*data, gpcc_amd.OU) as obj:
        ll0, a0, r0 = _fit(obj, cand)
        g_tol = 1e-6
        ll, alpha, rho, logz, cov, info, rounds, stats = obj.laplace_evidence(cand, a0, r0, g_tol=g_tol)
        assert np.all(info == 0), info
        assert np.all(ll >= ll0 - 1e-9 * np.abs(ll0)), ll - ll0          # the polish never loses against its Nelder-Mead start
        _, grad, hess, _, hinfo = obj.loglik_hess_hyper_batch(cand, alpha, rho)
        theta = np.concatenate([alpha, rho[:, None]], 1)
        assert np.max(np.abs(theta * grad[:, :3])) <= g_tol                # |grad_u l|_inf <= g_tol at the returned mode
    print("Newton rounds per delay:", rounds, "evaluations, batches:", stats)
    for g in range(len(cand)):
        v, gr, H, _ = HW.hessian_and_fisher("OU", *data, cand[g], alpha[g], rho[g])
        gu, Hu = laplace.hyper_to_u(theta[g], gr, H[:3, :3])
        ref = v + 1.5 * math.log(2 * math.pi) - 0.5 * np.linalg.slogdet(-Hu)[1]
        band, t, _, Kn = HW._setup(*data, True)
        u = t - cand[g][band]
        K = alpha[g][band][:, None] * alpha[g][band][None, :] * HW.derivatives("OU", u[:, None] - u[None, :], rho[g])[0] + Kn
        bar = max(1e-6, 64 * EPS * np.linalg.cond(K, 1) * abs(ll[g]))
        assert abs(logz[g] - ref) <= bar, (g, logz[g], ref, bar)
        assert np.allclose(cov[g], np.linalg.inv(-Hu), rtol=1e-6, atol=0)


# The delay-dependent part of log Z_Laplace - log Z_quad (nats) and the total-variation distance of the two delay posteriors.
# Started at 0.05 nats and 0.02; observed at the first run on an MI355X: 0.0407 nats and 1.07e-7.
QUAD_BAR_NATS = 0.05
QUAD_BAR_TV = 2e-7


def _quad_device(obj, delay, u_hat, cov, nodes=41, R=7.0):
    C = np.linalg.cholesky(cov)
    z = np.linspace(-R, R, nodes)
    Z = np.stack(np.meshgrid(z, z, z, indexing="ij"), -1).reshape(-1, 3)
    U = u_hat + Z @ C.T
    M = len(U)
    ll, info = obj.loglik_batch(np.tile(delay, (M, 1)), np.exp(U[:, :2]), np.exp(U[:, 2]))   # the value path
    assert np.all(info == 0)
    w = np.full(nodes, z[1] - z[0])
    w[[0, -1]] *= 0.5
    W = (w[:, None, None] * w[None, :, None] * w[None, None, :]).ravel()
    top = ll.max()
    cube = ll.reshape(nodes, nodes, nodes) - top
    face = max(cube[[0, -1]].max(), cube[:, [0, -1]].max(), cube[:, :, [0, -1]].max())
    return top + math.log(np.sum(W * np.exp(ll - top))) + np.linalg.slogdet(C)[1], face


def test_laplace_against_quadrature_on_the_device():
    data, true = _curve(300, seed=2)
    cand = np.array([[0.0, true + d] for d in np.linspace(-1.4, 1.4, 8)])
    with gpcc_amd.Objective(*data, gpcc_amd.OU) as obj:
        _, a0, r0 = _fit(obj, cand)
        ll, alpha, rho, logz, cov, info, rounds, _ = obj.laplace_evidence(cand, a0, r0)
        assert np.all(info == 0), info
        quad, faces = [], []
        for g in range(len(cand)):
            u_hat = np.concatenate([np.log(alpha[g]), [np.log(rho[g])]])
            q, face = _quad_device(obj, cand[g], u_hat, cov[g])
            quad.append(q)
            faces.append(face)
        _, grad, hess, _, _ = obj.loglik_hess_hyper_batch(cand, alpha, rho)
    quad = np.array(quad)
    diff = logz - quad
    dd = np.max(np.abs(diff - diff.mean()))

    def post(x):
        e = np.exp(x - x.max())
        return e / e.sum()

    tv = 0.5 * np.abs(post(logz) - post(quad)).sum()
    # the log-Jacobian mutation (H_theta for H_u), from the device's outputs
    mut = np.array([ll[g] + 1.5 * math.log(2 * math.pi) - 0.5 * np.linalg.slogdet(-hess[g])[1] for g in range(len(cand))])
    dm = mut - quad
    ddm = np.max(np.abs(dm - dm.mean()))
    print("quadrature: delay-dependent |diff| %.4g nats (bar %g), TV %.4g (bar %g), log-Jacobian mutation %.4g nats; faces %.1f; "
          "rounds %s" % (dd, QUAD_BAR_NATS, tv, QUAD_BAR_TV, ddm, max(faces), list(rounds)))
    assert dd <= QUAD_BAR_NATS and tv <= QUAD_BAR_TV
    assert ddm > QUAD_BAR_NATS


def test_failure_codes():
    data, true = _curve(200, seed=5)
    cand = np.array([[0.0, true], [0.0, true + 0.5]])
    with gpcc_amd.Objective(*data, gpcc_amd.OU) as obj:
        _, a0, r0 = _fit(obj, cand)
        # the boundary: rho's box far below the data's rho
        ll, alpha, rho, logz, cov, info, rounds, _ = obj.laplace_evidence(cand, a0, np.full(2, 0.02), rhomin=0.01, rhomax=0.02)
        assert np.all(info == gpcc_amd._capi.LAPLACE_ON_BOUND), info
        assert np.all(rho == 0.02) or np.allclose(rho, 0.02, rtol=1e-15) and np.all(np.isnan(logz)) and np.all(np.isfinite(ll))
        assert np.all(np.isnan(logz))
        # not converged: one evaluation only
        ll, alpha, rho, logz, cov, info, rounds, _ = obj.laplace_evidence(cand, a0 * 1.3, r0 * 0.7, max_rounds=1)
        assert np.all(info == gpcc_amd._capi.LAPLACE_NOT_CONVERGED) and np.all(rounds == 1) and np.all(np.isnan(logz)), info
    # a start the device cannot evaluate (rbf, huge alpha and rho: a non-positive pivot) keeps the device's code; the other row is unaffected
    with gpcc_amd.Objective(*data, gpcc_amd.rbf) as obj:
        ref = obj.laplace_evidence(cand[:1], a0[:1], r0[:1])
        bad = obj.laplace_evidence(cand, np.array([a0[0], [1e10, 1e10]]), np.array([r0[0], 1e4]))
        assert bad[5][1] > 0 and np.isnan(bad[3][1]) and np.isnan(bad[0][1])
        for x, y in zip(ref[:7], bad[:7]):
            assert np.array_equal(np.asarray(x)[:1], np.asarray(y)[:1], equal_nan=True)


def test_gpcc_grid_with_laplace_evidence():
    data, true = _curve(110, seed=1)
    grid = np.arange(0.0, 5.01, 0.5)
    cand = np.stack([np.zeros_like(grid), grid], 1)
    res0 = gpcc_amd.fit.gpcc_grid(*data, kernel=gpcc_amd.OU, candidatedelays=cand, iterations=1000)
    res = gpcc_amd.fit.gpcc_grid(*data, kernel=gpcc_amd.OU, candidatedelays=cand, iterations=1000, evidence="laplace")
    assert res0.log_evidence is None
    assert np.array_equal(res0.loglikel, res.loglikel) and np.array_equal(res0.alpha, res.alpha)
    ok = res.laplace_info == 0
    assert ok.sum() >= len(grid) // 2, res.laplace_info
    assert np.all(np.isnan(res.log_evidence[~ok]))
    assert res.hyper_cov.shape == (len(grid), 3, 3) and np.all(np.isfinite(res.log_evidence[ok]))
    p = gpcc_amd.getprobabilities(res.log_evidence[ok])
    assert abs(p.sum() - 1.0) < 1e-12
