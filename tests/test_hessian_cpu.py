"""The Hessian's witnesses on the CPU (tests/_hess_witness.py): the torch Hessian against central differences of the gradient witness,
the term-by-term numpy formula against the torch Hessian and Fisher information, and fit.unpack_hessian / fit.laplace_covariance."""
import numpy as np
import pytest
import torch

import _grad_witness as GW
import _hess_witness as HW
from gpcc_amd import fit

KERNELS = ["OU", "rbf", "matern32", "matern52"]
SIZES = {1: [23], 2: [19, 31], 3: [17, 9, 26]}


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("mb", [True, False])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_witness_hessian_against_gradient_differences(kernel, mb, L):
    data = GW.ragged_data(SIZES[L], seed=20 * L + KERNELS.index(kernel))
    delays, alpha, rho = GW.random_params(L, 2, seed=L + 7)
    for i in range(2):
        ll, g, H, F = HW.hessian_and_fisher(kernel, *data, delays[i], alpha[i], rho[i], mb)
        lw, gw = GW.loglik_and_grad(kernel, *data, delays[i], alpha[i], rho[i], mb)
        assert abs(ll - lw) <= 1e-12 * abs(lw) and np.max(np.abs(g - gw)) <= 1e-10 * max(1.0, np.max(np.abs(gw)))
        x0 = np.concatenate([alpha[i], [rho[i]], delays[i]])
        cols = []
        for j in range(len(x0)):
            h = 1e-5 * max(1.0, abs(x0[j]))
            xp, xm = x0.copy(), x0.copy()
            xp[j] += h
            xm[j] -= h
            gp = GW.loglik_and_grad(kernel, *data, xp[L + 1:], xp[:L], xp[L], mb)[1]
            gm = GW.loglik_and_grad(kernel, *data, xm[L + 1:], xm[:L], xm[L], mb)[1]
            cols.append((gp - gm) / (2 * h))
        fd = np.array(cols).T
        assert np.max(np.abs(H - fd)) <= 1e-6 * max(1.0, np.max(np.abs(H))), (H, fd)
        assert np.array_equal(H, H.T) or np.max(np.abs(H - H.T)) <= 1e-12 * np.max(np.abs(H))
        assert np.linalg.eigvalsh(0.5 * (F + F.T)).min() >= -1e-10 * np.max(np.abs(F))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("mb", [True, False])
def test_formula_matches_the_torch_witness(kernel, mb):
    data = GW.ragged_data([21, 17, 12], seed=3 + KERNELS.index(kernel))
    delays, alpha, rho = GW.random_params(3, 2, seed=9)
    for i in range(2):
        _, _, H, F = HW.hessian_and_fisher(kernel, *data, delays[i], alpha[i], rho[i], mb)
        Hf, Ff = HW.formula(kernel, *data, delays[i], alpha[i], rho[i], mb)
        scale = np.max(np.abs(H))
        assert np.max(np.abs(Hf - H)) <= 1e-10 * scale, (Hf, H)
        assert np.max(np.abs(Ff - F)) <= 1e-10 * np.max(np.abs(F)), (Ff, F)
        # translation invariance: each row sums to zero over the delays
        assert np.max(np.abs(Hf[:, 4:].sum(1))) <= 1e-10 * scale


def test_fisher_is_the_trace_with_numpy():
    """F = 1/2 tr(K^-1 D_i K^-1 D_j) with D_i by central differences of K in numpy."""
    data = GW.ragged_data([15, 20], seed=4)
    delays, alpha, rho = np.array([0.0, 1.3]), np.array([0.8, 1.4]), 2.2
    _, _, _, F = HW.hessian_and_fisher("matern52", *data, delays, alpha, rho, True)
    band, t, _, Kn = HW._setup(*data, True)

    def K(x):
        u = t - x[3:][band]
        S = u[:, None] - u[None, :]
        return x[:2][band][:, None] * x[:2][band][None, :] * HW.derivatives("matern52", S, x[2])[0] + Kn

    x0 = np.concatenate([alpha, [rho], delays])
    D = []
    for j in range(5):
        e = np.zeros(5)
        e[j] = 1e-6
        D.append((K(x0 + e) - K(x0 - e)) / 2e-6)
    C = np.linalg.inv(K(x0))
    Fn = np.array([[0.5 * np.trace(C @ D[a] @ C @ D[b]) for b in range(5)] for a in range(5)])
    assert np.max(np.abs(F - Fn)) <= 1e-7 * np.max(np.abs(F)), (F, Fn)


def test_ou_convention_at_coinciding_shifted_times():
    """At s = 0 the formula takes k_s = 0, k_rs = 0 and k_ss = 1/rho^2; the entries without an s-derivative, (alpha, rho) x (alpha,
    rho), are continuous through the kink and match torch just beside it."""
    data = HW.ou_coincident_data()
    alpha, rho = np.array([1.1, 0.9]), 2.0
    band, t, _, _ = HW._setup(*data, False)
    u = t - np.array([0.0, 1.5])[band]
    S = u[:, None] - u[None, :]
    assert S[0, 6] == 0.0
    k = HW.derivatives("OU", S, rho)
    assert k[2][0, 6] == 0.0 and k[4][0, 6] == 0.0 and k[5][0, 6] == 1.0 / rho ** 2
    H, F = HW.formula("OU", *data, [0.0, 1.5], alpha, rho, False)
    assert np.isfinite(H).all() and np.array_equal(H, H.T) and np.array_equal(F, F.T)
    _, _, Ht, _ = HW.hessian_and_fisher("OU", *data, [0.0, 1.5 + 1e-9], alpha, rho, False)
    assert np.max(np.abs(H[:3, :3] - Ht[:3, :3])) <= 1e-6 * np.max(np.abs(Ht[:3, :3]))


@pytest.mark.parametrize("L", [1, 2, 3])
def test_unpack_hessian_against_autograd_through_the_transforms(L):
    data = GW.ragged_data(SIZES[L], seed=30 + L)
    rhomin, rhomax = 0.1, 20.0
    rg = np.random.default_rng(L)
    delays = np.concatenate([[0.0], rg.uniform(-2, 4, L - 1)])
    x = np.concatenate([rg.uniform(-1.0, 1.5, L), [rg.uniform(-2.0, 1.0)]])
    if L >= 2:
        x[1] = 31.0   # the identity branch of makepositive
    a = fit.makepositive(x[:L]) + 1e-8
    r = float(fit.transformbetween(x[L], rhomin, rhomax))
    _, g, H, _ = HW.hessian_and_fisher("matern32", *data, delays, a, r, True)
    Hx = fit.unpack_hessian(x, g, H, L, rhomin, rhomax)
    assert Hx.shape == H.shape
    # torch: the objective through softplus / logistic in (x, tau)
    band, t_np, r_np, Kn_np = HW._setup(*data, True)
    b = torch.tensor(band)
    t = torch.tensor(t_np, dtype=torch.float64)
    rr = torch.tensor(r_np, dtype=torch.float64)[:, None]
    Kn = torch.tensor(Kn_np, dtype=torch.float64)

    def ll(z):
        xa, xr, tau = z[:L], z[L], z[L + 1:]
        al = torch.where(xa > 30.0, xa, torch.log1p(torch.exp(torch.clamp(xa, max=30.0)))) + 1e-8
        rh = rhomin + (rhomax - rhomin) / (1.0 + torch.exp(-xr))
        u = t - tau[b]
        S = u[:, None] - u[None, :]
        K = al[b][:, None] * al[b][None, :] * GW._kernel("matern32", S, rh) + Kn
        C = torch.linalg.cholesky(K)
        zz = torch.linalg.solve_triangular(C, rr, upper=False)
        return -0.5 * (zz * zz).sum() - torch.log(torch.diagonal(C)).sum()

    z0 = torch.tensor(np.concatenate([x, delays]), dtype=torch.float64)
    Ht = torch.autograd.functional.hessian(ll, z0).numpy()
    assert np.max(np.abs(Hx - Ht)) <= 1e-9 * max(1.0, np.max(np.abs(Ht))), (Hx, Ht)
    # without the delays, and a batch of two
    Hs = fit.unpack_hessian(np.stack([x, x]), np.stack([g[:L + 1]] * 2), np.stack([H[:L + 1, :L + 1]] * 2), L, rhomin, rhomax)
    assert np.array_equal(Hs[0], Hx[:L + 1, :L + 1]) and np.array_equal(Hs[1], Hx[:L + 1, :L + 1])


def test_laplace_covariance_on_a_known_quadratic():
    rg = np.random.default_rng(0)
    A = rg.standard_normal((5, 5))
    A = A @ A.T + 5 * np.eye(5)
    H = -A                                      # L = 2: [a1, a2, rho, tau1, tau2]
    free = [0, 1, 2, 4]
    cov, ok = fit.laplace_covariance(H, free)
    assert ok and np.allclose(cov, np.linalg.inv(A[np.ix_(free, free)]), rtol=1e-12, atol=0)
    mask = np.array([True, True, True, False, True])
    cov2, ok2 = fit.laplace_covariance(H, mask)
    assert ok2 and np.array_equal(cov, cov2)
    with pytest.raises(ValueError):
        fit.laplace_covariance(H, [0, 1, 2, 3, 4])
    # not a maximum: NaN and the flag
    Hb = H.copy()
    Hb[0, 0] = 10.0
    cov3, ok3 = fit.laplace_covariance(Hb, [0, 1, 2])
    assert not ok3 and np.isnan(cov3).all() and cov3.shape == (3, 3)
