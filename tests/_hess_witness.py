"""Independent restatements of the Hessian and the expected (Fisher) information of objective(alpha, rho) on the CPU, in
theta = [alpha_1..alpha_L, rho, tau_1..tau_L] order.

- hessian_and_fisher: torch fp64.  H by torch.autograd.functional.hessian of the objective; F = 1/2 tr(K^-1 D_i K^-1 D_j) with D_i from
  the forward-mode jacobian of the Kd builder.  torch takes abs''(0) = 0, so for OU the data must avoid shifted times that coincide
  across bands.
- formula: numpy, the decomposition H = T1 - T2 + T3 term by term with the kernels' derivatives written out, and the library's OU
  convention at s = 0 (k_s = 0, k_rs = 0, k_ss = 1/rho^2).  `slip` injects one of the mistakes the device tests' bar must reject."""
import math

import numpy as np
import torch

from _grad_witness import _kernel


def _setup(tarray, yarray, stdarray, marginalise_b):
    band = np.concatenate([np.full(len(t), l) for l, t in enumerate(tarray)])
    t = np.concatenate([np.asarray(a, float) for a in tarray])
    y = np.concatenate([np.asarray(a, float) for a in yarray])
    s2 = np.concatenate([np.asarray(a, float) for a in stdarray]) ** 2
    mu = np.array([np.mean(a) for a in yarray])
    Kn = np.diag(s2)
    if marginalise_b:
        var = np.array([np.var(np.asarray(a, float), ddof=1) for a in yarray])
        Kn = Kn + 100.0 * var[band][:, None] * (band[:, None] == band[None, :])
    return band, t, y - mu[band], Kn


def hessian_and_fisher(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True):
    """-> (loglik, grad[P], H[P, P], F[P, P])."""
    L = len(tarray)
    band, t_np, r_np, Kn_np = _setup(tarray, yarray, stdarray, marginalise_b)
    b = torch.tensor(band)
    t = torch.tensor(t_np, dtype=torch.float64)
    r = torch.tensor(r_np, dtype=torch.float64)[:, None]
    Kn = torch.tensor(Kn_np, dtype=torch.float64)
    n = len(t_np)

    def kd(theta):
        al, rh, tau = theta[:L], theta[L], theta[L + 1:]
        u = t - tau[b]
        S = u[:, None] - u[None, :]
        return al[b][:, None] * al[b][None, :] * _kernel(kernel, S, rh)

    def ll(theta):
        K = kd(theta) + Kn
        C = torch.linalg.cholesky(K)
        z = torch.linalg.solve_triangular(C, r, upper=False)
        return -0.5 * (z * z).sum() - torch.log(torch.diagonal(C)).sum() - 0.5 * n * math.log(2.0 * math.pi)

    theta = torch.tensor(np.concatenate([np.asarray(alpha, float), [float(rho)], np.asarray(delays, float)]), dtype=torch.float64)
    th = theta.clone().requires_grad_(True)
    v = ll(th)
    g = torch.autograd.grad(v, th)[0]
    H = torch.autograd.functional.hessian(ll, theta)
    D = torch.autograd.functional.jacobian(kd, theta, vectorize=True, strategy="forward-mode")   # (n, n, P)
    with torch.no_grad():
        Ci = torch.cholesky_inverse(torch.linalg.cholesky(kd(theta) + Kn))
        Mx = torch.einsum("ik,kjp->pij", Ci, D)                                                      # C D_p
        F = 0.5 * torch.einsum("pij,qji->pq", Mx, Mx)
    return v.item(), g.numpy(), H.numpy(), F.numpy()


def derivatives(kernel, s, rho):
    """k(s; rho), k_r, k_s, k_rr, k_rs, k_ss (numpy), with OU's convention at s = 0."""
    r = np.abs(s)
    sg = np.sign(s)
    ir = 1.0 / rho
    if kernel == "OU":
        x = r * ir
        e = np.exp(-x)
        return e, x * ir * e, -sg * ir * e, e * x * ir ** 2 * (x - 2), sg * ir ** 2 * e * (1 - x), ir ** 2 * e
    if kernel == "rbf":
        u = s * s * ir / 4
        e = np.exp(-u)
        return e, e * u * ir, -e * s * ir / 2, e * ir ** 2 * u * (u - 2), s / 2 * e * ir ** 2 * (1 - u), -ir / 2 * e * (1 - 2 * u)
    if kernel == "matern32":
        a = math.sqrt(3.0) * r * ir
        e = np.exp(-a)
        return ((1 + a) * e, a * a * e * ir, -3 * s * ir ** 2 * e, e * ir ** 2 * a * a * (a - 3), 3 * s * ir ** 3 * e * (2 - a),
                -3 * ir ** 2 * e * (1 - a))
    a = math.sqrt(5.0) * r * ir
    e = np.exp(-a)
    return ((1 + a + a * a / 3) * e, a * a / 3 * (1 + a) * e * ir, -5 / 3 * s * ir ** 2 * (1 + a) * e,
            ir ** 2 * e * a * a / 3 * (a * a - 3 * a - 3), 5 / 3 * s * ir ** 3 * e * (2 + 2 * a - a * a), -5 / 3 * ir ** 2 * e * (1 + a - a * a))


def formula(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True, slip=None):
    """H = T1 - T2 + T3 and F = T3 term by term -> (H, F).  slip: None, "no_t2" (T2 dropped), "t3_tile_once" (the elements
    i in rows 128..255, j in columns 0..127 of the trace left out: tile pair (1, 0) counted once) or "krr" (k_rr off by 1e-6)."""
    L = len(tarray)
    band, t, r, Kn = _setup(tarray, yarray, stdarray, marginalise_b)
    alpha = np.asarray(alpha, float)
    delays = np.asarray(delays, float)
    u = t - delays[band]
    S = u[:, None] - u[None, :]
    k, kr, ks, krr, krs, kss = derivatives(kernel, S, float(rho))
    if slip == "krr":
        krr = krr * (1.0 + 1e-6)
    ap, aq = alpha[band][:, None], alpha[band][None, :]
    K = ap * aq * k + Kn
    C = np.linalg.inv(K)
    C = 0.5 * (C + C.T)
    w = C @ r
    G = np.outer(w, w) - C
    bi, bj = band[:, None], band[None, :]

    def e_(a, l):   # indicator of band l on the row (a = 0) or column (a = 1) index
        return (bi == l).astype(float) if a == 0 else (bj == l).astype(float)

    P = 2 * L + 1
    D = []
    for l in range(L):
        D.append((e_(0, l) * aq + e_(1, l) * ap) * k)
    D.append(ap * aq * kr)
    for l in range(L):
        D.append(ap * aq * ks * (e_(1, l) - e_(0, l)))

    def d2(a, b):
        ka, la = (0, a) if a < L else (1, 0) if a == L else (2, a - L - 1)
        kb, lb = (0, b) if b < L else (1, 0) if b == L else (2, b - L - 1)
        if ka > kb:
            ka, la, kb, lb = kb, lb, ka, la
        da = lambda l: e_(0, l) * aq + e_(1, l) * ap   # noqa: E731
        dt = lambda l: e_(1, l) - e_(0, l)             # noqa: E731
        if ka == 0 and kb == 0:
            return (e_(0, la) * e_(1, lb) + e_(1, la) * e_(0, lb)) * k
        if ka == 0 and kb == 1:
            return da(la) * kr
        if ka == 0:
            return da(la) * dt(lb) * ks
        if kb == 1:
            return ap * aq * krr
        if ka == 1:
            return ap * aq * dt(lb) * krs
        return ap * aq * dt(la) * dt(lb) * kss

    M = [C @ Dp for Dp in D]
    u_ = [Dp @ w for Dp in D]
    H = np.zeros((P, P))
    F = np.zeros((P, P))
    for a in range(P):
        for b in range(a, P):
            prod = M[a] * M[b].T
            if slip == "t3_tile_once":
                prod = prod.copy()
                prod[128:256, 0:128] = 0.0
            t3 = 0.5 * prod.sum()
            t2 = 0.0 if slip == "no_t2" else u_[a] @ C @ u_[b]
            t1 = 0.5 * np.sum(G * d2(a, b))
            H[a, b] = H[b, a] = t1 - t2 + t3
            F[a, b] = F[b, a] = t3
    return H, F


def ou_coincident_data():
    """Two bands whose shifted times coincide at tau = [0, 1.5]: t2[0] - 1.5 = t1[0]."""
    t1 = np.array([0.0, 1.0, 2.5, 4.0, 6.1, 7.3])
    t2 = np.array([1.5, 3.0, 5.2, 6.6, 9.9])
    return [t1, t2], [np.sin(t1), np.cos(t2)], [np.full(6, 0.3), np.full(5, 0.3)]
