"""An independent fp64 torch-autograd restatement of objective(alpha, rho) (src/gpccfixdelay_marginaliseb.jl:133-141;
src/gpccfixdelay.jl:131-139 without the marginalised offsets) on the CPU: K from the reference formulas, torch's Cholesky, the
Gaussian log-density.  The gradient tests measure the library's gradient against it."""
import math

import numpy as np
import torch


def _kernel(name, s, rho):
    r = s.abs()
    if name == "OU":
        return torch.exp(-r / rho)
    if name == "rbf":                       # src/util.jl:28: exp(-r^2 / (4 rho))
        return torch.exp(-(s * s) / (4.0 * rho))
    if name == "matern32":
        a = math.sqrt(3.0) * r / rho
        return (1.0 + a) * torch.exp(-a)
    a = math.sqrt(5.0) * r / rho             # matern52
    return (1.0 + a + a * a / 3.0) * torch.exp(-a)


def loglik_and_grad(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True):
    """-> (loglik, grad[2L+1] = [d/dalpha_1..L, d/drho, d/dtau_1..L])."""
    L = len(tarray)
    band = np.concatenate([np.full(len(t), l) for l, t in enumerate(tarray)])
    t = torch.tensor(np.concatenate([np.asarray(a, float) for a in tarray]), dtype=torch.float64)
    y = torch.tensor(np.concatenate([np.asarray(a, float) for a in yarray]), dtype=torch.float64)
    s2 = torch.tensor(np.concatenate([np.asarray(a, float) for a in stdarray]) ** 2, dtype=torch.float64)
    b = torch.tensor(band)
    tau = torch.tensor(np.asarray(delays, float), dtype=torch.float64, requires_grad=True)
    al = torch.tensor(np.asarray(alpha, float), dtype=torch.float64, requires_grad=True)
    rh = torch.tensor(float(rho), dtype=torch.float64, requires_grad=True)
    u = t - tau[b]
    S = u[:, None] - u[None, :]
    K = al[b][:, None] * al[b][None, :] * _kernel(kernel, S, rh) + torch.diag(s2)
    mu = torch.tensor([np.mean(a) for a in yarray], dtype=torch.float64)
    if marginalise_b:
        var = torch.tensor([np.var(np.asarray(a, float), ddof=1) for a in yarray], dtype=torch.float64)
        K = K + 100.0 * var[b][:, None] * (b[:, None] == b[None, :]).to(torch.float64)
    r = (y - mu[b])[:, None]
    C = torch.linalg.cholesky(K)
    z = torch.linalg.solve_triangular(C, r, upper=False)
    ll = -0.5 * (z * z).sum() - torch.log(torch.diagonal(C)).sum() - 0.5 * len(y) * math.log(2.0 * math.pi)
    ll.backward()
    g = np.concatenate([al.grad.numpy(), [rh.grad.item()], tau.grad.numpy()])
    return ll.item(), g


def ragged_data(Nl, seed):
    """Light curves with bands of the given lengths at irregular times (a gap in one band), y from a smooth signal + noise."""
    rg = np.random.default_rng(seed)
    tarray, yarray, sarray = [], [], []
    for l, n in enumerate(Nl):
        t = np.sort(rg.uniform(0.0, 30.0, n))
        y = np.sin(0.4 * t + l) + 0.3 * l + 0.2 * rg.standard_normal(n)
        tarray.append(t)
        yarray.append(y)
        sarray.append(np.full(n, 0.2) + 0.05 * rg.random(n))
    return tarray, yarray, sarray


def random_params(L, M, seed):
    """M mixed (tau, alpha, rho): delays 0 for band 1, alpha around 1, rho in 0.5 .. 6."""
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), rg.uniform(-3.0, 5.0, (M, L - 1))], 1)
    alpha = rg.uniform(0.4, 2.0, (M, L))
    rho = rg.uniform(0.5, 6.0, M)
    return delays, alpha, rho
