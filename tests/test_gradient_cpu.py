"""The gradient's witness on the CPU: the torch-autograd restatement of objective(alpha, rho) (tests/_grad_witness.py) against
the CPU oracle's values and their central finite differences, and fit.unpack_grad against finite differences through `unpack`."""
import numpy as np
import pytest

import _grad_witness as W
from gpcc_amd import fit

KERNELS = ["OU", "rbf", "matern32", "matern52"]
SIZES = {1: [23], 2: [19, 31], 3: [17, 9, 26]}   # ragged bands


def _fd(oracle, kernel, data, delays, alpha, rho, mb, rel=1e-5):
    """Central differences of oracle.loglik_batch in [alpha, rho, tau], one batch."""
    L = len(alpha)
    x0 = np.concatenate([alpha, [rho], delays])
    H = rel * np.maximum(np.abs(x0), 1.0)
    X = np.repeat(x0[None, :], 2 * len(x0), 0)
    for i in range(len(x0)):
        X[2 * i, i] += H[i]
        X[2 * i + 1, i] -= H[i]
    ll, info = oracle.loglik_batch(kernel, *data, X[:, L + 1:], X[:, :L], X[:, L], mb)
    assert (info == 0).all()
    return (ll[0::2] - ll[1::2]) / (2 * H)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("mb", [True, False])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_witness_value_and_gradient_against_oracle(oracle, kernel, mb, L):
    data = W.ragged_data(SIZES[L], seed=10 * L + KERNELS.index(kernel))
    delays, alpha, rho = W.random_params(L, 3, seed=L)
    ref, info = oracle.loglik_batch(kernel, *data, delays, alpha, rho, mb)
    assert (info == 0).all()
    for i in range(3):
        ll, g = W.loglik_and_grad(kernel, *data, delays[i], alpha[i], rho[i], mb)
        assert abs(ll - ref[i]) <= 1e-12 * abs(ref[i]), (ll, ref[i])
        fd = _fd(oracle, kernel, data, delays[i], alpha[i], rho[i], mb)
        assert np.max(np.abs(g - fd)) <= 1e-6 * np.linalg.norm(g), (g, fd)
        if L > 1:   # the likelihood does not change when all delays shift together
            assert abs(g[L + 1:].sum()) <= 1e-9 * np.linalg.norm(g[L + 1:])


@pytest.mark.parametrize("L", [1, 2, 3])
def test_unpack_grad_matches_finite_differences(L):
    data = W.ragged_data(SIZES[L], seed=5 + L)
    rhomin, rhomax = 0.1, 20.0
    rg = np.random.default_rng(L)
    delays = np.concatenate([[0.0], rg.uniform(-2, 4, L - 1)])
    x = np.concatenate([rg.uniform(-1.0, 1.5, L), [rg.uniform(-2.0, 1.0)]])

    def ell(xv):
        a = fit.makepositive(xv[:L]) + 1e-8
        r = float(fit.transformbetween(xv[L], rhomin, rhomax))
        return W.loglik_and_grad("matern32", *data, delays, a, r)

    _, g = ell(x)
    gx = fit.unpack_grad(x, g, L, rhomin, rhomax)
    assert gx.shape == (2 * L + 1,)
    assert np.array_equal(gx[L + 1:], g[L + 1:])   # delays pass through
    h = 1e-4   # (five-point stencil: truncation ~h^4)
    fd = np.array([(8 * (ell(x + h * e)[0] - ell(x - h * e)[0]) - (ell(x + 2 * h * e)[0] - ell(x - 2 * h * e)[0])) / (12 * h)
                   for e in np.eye(L + 1)])
    assert np.max(np.abs(gx[:L + 1] - fd)) <= 1e-7 * max(1.0, np.linalg.norm(fd)), (gx, fd)
    # a batch of vectors at once, and the gradient without the delays
    X2 = np.stack([x, x])
    G2 = fit.unpack_grad(X2, np.stack([g[:L + 1], g[:L + 1]]), L, rhomin, rhomax)
    assert np.array_equal(G2[0], gx[:L + 1]) and np.array_equal(G2[1], gx[:L + 1])
