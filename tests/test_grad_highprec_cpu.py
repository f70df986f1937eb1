"""The extended-precision gradient reference (tests/_grad_highprec.py) checked on the CPU: against the fp64 torch witness and the
CPU oracle, against mpmath central differences at 40 digits, its tiled recomputation against its trace formula, and the
comparator of the device tests against deliberately wrong (mutated) versions of the reference."""
import time

import numpy as np
import pytest

import _grad_highprec as H
import _grad_witness as W

pytestmark = pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)

KERNELS = ["OU", "rbf", "matern32", "matern52"]
SIZES = {1: [23], 2: [19, 31], 3: [17, 9, 26]}   # test_gradient_cpu.py's shapes


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("mb", [True, False])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_reference_against_witness_and_oracle(oracle, kernel, mb, L):
    data = W.ragged_data(SIZES[L], seed=10 * L + KERNELS.index(kernel))
    delays, alpha, rho = W.random_params(L, 3, seed=L)
    orc, info = oracle.loglik_batch(kernel, *data, delays, alpha, rho, mb)
    assert (info == 0).all()
    for i in range(3):
        ref = H.evaluate(kernel, *data, delays[i], alpha[i], rho[i], mb)
        assert ref.info == 0
        lw, gw = W.loglik_and_grad(kernel, *data, delays[i], alpha[i], rho[i], mb)
        assert abs(ref.loglik - orc[i]) <= 1e-12 * abs(orc[i]), (ref.loglik, orc[i])
        assert abs(ref.loglik - lw) <= 1e-12 * abs(lw)
        assert np.max(np.abs(gw - ref.grad)) <= 1e-11 * max(1.0, np.max(np.abs(ref.grad))), (gw, ref.grad)
        assert H.ratio(gw, ref) <= 1.0
        if L > 1:   # a common shift of all delays leaves the likelihood unchanged
            assert abs(float(np.sum(ref.grad_ld[L + 1:]))) <= 1e-15 * max(1.0, float(np.max(ref.scale)))
        else:
            assert ref.grad[L + 1] == 0.0


def _mp_loglik(mp, kernel, tarray, yarray, stdarray, delays, alpha, rho, mb):
    """objective(alpha, rho) in mpmath at the working precision, from the reference formulas."""
    band = [l for l, t in enumerate(tarray) for _ in t]
    t = [mp.mpf(float(v)) for a in tarray for v in a]
    y = [mp.mpf(float(v)) for a in yarray for v in a]
    sd = [mp.mpf(float(v)) for a in stdarray for v in a]
    N = len(t)
    mean = [mp.fsum(mp.mpf(float(v)) for v in a) / len(a) for a in yarray]
    var = [mp.fsum((mp.mpf(float(v)) - m) ** 2 for v in a) / (len(a) - 1) for a, m in zip(yarray, mean)]
    u = [t[i] - delays[band[i]] for i in range(N)]

    def k(s):
        r = abs(s)
        if kernel == "OU":
            return mp.exp(-r / rho)
        if kernel == "rbf":
            return mp.exp(-s * s / (4 * rho))
        if kernel == "matern32":
            a = mp.sqrt(3) * r / rho
            return (1 + a) * mp.exp(-a)
        a = mp.sqrt(5) * r / rho
        return (1 + a + a * a / 3) * mp.exp(-a)

    K = mp.matrix(N, N)
    for i in range(N):
        for j in range(i + 1):
            v = alpha[band[i]] * alpha[band[j]] * k(u[i] - u[j])
            if mb and band[i] == band[j]:
                v += 100 * var[band[i]]
            if i == j:
                v += sd[i] ** 2
            K[i, j] = K[j, i] = v
    C = mp.cholesky(K)
    z = []
    for i in range(N):
        z.append((y[i] - mean[band[i]] - mp.fsum(C[i, j] * z[j] for j in range(i))) / C[i, i])
    return -mp.fsum(v * v for v in z) / 2 - mp.fsum(mp.log(C[i, i]) for i in range(N)) - N * mp.log(2 * mp.pi) / 2


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("mb", [True, False])
def test_reference_against_mpmath_differences(kernel, mb):
    """Central differences of the 40-digit log-likelihood (h = 1e-18: truncation ~1e-36, rounding ~1e-20) verify the reference's
    derivatives to its own precision.  OU also gets two bands with one pair of points at the same shifted time: there the
    central difference in the delays tends to the mean of the one-sided ones, the convention dk/ds(0) = 0 of the reference (at
    the kink its error is O(h), not O(h^2): hence the small h)."""
    mp = pytest.importorskip("mpmath").mp
    mp.dps = 40
    data = W.ragged_data([13, 11], seed=3 + KERNELS.index(kernel))
    delays = np.array([0.0, 1.25])
    alpha = np.array([0.9, 1.4])
    rho = 2.5
    if kernel == "OU":
        data[0][0][6] = np.round(data[0][0][6] * 1024) / 1024    # (so that t + tau is exact)
        data[0][1][4] = data[0][0][6] + delays[1]   # t - tau equal across the bands: s = 0 off the diagonal
    ref = H.evaluate(kernel, *data, delays, alpha, rho, mb)
    assert ref.info == 0
    x0 = [mp.mpf(float(v)) for v in np.concatenate([alpha, [rho], delays])]
    L = 2
    h = mp.mpf(10) ** -18
    fd = []
    for i in range(len(x0)):
        xs = []
        for sgn in (1, -1):
            x = list(x0)
            x[i] += sgn * h
            xs.append(_mp_loglik(mp, kernel, *data, x[L + 1:], x[:L], x[L], mb))
        fd.append((xs[0] - xs[1]) / (2 * h))
    ll = _mp_loglik(mp, kernel, *data, x0[L + 1:], x0[:L], x0[L], mb)
    assert abs(float(ll) - ref.loglik) <= 1e-15 * abs(ref.loglik)
    fd = np.array([float(v) for v in fd])
    err = np.max(np.abs(fd - ref.grad))
    assert err <= 1e-15 * max(1.0, float(np.max(ref.scale))), (fd, ref.grad)


def _mutation_case(kernel):
    data = W.ragged_data([100, 110, 90], seed=21)   # N = 300: three tiles, bands crossing both tile edges, 84 padded points
    delays, alpha, rho = np.array([0.0, 1.5, -2.0]), np.array([0.8, 1.3, 1.1]), 2.2
    return H.evaluate(kernel, *data, delays, alpha, rho, True, keep=True)


def test_tiled_recomputation_matches_trace_formula():
    for kernel in KERNELS:
        ref = _mutation_case(kernel)
        g = H.tile_gradient(ref)
        assert float(np.max(np.abs(g - ref.grad_ld))) <= 1e-16 * float(np.max(ref.scale)), kernel
        assert H.ratio(g.astype(np.float64), ref) <= 1e-4


def test_comparator_rejects_each_injected_fault():
    """Every fault a tiled gradient can make, in every place it can make it at N = 300 (3 tiles, 3 bands): the device tests'
    comparator must reject each one.  The smallest rejection ratio is printed."""
    ref = _mutation_case("matern32")
    nt = 3
    faults = [("drop_transpose", I, J) for I in range(nt) for J in range(I)]
    faults += [("flip_S", p, q) for p in range(3) for q in range(3) if p != q]
    faults += [("omit_kinv", I, J, Kt) for I in range(nt) for J in range(I + 1) for Kt in range(I, nt)]
    faults += [("pad_real",)]
    worst = np.inf
    for f in faults:
        r = H.ratio(H.tile_gradient(ref, f).astype(np.float64), ref)
        worst = min(worst, r)
        assert r > 1.0, (f, r)
    for kernel in KERNELS:   # dk/drho of one kernel off by 1e-6 relative
        rk = _mutation_case(kernel)
        r = H.ratio(H.tile_gradient(rk, ("drho_scale", 1 + 1e-6)).astype(np.float64), rk)
        worst = min(worst, r)
        assert r > 1.0, (kernel, r)
    print("smallest error / bar over %d injected faults: %.3g" % (len(faults) + len(KERNELS), worst))


def test_reference_time_at_n_1030():
    """The reference's cost at the largest size the device tests give it (one evaluation, L = 8)."""
    Nl = [1, 2, 3, 40, 127, 128, 129, 600]
    data = W.ragged_data(Nl, seed=5)
    delays, alpha, rho = W.random_params(8, 1, seed=6)
    t0 = time.perf_counter()
    ref = H.evaluate("matern52", *data, delays[0], alpha[0], rho[0], False)
    dt = time.perf_counter() - t0
    print("extended-precision reference at N = %d: %.2f s" % (sum(Nl), dt))
    assert ref.info == 0 and np.all(np.isfinite(ref.grad))
