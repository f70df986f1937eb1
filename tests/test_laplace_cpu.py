"""The Laplace-marginalised evidence on the CPU: the C++ Newton polish (gpcc_newton_batch, gpcc_laplace.h) against its
numpy mirror (gpcc_amd.laplace) step by step and bit by bit, an exact known-answer test, the Laplace formula against a converged
quadrature at N = 40 (CPU oracle values, torch-witness Hessian), the mutations that quadrature must catch, and gpcc_laplace.h under
AddressSanitizer + UBSan."""
import ctypes
import math
import os

import numpy as np
import pytest

import _hess_witness as HW
from gpcc_amd import _capi, laplace, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int)


def native_newton(fun, u0, max_rounds=60, g_tol=1e-9, lo=None, hi=None):
    """gpcc_newton_batch over a Python fun(pidx, U) -> (val, grad, hess); returns its outputs and every batch it requested."""
    lib = _capi.load()
    u0 = np.ascontiguousarray(u0, dtype=np.float64)
    P, n = u0.shape
    seen = []

    def cb(ctx, K, pidx, U, val, grad, hess):
        Ua = np.ctypeslib.as_array(U, shape=(K, n)).copy()
        pa = np.ctypeslib.as_array(pidx, shape=(K,)).copy()
        seen.append((list(pa), [list(r) for r in Ua]))
        v, g, h = fun(pa, Ua)
        v = np.asarray(v, float).ravel()
        g = np.asarray(g, float).reshape(K * n)
        h = np.asarray(h, float).reshape(K * n * n)
        for i in range(K):
            val[i] = v[i]
        for i in range(K * n):
            grad[i] = g[i]
        for i in range(K * n * n):
            hess[i] = h[i]
        return 0

    cfun = _capi.BATCH_HESSIAN(cb)
    umax, fmax, logz = np.empty((P, n)), np.empty(P), np.empty(P)
    cov = np.empty((P, n, n))
    info, rounds = np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int32)
    stats = (ctypes.c_longlong * 2)()
    lo_a = None if lo is None else np.ascontiguousarray(lo, dtype=np.float64)
    hi_a = None if hi is None else np.ascontiguousarray(hi, dtype=np.float64)
    rc = lib.gpcc_newton_batch(P, n, max_rounds, g_tol, None if lo_a is None else lo_a.ctypes.data_as(dp),
                               None if hi_a is None else hi_a.ctypes.data_as(dp), u0.ctypes.data_as(dp), cfun, None,
                               umax.ctypes.data_as(dp), fmax.ctypes.data_as(dp), logz.ctypes.data_as(dp), cov.ctypes.data_as(dp),
                               info.ctypes.data_as(ip), rounds.ctypes.data_as(ip), stats)
    assert rc == 0, _capi.last_error()
    return (umax, fmax, logz, cov, info, rounds), seen


def mirror_newton(fun, u0, max_rounds=60, g_tol=1e-9, lo=None, hi=None):
    nt = laplace.BatchedNewton(u0, fun, max_rounds=max_rounds, g_tol=g_tol, lo=lo, hi=hi)
    return nt.run(), nt.trace


# --- test problems: l(u), its gradient and Hessian, problem by problem (pidx selects the parameters) ---------------------------
def quadratic(c, m, A):
    def f(pidx, U):
        v, g, h = [], [], []
        for p, u in zip(pidx, U):
            d = u - m[p]
            Ad = A[p] @ d
            v.append(c[p] - 0.5 * float(d @ Ad))
            g.append(-Ad)
            h.append(-A[p])
        return np.array(v), np.array(g), np.array(h)
    return f


def rosenbrock(pidx, U):
    """l(u) = -(100 (u1 - u0^2)^2 + (1 - u0)^2) - u2^2 / 2: a curved ridge, indefinite -H away from it"""
    v, g, h = [], [], []
    for u in U:
        x, y, z = u
        v.append(-(100.0 * (y - x * x) ** 2 + (1.0 - x) ** 2) - 0.5 * z * z)
        g.append([400.0 * x * (y - x * x) + 2.0 * (1.0 - x), -200.0 * (y - x * x), -z])
        h.append([[400.0 * (y - x * x) - 800.0 * x * x - 2.0, 400.0 * x, 0.0], [400.0 * x, -200.0, 0.0], [0.0, 0.0, -1.0]])
    return np.array(v), np.array(g), np.array(h)


def double_well(pidx, U):
    """l(u) = -(u0^2 - 1)^2 - u1^2 / 2 - u2^2 / 2: -H is indefinite near u0 = 0 (Levenberg damping)"""
    v, g, h = [], [], []
    for u in U:
        x, y, z = u
        v.append(-(x * x - 1.0) ** 2 - 0.5 * y * y - 0.5 * z * z)
        g.append([-4.0 * x * (x * x - 1.0), -y, -z])
        h.append([[-12.0 * x * x + 4.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])
    return np.array(v), np.array(g), np.array(h)


def _spd(rng, n):
    B = rng.standard_normal((n, n))
    return B @ B.T + n * np.eye(n)


def test_exact_kat_quadratic():
    """l(u) = c - 1/2 (u - m)' A (u - m): one Newton step to the mode, log Z = c + d/2 log 2 pi - 1/2 log det A to 1e-12."""
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 5, 9):
        P = 6
        A = [_spd(rng, n) for _ in range(P)]
        m = rng.standard_normal((P, n))
        c = rng.standard_normal(P) * 100
        f = quadratic(c, m, A)
        u0 = m + rng.standard_normal((P, n))
        exact = np.array([c[p] + 0.5 * n * math.log(2 * math.pi) - 0.5 * np.linalg.slogdet(A[p])[1] for p in range(P)])
        for run in (native_newton, mirror_newton):
            (u, fm, logz, cov, info, rounds), _ = run(f, u0, g_tol=1e-8)
            assert np.all(info == 0), info
            assert np.all(rounds == 2), rounds          # the start, and the one step that lands on the mode
            assert np.max(np.abs(logz - exact)) <= 1e-12 * max(1.0, np.max(np.abs(exact))), (logz, exact)
            assert np.allclose(u, m, rtol=0, atol=1e-12)
            for p in range(P):
                assert np.allclose(cov[p], np.linalg.inv(A[p]), rtol=1e-12, atol=1e-14)
                assert np.array_equal(cov[p], cov[p].T)


def _problems():
    """(name, fun, u0, lo, hi): the bowl, the ridge, an indefinite start, a mode beyond the box"""
    rng = np.random.default_rng(11)
    A = [_spd(rng, 3) for _ in range(4)]
    m = rng.standard_normal((4, 3))
    c = rng.standard_normal(4)
    bowl = quadratic(c, m, A)
    mb = np.array([[0.3, -0.2, 5.0]] * 4)           # the mode's last coordinate (5) lies beyond hi = 2
    beyond = quadratic(c, mb, A)
    inf = float("inf")
    return [
        ("bowl", bowl, m + rng.standard_normal((4, 3)), None, None),
        ("ridge", rosenbrock, np.array([[-1.2, 1.0, 0.5], [0.5, -0.5, 0.0], [2.0, 2.0, -1.0], [-0.3, 0.9, 2.0]]), None, None),
        ("indefinite", double_well, np.array([[0.1, 0.5, -0.5], [-0.05, 1.0, 0.0], [0.3, 0.0, 0.2], [-0.02, 0.1, 0.1]]), None, None),
        ("beyond", beyond, np.zeros((4, 3)), [-inf, -inf, -1.0], [inf, inf, 2.0]),
    ]


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["bowl", "ridge", "indefinite", "beyond"])
def test_native_and_mirror_take_bitwise_the_same_steps(name):
    prob = {p[0]: p for p in _problems()}[name]
    _, fun, u0, lo, hi = prob
    outn, seen_n = native_newton(fun, u0, max_rounds=200, lo=lo, hi=hi)
    outm, seen_m = mirror_newton(fun, u0, max_rounds=200, lo=lo, hi=hi)
    assert len(seen_n) == len(seen_m)
    for (pa, ua), (pb, ub) in zip(seen_n, seen_m):
        assert list(pa) == list(pb)
        assert np.array_equal(np.array(ua), np.array(ub))          # every requested point, bit for bit
    assert _same(outn, outm)
    umax, fmax, logz, cov, info, rounds = outn
    if name == "beyond":
        assert np.all(info == laplace.ON_BOUND) and np.all(np.isnan(logz)) and np.all(umax[:, 2] == 2.0)
    else:
        assert np.all(info == 0), info
        assert np.all(np.isfinite(logz))
    if name == "indefinite":        # started where -H is not positive definite: damping, then the nearer well
        assert np.allclose(np.abs(umax[:, 0]), 1.0, atol=1e-9)
    if name == "ridge":
        assert np.allclose(umax, [[1.0, 1.0, 0.0]] * 4, atol=1e-8)
    # each problem follows in the batch the trajectory it follows alone
    for p in range(u0.shape[0]):
        alone, seen_a = native_newton(lambda pidx, U: fun(np.full_like(pidx, p), U), u0[p:p + 1], max_rounds=200, lo=lo, hi=hi)
        mine = [u for pa, us in seen_n for q, u in zip(pa, us) if q == p]
        assert [u for _, us in seen_a for u in us] == mine
        assert _same([x[0] for x in alone], [x[p] for x in outn])


def test_not_converged_and_bad_start_codes():
    _, fun, u0, _, _ = _problems()[1]
    (u, f, logz, cov, info, rounds), _ = native_newton(fun, u0, max_rounds=1)
    assert np.all(info == laplace.NOT_CONVERGED) and np.all(rounds == 1) and np.all(np.isnan(logz))
    nanfun = lambda pidx, U: (np.where(pidx == 1, np.nan, 0.0) - (U ** 2).sum(1), -2 * U,              # noqa: E731
                              np.tile(-2 * np.eye(3), (len(pidx), 1, 1)))
    for run in (native_newton, mirror_newton):
        (u, f, logz, cov, info, rounds), _ = run(nanfun, np.ones((3, 3)))
        assert list(info) == [0, laplace.BAD_START, 0] and np.isnan(logz[1]) and np.all(np.isfinite(logz[[0, 2]]))


def test_library_rejects_bad_arguments():
    lib = _capi.load()
    f = _capi.BATCH_HESSIAN(lambda *a: 0)
    assert lib.gpcc_newton_batch(3, 0, 5, 1e-6, None, None, None, f, None, None, None, None, None, None, None, None) != 0
    assert lib.gpcc_newton_batch(3, 2, 0, 1e-6, None, None, None, f, None, None, None, None, None, None, None, None) != 0
    assert lib.gpcc_newton_batch(0, 2, 5, 1e-6, None, None, None, f, None, None, None, None, None, None, None, None) == 0


# --- Laplace against quadrature at N = 40 -----------------------------------------------------------------------------------
class WitnessObjective:
    """loglik_hess_hyper_batch from the torch witness (tests/_hess_witness.py) -- what the device computes, on the CPU."""

    def __init__(self, data, kernel="OU"):
        self.data, self.kernel = data, kernel
        self.L = len(data[0])

    def loglik_hess_hyper_batch(self, delays, alpha, rho):
        M, n = len(rho), self.L + 1
        ll, grad, hess = np.empty(M), np.empty((M, 2 * self.L + 1)), np.empty((M, n, n))
        for i in range(M):
            v, g, H, _ = HW.hessian_and_fisher(self.kernel, *self.data, delays[i], alpha[i], rho[i])
            ll[i], grad[i], hess[i] = v, g, H[:n, :n]
        return ll, grad, hess, hess * np.nan, np.zeros(M, dtype=np.int32)


def _quadrature(oracle, data, delay, u_hat, cov, nodes, R):
    """log of the integral of exp(l(u)) over u = u^ + C z, z in [-R, R]^3 (trapezoid, `nodes` per axis), C = chol(cov)"""
    C = np.linalg.cholesky(cov)
    z = np.linspace(-R, R, nodes)
    Z = np.stack(np.meshgrid(z, z, z, indexing="ij"), -1).reshape(-1, 3)
    U = u_hat + Z @ C.T
    M = len(U)
    ll, info = oracle.loglik_batch("OU", *data, np.tile(delay, (M, 1)), np.exp(U[:, :2]), np.exp(U[:, 2]), True,
                                   nthreads=oracle.max_threads())
    assert np.all(info == 0)
    w = np.full(nodes, z[1] - z[0])
    w[[0, -1]] *= 0.5
    W = (w[:, None, None] * w[None, :, None] * w[None, None, :]).ravel()
    top = ll.max()
    face = np.max(ll.reshape(nodes, nodes, nodes)[[0, -1]]), np.max(ll.reshape(nodes, nodes, nodes)[:, [0, -1]]), \
        np.max(ll.reshape(nodes, nodes, nodes)[:, :, [0, -1]])
    return top + math.log(np.sum(W * np.exp(ll - top))) + np.linalg.slogdet(C)[1], max(face) - top


QUAD_DELAYS = [0.0, 1.0, 2.0, 3.0, 5.0]


@pytest.fixture(scope="module")
def quad_setup(oracle):
    t, y, s, _ = synthetic.simulate_lightcurves([20, 20], seed=3, span=20.0, sigma=0.3)
    data = (t, y, s)
    obj = WitnessObjective(data)
    delays = np.array([[0.0, d] for d in QUAD_DELAYS])
    a0, r0 = synthetic.default_hyperparameters(y)
    G = len(delays)
    out = laplace.laplace_evidence(obj, delays, np.tile(a0, (G, 1)), np.full(G, r0), rhomin=1e-3, rhomax=1e3, g_tol=1e-7)
    ll, alpha, rho, logz, cov, info, rounds = out
    assert np.all(info == 0), info
    quad = {}
    for nodes in (41, 57):
        quad[nodes] = []
        for g in range(G):
            u_hat = np.concatenate([np.log(alpha[g]), [np.log(rho[g])]])
            q, _ = _quadrature(oracle, data, delays[g], u_hat, cov[g], nodes, 7.0)
            quad[nodes].append(q)
    return data, obj, delays, out, {k: np.array(v) for k, v in quad.items()}


# The delay-dependent part of log Z_Laplace - log Z_quad (nats).  At N = 40 the posterior in u is visibly skewed (the integrand is still
# e^-2 .. e^-5 of its peak on the faces of the +-7 sigma box), so Laplace and the box integral differ by 0.07 .. 0.2 nats, and by
# 0.13 nats delay to delay; the quadrature's nodes converge to 4e-5 (41 against 57 per axis), not 1e-6.
QUAD_BAR = 0.2
NODE_TOL = 1e-4


def _dd(x):
    return float(np.max(np.abs(x - np.mean(x))))


def test_laplace_against_converged_quadrature(quad_setup):
    data, obj, delays, (ll, alpha, rho, logz, cov, info, rounds), quad = quad_setup
    assert np.max(np.abs(quad[41] - quad[57])) <= NODE_TOL, quad[41] - quad[57]
    diff = logz - quad[57]
    print("laplace - quadrature:", diff, "delay-dependent part %.4g" % _dd(diff))
    assert _dd(diff) <= QUAD_BAR, diff


def test_quadrature_catches_the_mutations(quad_setup):
    """Omitting the log-Jacobian (H_theta for H_u) and dropping the 1/2 move the delay-dependent part above the bar.  Dropping the
    diag(theta g) term is invisible at the mode (g = 0), so it is caught away from it: 0.5 sigma off the mode, H_u matches central
    differences of the witness's g_u to 1e-6 of max |H_u| with the term, and misses by more than 100 times that without it."""
    data, obj, delays, (ll, alpha, rho, logz, cov, info, rounds), quad = quad_setup
    G, n = len(delays), 3
    no_jac, no_half, fd_ok, fd_mut = [], [], [], []
    for g in range(G):
        theta = np.concatenate([alpha[g], [rho[g]]])
        _, gr, Ht, _, _ = obj.loglik_hess_hyper_batch(delays[g:g + 1], alpha[g:g + 1], rho[g:g + 1])
        no_jac.append(ll[g] + 0.5 * n * math.log(2 * math.pi) - 0.5 * np.linalg.slogdet(-Ht[0])[1])
        no_half.append(ll[g] + 0.5 * n * math.log(2 * math.pi) - np.linalg.slogdet(-laplace.hyper_to_u(theta, gr[0], Ht[0])[1])[1])
        u1 = np.log(theta) + 0.5 * np.sqrt(np.diag(cov[g]))

        def gu_at(u):
            th = np.exp(u)
            _, gg, HH, _, _ = obj.loglik_hess_hyper_batch(delays[g:g + 1], th[None, :2], th[2:])
            return laplace.hyper_to_u(th, gg[0], HH[0])

        gu1, Hu1 = gu_at(u1)
        h = 1e-5
        fd = np.array([(gu_at(u1 + h * e)[0] - gu_at(u1 - h * e)[0]) / (2 * h) for e in np.eye(n)])
        sc = np.max(np.abs(Hu1))
        fd_ok.append(np.max(np.abs(Hu1 - fd)) / sc)
        fd_mut.append(np.max(np.abs(Hu1 - np.diag(gu1) - fd)) / sc)
    q = quad[57]
    ratios = {"no_jacobian": _dd(np.array(no_jac) - q) / QUAD_BAR, "no_half": _dd(np.array(no_half) - q) / QUAD_BAR}
    print("delay-dependent error / bar:", ratios, "off-mode H_u vs differences: %.3g, without diag(theta g): %.3g" %
          (max(fd_ok), min(fd_mut)))
    assert ratios["no_jacobian"] > 1.0 and ratios["no_half"] > 1.0
    assert max(fd_ok) <= 1e-6 and min(fd_mut) > 1e-4


def test_laplace_header_under_sanitizers(tmp_path):
    """gpcc_laplace.h (the C++ host logic of gpcc_laplace_evidence) compiled host-only with AddressSanitizer + UBSan."""
    import subprocess
    exe = str(tmp_path / "laplace_sanitize")
    src = os.path.join(ROOT, "tests", "abi", "laplace_host_sanitize.cpp")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr[-3000:]
    assert "quadratic: ok" in run.stdout and "ridge: ok" in run.stdout and "bound: ok" in run.stdout and "empty: ok" in run.stdout
