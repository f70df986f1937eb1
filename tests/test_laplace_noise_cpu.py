"""The Laplace evidence under a fitted noise model on the CPU (gpcc_amd.laplace.laplace_evidence_noise, fit.noise_evidence, DESIGN.md
4.26): BatchedNewton with one_sided=() against a trace recorded before the keyword existed, the one-sided convention on the same
problems, the evidence over the numpy mirror against its own definition with a Hessian from central differences of the mirror's
gradient, clean data (w pinned) and data with injected excess variance (nothing pinned), and the chain rule of shared and fixed
variables by hand."""
import math

import numpy as np

from gpcc_amd import fit, laplace, markov

# ---- BatchedNewton: the recorded trace ---------------------------------------------------------------------------------------------
# Three problems in two variables, l_p(x, y) = -(x - a)^4 / 4 - (x - a)^2 / 2 - (y - b)^2 - c x y, box y >= -1/4, x <= 3/2, starts
# (3, 2), (-1, -2), (1/2, 1/2), max_rounds 30, g_tol 1e-9: every batch's rows, the modes, values, covariances, codes and rounds as the
# polish produced them before `one_sided` existed (recorded on the CPU; the arithmetic is Python floats with +, -, *, / and sqrt only,
# so the bits do not depend on the platform).  Problems 0 and 2 end on a bound with the gradient pointing out: ON_BOUND.
C = [(1.0, -0.5, 0.3), (0.25, 0.75, -0.4), (2.0, 0.1, 0.0)]
TRACE = [([0, 1, 2], [['0x1.8000000000000p+0', '0x1.0000000000000p+1'], ['-0x1.0000000000000p+0', '-0x1.0000000000000p-2'], ['0x1.0000000000000p-1', '0x1.0000000000000p-1']]),
         ([0, 1, 2], [['0x1.42d0b42d0b42dp+0', '-0x1.0000000000000p-2'], ['-0x1.8ee4f354ccfb8p-2', '0x1.581c4e111eb3ap-1'], ['0x1.2108421084211p+0', '0x1.999999999999cp-4']]),
         ([0, 1, 2], [['0x1.178016a3c57c6p+0', '-0x1.0000000000000p-2'], ['0x1.3e33bcf0a31c0p-3', '0x1.8fe8fca5a1c16p-1'], ['0x1.8000000000000p+0', '0x1.999999999999ap-4']]),
         ([0, 1], [['0x1.131ce5e519ff5p+0', '-0x1.0000000000000p-2'], ['0x1.2c1e3c9429bdap-1', '0x1.bc060c1da1f2cp-1']]),
         ([0, 1], [['0x1.13180226e6000p+0', '-0x1.0000000000000p-2'], ['0x1.2107d0c7cee71p-1', '0x1.b9ce5cf4c2fb0p-1']]),
         ([0, 1], [['0x1.13180221a213bp+0', '-0x1.0000000000000p-2'], ['0x1.20d5f668c07fdp-1', '0x1.b9c4647b59b33p-1']]),
         ([1], [['0x1.20d5f2a4f1cc4p-1', '0x1.b9c463ba96c27p-1']])]
U = [['0x1.13180221a213bp+0', '-0x1.0000000000000p-2'], ['0x1.20d5f2a4f1cc4p-1', '0x1.b9c463ba96c27p-1'], ['0x1.8000000000000p+0', '0x1.999999999999ap-4']]
F = ['0x1.f580f05f35ec0p-7', '0x1.0aa3f7f7ef07fp-3', '-0x1.2000000000000p-3']
LOGZ1 = 1.5237003088005827
COV = [['0x1.07757627afcaep+0', '-0x1.3c268dc93959dp-3', '-0x1.3c268dc93959dp-3', '0x1.0bdb0bb78bc03p-1'],
       ['0x1.a50a2b0db8e2bp-1', '0x1.50d4ef3e2d823p-3', '0x1.50d4ef3e2d823p-3', '0x1.10d7725cb579cp-1'],
       ['0x1.2492492492491p-1', '0x0.0p+0', '0x0.0p+0', '0x1.ffffffffffffep-2']]
INFO, ROUNDS = [-12, 0, -12], [6, 7, 3]


def _fbatch(pidx, X):
    val, grad, hess = [], [], []
    for p, (x, y) in zip(pidx, X):
        a, b, c = C[int(p)]
        dx, dy = x - a, y - b
        val.append(-0.25 * dx * dx * dx * dx - 0.5 * dx * dx - dy * dy - c * x * y)
        grad.append([-dx * dx * dx - dx - c * y, -2.0 * dy - c * x])
        hess.append([[-3.0 * dx * dx - 1.0, -c], [-c, -2.0]])
    return np.array(val), np.array(grad), np.array(hess)


def _newton(**kw):
    nt = laplace.BatchedNewton([[3.0, 2.0], [-1.0, -2.0], [0.5, 0.5]], _fbatch, max_rounds=30, g_tol=1e-9, lo=[-laplace.INF, -0.25],
                               hi=[1.5, laplace.INF], **kw)
    return nt, nt.run()


def _hex(rows):
    return [[float(v).hex() for v in np.ravel(r)] for r in rows]


def test_newton_without_one_sided_variables_is_bitwise_the_recorded_polish():
    for kw in ({}, {"one_sided": ()}):
        nt, (u, f, logz, cov, info, rounds) = _newton(**kw)
        assert [(p, _hex(X)) for p, X in nt.trace] == TRACE
        assert _hex(u) == U and [float(v).hex() for v in f] == F and _hex(cov) == COV
        assert list(info) == INFO and list(rounds) == ROUNDS
        assert math.isnan(logz[0]) and math.isnan(logz[2]) and abs(logz[1] - LOGZ1) <= 4 * np.finfo(float).eps * abs(LOGZ1)   # (libm's log)
        assert not np.array(nt.pinned).any()


def test_one_sided_variables_are_pinned_with_the_boundary_term():
    """The same three problems with both variables one-sided: the same steps (the trace is the recorded one), and problems 0 (y on its
    lower bound) and 2 (x on its upper bound) now finish with info 0, the pinned variable out of -H and of the 1/2 log 2 pi count and
    -log|g_k| in its place; problem 1, in the interior, is untouched."""
    nt, (u, f, logz, cov, info, rounds) = _newton(one_sided=(0, 1))
    assert [(p, _hex(X)) for p, X in nt.trace] == TRACE and _hex(u) == U and list(rounds) == ROUNDS
    assert list(info) == [0, 0, 0] and np.array(nt.pinned).tolist() == [[False, True], [False, False], [True, False]]
    assert abs(logz[1] - LOGZ1) <= 4 * np.finfo(float).eps * abs(LOGZ1) and _hex(cov[1:2]) == COV[1:2]
    for p, (free, pin) in ((0, (0, 1)), (2, (1, 0))):
        val, grad, hess = _fbatch([p], [u[p]])
        want = val[0] + 0.5 * laplace.LOG2PI - 0.5 * math.log(-hess[0][free][free]) - math.log(abs(grad[0][pin]))
        assert abs(logz[p] - want) <= 1e-14 * max(1.0, abs(want)), (p, logz[p], want)
        assert abs(grad[0][pin]) > 1e-9 and abs(grad[0][free]) <= 1e-9
        assert cov[p][pin, pin] == 0.0 and cov[p][free, pin] == 0.0 and abs(cov[p][free, free] + 1.0 / hess[0][free][free]) <= 1e-15
    # only the first variable one-sided: problem 0 (pinned in y) stays ON_BOUND
    _, (_, _, logz, _, info, _) = _newton(one_sided=(0,))
    assert list(info) == [laplace.ON_BOUND, 0, 0] and math.isnan(logz[0])


# ---- the evidence over the mirror --------------------------------------------------------------------------------------------------
def _data(seed, excess):
    """Two bands (22 + 18 points in 20 days) of one OU process (rho = 3), the second delayed by 2, scaled by 1.5 and offset; the
    reported error bars (0.1 and 0.15) are exact for excess = 0, and excess * sigma^2 more variance is injected otherwise."""
    rg = np.random.default_rng(seed)
    Nl, delay, rho = [22, 18], 2.0, 3.0
    t = [np.sort(rg.uniform(0.0, 20.0, n)) for n in Nl]
    u = np.concatenate([t[0], t[1] - delay])
    K = np.exp(-np.abs(u[:, None] - u[None, :]) / rho)
    f = np.linalg.cholesky(K + 1e-12 * np.eye(len(u))) @ rg.standard_normal(len(u))
    amp, sig = [1.0, 1.5], [0.1, 0.15]
    y, s, o = [], [], 0
    for l, n in enumerate(Nl):
        y.append(amp[l] * f[o:o + n] + 3.0 * l + sig[l] * rg.standard_normal(n) + math.sqrt(excess) * sig[l] * rg.standard_normal(n))
        s.append(np.full(n, sig[l]))
        o += n
    return t, y, s


DELAYS = np.array([[0.0, 1.0], [0.0, 2.0], [0.0, 3.0]])
KW = dict(noise="excess", rhomin=1e-2, rhomax=1e3, g_tol=1e-6)


def _evidence(t, y, s, **kw):
    obj = markov.MarkovObjective(t, y, s, "OU")
    ms2 = laplace.band_mean_sigma2(obj)
    out = laplace.laplace_evidence_noise(obj, DELAYS, np.tile([1.0, 1.5], (3, 1)), np.full(3, 3.0), np.ones((3, 2)), np.tile(0.5 * ms2, (3, 1)),
                                         **{**KW, **kw})
    return obj, ms2, out


def _grad_u(obj, ms2, delay, u):
    """The mirror's gradient in u = (log alpha_1, log alpha_2, log rho, log w_1, log w_2) at kappa = 1, by the chain rule on its
    gradient row."""
    x = np.exp(u)
    ll, g, info = obj.loglik_grad_markov_noise_batch([delay], [x[:2]], [x[2]], [[1.0, 1.0]], [x[3:] * ms2])
    assert info[0] == 0
    return ll[0], x * np.concatenate([g[0][:3], g[0][7:9] * ms2])


def test_evidence_is_its_definition_at_the_mode():
    """N = 40, L = 2, 3 delays, an excess variance per band (seed 3: every variable ends in the interior at two delays and w_2 is pinned
    at one, so both forms of the formula are met): at the returned mode |g_u| <= g_tol on the free variables, and
        log Z = f + (n_free / 2) log 2 pi - 1/2 log det(-H_free) - sum over the pinned k of log|g_k|
    with H from central differences of the mirror's GRADIENT in u (step h = 1e-3) through numpy.linalg.slogdet.  The tolerance is the
    difference scheme's own truncation estimate: the change of its 1/2 log det from step 2h to step h (the coarser step's truncation
    error is four times the finer one's, so the change is three times the error that is tolerated), and never less than 64 eps |f|,
    the rounding of the sum itself."""
    t, y, s = _data(3, 8.0)
    obj, ms2, (f, alpha, rho, kappa, nu, logz, cov, info, rounds, pinned) = _evidence(t, y, s)
    assert (info == 0).all() and np.isfinite(logz).all() and (kappa == 1.0).all() and pinned.shape == (3, 5)
    assert not pinned[:, :3].any() and pinned.any() and not pinned.all(axis=1).any()
    for g in range(3):
        u = np.log(np.concatenate([alpha[g], [rho[g]], nu[g] / ms2]))
        val, gu = _grad_u(obj, ms2, DELAYS[g], u)
        free = np.flatnonzero(~pinned[g])
        assert val == f[g] and np.max(np.abs(gu[free])) <= 1e-6, (g, gu)
        for k in np.flatnonzero(pinned[g]):
            assert abs(u[k] - math.log(1e-4)) <= 1e-12 and gu[k] < -1e-6          # on the lower bound, the gradient pointing out

        def half_logdet(h):
            H = np.empty((5, 5))
            for k in range(5):
                e = np.zeros(5)
                e[k] = h
                H[k] = (_grad_u(obj, ms2, DELAYS[g], u + e)[1] - _grad_u(obj, ms2, DELAYS[g], u - e)[1]) / (2 * h)
            H = 0.5 * (H + H.T)[np.ix_(free, free)]
            sign, ld = np.linalg.slogdet(-H)
            assert sign > 0
            return 0.5 * ld

        coarse, fine = half_logdet(2e-3), half_logdet(1e-3)
        want = f[g] + 0.5 * len(free) * laplace.LOG2PI - fine - sum(math.log(abs(gu[k])) for k in np.flatnonzero(pinned[g]))
        tol = max(abs(coarse - fine), 64 * np.finfo(float).eps * abs(f[g]))
        print("delay %d: log Z %.10f, by differences %.10f, tolerance %.3g, pinned %s, rounds %d" % (g, logz[g], want, tol, pinned[g].astype(int), rounds[g]))
        assert abs(logz[g] - want) <= tol, (g, logz[g], want, tol)
    # cov is the inverse of -H_free, zero on the pinned variables
    g = int(np.flatnonzero(pinned.any(axis=1))[0])
    k = int(np.flatnonzero(pinned[g])[0])
    assert (cov[g][k] == 0.0).all() and (cov[g][:, k] == 0.0).all() and (np.diagonal(cov[g])[~pinned[g]] > 0).all()


def test_clean_data_pins_w_and_injected_variance_frees_it():
    """Exact error bars (seed 7, shared w): w ends on wmin at every delay with the gradient pointing out -- pinned, info 0, a finite
    evidence, where ON_BOUND would have made every delay NaN.  The same kind of data with 8 sigma^2 of injected variance (seed 8, a w
    per band): nothing is pinned and w is far from both bounds.  The seeds were chosen on the CPU so that the mirror decides so."""
    t, y, s = _data(7, 0.0)
    obj, ms2, out = _evidence(t, y, s, shared=True)
    f, alpha, rho, kappa, nu, logz, cov, info, rounds, pinned = out
    assert pinned.shape == (3, 4) and pinned[:, 3].all() and not pinned[:, :3].any(), pinned
    assert (info == 0).all() and np.isfinite(logz).all() and np.allclose(nu, 1e-4 * ms2, rtol=1e-12, atol=0.0)
    res = fit.noise_evidence(obj, DELAYS, fit.NoiseGridFit(f, alpha, rho, kappa, nu, 0, 0, None), noise="excess", shared=True, rhomin=1e-2,
                             rhomax=1e3)
    assert isinstance(res, fit.NoiseEvidence) and res._fields == ("loglik", "alpha", "rho", "kappa", "nu", "log_evidence", "cov", "info", "rounds",
                                                                  "pinned")
    assert (res.info == 0).all() and np.array_equal(res.pinned, pinned) and np.allclose(res.log_evidence, logz, rtol=0, atol=1e-6)
    assert (res.rounds <= 2).all()                                   # started at the mode
    t, y, s = _data(8, 8.0)
    _, ms2, out = _evidence(t, y, s)
    assert (out[7] == 0).all() and not out[9].any() and np.isfinite(out[5]).all()
    assert (out[4] / ms2 > 1.0).all() and (out[4] / ms2 < 50.0).all()


# ---- shared and fixed variables ----------------------------------------------------------------------------------------------------
def test_shared_and_fixed_variables_follow_the_chain_rule_by_hand():
    """noise = "scale" with shared = True (one log kappa for both bands, nu fixed) and noise = "both" with a w per band: (g_u, H_u) as
    laplace_evidence_noise forms them from one row of the mirror's full block, against the chain rule written out entry by entry, and
    the shared kappa's two derivatives against central differences of the mirror's value along kappa_1 = kappa_2."""
    t, y, s = _data(5, 2.0)
    obj = markov.MarkovObjective(t, y, s, "matern32")
    ms2 = laplace.band_mean_sigma2(obj)
    L = 2
    d, a, r, kap, exc = DELAYS[1], np.array([0.9, 1.4]), 2.5, np.array([1.3, 1.3]), np.array([0.004, 0.01])
    ll, grad, hess, info = obj.loglik_hess_markov_noise_batch([d], [a], [r], [kap], [exc])
    assert info[0] == 0
    gt = np.concatenate([grad[0][:L + 1], grad[0][2 * L + 1:]])      # theta = [alpha_1, alpha_2, rho, kappa_1, kappa_2, nu_1, nu_2]
    H = hess[0]
    # shared kappa, nu fixed: x = [alpha_1, alpha_2, rho, kappa]
    nk, nv, J = laplace.noise_variables(L, ms2, "scale", True)
    assert (nk, nv) == (1, 0) and J.shape == (7, 4)
    gx, Hx = laplace.noise_to_x(J, grad[0], H)
    x = np.array([a[0], a[1], r, kap[0]])
    gu, Hu = laplace.hyper_to_u(x, gx, Hx)
    want_g = np.array([gt[0], gt[1], gt[2], gt[3] + gt[4]])
    want_H = np.empty((4, 4))
    for i in range(3):
        for j in range(3):
            want_H[i, j] = H[i, j]
        want_H[i, 3] = want_H[3, i] = H[i, 3] + H[i, 4]
    want_H[3, 3] = H[3, 3] + H[3, 4] + H[4, 3] + H[4, 4]
    assert np.allclose(gx, want_g, rtol=1e-14, atol=0) and np.allclose(Hx, want_H, rtol=1e-14, atol=0)
    for i in range(4):
        assert abs(gu[i] - x[i] * want_g[i]) <= 1e-14 * abs(gu[i])
        for j in range(4):
            w = x[i] * want_H[i, j] * x[j] + (x[i] * want_g[i] if i == j else 0.0)
            assert abs(Hu[i, j] - w) <= 1e-13 * max(abs(w), abs(x[i] * want_g[i])), (i, j)
    h = 1e-3 * kap[0]
    f = [obj.loglik_markov_noise_batch([d], [a], [r], [kap + q * h], [exc])[0][0] for q in (1, -1, 2, -2)]
    d1 = (8 * (f[0] - f[1]) - (f[2] - f[3])) / (12 * h)
    d2 = (16 * (f[0] + f[1]) - (f[2] + f[3]) - 30 * ll[0]) / (12 * h * h)
    assert abs(d1 - want_g[3]) <= 1e-8 * abs(want_g[3]) and abs(d2 - want_H[3, 3]) <= 1e-5 * abs(want_H[3, 3]), (d1, want_g[3], d2, want_H[3, 3])
    # a w per band beside a kappa per band: the rows of nu are scaled by mean(sigma_l^2)
    nk, nv, J = laplace.noise_variables(L, ms2, "both", False)
    gx, Hx = laplace.noise_to_x(J, grad[0], H)
    scale = np.array([1.0, 1.0, 1.0, 1.0, 1.0, ms2[0], ms2[1]])
    assert (nk, nv) == (2, 2) and np.allclose(gx, gt * scale, rtol=1e-15, atol=0) and np.allclose(Hx, H * scale[:, None] * scale[None, :], rtol=1e-15, atol=0)
    # "excess", shared: one w, kappa has no variable
    nk, nv, J = laplace.noise_variables(L, ms2, "excess", True)
    gx, Hx = laplace.noise_to_x(J, grad[0], H)
    assert (nk, nv) == (0, 1) and abs(gx[3] - (ms2[0] * gt[5] + ms2[1] * gt[6])) <= 1e-14 * abs(gx[3])
    assert abs(Hx[3, 3] - (ms2[0] ** 2 * H[5, 5] + 2 * ms2[0] * ms2[1] * H[5, 6] + ms2[1] ** 2 * H[6, 6])) <= 1e-13 * abs(Hx[3, 3])
    # through the evidence: the fixed part keeps its value, the shared variable is one number
    out = laplace.laplace_evidence_noise(obj, DELAYS[1:2], [a], [r], [kap], [exc], noise="scale", shared=True, rhomin=1e-2, rhomax=1e3)
    assert out[7][0] == 0 and np.array_equal(out[4][0], exc) and out[3][0][0] == out[3][0][1] and out[6].shape == (1, 4, 4)
