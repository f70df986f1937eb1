"""The Laplace-marginalised evidence over alpha and rho, host logic in Python: the numpy mirror of the lock-step
damped Newton polish of csrc/gpcc_laplace.h (gpcc_newton_batch, gpcc_laplace_evidence), as neldermead.py mirrors the Nelder-Mead
of gpcc_fit.h.

Prior convention: log-uniform in every alpha_l on (0, inf) and in rho on [rhomin, rhomax], i.e. flat in
u = (log alpha_1 .. log alpha_L, log rho), the same measure at every delay.  Its normalising constant (improper in alpha) is common
to all delays and cancels in getprobabilities, so log_evidence is log Z(tau) up to ONE ADDITIVE CONSTANT SHARED BY ALL DELAYS: only
differences and normalised probabilities mean anything.  At the mode u^ of l(u):

    log Z(tau) ~ l(u^) + (L+1)/2 log 2 pi - 1/2 log det(-H_u(u^)),   g_u = theta g_theta,
    H_u = diag(theta) H_theta diag(theta) + diag(theta g_theta).

Every (n x n) system is solved by the same explicit scalar Cholesky, in the same order, as the C++ code (not numpy.linalg), and all
arithmetic is on Python floats with the math module (no FMA, libm's log / exp / sqrt), so the steps are bitwise those of
gpcc_newton_batch."""
import math

import numpy as np

NOT_CONVERGED, NOT_MAXIMUM, ON_BOUND, BAD_START = -10, -11, -12, -13   # include/gpcc_hip.h: GPCC_LAPLACE_*
LOG2PI = 1.8378770664093453
INF = float("inf")
FTOL = 1e-12   # a step is accepted unless l decreases by more than FTOL max(1, |l|) (the rounding of an evaluated l)


def chol(n, A, pmin=0.0):
    """A = Lc Lc' (A: n*n list, row-major) -> Lc (list) or None when a pivot is not > pmin."""
    Lc = [0.0] * (n * n)
    for j in range(n):
        d = A[j * n + j]
        for k in range(j):
            d = d - Lc[j * n + k] * Lc[j * n + k]
        if not (d > pmin):
            return None
        ljj = math.sqrt(d)
        Lc[j * n + j] = ljj
        for i in range(j + 1, n):
            s = A[i * n + j]
            for k in range(j):
                s = s - Lc[i * n + k] * Lc[j * n + k]
            Lc[i * n + j] = s / ljj
    return Lc


def chol_solve(n, Lc, b):
    x = [0.0] * n
    for i in range(n):
        s = b[i]
        for k in range(i):
            s = s - Lc[i * n + k] * x[k]
        x[i] = s / Lc[i * n + i]
    for i in range(n - 1, -1, -1):
        s = x[i]
        for k in range(i + 1, n):
            s = s - Lc[k * n + i] * x[k]
        x[i] = s / Lc[i * n + i]
    return x


def chol_inverse(n, Lc):
    Li = [0.0] * (n * n)
    for j in range(n):
        Li[j * n + j] = 1.0 / Lc[j * n + j]
        for i in range(j + 1, n):
            s = 0.0
            for k in range(j, i):
                s = s + Lc[i * n + k] * Li[k * n + j]
            Li[i * n + j] = -s / Lc[i * n + i]
    cov = [0.0] * (n * n)
    for i in range(n):
        for j in range(i, n):
            s = 0.0
            for k in range(j, n):
                s = s + Li[k * n + i] * Li[k * n + j]
            cov[i * n + j] = s
            cov[j * n + i] = s
    return cov


def hyper_to_u(theta, gt, Ht):
    """Chain rule theta = exp(u) for one evaluation: theta (n), gt (>= n: the leading n entries of a gradient row), Ht (n x n) ->
    (g_u, H_u) as numpy arrays, bitwise gpcc_laplace.h's hyper_to_u."""
    n = len(theta)
    th = [float(v) for v in theta]
    gu = [th[i] * float(gt[i]) for i in range(n)]
    Hu = [[(th[i] * float(Ht[i][j])) * th[j] for j in range(n)] for i in range(n)]
    for i in range(n):
        Hu[i][i] = Hu[i][i] + gu[i]
    return np.array(gu), np.array(Hu)


class BatchedNewton:
    """Maximise l for P problems of dimension n.  fbatch(pidx, U) -> (val[K], grad[K, n], hess[K, n, n]) for the rows of U (K, n),
    row i belonging to problem pidx[i]; a non-finite value = rejected point.  lo, hi: the box (n each, None = unbounded).

    one_sided: indices of variables that may END on a bound.  A variable that finishes fixed at a bound with the gradient pointing out
    (|g_k| > g_tol) makes the problem ON_BOUND; a one-sided one is PINNED instead: it is left out of -H and of the 1/2 log 2 pi count
    and contributes -log|g_k|, the leading-order boundary Laplace term (the integral of exp(-|g_k| x) over x >= 0), so that
        log Z = f + (n_free / 2) log 2 pi - 1/2 log det(-H_free) - sum over the pinned k of log|g_k|,
    info stays 0, `pinned` [P][n] says which, and cov holds the inverse of -H_free with zero rows and columns for the pinned variables.
    Evidences with different pinned sets are comparable only to the order of that approximation.  With the empty default every step
    and every result is what it was."""

    def __init__(self, u0, fbatch, max_rounds=50, g_tol=1e-6, lo=None, hi=None, one_sided=()):
        self.u0 = np.array(u0, dtype=np.float64)
        self.P, self.n = self.u0.shape
        self.fbatch = fbatch
        self.max_rounds, self.g_tol = int(max_rounds), float(g_tol)
        self.lo = [-INF] * self.n if lo is None else [float(v) for v in lo]
        self.hi = [INF] * self.n if hi is None else [float(v) for v in hi]
        self.f_calls = 0
        self.batches = 0
        self.trace = []   # (pidx list, U rows) of every batch, in order
        self.one_sided = frozenset(int(k) for k in one_sided)
        self.pinned = [[False] * self.n for _ in range(self.P)]

    def _fixed(self, p, k):
        uk, gk = self.u[p][k], self.g[p][k]
        return (uk <= self.lo[k] and gk < 0.0) or (uk >= self.hi[k] and gk > 0.0)

    def _direction(self, p):
        n = self.n
        Hp, gp = self.H[p], self.g[p]
        fx = [self._fixed(p, i) for i in range(n)]
        A = [0.0] * (n * n)
        rhs = [0.0] * n
        s = 0.0
        for i in range(n):
            rhs[i] = 0.0 if fx[i] else gp[i]
            for j in range(n):
                A[i * n + j] = (1.0 if i == j else 0.0) if (fx[i] or fx[j]) else -Hp[i * n + j]
            if not fx[i] and abs(A[i * n + i]) > s:
                s = abs(A[i * n + i])
        if not (s > 0.0) or not math.isfinite(s):
            s = 1.0
        lam = 0.0
        for _ in range(40):
            B = list(A)
            for i in range(n):
                if not fx[i]:
                    B[i * n + i] = B[i * n + i] + lam
            Lc = chol(n, B, 1e-8 * s)
            if Lc is not None:
                d = chol_solve(n, Lc, rhs)
                if not all(math.isfinite(v) for v in d):
                    return None
                return d
            lam = 1e-3 * s if lam == 0.0 else lam * 10.0
        return None

    def _finish_pinned(self, p, pin):
        """_finish(p, 0) with the one-sided variables `pin` fixed at a bound with an outward gradient."""
        n = self.n
        free = [k for k in range(n) if k not in pin]
        m = len(free)
        A = [-self.H[p][i * n + j] for i in free for j in free]
        Lc = chol(m, A)
        cov = [0.0 if Lc is not None else float("nan")] * (n * n)
        if Lc is not None:
            ci = chol_inverse(m, Lc)
            for a, i in enumerate(free):
                for b, j in enumerate(free):
                    cov[i * n + j] = ci[a * m + b]
        self.cov[p] = cov
        code = 0
        for k in free:
            if self._fixed(p, k) and abs(self.g[p][k]) > self.g_tol:
                code = ON_BOUND
        if code == 0 and Lc is None:
            code = NOT_MAXIMUM
        self.info[p] = code
        if code == 0:
            hl = 0.0
            for k in range(m):
                hl = hl + math.log(Lc[k * m + k])
            for k in pin:
                hl = hl + math.log(abs(self.g[p][k]))
                self.pinned[p][k] = True
            self.logz[p] = self.f[p] + 0.5 * float(m) * LOG2PI - hl
        else:
            self.logz[p] = float("nan")

    def _finish(self, p, code):
        n = self.n
        if code == 0 and self.one_sided:
            pin = [k for k in sorted(self.one_sided) if self._fixed(p, k) and abs(self.g[p][k]) > self.g_tol]
            if pin:
                self._finish_pinned(p, pin)
                return
        A = [-v for v in self.H[p]]
        Lc = chol(n, A)
        self.cov[p] = chol_inverse(n, Lc) if Lc is not None else [float("nan")] * (n * n)
        if code == 0:
            for k in range(n):
                if self._fixed(p, k) and abs(self.g[p][k]) > self.g_tol:
                    code = ON_BOUND
        if code == 0 and Lc is None:
            code = NOT_MAXIMUM
        self.info[p] = code
        if code == 0:
            hl = 0.0
            for k in range(n):
                hl = hl + math.log(Lc[k * n + k])
            self.logz[p] = self.f[p] + 0.5 * float(n) * LOG2PI - hl
        else:
            self.logz[p] = float("nan")

    def _decide(self, p):
        n = self.n
        pg = 0.0
        for k in range(n):
            if not self._fixed(p, k):
                a = abs(self.g[p][k])
                if not (a <= pg):
                    pg = INF if math.isnan(a) else a
        self.active[p] = False
        if pg <= self.g_tol:
            self._finish(p, 0)
            return
        d = None if self.rounds[p] >= self.max_rounds else self._direction(p)
        if d is None:
            self._finish(p, NOT_CONVERGED)
        else:
            self.dir[p] = d
            self.t[p] = 1.0
            self.active[p] = True

    def _eval(self, pidx, X):
        val, grad, hess = self.fbatch(np.array(pidx, dtype=np.int64), np.array(X, dtype=np.float64).reshape(len(pidx), self.n))
        val = [float(v) for v in np.asarray(val, dtype=np.float64).ravel()]
        grad = np.asarray(grad, dtype=np.float64).reshape(len(pidx), self.n)
        hess = np.asarray(hess, dtype=np.float64).reshape(len(pidx), self.n * self.n)
        self.f_calls += len(pidx)
        self.batches += 1
        self.trace.append((list(pidx), [list(x) for x in X]))
        for p in pidx:
            self.rounds[p] += 1
        return val, [[float(v) for v in r] for r in grad], [[float(v) for v in r] for r in hess]

    def _clip(self, k, v):
        if v < self.lo[k]:
            v = self.lo[k]
        if v > self.hi[k]:
            v = self.hi[k]
        return v

    def run(self):
        """-> (umax[P, n], fmax[P], log_evidence[P], cov[P, n, n], info[P], rounds[P])"""
        P, n = self.P, self.n
        nan = float("nan")
        self.u = [[0.0] * n for _ in range(P)]
        self.f = [0.0] * P
        self.g = [[0.0] * n for _ in range(P)]
        self.H = [[0.0] * (n * n) for _ in range(P)]
        self.logz = [nan] * P
        self.cov = [[nan] * (n * n) for _ in range(P)]
        self.info = [0] * P
        self.rounds = [0] * P
        self.t = [1.0] * P
        self.dir = [[0.0] * n for _ in range(P)]
        self.active = [False] * P
        pidx = list(range(P))
        X = [[self._clip(k, float(self.u0[p, k])) for k in range(n)] for p in range(P)]
        fv, gv, hv = self._eval(pidx, X)
        for p in range(P):
            self.u[p], self.f[p], self.g[p], self.H[p] = X[p], fv[p], gv[p], hv[p]
            if not math.isfinite(fv[p]):
                self.info[p] = BAD_START
                continue
            self._decide(p)
        while True:
            pidx = [p for p in range(P) if self.active[p]]
            if not pidx:
                break
            X = [[self._clip(k, self.u[p][k] + self.t[p] * self.dir[p][k]) for k in range(n)] for p in pidx]
            fv, gv, hv = self._eval(pidx, X)
            for i, p in enumerate(pidx):
                if math.isfinite(fv[i]) and fv[i] >= self.f[p] - FTOL * max(1.0, abs(self.f[p])):
                    self.u[p], self.f[p], self.g[p], self.H[p] = X[i], fv[i], gv[i], hv[i]
                    self._decide(p)
                else:
                    self.t[p] = 0.5 * self.t[p]
                    if self.rounds[p] >= self.max_rounds or self.t[p] < 1e-12:
                        self.active[p] = False
                        self._finish(p, NOT_CONVERGED)
        return (np.array(self.u), np.array(self.f), np.array(self.logz), np.array(self.cov).reshape(P, n, n),
                np.array(self.info, dtype=np.int32), np.array(self.rounds, dtype=np.int32))


def laplace_evidence(objective, delays, alpha0, rho0, rhomin=0.1, rhomax=20.0, max_rounds=50, g_tol=1e-6, solver="dense"):
    """The numpy mirror of gpcc_laplace_evidence over any objective with loglik_hess_hyper_batch(delays, alpha, rho) -> (loglik,
    grad, hess[M, L+1, L+1], fisher, info) (Objective's, or a CPU witness) -> (loglik, alpha, rho, log_evidence, cov, info, rounds).
    Same steps as the C++ polish (bitwise, given bitwise the same objective values).  solver "markov": the rounds call the objective's
    loglik_hess_hyper_markov_batch -> (loglik, grad, hess, info), the block in linear time (Objective's, or markov.MarkovObjective's)."""
    if solver not in ("dense", "markov"):
        raise ValueError("solver must be 'dense' or 'markov', got %r" % (solver,))
    delays = np.ascontiguousarray(np.atleast_2d(delays), dtype=np.float64)
    G, L = delays.shape
    alpha0 = np.asarray(alpha0, dtype=np.float64).reshape(G, L)
    rho0 = np.asarray(rho0, dtype=np.float64).reshape(G)
    n = L + 1
    u0 = np.array([[math.log(float(alpha0[g, l])) for l in range(L)] + [math.log(float(rho0[g]))] for g in range(G)])
    lo = [-INF] * L + [math.log(rhomin)]
    hi = [INF] * L + [math.log(rhomax)]
    start_info = np.zeros(G, dtype=np.int32)
    first = [True]

    def fb(pidx, U):
        a = np.array([[math.exp(float(U[i, l])) for l in range(L)] for i in range(len(pidx))]).reshape(len(pidx), L)
        r = np.array([math.exp(float(U[i, L])) for i in range(len(pidx))])
        if solver == "markov":
            ll, grad, hess, info = objective.loglik_hess_hyper_markov_batch(delays[pidx], a, r)
        else:
            ll, grad, hess, _, info = objective.loglik_hess_hyper_batch(delays[pidx], a, r)
        if first[0]:
            start_info[pidx] = info
            first[0] = False
        val = np.where(info == 0, ll, np.nan)
        gu = np.empty((len(pidx), n))
        Hu = np.empty((len(pidx), n, n))
        for i in range(len(pidx)):
            gu[i], Hu[i] = hyper_to_u(list(a[i]) + [r[i]], grad[i], hess[i][:n, :n])
        return val, gu, Hu

    nt = BatchedNewton(u0, fb, max_rounds=max_rounds, g_tol=g_tol, lo=lo, hi=hi)
    u, f, logz, cov, info, rounds = nt.run()
    alpha = np.array([[math.exp(float(u[g, l])) for l in range(L)] for g in range(G)]).reshape(G, L)
    rho = np.array([math.exp(float(u[g, L])) for g in range(G)])
    info = np.where((info == BAD_START) & (start_info != 0), start_info, info).astype(np.int32)
    return f, alpha, rho, logz, cov, info, rounds


NOISE_KINDS = ("scale", "excess", "both")


def noise_variables(L, ms2, noise="both", shared=False):
    """The variables of laplace_evidence_noise and their map to theta = [alpha_1..L, rho, kappa_1..L, nu_1..L]: (nk, nv, J) with nk
    kappa variables and nv variables w (nu_l = w mean(sigma_l^2)), and J [3L+1, n] the constant Jacobian d theta / d x of
    x = [alpha, rho, kappa variables, w variables]: rows and columns of the block are selected by it, summed where a variable is
    shared, and the rows of nu scaled by mean(sigma_l^2)."""
    if noise not in NOISE_KINDS:
        raise ValueError('noise must be "scale", "excess" or "both", got %r' % (noise,))
    nk = 0 if noise == "excess" else (1 if shared else L)
    nv = 0 if noise == "scale" else (1 if shared else L)
    n = L + 1 + nk + nv
    J = np.zeros((3 * L + 1, n))
    for i in range(L + 1):
        J[i, i] = 1.0
    for l in range(L):
        if nk:
            J[L + 1 + l, L + 1 + (0 if shared else l)] = 1.0
        if nv:
            J[2 * L + 1 + l, L + 1 + nk + (0 if shared else l)] = float(ms2[l])
    return nk, nv, J


def noise_to_x(J, grad_row, hess):
    """(g_x, H_x) of one row: grad_row the entry's [alpha, rho, tau, kappa, nu] row (4L+1), hess its (3L+1)^2 block."""
    L = (J.shape[0] - 1) // 3
    gt = np.concatenate([np.asarray(grad_row, np.float64)[:L + 1], np.asarray(grad_row, np.float64)[2 * L + 1:]])
    return J.T @ gt, J.T @ np.asarray(hess, np.float64) @ J


def band_mean_sigma2(objective):
    """mean(sigma_l^2) per band of an Objective or a markov.MarkovObjective: the unit of gpcc_grid_noise's dimensionless w."""
    edges = np.concatenate([[0], np.cumsum(objective.Nl if hasattr(objective, "Nl") else [len(t) for t in objective.data[0]])])
    return np.array([np.mean(objective.sflat[edges[l]:edges[l + 1]] ** 2) for l in range(len(edges) - 1)])


def laplace_evidence_noise(objective, delays, alpha0, rho0, kappa0, nu0, *, noise="both", shared=False, rhomin=0.1, rhomax=20.0,
                           kappamin=0.1, kappamax=10.0, wmin=1e-4, wmax=1e2, max_rounds=50, g_tol=1e-6):
    """The Laplace-marginalised evidence at every delay under a FITTED NOISE MODEL v_i = kappa_l^2 sigma_i^2 + nu_l: the
    lock-step damped Newton polish of laplace_evidence over objective.loglik_hess_markov_noise_batch (an Objective's, in linear time on
    the device, or a markov.MarkovObjective's, without a GPU) -> (loglik, alpha, rho, kappa, nu, log_evidence, cov, info, rounds, pinned).

    Variables u: log alpha_l, log rho, log kappa (L of them, or one when shared) and log w with nu_l = w mean(sigma_l^2) (L, or one when
    shared), gpcc_grid_noise's dimensionless variable.  noise: "scale" fits kappa, "excess" fits w, "both" both; the part that is not
    fitted stays at kappa0 / nu0 and has no variable.  alpha0 [G, L], rho0 [G], kappa0, nu0 [G, L] (or (L,)): the start, usually a
    NoiseGridFit; with shared=True band 1's kappa0 and nu0 / mean(sigma^2) start the shared variable.  The chain rule is on the host:
    rows and columns of the entry's (3L+1)^2 block are selected (summed for a shared variable), then theta = exp(u) as in hyper_to_u.

    Prior: flat in u -- alpha and rho as laplace_evidence, kappa on [kappamin, kappamax], w on [wmin, wmax]; the constant is shared by
    all delays, so only differences of log_evidence mean anything.

    ONE-SIDED VARIABLES.  Clean data puts w at its lower bound with the gradient pointing out.  kappa and w are one-sided
    (BatchedNewton): such a variable is pinned -- left out of -H and of the 1/2 log 2 pi count, contributing -log|g_k| instead, the
    leading-order boundary Laplace term -- info stays 0 and pinned[G, n] says which.  Evidences of delays with different pinned sets
    are comparable only to the order of that approximation.  alpha and rho keep ON_BOUND.  cov [G, n, n] is the covariance in u, with
    zero rows and columns for the pinned variables."""
    delays = np.ascontiguousarray(np.atleast_2d(delays), dtype=np.float64)
    G, L = delays.shape
    ms2 = band_mean_sigma2(objective)
    nk, nv, J = noise_variables(L, ms2, noise, shared)
    n = L + 1 + nk + nv
    alpha0 = np.asarray(alpha0, dtype=np.float64).reshape(G, L)
    rho0 = np.asarray(rho0, dtype=np.float64).reshape(G)
    kappa0 = np.broadcast_to(np.asarray(kappa0, dtype=np.float64), (G, L))
    nu0 = np.broadcast_to(np.asarray(nu0, dtype=np.float64), (G, L))
    lo = [-INF] * L + [math.log(rhomin)] + [math.log(kappamin)] * nk + [math.log(wmin)] * nv
    hi = [INF] * L + [math.log(rhomax)] + [math.log(kappamax)] * nk + [math.log(wmax)] * nv

    def safe_log(v, floor):
        return math.log(max(float(v), floor))

    u0 = np.array([[math.log(float(alpha0[g, l])) for l in range(L)] + [math.log(float(rho0[g]))]
                   + [safe_log(kappa0[g, l], kappamin) for l in range(nk)]
                   + [safe_log(nu0[g, l] / ms2[l], wmin) for l in range(nv)] for g in range(G)])
    start_info = np.zeros(G, dtype=np.int32)
    first = [True]

    def unpack(U, rows):
        K = len(U)
        x = np.array([[math.exp(float(U[i, k])) for k in range(n)] for i in range(K)]).reshape(K, n)
        kap = np.array(kappa0[rows]) if not nk else np.broadcast_to(x[:, L + 1:L + 1 + nk], (K, L)).copy()
        exc = np.array(nu0[rows]) if not nv else np.broadcast_to(x[:, L + 1 + nk:], (K, L)) * ms2
        return x, x[:, :L].copy(), x[:, L].copy(), kap, exc

    def fb(pidx, U):
        x, a, r, kap, exc = unpack(U, pidx)
        ll, grad, hess, info = objective.loglik_hess_markov_noise_batch(delays[pidx], a, r, kap, exc)
        if first[0]:
            start_info[pidx] = info
            first[0] = False
        val = np.where(info == 0, ll, np.nan)
        gu = np.empty((len(pidx), n))
        Hu = np.empty((len(pidx), n, n))
        for i in range(len(pidx)):
            gx, Hx = noise_to_x(J, grad[i], hess[i])
            gu[i], Hu[i] = hyper_to_u(x[i], gx, Hx)
        return val, gu, Hu

    nt = BatchedNewton(u0, fb, max_rounds=max_rounds, g_tol=g_tol, lo=lo, hi=hi, one_sided=range(L + 1, n))
    u, f, logz, cov, info, rounds = nt.run()
    _, alpha, rho, kappa, nu = unpack(u, np.arange(G))
    info = np.where((info == BAD_START) & (start_info != 0), start_info, info).astype(np.int32)
    return f, alpha, rho, kappa, nu, logz, cov, info, rounds, np.array(nt.pinned, dtype=bool).reshape(G, n)
