"""Lock-step batched BFGS (host logic, numpy): P independent minimisations with gradients advance together so that every round
submits ONE batch of value-and-gradient evaluations -- the peer of neldermead.BatchedNelderMead for the entries that return an exact
gradient (Objective.loglik_grad_markov_resampled: fit.realisation_refits(optimiser="bfgs"), fit.realisation_peaks).

The per-problem algorithm is the textbook one (Nocedal & Wright, Numerical Optimization, algorithm 6.1 with a backtracking line search):
    direction   p = -H g, H the inverse-Hessian approximation, H = I at the start; should g'p >= 0, H is reset to I (p = -g)
    line search Armijo backtracking by halving, every trial ONE round: t = 1 (in the first iteration and after a reset
                min(1, 1 / ||g||_1), the step has no scale yet), accepted when f(x + t p) <= f + 1e-4 t g'p, else t <- t / 2; after
                MAX_HALVINGS rejected trials H is reset to I once, and a second exhausted search ends the problem where it stands
    update      s = t p, y = g_new - g; skipped when y's <= 0; before the first update H = (y's / y'y) I (N&W 6.20); then
                H <- (I - r s y') H (I - r y s') + r s s', r = 1 / y's
    stop        ||g||_inf <= g_tol (converged) or `iterations` accepted steps
A value that is not finite, or a finite value with a gradient that is not, counts as +inf: such a trial is rejected; a start of this
kind ends the problem at once, not converged.  Nothing is random, and a problem's arithmetic is elementwise or a sum over its own
short rows, so its trajectory does not depend on which other problems are in the batch or on when they stop."""
import numpy as np

C1 = 1e-4
MAX_HALVINGS = 40


class BatchedBFGS:
    """Minimise f for P problems of dimension n.  `fg(pidx, X)` evaluates the rows of X (K, n), row i belonging to problem pidx[i],
    and returns (f[K], g[K, n]).  run() -> (xmin[P, n], fmin[P]); afterwards f_calls, rounds, converged[P], iterations_done[P],
    gmin[P, n] (the gradient at xmin) and f_start[P] (the value at x0)."""

    def __init__(self, x0, fg, iterations, g_tol=1e-6):
        self.x0 = np.array(x0, dtype=np.float64)
        self.P, self.n = self.x0.shape
        self.fg = fg
        self.iterations = int(iterations)
        self.g_tol = g_tol
        self.f_calls = 0
        self.rounds = 0

    def _eval(self, pidx, X):
        f, g = self.fg(pidx, X)
        f = np.array(f, dtype=np.float64).reshape(len(pidx))
        g = np.array(g, dtype=np.float64).reshape(len(pidx), self.n)
        self.f_calls += len(pidx)
        self.rounds += 1
        bad = ~np.isfinite(f) | ~np.isfinite(g).all(axis=1)
        f[bad] = np.inf
        return f, g

    @staticmethod
    def _matvec(H, v):
        return (H * v[:, None, :]).sum(axis=2)

    def run(self):
        P, n = self.P, self.n
        x = self.x0.copy()
        f, g = self._eval(np.arange(P), x)
        self.f_start = f.copy()
        eye = np.eye(n)
        H = np.repeat(eye[None], P, axis=0)
        fresh = np.ones(P, dtype=bool)               # H is the identity and has no scale yet
        retried = np.zeros(P, dtype=bool)            # the line search was exhausted once since the last accepted step
        it = np.zeros(P, dtype=np.int64)
        halvings = np.zeros(P, dtype=np.int64)
        self.converged = np.isfinite(f) & (np.abs(g).max(axis=1) <= self.g_tol)
        active = np.isfinite(f) & ~self.converged & (self.iterations > 0)
        p, t, slope = np.zeros((P, n)), np.zeros(P), np.zeros(P)

        def new_direction(idx):
            """p, t and g'p of the problems idx from their H and g; halvings back to 0"""
            if not len(idx):
                return
            d = -self._matvec(H[idx], g[idx])
            sl = (g[idx] * d).sum(axis=1)
            up = ~(sl < 0.0)
            if up.any():
                r = idx[up]
                H[r], fresh[r] = eye, True
                d[up] = -g[r]
                sl[up] = -(g[r] * g[r]).sum(axis=1)
            p[idx], slope[idx] = d, sl
            t[idx] = np.where(fresh[idx], np.minimum(1.0, 1.0 / np.abs(g[idx]).sum(axis=1)), 1.0)
            halvings[idx] = 0

        new_direction(np.flatnonzero(active))
        while active.any():
            idx = np.flatnonzero(active)
            xt = x[idx] + t[idx, None] * p[idx]
            ft, gt = self._eval(idx, xt)
            ok = ft <= f[idx] + C1 * t[idx] * slope[idx]
            # rejected: halve; an exhausted search resets H once, then gives up
            rej = idx[~ok]
            if len(rej):
                t[rej] *= 0.5
                halvings[rej] += 1
                out = rej[halvings[rej] >= MAX_HALVINGS]
                if len(out):
                    stop = out[retried[out] | fresh[out]]
                    active[stop] = False
                    again = out[~(retried[out] | fresh[out])]
                    H[again], fresh[again], retried[again] = eye, True, True
                    new_direction(again)
            acc = idx[ok]
            if len(acc):
                s = xt[ok] - x[acc]
                y = gt[ok] - g[acc]
                ys = (y * s).sum(axis=1)
                upd = ys > 0.0
                if upd.any():
                    u, su, yu, r = acc[upd], s[upd], y[upd], 1.0 / ys[upd]
                    scale = fresh[u]
                    if scale.any():
                        H[u[scale]] = eye[None] * (ys[upd][scale] / (yu[scale] * yu[scale]).sum(axis=1))[:, None, None]
                        fresh[u[scale]] = False
                    Hy = self._matvec(H[u], yu)
                    yHy = (yu * Hy).sum(axis=1)
                    H[u] = (H[u] - r[:, None, None] * (su[:, :, None] * Hy[:, None, :] + Hy[:, :, None] * su[:, None, :])
                            + ((r * r * yHy + r)[:, None, None]) * (su[:, :, None] * su[:, None, :]))
                x[acc], f[acc], g[acc] = xt[ok], ft[ok], gt[ok]
                it[acc] += 1
                retried[acc] = False
                conv = np.abs(g[acc]).max(axis=1) <= self.g_tol
                self.converged[acc[conv]] = True
                done = conv | (it[acc] >= self.iterations)
                active[acc[done]] = False
                new_direction(acc[~done])
        self.iterations_done = it
        self.gmin = g
        return x, f
