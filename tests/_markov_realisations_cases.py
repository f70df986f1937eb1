"""Cases, realisations and references of the many-realisations linear-time log-likelihood's tests
(tests/test_markov_realisations_cpu.py, tests/test_gpu_markov_realisations.py).

Cases: those of tests/_markov_cases.py with rho in {0.1, 3, 300} (OU / matern32 / matern52 x L in {1, 2, 3} x both b-modes, the
"ties", "before" and "plain" delay kinds as that module deals them).  Per case R = 5 realisations on the case's cadence: the case's
own y, three flux-randomised ones (y + sigma z), and the first randomised one with its last band shifted by a constant.

The reference of loglik[m][r] is the dense value logpdf(N(Q mean_r, K + Sobs + B), Y_r): K from the model of the HANDLE's data set
(B from the prior variances markov.prepare reports for the original y), the same for every realisation, so a case is factorised
once (DenseModel) and solved per realisation.  Where numpy.longdouble is extended the reference is that value in extended precision
(K from _grad_highprec's kernels, its blocked Cholesky) and e_dense the relative error of the fp64 dense value (K from the oracle's
delayed covariance, the oracle's Cholesky) against it; otherwise the reference is that fp64 value and e_dense its relative
disagreement with a second, independent fp64 route (K from _grad_highprec's kernels, LAPACK's Cholesky through numpy).  The bar is
tests/_markov_cases.py's, measured on the reference side, per realisation: MC.bar(e_dense, N, MC.factor(alpha, stdarray)).

The shortcuts reach the existing references directly: without marginalise_b and with each realisation's own band means the value is
that of a fresh data set (t, Y_r, sigma) (fresh_reference: _markov_cases.reference_and_bar on it); with marginalise_b the same holds
for a realisation whose bands were affinely rescaled to the handle's band means and variances (rescale_to)."""
import math

import numpy as np

import _grad_highprec as H
import _markov_cases as MC

LD = H.LD
RHOS = (0.1, 3.0, 300.0)
SHIFT = 0.75
R = 5
_models = {}


def cases(sizes=(110,)):
    """The cases of MC.cpu_cases() at these N with rho in RHOS."""
    return [c for c in MC.cpu_cases() if c[7] in sizes and c[5] in RHOS]


def realisations(case, R=R):
    """The case's R >= 3 realisations, a list of L arrays (R, N_l): y, R - 2 flux-randomised, the first randomised one with its last
    band shifted by SHIFT."""
    from gpcc_amd import synthetic
    cid, _, (t, y, s), _, _, _, _, _ = case
    seed = sum(ord(ch) for ch in cid)
    rnd = synthetic.flux_randomise(y, s, R - 2, seed)
    out = []
    for l in range(len(t)):
        shifted = rnd[l][:1] + (SHIFT if l == len(t) - 1 else 0.0)
        out.append(np.concatenate([np.asarray(y[l], np.float64)[None, :], rnd[l], shifted], axis=0))
    return out


def own_means(Y):
    return np.stack([a.sum(axis=1) / a.shape[1] for a in Y], axis=1)


def rescale_to(yarray, Y):
    """Y with every band of every realisation affinely rescaled to the band mean and sample variance of yarray."""
    out = []
    for y, a in zip(yarray, Y):
        y = np.asarray(y, np.float64)
        m, sd = y.mean(), y.std(ddof=1)
        am, asd = a.mean(axis=1, keepdims=True), a.std(axis=1, ddof=1, keepdims=True)
        out.append(m + (a - am) * (sd / asd))
    return out


def _solve_lower(C, r):
    z = np.zeros_like(r)
    for i in range(len(r)):
        z[i] = (r[i] - C[i, :i] @ z[:i]) / C[i, i]
    return z


class DenseModel:
    """The dense model of one (handle data set, tau, alpha, rho): factorised once, value(y_r, mean_r) per realisation."""

    def __init__(self, oracle, kernel, data, delays, alpha, rho, mb):
        from gpcc_amd import markov
        t, y, s = data
        self.L, self.N = len(t), sum(len(a) for a in t)
        self.band = np.concatenate([np.full(len(a), l) for l, a in enumerate(t)])
        vb = markov.prepare(t, y, s, mb)[3]                          # the handle's Sigma_b (zeros without marginalise_b)
        s2 = np.concatenate([np.asarray(a, np.float64) ** 2 for a in s])
        same = self.band[:, None] == self.band[None, :]
        # fp64, the oracle's route
        K = np.array(oracle.delayed_covariance(kernel, alpha, delays, rho, t), dtype=np.float64)
        K[np.diag_indices(self.N)] += s2
        K = K + vb[self.band][:, None] * same
        self.C64, info = oracle.potrf_lower(K)
        assert info == 0
        # the second route: extended precision where there is one, else LAPACK on an independently built K
        tt = np.concatenate([np.asarray(a, np.float64) for a in t]).astype(LD)
        u = tt - np.asarray(delays, np.float64).astype(LD)[self.band]
        k = H._kernel(kernel, u[:, None] - u[None, :], np.float64(rho))[0]
        ab = np.asarray(alpha, np.float64).astype(LD)[self.band]
        K2 = ab[:, None] * ab[None, :] * k
        K2[np.diag_indices(self.N)] += s2.astype(LD)
        K2 = K2 + vb.astype(LD)[self.band][:, None] * same
        if H.EXTENDED:
            self.C2, self.Xd, info = H.cholesky_blocked(K2)
            assert info == 0
        else:
            self.C2, self.Xd = np.linalg.cholesky(K2.astype(np.float64)), None
        self.logdet64 = float(np.sum(np.log(np.diagonal(self.C64))))
        self.logdet2 = np.sum(np.log(np.diagonal(self.C2)))

    def value(self, y_r, mean_r):
        """(reference, e_dense) of one realisation: y_r the N fluxes in the bands' order, mean_r its L offsets."""
        r = np.asarray(y_r, np.float64) - np.asarray(mean_r, np.float64)[self.band]
        z = _solve_lower(self.C64, r)
        d64 = -(z @ z) / 2 - self.logdet64 - self.N * math.log(2 * math.pi) / 2
        if H.EXTENDED:
            r2 = np.asarray(y_r, np.float64).astype(LD) - np.asarray(mean_r, np.float64).astype(LD)[self.band]
            z2 = H.forward_solve(self.C2, self.Xd, r2)
            ref = float(-(z2 @ z2) / 2 - self.logdet2 - self.N * np.log(2 * np.pi * LD(1)) / 2)
            return ref, abs(d64 - ref) / abs(ref)
        z2 = _solve_lower(self.C2, r)
        other = float(-(z2 @ z2) / 2 - self.logdet2 - self.N * math.log(2 * math.pi) / 2)
        return d64, abs(other - d64) / abs(d64)


def general_reference(oracle, case, Y, mean):
    """[(reference, bar, e_dense)] per realisation of a case through the explicit dense route.  mean: (R, L)."""
    cid, kernel, data, delays, alpha, rho, mb, N = case
    if cid not in _models:
        _models[cid] = DenseModel(oracle, kernel, data, delays, alpha, rho, mb)
    model = _models[cid]
    flat = np.concatenate(Y, axis=1)
    F = MC.factor(alpha, data[2])
    out = []
    for r in range(flat.shape[0]):
        ref, e = model.value(flat[r], mean[r])
        out.append((ref, MC.bar(e, N, F), e))
    return out


def fresh_reference(oracle, case, Y, r, tag="fresh"):
    """(reference, bar, e_dense) of realisation r as a data set of its own: MC.reference_and_bar on (t, Y_r, sigma).  tag: names Y in
    that module's cache."""
    cid, kernel, (t, _, s), delays, alpha, rho, mb, N = case
    fresh = ("%s/%s%d" % (cid, tag, r), kernel, (t, [a[r] for a in Y], s), delays, alpha, rho, mb, N)
    return MC.reference_and_bar(oracle, fresh)
