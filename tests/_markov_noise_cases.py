"""Cases, references and bars of the tests of the linear-time log-likelihood under a per-row noise model v_i = kappa_l^2 sigma_i^2 +
nu_l (tests/test_markov_noise_cpu.py, tests/test_gpu_markov_noise.py).

Cases: _markov_cases.cpu_cases(), unchanged, each with a noise model drawn from one default_rng(7) in the cases' order: kappa_l uniform
in [0.5, 2], nu_l uniform in [0, 0.05]; on every second case band 1 gets kappa = 0, nu = 0.01, the shape of the reference's unused
global-noise model (no reported error bar enters at all).

Reference: the value of a row is the value of a fresh data set with the error bars effective_std = sqrt(kappa^2 sigma^2 + nu) -- the
feature's contract -- so the reference is _grad_highprec.evaluate on those error bars, in extended precision: its loglik, its gradient
for the first 2L+1 entries, and from its kept G = w w' - K^-1 the noise entries, d/d nu_l = 1/2 sum_{i in l} G_ii and d/d kappa_l =
kappa_l sum_{i in l} G_ii sigma_i^2 (dK/d nu_l is the indicator of band l on the diagonal, dK/d kappa_l = 2 kappa_l sigma_i^2 there).

Bars, none from the code under test: the value's is _markov_cases.bar(e_dense, N, factor(alpha, effective_std)), e_dense the oracle's
dense fp64 error against the extended value on the same error bars; the first 2L+1 gradient entries' is _grad_highprec.bar(ref); the
noise entries' is the same factor max(1e-11, 64 eps cond_1(K)) times max(1, max|g_noise|)."""
import numpy as np

import _grad_highprec as H
import _markov_cases as MC
import _markov_grad_cases as GC

SLIPS = ("kappa_linear", "noise_all_bands", "nu_scaled")
_noise = {}


def noise_of(cid):
    """(kappa[L], nu[L]) of a case."""
    if not _noise:
        rg = np.random.default_rng(7)
        for idx, c in enumerate(MC.cpu_cases()):
            L = len(c[4])
            kappa, nu = rg.uniform(0.5, 2.0, L), rg.uniform(0.0, 0.05, L)
            if idx % 2 == 1:
                kappa[0], nu[0] = 0.0, 0.01
            _noise[c[0]] = (kappa, nu)
    return _noise[cid]


def effective(s, kappa, nu):
    """The error bars sqrt(kappa_l^2 sigma_l^2 + nu_l) per band, written out here: the oracle does not go through the package's
    fit.effective_std."""
    return [np.sqrt(kappa[l] ** 2 * np.asarray(s[l], np.float64) ** 2 + nu[l]) for l in range(len(s))]


def cases(N):
    """The cases at N = 110 or 150 (72 each), or subset_767() (12), each with its noise model appended: (..., N, kappa, nu)."""
    base = GC.subset_767() if N == 767 else GC.cases(N)
    return [c + noise_of(c[0]) for c in base]


def job(case):
    """The arguments of reference_job for a case."""
    cid, kernel, (t, y, s), delays, alpha, rho, mb, N, kappa, nu = case
    return (kernel, t, y, effective(s, kappa, nu), delays, alpha, rho, mb, s, kappa)


def reference_job(args):
    """(Reference on the effective error bars, g_kappa[L], g_nu[L]) in extended precision: a top-level function, for a process pool."""
    kernel, t, y, eff, delays, alpha, rho, mb, s, kappa = args
    ref = H.evaluate(kernel, t, y, eff, delays, alpha, rho, mb, keep=True)
    if ref.info:
        return ref, None, None
    Gd = np.diagonal(ref.parts["G"])
    band = ref.parts["band"]
    s2 = np.concatenate([np.asarray(a, np.float64) for a in s]).astype(H.LD) ** 2
    L = len(t)
    gk = np.array([float(H.LD(kappa[l]) * np.sum((Gd * s2)[band == l])) for l in range(L)])
    gv = np.array([float(np.sum(Gd[band == l]) / 2) for l in range(L)])
    ref.parts = {}
    return ref, gk, gv


def value_bar(oracle, case, ref):
    """Relative bar of the value of a case, from the reference side: (bar, e_dense)."""
    cid, kernel, (t, y, s), delays, alpha, rho, mb, N, kappa, nu = case
    eff = effective(s, kappa, nu)
    d, info = oracle.loglik_batch(kernel, t, y, eff, delays[None, :], alpha[None, :], [rho], mb)
    assert info[0] == 0, cid
    e = abs(float(d[0]) - ref.loglik) / abs(ref.loglik)
    return MC.bar(e, N, MC.factor(alpha, eff)), e


def noise_bar(ref, gk, gv):
    """The largest |g - reference| accepted for a noise entry."""
    return max(1e-11, 64 * H.EPS64 * ref.cond) * max(1.0, float(np.max(np.abs(np.concatenate([gk, gv])))))


def ratios(ll, grad, oracle, case, reference):
    """(value, first 2L+1 entries, noise entries): error / bar of one row (ll, grad[4L+1]) against a case's reference_job result."""
    ref, gk, gv = reference
    L = len(case[4])
    b, _ = value_bar(oracle, case, ref)
    rv = abs(ll - ref.loglik) / abs(ref.loglik) / b
    rg = H.ratio(grad[:2 * L + 1], ref)
    rn = float(np.max(np.abs(np.asarray(grad[2 * L + 1:]) - np.concatenate([gk, gv])))) / noise_bar(ref, gk, gv)
    return rv, rg, rn
