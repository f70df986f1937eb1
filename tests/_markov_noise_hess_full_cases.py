"""Cases, references and bars of the tests of the linear-time full Hessian under a per-row noise model -- the rows of tau --
(tests/test_markov_noise_hess_full_cpu.py, tests/test_gpu_markov_noise_hess_full.py), over the gradient row's order
theta = [alpha_1..alpha_L, rho, tau_1..tau_L, kappa_1..kappa_L, nu_1..nu_L], n = 4L + 1.

Cases: _markov_noise_cases.cases(N) for N = 110 and 150 (72 each), each with its noise model.  12 of the 144 are OU with a cross-band
tie in shifted time (six at each N; their names end in "-ties", _markov_hess_full_cases.tie_rows finds them): no second derivative by
tau exists there, they check the NaN contract instead of the bars.  Every other case is held to its bars.

Reference: _hess_highprec.evaluate(..., keep=True) on the effective error bars sqrt(kappa^2 sigma^2 + nu), extended to n = 4L + 1 by
_markov_noise_hess_cases.trace_hessian's formulas in numpy.longdouble,
    H = T1 - T2 + T3,  T1 = 1/2 sum_ij G_ij d2K_ij,  T2 = (D_a w)' C (D_b w),  T3 = 1/2 tr(C D_a C D_b),  G = w w' - C,  C = K^-1,
_hess_highprec._dmat and _d2 for the pairs of alpha, rho and tau; D_nu_l the indicator of band l on the diagonal, D_kappa_l =
2 kappa_l sigma^2 there; d2K = 2 sigma^2 on the diagonal of band l for (kappa_l, kappa_l) and zero for every other pair with a noise
parameter, so for a (tau, noise) pair T1 = 0, T2 = (D_tau w)' C (D_n w), T3 = 1/2 tr(C D_tau C D_n).

Blocks: aa, ar, rr, an, rn, nn, at, rt, tt, tn.  Bars, from the reference side only, exactly as _markov_noise_hess_cases computes them:
    bar_B = FACTOR max(e_dense_B, floor_B),
e_dense_B the largest error over B of the same trace formula in fp64 against the extended value over _hess_highprec.MIRRORS'
factorisation orders, floor_B = N 2^-53 max over B of (|T1| + |T2| + |T3|); the ratio error / bar is multiplied by 16 / factor with
factor = _markov_cases.factor(alpha, effective_std).  Nothing in a bar comes from the code under test."""
import math

import numpy as np

import _hess_highprec as HH
import _markov_cases as MC
import _markov_hess_full_cases as FC
import _markov_noise_cases as NC
import _markov_noise_hess_cases as NH

SIZES = (110, 150)
# slip: the blocks it touches
SLIPS = {"tau_noise_no_dvar": ("tn",), "tau_noise_as_state": ("tn",), "plain_variance": ("at", "rt", "tt"), "tau_noise_own_band": ("tn",)}
BLOCKS = ("aa", "ar", "rr", "an", "rn", "nn", "at", "rt", "tt", "tn")
TAU_BLOCKS = ("at", "rt", "tt", "tn")
_KINDS = {"aa": (0, 0), "ar": (0, 1), "rr": (1, 1), "an": (0, 3), "rn": (1, 3), "nn": (3, 3), "at": (0, 2), "rt": (1, 2), "tt": (2, 2), "tn": (2, 3)}
LD = HH.LD
README_DELAYS = FC.README_DELAYS
README_MODE = FC.README_MODE


def cases(N=None):
    return [c for n in (SIZES if N is None else (N,)) for c in NC.cases(n)]


def is_tie(case):
    """Whether a case is OU with two points of different bands at exactly the same shifted time: the NaN contract, not the bars."""
    return FC.ou_tie(case[:8])


job = NH.job


def kinds(L):
    """0 alpha, 1 rho, 2 tau, 3 noise per index of the 4L + 1 order."""
    return np.array([0] * L + [1] + [2] * L + [3] * (2 * L))


def block_masks(L):
    """{block: boolean [n, n] mask}, n = 4L + 1."""
    kind = kinds(L)
    out = {}
    for name in BLOCKS:
        a, b = _KINDS[name]
        m = (kind[:, None] == a) & (kind[None, :] == b)
        out[name] = m | m.T
    return out


def block_of(L):
    """[n, n] array of block names."""
    out = np.empty((4 * L + 1, 4 * L + 1), dtype=object)
    for name, m in block_masks(L).items():
        out[m] = name
    return out


def tau_mask(L):
    """Boolean [4L+1, 4L+1]: the entries with a tau index."""
    m = np.zeros((4 * L + 1, 4 * L + 1), bool)
    m[L + 1:2 * L + 1, :] = m[:, L + 1:2 * L + 1] = True
    return m


def noise_index(L):
    """The indices {0..L, 2L+1..4L} of the [alpha, rho, kappa, nu] sub-block."""
    return list(range(L + 1)) + list(range(2 * L + 1, 4 * L + 1))


def trace_hessian(st, s2, kappa):
    """(H[n, n], terms[3, n, n]) in st's type by the trace formulas over [alpha, rho, tau, kappa, nu]; st: _hess_highprec._state's, on
    the effective error bars; s2: the reported sigma^2 per point in st's order of points."""
    T, L, band = st["T"], st["L"], st["band"]
    n, K = 4 * L + 1, 2 * L + 1
    C, w = st["C"], st["w"]
    G = w[:, None] * w[None, :] - C
    Gd = np.diagonal(G)
    s2 = np.asarray(s2).astype(T)
    diag = {}                                  # the diagonal of D_theta of a noise parameter
    for l in range(L):
        e = (band == l).astype(T)
        diag[K + l] = 2 * T(np.float64(kappa[l])) * s2 * e
        diag[K + L + l] = e
    U, M = [], []
    for th in range(n):
        if th < K:
            U.append(HH._dmat(st, th) @ w)
            M.append(st["M"][th])
        else:
            U.append(diag[th] * w)
            M.append(C * diag[th][None, :])
    Z = [C @ u for u in U]
    terms = np.zeros((3, n, n), dtype=T)
    for a in range(n):
        for b in range(a, n):
            if b < K:
                t1 = np.sum(G * HH._d2(st, a, b)) / 2
            elif a == b and b < K + L:         # (kappa_l, kappa_l): d2K = 2 sigma^2 on the diagonal of band l
                t1 = np.sum(Gd * (2 * s2 * (band == b - K).astype(T))) / 2
            else:
                t1 = T(0)
            terms[0, a, b] = terms[0, b, a] = t1
            terms[1, a, b] = terms[1, b, a] = U[a] @ Z[b]
            terms[2, a, b] = terms[2, b, a] = np.sum(M[a] * M[b].T) / 2
    return terms[0] - terms[1] + terms[2], terms


def reference_job(args):
    """The NoiseReference (H over 4L + 1, bars over the ten blocks) of job(case): a top-level function, for a process pool."""
    kernel, t, y, eff, delays, alpha, rho, mb, s, kappa = args
    ref = HH.evaluate(kernel, t, y, eff, delays, alpha, rho, mb, keep=True)
    out = NH.NoiseReference()
    out.info, out.L, out.N, out.cond = ref.info, ref.L, ref.N, ref.cond
    if ref.info:
        return out
    L, N = ref.L, ref.N
    s2 = np.concatenate([np.asarray(a, np.float64) for a in s]) ** 2
    H, terms = trace_hessian(ref.parts["st"], s2, kappa)
    out.H_ld, out.H = H, H.astype(np.float64)
    masks = block_masks(L)
    size = np.abs(terms[0]) + np.abs(terms[1]) + np.abs(terms[2])
    out.floor = {b: N * 2.0 ** -53 * float(np.max(size[m])) for b, m in masks.items() if m.any()}
    out.e_dense = {b: 0.0 for b in out.floor}
    pargs = (kernel, t, y, eff, delays, alpha, rho, mb)
    for which in HH.MIRRORS:
        p = HH._problem(*pargs, np.float64)
        rev = which == "reversed"
        st = HH._state(HH._reverse(p) if rev else p, blocked=HH.BLOCKED.get(which, 0))
        if st["info"]:
            continue
        H64, _ = trace_hessian(st, s2[::-1] if rev else s2, kappa)
        err = np.abs(H64.astype(LD) - H)
        for b in out.e_dense:
            out.e_dense[b] = max(out.e_dense[b], float(np.max(err[masks[b]])))
    out.bars = {b: MC.FACTOR * max(out.e_dense[b], out.floor[b]) for b in out.e_dense}
    return out


def mirror_job(case):
    """markov.loglik_hess_full_noise of a case -> (loglik, grad, hess, info): a top-level function, for a process pool."""
    from gpcc_amd import markov
    cid, kernel, data, delays, alpha, rho, mb, N, kappa, nu = case
    return markov.loglik_hess_full_noise(kernel, *data, delays, alpha, rho, kappa, nu, mb)


def slip_job(args):
    """markov.loglik_hess_full_noise of (case, slip, pairs): a top-level function, for a process pool."""
    from gpcc_amd import markov
    (cid, kernel, data, delays, alpha, rho, mb, N, kappa, nu), slip, pairs = args
    return markov.loglik_hess_full_noise(kernel, *data, delays, alpha, rho, kappa, nu, mb, pairs=pairs, _slip=slip)


def pairs_of(L, blocks):
    """The pairs (a <= b) of the 4L + 1 order that lie in the given blocks."""
    masks = block_masks(L)
    n = 4 * L + 1
    return [(a, b) for a in range(n) for b in range(a, n) if any(masks[k][a, b] for k in blocks)]


scale = NH.scale


def entry_bars(ref, case, bars=1.0):
    """[n, n]: the largest error of an entry that `bars` bars of its block allow (bar_B / scale: the ratio is error / bar_B * scale)."""
    names = block_of(ref.L)
    out = np.zeros(names.shape)
    for b, bar in ref.bars.items():
        out[names == b] = bars * bar / scale(case)
    return out


def ratios(hess, ref, case, against=None, blocks=BLOCKS, index=None):
    """{block: error / bar} of a result against the reference, or against another result with the reference's bars.  index: the
    indices of the 4L + 1 order that the rows of hess (and of against) stand for (default: all of them).  Entries that are NaN in hess
    are an infinite error."""
    hess = np.asarray(hess, np.float64)
    n = 4 * ref.L + 1
    index = list(range(n)) if index is None else list(index)
    want = ref.H[np.ix_(index, index)] if against is None else np.asarray(against, np.float64)
    err = np.abs(hess - want)
    out = {}
    for b, m in block_masks(ref.L).items():
        m = m[np.ix_(index, index)]
        if b not in blocks or not m.any():
            continue
        e, bar = float(np.max(err[m])) if not np.isnan(err[m]).any() else math.inf, ref.bars[b]
        r = e / bar * scale(case) if bar > 0 else (0.0 if e == 0 else math.inf)
        out[b] = r if r == r else math.inf
    return out


def worst(r):
    return max(r.values())


def inverse_bound(cov, E):
    """The largest change of each entry of cov = A^-1 when every entry of A moves by at most E (same shape):
    (A + d)^-1 - A^-1 = -A^-1 d A^-1 + A^-1 d A^-1 d A^-1 - ..., so entrywise |change| <= |cov| E |cov| (1 + q + q^2 + ...) with
    q = || |cov| E ||_inf; for q <= 1/2 (asserted) the series is at most 2: the bound is 2 |cov| E |cov|."""
    cov, E = np.abs(np.asarray(cov, np.float64)), np.asarray(E, np.float64)
    q = float(np.max(np.sum(cov @ E, 1)))
    assert q <= 0.5, q
    return 2.0 * (cov @ E @ cov)
