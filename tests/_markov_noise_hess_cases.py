"""Cases, references and bars of the tests of the linear-time Hessian under a per-row noise model (tests/test_markov_noise_hess_cpu.py,
tests/test_gpu_markov_noise_hess.py), over theta = [alpha_1..alpha_L, rho, kappa_1..kappa_L, nu_1..nu_L], n = 3L + 1.

Cases: _markov_noise_cases.cases(N) for N = 110 and 150 (72 each), each with its noise model.

Reference: _hess_highprec.evaluate(..., keep=True) on the effective error bars sqrt(kappa^2 sigma^2 + nu) -- the feature's contract is the
value of a fresh data set on those error bars -- extended to the noise parameters by the same trace formulas in numpy.longdouble,
    H = T1 - T2 + T3,  T1 = 1/2 sum_ij G_ij d2K_ij,  T2 = (D_a w)' C (D_b w),  T3 = 1/2 tr(C D_a C D_b),  G = w w' - C,  C = K^-1,
with D_nu_l the indicator of band l on the diagonal, D_kappa_l = 2 kappa_l sigma^2 on that diagonal, d2K = 2 sigma^2 on the diagonal
of band l for (kappa_l, kappa_l) and zero for every other pair that contains a noise parameter; M_theta = C D_theta is a column
scaling of C.

Blocks: aa, ar, rr (the plain block's) and an, rn, nn.  Bars, in _hess_highprec.add_bars' manner and from the reference side only:
    bar_B = FACTOR max(e_dense_B, floor_B),
e_dense_B the largest error over B of the same trace formula in fp64 against the extended value over _hess_highprec.MIRRORS'
factorisation orders, floor_B = N 2^-53 max over B of (|T1| + |T2| + |T3|); the ratio error / bar is multiplied by 16 / factor with
factor = _markov_cases.factor(alpha, effective_std), as _markov_hess_cases.scale does.  Nothing in a bar comes from the code under test."""
import math

import numpy as np

import _hess_highprec as HH
import _markov_cases as MC
import _markov_noise_cases as NC

SIZES = (110, 150)
SLIPS = ("no_d2kappa", "dvar_one_side", "kappa_linear", "noise_noise_diag_only", "rho_noise_no_dA")
BLOCKS = ("aa", "ar", "rr", "an", "rn", "nn")
LD = HH.LD


def cases(N=None):
    return [c for n in (SIZES if N is None else (N,)) for c in NC.cases(n)]


def job(case):
    """The argument of reference_job for a case."""
    cid, kernel, (t, y, s), delays, alpha, rho, mb, N, kappa, nu = case
    return (kernel, t, y, NC.effective(s, kappa, nu), delays, alpha, rho, mb, s, kappa)


def block_masks(L):
    """{block: boolean [n, n] mask}, n = 3L + 1."""
    kind = np.array([0] * L + [1] + [2] * (2 * L))
    out = {}
    for name, (a, b) in zip(BLOCKS, [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2)]):
        m = (kind[:, None] == a) & (kind[None, :] == b)
        out[name] = m | m.T
    return out


def trace_hessian(st, s2, kappa):
    """(H[n, n], terms[3, n, n]) in st's type by the trace formulas over [alpha, rho, kappa, nu]; st: _hess_highprec._state's, on the
    effective error bars; s2: the reported sigma^2 per point in st's order of points."""
    T, L, band = st["T"], st["L"], st["band"]
    n = 3 * L + 1
    C, w = st["C"], st["w"]
    G = w[:, None] * w[None, :] - C
    Gd = np.diagonal(G)
    s2 = np.asarray(s2).astype(T)
    diag = {}                                  # the diagonal of D_theta of a noise parameter
    for l in range(L):
        e = (band == l).astype(T)
        diag[L + 1 + l] = 2 * T(np.float64(kappa[l])) * s2 * e
        diag[2 * L + 1 + l] = e
    U, M = [], []
    for th in range(n):
        if th <= L:
            U.append(HH._dmat(st, th) @ w)
            M.append(st["M"][th])
        else:
            U.append(diag[th] * w)
            M.append(C * diag[th][None, :])
    Z = [C @ u for u in U]
    terms = np.zeros((3, n, n), dtype=T)
    for a in range(n):
        for b in range(a, n):
            if b <= L:
                t1 = np.sum(G * HH._d2(st, a, b)) / 2
            elif a == b and b <= 2 * L:       # (kappa_l, kappa_l): d2K = 2 sigma^2 on the diagonal of band l
                t1 = np.sum(Gd * (2 * s2 * (band == b - L - 1).astype(T))) / 2
            else:
                t1 = T(0)
            terms[0, a, b] = terms[0, b, a] = t1
            terms[1, a, b] = terms[1, b, a] = U[a] @ Z[b]
            terms[2, a, b] = terms[2, b, a] = np.sum(M[a] * M[b].T) / 2
    return terms[0] - terms[1] + terms[2], terms


class NoiseReference:
    """H (float64 [n, n]) of the extended trace formula, the per-block bars and what they were made of."""

    def __init__(self):
        self.info, self.H, self.H_ld, self.bars, self.e_dense, self.floor, self.cond, self.L, self.N = 0, None, None, None, None, None, math.inf, 0, 0


def reference_job(args):
    """The NoiseReference of job(case): a top-level function, for a process pool."""
    kernel, t, y, eff, delays, alpha, rho, mb, s, kappa = args
    ref = HH.evaluate(kernel, t, y, eff, delays, alpha, rho, mb, keep=True)
    out = NoiseReference()
    out.info, out.L, out.N, out.cond = ref.info, ref.L, ref.N, ref.cond
    if ref.info:
        return out
    L, N = ref.L, ref.N
    s2 = np.concatenate([np.asarray(a, np.float64) for a in s]) ** 2
    H, terms = trace_hessian(ref.parts["st"], s2, kappa)
    out.H_ld, out.H = H, H.astype(np.float64)
    masks = block_masks(L)
    size = np.abs(terms[0]) + np.abs(terms[1]) + np.abs(terms[2])
    out.floor = {b: N * 2.0 ** -53 * float(np.max(size[m])) for b, m in masks.items()}
    out.e_dense = {b: 0.0 for b in masks}
    pargs = (kernel, t, y, eff, delays, alpha, rho, mb)
    for which in HH.MIRRORS:
        p = HH._problem(*pargs, np.float64)
        rev = which == "reversed"
        st = HH._state(HH._reverse(p) if rev else p, blocked=HH.BLOCKED.get(which, 0))
        if st["info"]:
            continue
        H64, _ = trace_hessian(st, s2[::-1] if rev else s2, kappa)
        err = np.abs(H64.astype(LD) - H)
        for b, m in masks.items():
            out.e_dense[b] = max(out.e_dense[b], float(np.max(err[m])))
    out.bars = {b: MC.FACTOR * max(out.e_dense[b], out.floor[b]) for b in masks}
    return out


def mirror_job(case):
    """markov.loglik_hess_noise of a case -> (loglik, grad, hess, info): a top-level function, for a process pool."""
    from gpcc_amd import markov
    cid, kernel, data, delays, alpha, rho, mb, N, kappa, nu = case
    return markov.loglik_hess_noise(kernel, *data, delays, alpha, rho, kappa, nu, mb)


def hess_noise_job(args):
    """markov.loglik_hess_noise(kernel, t, y, s, delays, alpha, rho, kappa, nu, mb, slip) of the tuple args: for a process pool."""
    from gpcc_amd import markov
    return markov.loglik_hess_noise(*args[:10], _slip=args[10] if len(args) > 10 else None)


def scale(case):
    """16 / factor on the effective error bars: what the dense bars' ratio is multiplied by."""
    cid, kernel, (t, y, s), delays, alpha, rho, mb, N, kappa, nu = case
    return MC.FACTOR / MC.factor(alpha, NC.effective(s, kappa, nu))


def ratios(hess, ref, case, against=None, blocks=BLOCKS):
    """{block: error / bar} of an n x n result (or of its leading (L + 1) x (L + 1) block: then aa, ar, rr only) against the reference, or
    against another result with the reference's bars."""
    hess = np.asarray(hess, np.float64)
    k = hess.shape[0]
    want = ref.H if against is None else np.asarray(against, np.float64)
    err = np.abs(hess - want[:k, :k])
    out = {}
    for b, m in block_masks(ref.L).items():
        m = m[:k, :k]
        if b not in blocks or not m.any():
            continue
        e, bar = float(np.max(err[m])), ref.bars[b]
        r = e / bar * scale(case) if bar > 0 else (0.0 if e == 0 else math.inf)
        out[b] = r if r == r else math.inf
    return out


def worst(r):
    return max(r.values())
