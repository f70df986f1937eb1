"""References and bars of the leave-one-out tests (tests/test_loo_cpu.py, tests/test_gpu_loo.py), from the reference side only: nothing
here is taken from the numpy mirror (gpcc_amd.markov.loo) or from the device.

The definition (gpcc_loo_batch), for one row (tau, alpha, rho) with K, bbar and Y of objective(alpha, rho):
    G = K^-1,  w = G (Y - bbar),  var_i = 1 / G_ii,  mu_i = y_i - w_i / G_ii,
    lp_i = -(log 2 pi + log var_i + (y_i - mu_i)^2 / var_i) / 2,  loo = sum_i lp_i
and over rows with weights p_m = w_m / sum w:  mix_lp_i = -log sum_m p_m exp(-lp_mi),  mix_loo = sum_i mix_lp_i.

Three evaluations of it:
  extended   the definition in numpy.longdouble (x87 80-bit), K from _predict_highprec.model -- the assembly _grad_highprec and
             _predict_highprec use -- factored by their blocked Cholesky, G_ii = sum_k X_ki^2 and w = X'X r with X = C^-1.  Checked
             against 40-digit mpmath on the smallest case (tests/test_loo_cpu.py) where mpmath is present.
  formula    the same lines in float64 on the 16-blocked Cholesky (the dense entries' own block).
  brute      float64 and independent of the identity: delete point i, condition on the rest (numpy.linalg.solve),
             mu_i = bbar_i + k_i' K_-i^-1 r_-i,  var_i = K_ii - k_i' K_-i^-1 k_i.  Computed at every point; the per-point quantities take it
             at BRUTE_POINTS = 8 points per row (the points that tie in shifted time with another point first, at most 5, the rest
             evenly spaced), the two sums at all N.

The bar of a quantity q (mu, var, lp, loo, mix_lp, mix_loo) of one case:
    bar(q) = 16 max(e_formula, e_brute, N 2^-53 terms(q))
e_formula = max |formula - extended| over q's entries (all rows), e_brute the same for the brute-force value: over its 8 points for
mu, var, lp and mix_lp, and for the two sums, loo and mix_loo, the error of the brute-force sum over all N points.  terms(q), per entry,
is the size of what was summed to give it -- what the rounding of an fp64 sum is relative to:
    mu     |y_i| + sum_j |G_ij r_j| / G_ii        var    var_i  (G_ii is a sum of squares: no cancellation)
    lp     (log 2 pi + |log var_i| + (y_i - mu_i)^2 / var_i) / 2
    loo    sum_i terms(lp_i)        mix_lp   max_m terms(lp_mi)        mix_loo   sum_i terms(mix_lp_i)
No cond-based floor.  For the linear-time entry and its mirror the bar is multiplied by _markov_cases.factor(alpha, sigma) / 16, the
filter's conditioning alpha^2 / sigma^2.

Cases: _markov_cases.cpu_cases() at N = 110 and 150 (OU / matern32 / matern52, L = 1 .. 3, both b-modes, rho 0.1 .. 300, ties / before /
plain, the last band handed over unsorted), each with a second row (delays of the later bands moved by 2^-4, alpha x 1.25, rho x 0.8) for
the mixture, weights (0.75, 0.25); rbf on the L = 2 cases for the dense side."""
from dataclasses import dataclass

import numpy as np

import _markov_cases as MC
import _predict_highprec as PH
from _grad_highprec import EXTENDED, LD, NB, SKIP_REASON, cholesky_inverse  # noqa: F401

FACTOR = MC.FACTOR
U53 = 2.0 ** -53
BLOCKED_NB = 16
BRUTE_POINTS = 8
WEIGHTS = np.array([0.75, 0.25])
QUANTITIES = ("mu", "var", "lp", "loo", "mix_lp", "mix_loo")
_cache = {}


def cases():
    """[(id, kernel, data, delays[R, L], alpha[R, L], rho[R], marginalise_b, N)]: the Markov cases at N = 110 and 150, two rows each."""
    out = []
    for cid, kernel, data, delays, alpha, rho, mb, N in MC.cpu_cases():
        if N not in (110, 150):
            continue
        d2 = delays.copy()
        d2[1:] += 2.0 ** -4
        out.append((cid, kernel, data, np.stack([delays, d2]), np.stack([alpha, 1.25 * alpha]), np.array([rho, 0.8 * rho]), mb, N))
    return out


def rbf_cases():
    """The L = 2 cases with the rbf kernel (dense side only), one per (N, b-mode, rho)."""
    return [("rbf" + c[0][len(c[1]):], "rbf") + c[2:] for c in cases() if c[1] == "OU" and len(c[2][0]) == 2]


def _empty_tests(L):
    return [np.zeros(0)] * L


def row_values(m, dtype=LD, nb=NB):
    """(mu, var, lp, terms of mu, terms of lp) of a _predict_highprec.Model by the definition, the algebra in `dtype`."""
    K, r, y = m.K.astype(dtype), m.r.astype(dtype), m.y.astype(dtype)
    _, X, info = cholesky_inverse(K, nb)
    assert info == 0, info
    g = np.sum(X * X, axis=0)
    w = X.T @ (X @ r)
    var = 1 / g
    d = w / g
    log2pi = np.log(2 * dtype(PH.PI))
    lp = -(log2pi + np.log(var) + d * d / var) / 2
    tmu = tlp = None
    if dtype is LD:
        G = X.T @ X
        tmu = (np.abs(y) + np.abs(G * r[None, :]).sum(axis=1) / g).astype(np.float64)
        tlp = ((log2pi + np.abs(np.log(var)) + d * d / var) / 2).astype(np.float64)
    return y - d, var, lp, tmu, tlp


def mix_values(lp, weights):
    """mix_lp[N] = -log sum_m p_m exp(-lp_mi) in lp's type (max-shifted), zero-weight rows skipped."""
    p = np.asarray(weights, np.float64)
    p = p / p.sum()
    keep = p > 0
    x = np.log(p[keep].astype(lp.dtype))[:, None] - lp[keep]
    mx = x.max(axis=0)
    return -(mx + np.log(np.exp(x - mx[None, :]).sum(axis=0)))


def _brute_points(shifted, count=BRUTE_POINTS):
    N = len(shifted)
    vals, inv, cnt = np.unique(shifted, return_inverse=True, return_counts=True)
    tied = [i for i in range(N) if cnt[inv[i]] > 1][:count - 3]
    rest = [i for i in np.linspace(0, N - 1, count).round().astype(int) if i not in tied]
    return np.array((tied + rest)[:count], dtype=int)


def brute_row(m, pts, batch=32):
    """(mu, var, lp) at the points pts by deleting each and conditioning on the rest, in float64 (LAPACK solves, `batch` at a time)."""
    K, r = m.K.astype(np.float64), m.r.astype(np.float64)
    y, N = m.y.astype(np.float64), len(m.r)
    pts = np.asarray(pts, dtype=int)
    mu, var = np.empty(len(pts)), np.empty(len(pts))
    for o in range(0, len(pts), batch):
        sel = pts[o:o + batch]
        keep = np.stack([np.delete(np.arange(N), i) for i in sel])               # [b, N - 1]
        A = K[keep[:, :, None], keep[:, None, :]]
        k = K[keep, sel[:, None]]
        S = np.linalg.solve(A, np.stack([r[keep], k], axis=2))
        mu[o:o + batch] = (y[sel] - r[sel]) + np.einsum("bi,bi->b", k, S[:, :, 0])
        var[o:o + batch] = K[sel, sel] - np.einsum("bi,bi->b", k, S[:, :, 1])
    e = y[pts] - mu
    return mu, var, -0.5 * (np.log(2.0 * np.pi) + np.log(var) + e * e / var)


@dataclass
class Reference:
    """The extended values of one case [rows, N] and the bar of each quantity, with what went into it."""
    mu: np.ndarray = None
    var: np.ndarray = None
    lp: np.ndarray = None
    loo: np.ndarray = None
    mix_lp: np.ndarray = None
    mix_loo: object = None
    bar: dict = None
    e_formula: dict = None
    e_brute: dict = None
    pts: np.ndarray = None
    scale: float = 1.0            # the linear-time bar's factor: _markov_cases.factor / 16

    def ratio(self, what, got, rows=None, markov=False):
        """max |got - reference| / bar over the entries (rows: the rows of the case that `got` holds): <= 1 passes."""
        ref, b = getattr(self, what), self.bar[what]
        if rows is not None and what in ("mu", "var", "lp", "loo"):
            ref, b = ref[rows], (b[rows] if np.ndim(b) else b)
        return float(np.max(PH.err(got, ref) / (b * (self.scale if markov else 1.0))))


def reference(case):
    """The Reference of a case (cached)."""
    cid, kernel, data, delays, alpha, rho, mb, N = case
    if (cid, kernel) in _cache:
        return _cache[(cid, kernel)]
    t, y, s = data
    L, R = len(t), len(rho)
    models = [PH.model(kernel, t, y, s, delays[m_], alpha[m_], rho[m_], _empty_tests(L), mb) for m_ in range(R)]
    ext = [row_values(m) for m in models]
    f64 = [row_values(m, np.float64, BLOCKED_NB) for m in models]
    band = models[0].band
    tflat = np.concatenate([np.asarray(a, np.float64) for a in t])
    pts = _brute_points(tflat - delays[0][band])
    full = [brute_row(m, np.arange(N)) for m in models]      # every point: the two sums need them all
    bru = [tuple(v[pts] for v in f) for f in full]

    def stack(rows, k):
        return np.stack([r_[k] for r_ in rows])

    ref = Reference(bar={}, e_formula={}, e_brute={}, pts=pts, scale=MC.factor(alpha, s) / FACTOR)
    ref.mu, ref.var, ref.lp = stack(ext, 0), stack(ext, 1), stack(ext, 2)
    ref.loo = ref.lp.sum(axis=1)
    ref.mix_lp = mix_values(ref.lp, WEIGHTS)
    ref.mix_loo = ref.mix_lp.sum()
    tmu, tlp = stack(ext, 3), stack(ext, 4)
    terms = {"mu": tmu, "var": ref.var.astype(np.float64), "lp": tlp, "loo": tlp.sum(axis=1), "mix_lp": tlp.max(axis=0),
             "mix_loo": float(tlp.max(axis=0).sum())}
    fm, fv, fl = stack(f64, 0), stack(f64, 1), stack(f64, 2)
    fmix = mix_values(fl, WEIGHTS)
    formula = {"mu": fm, "var": fv, "lp": fl, "loo": fl.sum(axis=1), "mix_lp": fmix, "mix_loo": fmix.sum()}
    bm, bv, bl = stack(bru, 0), stack(bru, 1), stack(bru, 2)
    bmix = mix_values(bl, WEIGHTS)
    bl_all = stack(full, 2)
    bmix_all = mix_values(bl_all, WEIGHTS)
    e_brute = {"mu": np.max(PH.err(bm, ref.mu[:, pts])), "var": np.max(PH.err(bv, ref.var[:, pts])),
               "lp": np.max(PH.err(bl, ref.lp[:, pts])),
               "loo": np.max(PH.err(bl_all.sum(axis=1), ref.loo)),
               "mix_lp": np.max(PH.err(bmix, ref.mix_lp[pts])),
               "mix_loo": float(PH.err(bmix_all.sum(), ref.mix_loo))}
    for q in QUANTITIES:
        ref.e_formula[q] = float(np.max(PH.err(formula[q], getattr(ref, q))))
        ref.e_brute[q] = float(e_brute[q])
        ref.bar[q] = FACTOR * np.maximum(max(ref.e_formula[q], ref.e_brute[q]), N * U53 * np.asarray(terms[q], np.float64))
    _cache[(cid, kernel)] = ref
    return ref


def mpmath_row(kernel, data, delays, alpha, rho, mb, digits=40):
    """(mu, var, lp) of one row by the definition in mpmath at `digits` digits: K from the fp64 inputs, inverted by mpmath."""
    import mpmath as mp
    mp.mp.dps = digits
    t, y, s = data
    band = PH._bands(t)
    tt = [mp.mpf(float(v)) for a in t for v in np.asarray(a, np.float64)]
    yy = [mp.mpf(float(v)) for a in y for v in np.asarray(a, np.float64)]
    ss = [mp.mpf(float(v)) for a in s for v in np.asarray(a, np.float64)]
    N, L = len(tt), len(t)
    off = np.concatenate([[0], np.cumsum([len(a) for a in t])])
    mean = [sum(yy[off[l]:off[l + 1]]) / (off[l + 1] - off[l]) for l in range(L)]
    sigb = [100 * sum((v - mean[l]) ** 2 for v in yy[off[l]:off[l + 1]]) / (off[l + 1] - off[l] - 1) if mb else mp.mpf(0) for l in range(L)]
    rho_, al, tau = mp.mpf(float(rho)), [mp.mpf(float(a)) for a in alpha], [mp.mpf(float(d)) for d in delays]

    def k(d):
        a = abs(d)
        if kernel == "OU":
            return mp.exp(-a / rho_)
        if kernel == "rbf":
            return mp.exp(-d * d / (4 * rho_))
        c = (mp.sqrt(3) if kernel == "matern32" else mp.sqrt(5)) * a / rho_
        return (1 + c) * mp.exp(-c) if kernel == "matern32" else (1 + c + c * c / 3) * mp.exp(-c)

    K = mp.matrix(N, N)
    for i in range(N):
        for j in range(N):
            K[i, j] = al[band[i]] * al[band[j]] * k((tt[i] - tau[band[i]]) - (tt[j] - tau[band[j]]))
            if band[i] == band[j]:
                K[i, j] += sigb[band[i]]
        K[i, i] += ss[i] ** 2
    G = K ** -1
    r = mp.matrix([yy[i] - mean[band[i]] for i in range(N)])
    w = G * r
    var = [1 / G[i, i] for i in range(N)]
    mu = [yy[i] - w[i] / G[i, i] for i in range(N)]
    lp = [-(mp.log(2 * mp.pi) + mp.log(var[i]) + (yy[i] - mu[i]) ** 2 / var[i]) / 2 for i in range(N)]
    return mu, var, lp


class Worst:
    """The worst error / bar of a group."""

    def __init__(self, group):
        self.group, self.worst, self.where = group, 0.0, None

    def add(self, r, where):
        if r >= self.worst:
            self.worst, self.where = r, where

    def line(self):
        return "%s: worst error / bar %.3g (%s)" % (self.group, self.worst, self.where)
