"""The exact linear-time log-likelihood of the Markov kernels (OU, Matern-3/2, Matern-5/2), in numpy on the CPU: the restatement of
csrc/gpcc_markov.hip.h (gpcc_loglik_markov_batch) that the tests compare it with and that the `engine="python"` fit uses.  It is NOT
a fallback of Objective: without a GPU Objective raises.

The model is objective(alpha, rho) of the reference: y_l(t) = alpha_l f(t - tau_l) + b_l + noise.  f with one of these kernels is a
stationary Gauss-Markov process of state dimension p = 1, 2, 3 (x = (f, f', f'')), so once all observations are merged in the order
of their shifted times s = t - tau_band the covariance K = alpha alpha' k(s - s') + Sobs (+ B) is that of a linear-Gaussian
state-space model, and logpdf(MvNormal(bbar, K), Y) is the sum of the Kalman filter's one-step predictive log-densities: O(N p^2)
work, O(1) memory, nothing approximated.

  merge   points ordered by s; ties by band index, then by position in the band (each band sorted by time first, stably)
  state   (f, f', ...) and, when b is marginalised, the L offsets as constant states with prior variance 100 var(y_l) (n - 1);
          residual r = y - mean(y_band) either way
  step    e = exp(-lambda d), d = s_i - s_prev >= 0, lambda = 1/rho, sqrt3/rho, sqrt5/rho:
          m <- A m,  P_xx <- A (P_xx - Pinf) A' + Pinf  (= A P_xx A' + Q, Q = Pinf - A Pinf A'),  P_xb <- A P_xb
  update  h = alpha_band e_1 (+ e_{p + band}), S = h'Ph + sigma_i^2, eps = r_i - h'm:
          loglik -= (log(2 pi S) + eps^2 / S) / 2,  m += P h eps / S,  P -= P h h' P / S
  S not finite or <= 0 at merged position j (1-based): info = j, loglik = NaN."""
import math

import numpy as np

KERNELS = ("OU", "matern32", "matern52")
MAX_OFFSET_BANDS = 4          # csrc/gpcc_markov.hip.h: the offset states a lane keeps in registers
_ORDER = {"OU": 1, "matern32": 2, "matern52": 3}
_SCALE = {"OU": 1.0, "matern32": math.sqrt(3.0), "matern52": math.sqrt(5.0)}
LOG2PI = math.log(2.0 * math.pi)


def _name(kernel):
    name = getattr(kernel, "name", kernel)
    if name not in _ORDER:
        raise ValueError("kernel %r is not Markov: the linear-time solver takes OU, matern32 and matern52" % (name,))
    return name


def order(kernel):
    """State dimension p of the kernel's process."""
    return _ORDER[_name(kernel)]


def rate(kernel, rho):
    """lambda: 1/rho (OU), sqrt3/rho (Matern-3/2), sqrt5/rho (Matern-5/2)."""
    return _SCALE[_name(kernel)] / rho


def stationary(kernel, rho):
    """Pinf, the stationary covariance of (f, f', ...): its (1, 1) entry is k(0) = 1."""
    name = _name(kernel)
    lam = rate(name, rho)
    if name == "OU":
        return np.array([[1.0]])
    if name == "matern32":
        return np.array([[1.0, 0.0], [0.0, lam * lam]])
    kap = lam * lam / 3.0
    return np.array([[1.0, 0.0, -kap], [0.0, kap, 0.0], [-kap, 0.0, lam ** 4]])


def transition(kernel, d, rho):
    """A(d) = expm(F d), the state transition over a lag d."""
    name = _name(kernel)
    lam = rate(name, rho)
    e = math.exp(-lam * d)
    x = lam * d
    if name == "OU":
        return np.array([[e]])
    if name == "matern32":
        return e * np.array([[1.0 + x, d], [-lam * lam * d, 1.0 - x]])
    l2 = lam * lam
    return e * np.array([[1.0 + x + 0.5 * x * x, d * (1.0 + x), 0.5 * d * d],
                         [-0.5 * l2 * lam * d * d, 1.0 + x - x * x, d * (1.0 - 0.5 * x)],
                         [l2 * x * (0.5 * x - 1.0), lam * x * (x - 3.0), 1.0 - 2.0 * x + 0.5 * x * x]])


def prepare(tarray, yarray, stdarray, marginalise_b=True):
    """What the handle keeps: per band the times sorted (stably), the residuals y - mean(y_l) and sigma^2 in that order, and the
    offsets' prior variances 100 var(y_l) (n - 1; zeros when b is not marginalised)."""
    ts, rs, s2, vb = [], [], [], []
    for t, y, sd in zip(tarray, yarray, stdarray):
        t, y, sd = (np.asarray(a, np.float64) for a in (t, y, sd))
        perm = np.argsort(t, kind="stable")
        mean = y.sum() / len(y)
        ts.append(t[perm])
        rs.append((y - mean)[perm])
        s2.append((sd * sd)[perm])
        vb.append(100.0 * (np.sum((y - mean) ** 2) / (len(y) - 1)) if marginalise_b else 0.0)
    return ts, rs, s2, np.array(vb)


def merge_order(ts, delays):
    """The merged order as (band, position) pairs: an L-way merge of the sorted bands by s = t - tau, the lowest band first on ties."""
    L = len(ts)
    cur = [0] * L
    out = []
    for _ in range(sum(len(t) for t in ts)):
        best, bs = -1, 0.0
        for l in range(L):
            if cur[l] < len(ts[l]):
                s = ts[l][cur[l]] - delays[l]
                if best < 0 or s < bs:
                    best, bs = l, s
        out.append((best, cur[best]))
        cur[best] += 1
    return out


def loglik(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True, _slip=None):
    """(loglik, info) of one (tau, alpha, rho): the filter of the module's docstring.  info: 0, -1 (some alpha <= 0), -2 (rho <= 0), or
    the merged position of the first predictive variance that is not positive and finite -- the codes of Objective.loglik_batch.
    _slip (tests only) injects one mistake an implementation can make: "order" (two neighbours of the merged order swapped where
    their shifted times differ: one negative lag), "no_q" (P <- A P A' without the process noise), "var_n" (offset prior 100 var with n
    instead of n - 1), "no_offset" (h without the offset entry)."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b,
                                                                       codes_first=True)
    if code:
        return math.nan, code
    if _slip == "var_n":
        vb = vb * np.array([(len(t) - 1.0) / len(t) for t in tarray])
    ll, info, _, _, _, _ = _pass(name, train, [], alpha, rho, p, n, vb, slip=_slip)
    return ll, info


def loglik_batch(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True):
    """loglik over M rows (delays and alpha M x L, rho M) -> (loglik[M], info[M]): Objective.loglik_markov_batch's shape."""
    L = len(tarray)
    delays = np.asarray(delays, np.float64).reshape(-1, L)
    alpha = np.asarray(alpha, np.float64).reshape(-1, L)
    rho = np.asarray(rho, np.float64).reshape(-1)
    out = [loglik(kernel, tarray, yarray, stdarray, delays[i], alpha[i], rho[i], marginalise_b) for i in range(len(rho))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32)


# ----------------------------------------------------------------------------------------------------------------------------------
# Many flux realisations per parameter row (csrc/gpcc_markov_multi.hip.h, gpcc_loglik_markov_multi_batch), the same
# algorithm in numpy.  In the filter of the module's docstring nothing but m, eps, eps^2 / S and m += P h eps / S reads a flux: the
# merged order, A, P, S, log S and the gain depend on (tau, alpha, rho), the times and the error bars alone.  Per parameter row they are
# computed once and R means (the columns of m) are driven through them.  The model is that of the data set the "handle" holds
# (tarray, yarray, stdarray): with marginalise_b the offsets' prior variances are 100 var(yarray_l), NOT 100 var(Y_r).
# ----------------------------------------------------------------------------------------------------------------------------------
def _bands(tarray, Y):
    """Y (a list of L arrays (R, N_l), or one (R, N) array in the bands' order) as a list of L arrays (R, N_l)."""
    L = len(tarray)
    Nl = [len(t) for t in tarray]
    if not isinstance(Y, (list, tuple)):
        Y = np.atleast_2d(np.asarray(Y, np.float64))
        edges = np.concatenate([[0], np.cumsum(Nl)])
        if Y.shape[1] != edges[-1]:
            raise ValueError("Y must be (R, N) = (R, %d)" % edges[-1])
        Y = [Y[:, edges[l]:edges[l + 1]] for l in range(L)]
    Y = [np.atleast_2d(np.asarray(a, np.float64)) for a in Y]
    R = Y[0].shape[0]
    if len(Y) != L or any(a.shape != (R, n) for a, n in zip(Y, Nl)):
        raise ValueError("Y must hold L arrays (R, N_l)")
    return Y


def band_means(tarray, Y):
    """(R, L): each realisation's own band means."""
    return np.stack([a.sum(axis=1) / a.shape[1] for a in _bands(tarray, Y)], axis=1)


def realisation_residuals(tarray, Y, mean):
    """Per band the residuals (R, N_l) of the realisations Y about mean (R, L), in the band's time-sorted order (prepare()'s); a
    residual that is not finite becomes NaN."""
    Y = _bands(tarray, Y)
    mean = np.asarray(mean, np.float64).reshape(Y[0].shape[0], len(Y))
    out = []
    for l in range(len(Y)):
        perm = np.argsort(np.asarray(tarray[l], np.float64), kind="stable")
        r = (Y[l] - mean[:, l:l + 1])[:, perm]
        out.append(np.where(np.isfinite(r), r, np.nan))
    return out


def _multi_pass(name, train, res, alpha, rho, p, n, vb):
    """_pass over the training points alone with R means at once: train is _setup's, res[band][:, position] the realisations'
    residuals.  -> (loglik[R], info); the flux-independent quantities of a step are computed once."""
    ev = sorted(train, key=lambda e: e[:3])       # shifted time, then band, then position in the band: merge_order()'s order
    R = res[0].shape[0]
    Pinf = stationary(name, rho)
    P = _prior(name, rho, p, n, vb)
    m = np.zeros((n, R))
    ll = np.zeros(R)
    sprev = None
    for step, (s, b, i, _, s2) in enumerate(ev, 1):
        d = 0.0 if sprev is None else s - sprev
        sprev = s
        m, P = _propagate(name, m, P, Pinf, d, rho, p)
        h = np.zeros(n)
        h[0] = alpha[b]
        if n > p:
            h[p + b] = 1.0
        Ph = P @ h
        S = h @ Ph + s2
        if not (S > 0.0 and math.isfinite(S)):
            return np.full(R, math.nan), step
        eps = res[b][:, i] - h @ m
        ll -= 0.5 * (LOG2PI + math.log(S) + eps * eps / S)
        m = m + np.outer(Ph, eps / S)
        P = P - np.outer(Ph, Ph) / S
        P = 0.5 * (P + P.T)
    return ll, 0


def loglik_realisations(kernel, tarray, yarray, stdarray, Y, delays, alpha, rho, marginalise_b=True, mean=None):
    """(loglik[M, R], info[M]) of R flux realisations Y on the cadence and under the model of (tarray, yarray, stdarray):
    Objective.loglik_markov_realisations' result.  loglik[m, r] = logpdf(MvNormal(Q mean_r, K_m), Y_r) with K_m built from the times,
    stdarray, the kernel and -- with marginalise_b -- the prior variances 100 var(yarray_l).  Y: a list of L arrays (R, N_l) or one
    (R, N) array; delays and alpha (M, L) or (L,), rho (M,) or a scalar.  mean: (R, L), the offset subtracted per realisation and band;
    None: the band means of yarray (the handle's) for every realisation.  info: loglik()'s codes, of the row; such a row is NaN
    throughout.  A flux that is not finite makes its own column NaN."""
    L = len(tarray)
    delays = np.asarray(delays, np.float64).reshape(-1, L)
    alpha = np.asarray(alpha, np.float64).reshape(-1, L)
    rho = np.asarray(rho, np.float64).reshape(-1)
    res = None
    out, infos = [], []
    for g in range(len(rho)):
        name, _, dg, ag, rg, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays[g], alpha[g], rho[g],
                                                                   marginalise_b, codes_first=True)
        if res is None:
            Y = _bands(tarray, Y)
            res = realisation_residuals(tarray, Y, np.tile(means, (Y[0].shape[0], 1)) if mean is None else mean)
        if code:
            ll, info = np.full(res[0].shape[0], math.nan), code
        else:
            ll, info = _multi_pass(name, train, res, ag, rg, p, n, vb)
        out.append(ll)
        infos.append(info)
    return np.array(out), np.array(infos, dtype=np.int32)


# ----------------------------------------------------------------------------------------------------------------------------------
# Rows with their own resampled data set (csrc/gpcc_markov_resample.hip.h, gpcc_loglik_markov_resampled_batch), the
# same algorithm in numpy.  A realisation is a flux vector on the cadence of (tarray, stdarray) and a multiplicity per point: a point
# with count 0 is dropped, a point drawn n times is the point once with variance sigma^2 / n.  Row m has its own (tau, alpha, rho) and
# the index real[m] of its realisation; its value is that of the reduced data set (the kept points, sigma / sqrt n).
# ----------------------------------------------------------------------------------------------------------------------------------
def _counts(tarray, counts, R):
    """counts (None: all 1; a list of L arrays (R, N_l) or one (R, N) array) as a list of L integer arrays (R, N_l); negative: ValueError."""
    if counts is None:
        return [np.ones((R, len(t)), dtype=np.int64) for t in tarray]
    c = [np.asarray(a) for a in _bands(tarray, counts)]
    if c[0].shape[0] != R:
        raise ValueError("counts must hold as many realisations as Y (%d)" % R)
    if any((a < 0).any() or (a != np.floor(a)).any() for a in c):
        raise ValueError("counts must be integers >= 0")
    return [a.astype(np.int64) for a in c]


def resample_constants(tarray, Y, counts=None, marginalise_b=True):
    """(mean[R, L], sigma_b[R, L]) of R resampled data sets as prepare() computes them for each reduced data set: the band means and
    100 var (n - 1) over a band's distinct kept points (count >= 1), unweighted; sigma_b is zeros without marginalise_b.  A band
    that keeps no point has mean 0 (it subtracts from nothing).  ValueError: marginalise_b and a band with fewer than 2 kept points."""
    Y = _bands(tarray, Y)
    R, L = Y[0].shape[0], len(Y)
    counts = _counts(tarray, counts, R)
    mean, vb = np.zeros((R, L)), np.zeros((R, L))
    for r in range(R):
        for l in range(L):
            y = Y[l][r][counts[l][r] > 0]
            if marginalise_b and len(y) < 2:
                raise ValueError("realisation %d keeps %d distinct points of band %d: marginalise_b needs at least 2 for the offset's "
                                 "prior variance" % (r, len(y), l + 1))
            if len(y):
                mean[r, l] = y.sum() / len(y)
            if marginalise_b:
                vb[r, l] = 100.0 * (np.sum((y - mean[r, l]) ** 2) / (len(y) - 1))
    return mean, vb


def resample_arguments(tarray, Y, counts, center, sigma_b, marginalise_b):
    """center and sigma_b of loglik_markov_resampled ("own", "handle" or an (R, L) array each) as (mean, sigma_b): an (R, L) array, or
    None for the handle's.  "own": resample_constants' (its ValueError for a band with fewer than 2 kept points under marginalise_b
    is raised only where sigma_b is "own")."""
    R = _bands(tarray, Y)[0].shape[0]
    L = len(tarray)
    for name, v in (("center", center), ("sigma_b", sigma_b)):
        if isinstance(v, str) and v not in ("own", "handle"):
            raise ValueError('%s must be "own", "handle" or an (R, L) array' % name)
    own = None
    if (isinstance(center, str) and center == "own") or (isinstance(sigma_b, str) and sigma_b == "own"):
        own = resample_constants(tarray, Y, counts, marginalise_b and isinstance(sigma_b, str) and sigma_b == "own")
    out = []
    for k, v in enumerate((center, sigma_b)):
        if isinstance(v, str):
            out.append(own[k] if v == "own" else None)
        else:
            a = np.ascontiguousarray(v, dtype=np.float64)
            if a.shape != (R, L):
                raise ValueError("%s must be (R, L) = (%d, %d)" % (("center", "sigma_b")[k], R, L))
            out.append(a)
    return out[0], out[1]


def loglik_resampled(kernel, tarray, yarray, stdarray, Y, counts, real, delays, alpha, rho, marginalise_b=True, mean=None, sigma_b=None):
    """(loglik[M], info[M]) of M rows (delays and alpha (M, L), rho (M)), row m scored on realisation real[m] of the R resampled data
    sets (Y, counts) on the cadence of (tarray, stdarray): Objective.loglik_markov_resampled's result with mean and sigma_b given.
    loglik[m] = logpdf(MvNormal(Q mean_r, K), Y_r[sel]), sel the points of r = real[m] with count >= 1, K from (tau, alpha, rho)_m on
    t[sel] with variances sigma^2[sel] / count and, with marginalise_b, B from sigma_b[r].  Y: a list of L arrays (R, N_l) or one (R, N)
    array; counts the same in integers, or None (all 1).  mean, sigma_b: (R, L); None: those of (tarray, yarray, stdarray), the
    handle's.  A realisation that keeps no point gives (0.0, 0).  info: loglik()'s codes, the position counted among the kept points.
    A flux that is not finite at a kept point makes the row NaN.  ValueError: a real[m] outside [0, R), negative counts."""
    name, L, delays, alpha, rho, real, vb, _, p, n, points = _resampled_setup(kernel, tarray, yarray, stdarray, Y, counts, real, delays,
                                                                              alpha, rho, marginalise_b, mean, sigma_b)
    ll, info = np.empty(len(rho)), np.zeros(len(rho), dtype=np.int32)
    for m in range(len(rho)):
        code = -1 if not np.all(alpha[m] > 0.0) else (-2 if rho[m] <= 0.0 else 0)
        if code:
            ll[m], info[m] = math.nan, code
            continue
        r = int(real[m])
        train = [(t - delays[m, l], l, i, res, s2) for (l, i, t, res, s2) in points(r)]
        ll[m], info[m] = _pass(name, train, [], alpha[m], float(rho[m]), p, n, vb[r])[:2]
    return ll, info


def _resampled_setup(kernel, tarray, yarray, stdarray, Y, counts, real, delays, alpha, rho, marginalise_b, mean, sigma_b):
    """The arguments of loglik_resampled and loglik_grad_resampled as arrays and what both walk: (name, L, delays[M, L], alpha[M, L],
    rho[M], real[M], vb[R, L], the handle's vb[L], p, n, points), points(r) the kept points of realisation r as [(band, position in the
    sorted band, time, residual, variance)] (cached).  Their ValueErrors."""
    name = _name(kernel)
    L = len(tarray)
    Y = _bands(tarray, Y)
    R = Y[0].shape[0]
    counts = _counts(tarray, counts, R)
    delays = np.asarray(delays, np.float64).reshape(-1, L)
    alpha = np.asarray(alpha, np.float64).reshape(-1, L)
    rho = np.asarray(rho, np.float64).reshape(-1)
    real = np.asarray(real).reshape(-1)
    if len(real) != len(rho) or (len(real) and (real.min() < 0 or real.max() >= R)):
        raise ValueError("real must hold one realisation in [0, %d) per row" % R)
    if marginalise_b and L > MAX_OFFSET_BANDS:
        raise ValueError("marginalise_b with %d bands: the linear-time solver keeps at most %d offset states" % (L, MAX_OFFSET_BANDS))
    _, _, _, hvb = prepare(tarray, yarray, stdarray, marginalise_b)
    hmean = np.array([np.asarray(y, np.float64).sum() / len(y) for y in yarray])
    mean = np.tile(hmean, (R, 1)) if mean is None else np.asarray(mean, np.float64).reshape(R, L)
    vb = np.tile(hvb, (R, 1)) if sigma_b is None else np.asarray(sigma_b, np.float64).reshape(R, L)
    if not marginalise_b:
        vb = np.zeros((R, L))
    p = _ORDER[name]
    n = p + (L if marginalise_b else 0)
    kept = {}

    def points(r):
        if r not in kept:
            out = []
            for l in range(L):
                t, sd = np.asarray(tarray[l], np.float64), np.asarray(stdarray[l], np.float64)
                perm = np.argsort(t, kind="stable")
                res = (Y[l][r] - mean[r, l])[perm]
                res = np.where(np.isfinite(res), res, np.nan)
                cnt, s2 = counts[l][r][perm], (sd * sd)[perm]
                out += [(l, i, t[perm][i], res[i], s2[i] / cnt[i]) for i in range(len(t)) if cnt[i] > 0]
            kept[r] = out
        return kept[r]

    return name, L, delays, alpha, rho, real, vb, hvb, p, n, points


# ----------------------------------------------------------------------------------------------------------------------------------
# The gradient in linear time (csrc/gpcc_markov_grad.hip.h), the same algorithm in numpy: the filter's forward
# sensitivities.  For one parameter theta the tangents (dm, dP) = d(m, P)/d theta are carried beside (m, P):
#
#   alpha_l   enters through h only: dh = e_1 on the observations of band l
#   rho       through lambda (d lambda / d rho = -lambda / rho): dA = dA/drho, dPinf = dPinf/drho, the prior's dP_xx = dPinf
#   tau_l     through the lags only: with the merged order fixed d_i = s_i - s_(i-1), d d_i / d tau_l = -[band_i = l] + [band_(i-1) = l]
#             (0 at the first point), and dA/dd = F A, F = companion()
#   step      dm <- dA m + A dm,  dP_xx <- dA D A' + A dD A' + A D dA' + dPinf  (D = P_xx - Pinf, dD = dP_xx - dPinf),
#             dP_xb <- dA P_xb + A dP_xb
#   update    Ph = P h, dPh = dP h + P dh, dS = 2 dh'Ph + h'dP h, deps = -dh'm - h'dm:
#             dloglik -= (dS / S + 2 eps deps / S - eps^2 dS / S^2) / 2,  then the tangents of m += Ph eps / S and P -= Ph Ph' / S
#
# Ties in shifted time: the merged order is piecewise constant in tau, so this is a one-sided derivative at an exact tie of two bands.
# The Matern kernels are C^1 there.  OU has a kink, and the dense gradient takes dk/ds(0) = 0, the mean of the one-sided derivatives;
# the trace formula is linear in dK, so that mean is (tangent with band l first among tied points + tangent with band l last) / 2,
# the other bands keeping the lowest-band-first rule: OU runs two passes per tau_l.  _grad_pass is the tangent-carrying sibling of
# _pass over the training points; value and info are loglik()'s.
# ----------------------------------------------------------------------------------------------------------------------------------
def companion(kernel, rho):
    """F, the companion matrix of (lambda + d/dt)^p: A(d) = expm(F d), dA/dd = F A."""
    name = _name(kernel)
    lam = rate(name, rho)
    if name == "OU":
        return np.array([[-lam]])
    if name == "matern32":
        return np.array([[0.0, 1.0], [-lam * lam, -2.0 * lam]])
    return np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-lam ** 3, -3.0 * lam * lam, -3.0 * lam]])


def transition_drho(kernel, d, rho):
    """dA(d)/drho = (dA/dlambda) (-lambda / rho), in closed form per kernel."""
    name = _name(kernel)
    lam = rate(name, rho)
    x = lam * d
    e = math.exp(-x) * (-lam / rho)
    if name == "OU":
        return np.array([[-e * d]])
    if name == "matern32":
        return e * np.array([[-d * x, -d * d], [x * (x - 2.0), d * (x - 2.0)]])
    q = 3.0 * x - 3.0 - 0.5 * x * x
    return e * np.array([[-0.5 * d * x * x, -d * d * x, -0.5 * d ** 3],
                         [0.5 * x * x * (x - 3.0), d * x * (x - 3.0), 0.5 * d * d * (x - 3.0)],
                         [lam * x * q, x * (6.0 * x - 6.0 - x * x), d * q]])


def stationary_drho(kernel, rho):
    """dPinf/drho: Matern-3/2 dPinf_22/dlambda = 2 lambda; Matern-5/2 dkappa/dlambda = 2 lambda / 3, d lambda^4 / dlambda = 4 lambda^3."""
    name = _name(kernel)
    lam = rate(name, rho)
    dl = -lam / rho
    if name == "OU":
        return np.array([[0.0]])
    if name == "matern32":
        return np.array([[0.0, 0.0], [0.0, 2.0 * lam * dl]])
    dk = 2.0 * lam / 3.0 * dl
    return np.array([[0.0, 0.0, -dk], [0.0, dk, 0.0], [-dk, 0.0, 4.0 * lam ** 3 * dl]])


def _grad_pass(name, train, alpha, rho, p, n, vb, kind, band=-1, rank=None, slip=None, prev_band=None):
    """d loglik / d theta by the tangent recursion over the training observations.  kind: "alpha" (of band `band`), "rho", "tau" (of
    band `band`).  rank: the rank of `band` among points that tie in shifted time (-1: first, L: last; None: its index, merge_order()'s
    rule).  slip: loglik_grad()'s.  prev_band (loglik_grad_resampled's slip "lag_from_merged" only): {(band, position): the band the
    tau tangent takes for the observation before}, in place of the band of the observation before."""
    ev = sorted(train, key=lambda e: (e[0], rank if (rank is not None and e[1] == band) else e[1], e[2]))
    Pinf = stationary(name, rho)
    dPinf = stationary_drho(name, rho) if (kind == "rho" and slip != "no_dpinf") else np.zeros((p, p))
    F = companion(name, rho)
    P = _prior(name, rho, p, n, vb)
    dP = np.zeros((n, n))
    dP[:p, :p] = dPinf
    m, dm = np.zeros(n), np.zeros(n)
    dll, sprev, bprev = 0.0, None, -1
    for (s, b, i, r, s2) in ev:
        d = 0.0 if sprev is None else s - sprev
        A = transition(name, d, rho)
        if kind == "rho":
            dA = transition_drho(name, d, rho)
        elif kind == "tau" and sprev is not None:
            if prev_band is not None:
                bprev = prev_band[(b, i)]
            dd = -float(b == band) + (0.0 if slip == "tau_one_lag" else float(bprev == band))
            dA = dd * (F @ A)
        else:
            dA = np.zeros((p, p))
        sprev, bprev = s, b
        D, dD = P[:p, :p] - Pinf, dP[:p, :p] - dPinf
        dm[:p] = dA @ m[:p] + A @ dm[:p]
        dP[:p, :p] = dA @ D @ A.T + A @ dD @ A.T + A @ D @ dA.T + dPinf
        dP[:p, p:] = dA @ P[:p, p:] + A @ dP[:p, p:]
        dP[p:, :p] = dP[:p, p:].T
        m[:p] = A @ m[:p]
        P[:p, :p] = A @ D @ A.T + Pinf
        P[:p, p:] = A @ P[:p, p:]
        P[p:, :p] = P[:p, p:].T
        h, dh = np.zeros(n), np.zeros(n)
        h[0] = alpha[b]
        if n > p:
            h[p + b] = 1.0
        if kind == "alpha" and b == band and slip != "no_dh":
            dh[0] = 1.0
        Ph = P @ h
        dPh = dP @ h + P @ dh
        S = h @ Ph + s2
        if not (S > 0.0 and math.isfinite(S)):
            return math.nan
        dS = dh @ Ph + h @ dPh
        eps = r - h @ m
        deps = -(dh @ m) - h @ dm
        g = eps / S
        dg = (deps - g * dS) / S
        dll -= 0.5 * (dS / S + 2.0 * g * deps - g * g * dS)
        dm = dm + dPh * g + Ph * dg
        m = m + Ph * g
        dP = dP - (np.outer(dPh, Ph) + np.outer(Ph, dPh)) / S + np.outer(Ph, Ph) * (dS / (S * S))
        P = P - np.outer(Ph, Ph) / S
        P = 0.5 * (P + P.T)
        dP = 0.5 * (dP + dP.T)
    return dll


def loglik_grad(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True, _slip=None):
    """(loglik, grad[2L+1], info) of one (tau, alpha, rho): loglik() and its gradient [d/dalpha_1..alpha_L, d/drho, d/dtau_1..tau_L] by
    the filter's forward sensitivities, Objective.loglik_grad_markov_batch's row.  grad is NaN where info != 0.
    _slip (tests only) injects one mistake: "one_sided" (OU without the mean of the two tie orders), "no_dpinf" (dPinf left out of the
    prior and the step), "tau_one_lag" (only the lag before a point of band l is differentiated, not the one after), "no_dh" (the
    dh terms left out)."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b,
                                                                       codes_first=True)
    nan = np.full(2 * L + 1, math.nan)
    if code:
        return math.nan, nan, code
    ll, info, _, _, _, _ = _pass(name, train, [], alpha, rho, p, n, vb)
    if info:
        return math.nan, nan, info
    grad = np.empty(2 * L + 1)
    for l in range(L):
        grad[l] = _grad_pass(name, train, alpha, rho, p, n, vb, "alpha", l, slip=_slip)
    grad[L] = _grad_pass(name, train, alpha, rho, p, n, vb, "rho", slip=_slip)
    for l in range(L):
        if name == "OU" and _slip != "one_sided":
            first = _grad_pass(name, train, alpha, rho, p, n, vb, "tau", l, rank=-1, slip=_slip)
            last = _grad_pass(name, train, alpha, rho, p, n, vb, "tau", l, rank=L, slip=_slip)
            grad[L + 1 + l] = 0.5 * (first + last)
        else:
            grad[L + 1 + l] = _grad_pass(name, train, alpha, rho, p, n, vb, "tau", l, slip=_slip)
    return ll, grad, 0


def loglik_grad_batch(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True):
    """loglik_grad over M rows -> (loglik[M], grad[M, 2L+1], info[M]): Objective.loglik_grad_markov_batch's shape."""
    L = len(tarray)
    delays = np.asarray(delays, np.float64).reshape(-1, L)
    alpha = np.asarray(alpha, np.float64).reshape(-1, L)
    rho = np.asarray(rho, np.float64).reshape(-1)
    out = [loglik_grad(kernel, tarray, yarray, stdarray, delays[i], alpha[i], rho[i], marginalise_b) for i in range(len(rho))]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]).reshape(-1, 2 * L + 1),
            np.array([o[2] for o in out], dtype=np.int32))


# ----------------------------------------------------------------------------------------------------------------------------------
# The gradient of rows with their own resampled data set (csrc/gpcc_markov_resample_grad.hip.h, gpcc_loglik_grad_markov_resampled_batch,
# DESIGN.md 4.28), the same algorithm in numpy: _grad_pass over the kept points of the row's realisation.  Dropping a point removes its
# step, so the lag of a kept point and the lag's tangent by tau_l, [band of the last KEPT point = l] - [band = l], are those of the
# reduced data set; a dropped point that ties with a kept one in shifted time is not there to tie.  The band means and the offsets'
# prior variances are constants of the data.
# ----------------------------------------------------------------------------------------------------------------------------------
RESAMPLED_GRAD_SLIPS = ("lag_from_merged", "handle_sigma_b", "one_sided")


def loglik_grad_resampled(kernel, tarray, yarray, stdarray, Y, counts, real, delays, alpha, rho, marginalise_b=True, mean=None, sigma_b=None,
                          _slip=None):
    """(loglik[M], grad[M, 2L+1], info[M]) of M rows, row m on realisation real[m]: loglik_resampled's value and info (the same
    arguments, the same ValueErrors) and the gradient [d/dalpha_1..alpha_L, d/drho, d/dtau_1..tau_L] of that value,
    Objective.loglik_grad_markov_resampled's result with mean and sigma_b given.  It is loglik_grad() of the reduced fresh data set when
    mean and sigma_b are that data set's.  grad is NaN where info != 0; a realisation that keeps no point gives (0.0, zeros, 0); at a tie
    in shifted time between two kept points of different bands OU returns the mean of the two tie orders.
    _slip (tests only) injects one mistake: "lag_from_merged" (the tau tangent reads the band of the point before in the handle's merged
    order, dropped points included, not the band of the last kept point), "handle_sigma_b" (the offsets' prior variances of
    (tarray, yarray, stdarray) for every realisation), and loglik_grad()'s "one_sided", "no_dpinf", "tau_one_lag", "no_dh"."""
    name, L, delays, alpha, rho, real, vb, hvb, p, n, points = _resampled_setup(kernel, tarray, yarray, stdarray, Y, counts, real, delays,
                                                                                alpha, rho, marginalise_b, mean, sigma_b)
    M, W = len(rho), 2 * L + 1
    ts = [np.sort(np.asarray(t, np.float64), kind="stable") for t in tarray]
    ll, grad, info = np.empty(M), np.full((M, W), math.nan), np.zeros(M, dtype=np.int32)
    for m in range(M):
        code = -1 if not np.all(alpha[m] > 0.0) else (-2 if rho[m] <= 0.0 else 0)
        if code:
            ll[m], info[m] = math.nan, code
            continue
        r, am, rm = int(real[m]), alpha[m], float(rho[m])
        train = [(t - delays[m, l], l, i, res, s2) for (l, i, t, res, s2) in points(r)]
        v = hvb if (_slip == "handle_sigma_b" and marginalise_b) else vb[r]
        ll[m], info[m] = _pass(name, train, [], am, rm, p, n, vb[r])[:2]
        if info[m]:
            continue

        def tau(l, rank=None):
            prev = None
            if _slip == "lag_from_merged":      # the band before in the merged order of ALL the handle's points, under the same tie rule
                ev = sorted(((ts[b][i] - delays[m, b], rank if (rank is not None and b == l) else b, i, b)
                             for b in range(L) for i in range(len(ts[b]))))
                prev = {(e[3], e[2]): (ev[k - 1][3] if k else -1) for k, e in enumerate(ev)}
            return _grad_pass(name, train, am, rm, p, n, v, "tau", l, rank=rank, slip=_slip, prev_band=prev)

        for l in range(L):
            grad[m, l] = _grad_pass(name, train, am, rm, p, n, v, "alpha", l, slip=_slip)
        grad[m, L] = _grad_pass(name, train, am, rm, p, n, v, "rho", slip=_slip)
        for l in range(L):
            grad[m, L + 1 + l] = 0.5 * (tau(l, -1) + tau(l, L)) if (name == "OU" and _slip != "one_sided") else tau(l)
    return ll, grad, info


# ----------------------------------------------------------------------------------------------------------------------------------
# A noise model per row (csrc/gpcc_markov_noise.hip.h, gpcc_loglik_noise_markov_batch and its gradient), the same
# algorithm in numpy.  Point i of band l is observed with the variance v_i = kappa_l^2 sigma_i^2 + nu_l: kappa >= 0 scales the reported
# error bars, nu >= 0 is an excess variance; kappa = 1, nu = 0 is loglik()'s model.  The band means and the offsets' prior variances
# depend on y only and stay those of (tarray, yarray, stdarray), so the value is loglik()'s on the error bars sqrt(v_i).  Value and the
# alpha, rho, tau entries of the gradient are _pass and _grad_pass on the mapped variances.  A noise parameter of band l moves the
# observation variance alone: dvar = [band_i = l] (2 kappa_l sigma_i^2 or 1) enters dS, and nothing else has a direct term -- no dA, no
# dPinf, no dh, the merged order merge_order()'s (_noise_pass).  Codes: loglik()'s, then -3: a kappa or nu negative or not finite.
# ----------------------------------------------------------------------------------------------------------------------------------
def _noise_setup(L, kappa, nu):
    """kappa and nu as (L,) arrays (None: ones / zeros) and the code -3 (one of them negative or not finite) or 0."""
    kappa = np.ones(L) if kappa is None else np.asarray(kappa, np.float64).reshape(L)
    nu = np.zeros(L) if nu is None else np.asarray(nu, np.float64).reshape(L)
    ok = np.all(np.isfinite(kappa)) and np.all(np.isfinite(nu)) and np.all(kappa >= 0.0) and np.all(nu >= 0.0)
    return kappa, nu, (0 if ok else -3)


def _noise_train(train, kappa, nu, slip=None):
    """_setup's training observations with the mapped variance in place of sigma^2, and the reported sigma^2 as a sixth entry."""
    k2 = kappa * kappa
    ex = nu * k2 if slip == "nu_scaled" else nu
    return [(s, b, i, r, k2[b] * s2 + ex[b], s2) for (s, b, i, r, s2) in train]


def _noise_pass(name, ntrain, alpha, rho, p, n, vb, kind, band, kappa, slip=None):
    """d loglik / d kappa_band (kind "kappa") or d nu_band ("nu") by the tangent recursion over _noise_train's observations: _grad_pass
    without dA, dPinf and dh, plus dvar in dS.  slip: loglik_grad_noise()'s."""
    ev = sorted(ntrain, key=lambda e: e[:3])
    Pinf = stationary(name, rho)
    P = _prior(name, rho, p, n, vb)
    dP = np.zeros((n, n))
    m, dm = np.zeros(n), np.zeros(n)
    dll, sprev = 0.0, None
    for (s, b, _, r, v, s2) in ev:
        d = 0.0 if sprev is None else s - sprev
        sprev = s
        A = transition(name, d, rho)
        D = P[:p, :p] - Pinf
        dm[:p] = A @ dm[:p]
        dP[:p, :p] = A @ dP[:p, :p] @ A.T
        dP[:p, p:] = A @ dP[:p, p:]
        dP[p:, :p] = dP[:p, p:].T
        m[:p] = A @ m[:p]
        P[:p, :p] = A @ D @ A.T + Pinf
        P[:p, p:] = A @ P[:p, p:]
        P[p:, :p] = P[:p, p:].T
        h = np.zeros(n)
        h[0] = alpha[b]
        if n > p:
            h[p + b] = 1.0
        dvar = 0.0
        if b == band or slip == "noise_all_bands":
            dvar = 1.0 if kind == "nu" else (s2 if slip == "kappa_linear" else 2.0 * kappa[band] * s2)
        Ph = P @ h
        dPh = dP @ h
        S = h @ Ph + v
        if not (S > 0.0 and math.isfinite(S)):
            return math.nan
        dS = h @ dPh + dvar
        eps = r - h @ m
        deps = -(h @ dm)
        g = eps / S
        dg = (deps - g * dS) / S
        dll -= 0.5 * (dS / S + 2.0 * g * deps - g * g * dS)
        dm = dm + dPh * g + Ph * dg
        m = m + Ph * g
        dP = dP - (np.outer(dPh, Ph) + np.outer(Ph, dPh)) / S + np.outer(Ph, Ph) * (dS / (S * S))
        P = P - np.outer(Ph, Ph) / S
        P = 0.5 * (P + P.T)
        dP = 0.5 * (dP + dP.T)
    return dll


def loglik_noise(kernel, tarray, yarray, stdarray, delays, alpha, rho, kappa=None, nu=None, marginalise_b=True, _slip=None):
    """(loglik, info) of one (tau, alpha, rho, kappa, nu): loglik() with the variances kappa_l^2 sigma_i^2 + nu_l, a row of
    Objective.loglik_markov_noise_batch.  kappa, nu: (L,) or None (ones / zeros: then the numbers are loglik()'s exactly).  info:
    loglik()'s codes and, after -1 and -2, -3: a kappa or nu negative or not finite.  _slip (tests only): "nu_scaled" (nu multiplied
    by kappa^2)."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b,
                                                                       codes_first=True)
    kappa, nu, ncode = _noise_setup(L, kappa, nu)
    code = code or ncode
    if code:
        return math.nan, code
    ll, info, _, _, _, _ = _pass(name, [e[:5] for e in _noise_train(train, kappa, nu, _slip)], [], alpha, rho, p, n, vb)
    return ll, info


def loglik_grad_noise(kernel, tarray, yarray, stdarray, delays, alpha, rho, kappa=None, nu=None, marginalise_b=True, _slip=None):
    """(loglik, grad[4L+1], info): loglik_noise() and its gradient [d/dalpha_1..L, d/drho, d/dtau_1..L, d/dkappa_1..L, d/dnu_1..L], a row
    of Objective.loglik_grad_markov_noise_batch.  The first 2L+1 entries are loglik_grad()'s on the mapped variances (exactly its
    numbers at kappa = 1, nu = 0).  grad is NaN where info != 0.  _slip (tests only) injects one mistake: "kappa_linear" (dvar/dkappa
    = sigma^2 instead of 2 kappa sigma^2), "noise_all_bands" (dvar on every band, not band l alone), "nu_scaled" (nu multiplied by
    kappa^2 in the variance)."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b,
                                                                       codes_first=True)
    kappa, nu, ncode = _noise_setup(L, kappa, nu)
    code = code or ncode
    nan = np.full(4 * L + 1, math.nan)
    if code:
        return math.nan, nan, code
    ntrain = _noise_train(train, kappa, nu, _slip)
    mapped = [e[:5] for e in ntrain]
    ll, info, _, _, _, _ = _pass(name, mapped, [], alpha, rho, p, n, vb)
    if info:
        return math.nan, nan, info
    grad = np.empty(4 * L + 1)
    for l in range(L):
        grad[l] = _grad_pass(name, mapped, alpha, rho, p, n, vb, "alpha", l)
    grad[L] = _grad_pass(name, mapped, alpha, rho, p, n, vb, "rho")
    for l in range(L):
        if name == "OU":
            first = _grad_pass(name, mapped, alpha, rho, p, n, vb, "tau", l, rank=-1)
            last = _grad_pass(name, mapped, alpha, rho, p, n, vb, "tau", l, rank=L)
            grad[L + 1 + l] = 0.5 * (first + last)
        else:
            grad[L + 1 + l] = _grad_pass(name, mapped, alpha, rho, p, n, vb, "tau", l)
    for l in range(L):
        grad[2 * L + 1 + l] = _noise_pass(name, ntrain, alpha, rho, p, n, vb, "kappa", l, kappa, slip=_slip)
        grad[3 * L + 1 + l] = _noise_pass(name, ntrain, alpha, rho, p, n, vb, "nu", l, kappa, slip=_slip)
    return ll, grad, 0


def _noise_rows(L, M, x):
    """kappa or nu of M rows: (M, L), (L,) broadcast, or None for every row."""
    if x is None:
        return [None] * M
    x = np.asarray(x, np.float64)
    if x.shape == (L,):
        x = np.broadcast_to(x, (M, L))
    if x.shape != (M, L):
        raise ValueError("kappa and nu must be (M, L) = (%d, %d), (L,) or None" % (M, L))
    return x


def loglik_noise_batch(kernel, tarray, yarray, stdarray, delays, alpha, rho, kappa=None, nu=None, marginalise_b=True):
    """loglik_noise over M rows -> (loglik[M], info[M]): Objective.loglik_markov_noise_batch's shape."""
    L = len(tarray)
    delays = np.asarray(delays, np.float64).reshape(-1, L)
    alpha = np.asarray(alpha, np.float64).reshape(-1, L)
    rho = np.asarray(rho, np.float64).reshape(-1)
    kappa, nu = _noise_rows(L, len(rho), kappa), _noise_rows(L, len(rho), nu)
    out = [loglik_noise(kernel, tarray, yarray, stdarray, delays[i], alpha[i], rho[i], kappa[i], nu[i], marginalise_b)
           for i in range(len(rho))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32)


def loglik_grad_noise_batch(kernel, tarray, yarray, stdarray, delays, alpha, rho, kappa=None, nu=None, marginalise_b=True):
    """loglik_grad_noise over M rows -> (loglik[M], grad[M, 4L+1], info[M]): Objective.loglik_grad_markov_noise_batch's shape."""
    L = len(tarray)
    delays = np.asarray(delays, np.float64).reshape(-1, L)
    alpha = np.asarray(alpha, np.float64).reshape(-1, L)
    rho = np.asarray(rho, np.float64).reshape(-1)
    kappa, nu = _noise_rows(L, len(rho), kappa), _noise_rows(L, len(rho), nu)
    out = [loglik_grad_noise(kernel, tarray, yarray, stdarray, delays[i], alpha[i], rho[i], kappa[i], nu[i], marginalise_b)
           for i in range(len(rho))]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]).reshape(-1, 4 * L + 1),
            np.array([o[2] for o in out], dtype=np.int32))


# ----------------------------------------------------------------------------------------------------------------------------------
# The (alpha, rho) block of the Hessian in linear time (csrc/gpcc_markov_hess.hip.h), the same algorithm in numpy: the
# filter's second-order forward sensitivities.  For a pair (a, b) of theta = (alpha_1..alpha_L, rho) four sets are carried: (m, P),
# (m_a, P_a), (m_b, P_b), (m_ab, P_ab).  For alpha and rho the merged order is fixed and no kink is crossed: no tie convention.
#
#   rho rho   d/drho = (-lambda / rho) d/dlambda, so d2/drho2 = (lambda / rho)^2 d2/dlambda2 + (2 lambda / rho^2) d/dlambda:
#             transition_d2rho and stationary_d2rho in closed form per kernel; the prior's second tangent is Pinf_ab
#   step      the product rule on _grad_pass's step: m_ab <- A_ab m + A_a m_b + A_b m_a + A m_ab, the nine terms of A D A' (D = P_xx - Pinf)
#             plus Pinf_ab, P_xb as m.  A_a = 0 for an alpha; A_ab and Pinf_ab are nonzero for (rho, rho) only
#   update    h_a = e_1 on the observations of band a, h_ab = 0:
#             (Ph)_a = P_a h + P h_a,  (Ph)_ab = P_ab h + P_a h_b + P_b h_a,  S_a = h_a'Ph + h'(Ph)_a,
#             S_ab = h_a'(Ph)_b + h_b'(Ph)_a + h'(Ph)_ab,  eps_a = -h_a'm - h'm_a,  eps_ab = -h_a'm_b - h_b'm_a - h'm_ab,
#             g = eps / S, g_a = (eps_a - g S_a) / S, g_ab = (eps_ab - g_a S_b - g_b S_a - g S_ab) / S:
#             l_ab -= (S_ab / S - S_a S_b / S^2 + 2 eps_a eps_b / S + 2 g eps_ab - 2 g (eps_a S_b + eps_b S_a) / S - g^2 S_ab
#                      + 2 g^2 S_a S_b / S) / 2,
#             then the second tangents of m += Ph g and P -= k Ph', k = Ph / S
#
# The rows of tau (loglik_hess; csrc/gpcc_markov_hess_tau.hip.h) are the same recursion with other tangents of the
# transition.  With c_l = d lag / d tau_l = -[band = l] + [bprev = l] (0 at the first point; _grad_pass's dd) and F = companion():
#
#   A_tau_l = c_l F A,   A_rho,tau_l = c_l (F_rho A + F A_rho),   A_tau_l,tau_m = c_l c_m F F A,   A_alpha,. = 0,
#
# and every tangent of Pinf, of the prior and of h by a tau is zero.  The Matern kernels are twice differentiable at zero lag, so the
# fixed-order second tangent is the derivative, ties or not.  OU is not: on a row where two points of different bands have exactly
# equal shifted times (a step with d == 0 and band != bprev) no second derivative by tau exists, the dense Hessian's convention there
# (k_ss = 1 / rho^2, k_rs = 0) is bilinear in the one-sided dK's, so no filter order returns it, and every entry with a tau index is
# NaN (info stays 0; value, gradient and the (alpha, rho) block are untouched): use the dense Hessian for OU on a grid of delays that
# collides with the cadence.
#
# The Fisher information has a recursion of its own (loglik_fisher below; csrc/gpcc_markov_fisher.hip.h): it carries
# second moments of the filter's means in place of the means and the second tangents.
# ----------------------------------------------------------------------------------------------------------------------------------
def transition_d2lambda(kernel, d, rho):
    """d2A(d)/dlambda2, in closed form per kernel."""
    name = _name(kernel)
    lam = rate(name, rho)
    x = lam * d
    e = math.exp(-x)
    if name == "OU":
        return np.array([[e * d * d]])
    if name == "matern32":
        return e * np.array([[d * d * (x - 1.0), d ** 3], [d * (4.0 * x - 2.0 - x * x), d * d * (3.0 - x)]])
    return e * np.array([[d * d * x * (0.5 * x - 1.0), d ** 3 * (x - 1.0), 0.5 * d ** 4],
                         [0.5 * d * x * (6.0 * x - 6.0 - x * x), d * d * (5.0 * x - 3.0 - x * x), 0.5 * d ** 3 * (4.0 - x)],
                         [x * (0.5 * x ** 3 - 5.0 * x * x + 12.0 * x - 6.0), d * (x ** 3 - 9.0 * x * x + 18.0 * x - 6.0),
                          d * d * (0.5 * x * x - 4.0 * x + 6.0)]])


def stationary_d2lambda(kernel, rho):
    """d2Pinf/dlambda2: Matern-3/2 d2(lambda^2) = 2; Matern-5/2 d2 kappa = 2/3, d2(lambda^4) = 12 lambda^2."""
    name = _name(kernel)
    lam = rate(name, rho)
    if name == "OU":
        return np.array([[0.0]])
    if name == "matern32":
        return np.array([[0.0, 0.0], [0.0, 2.0]])
    return np.array([[0.0, 0.0, -2.0 / 3.0], [0.0, 2.0 / 3.0, 0.0], [-2.0 / 3.0, 0.0, 12.0 * lam * lam]])


def transition_d2rho(kernel, d, rho, _chain=True):
    """d2A(d)/drho2 = (lambda / rho)^2 d2A/dlambda2 + (2 lambda / rho^2) dA/dlambda  (_chain=False, tests only: the second term dropped)."""
    lam = rate(kernel, rho)
    out = (lam / rho) ** 2 * transition_d2lambda(kernel, d, rho)
    if _chain:      # transition_drho = (-lambda / rho) dA/dlambda
        out = out - (2.0 / rho) * transition_drho(kernel, d, rho)
    return out


def stationary_d2rho(kernel, rho, _chain=True):
    """d2Pinf/drho2, by the same chain rule."""
    lam = rate(kernel, rho)
    out = (lam / rho) ** 2 * stationary_d2lambda(kernel, rho)
    if _chain:
        out = out - (2.0 / rho) * stationary_drho(kernel, rho)
    return out


def companion_drho(kernel, rho):
    """dF/drho, with dlambda/drho = -lambda / rho."""
    name = _name(kernel)
    lam = rate(name, rho)
    dl = -lam / rho
    if name == "OU":
        return np.array([[-dl]])
    if name == "matern32":
        return np.array([[0.0, 0.0], [-2.0 * lam * dl, -2.0 * dl]])
    return np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [-3.0 * lam * lam * dl, -6.0 * lam * dl, -3.0 * dl]])


def _hess_pass(name, train, alpha, rho, p, n, vb, a, b, slip=None):
    """d2 loglik / d theta_a d theta_b (a <= b in 0..2L: alpha_1..alpha_L, rho, tau_1..tau_L) by the second-order tangent recursion
    over the training observations in merge_order()'s order.  A pair with a tau on an OU row with a cross-band tie in shifted time has
    no second derivative: NaN.  slip: loglik_hess_hyper()'s and loglik_hess()'s."""
    L = len(alpha)
    ev = sorted(train, key=lambda e: (e[0], e[1], e[2]))
    ra, rb = a == L, b == L
    ta, tb = a - L - 1, b - L - 1           # the band of a tau (negative: not a tau)
    chain = slip != "chain_rho"
    zero = np.zeros((p, p))
    Pinf = stationary(name, rho)
    Qa = stationary_drho(name, rho) if ra else zero
    Qb = stationary_drho(name, rho) if rb else zero
    Qab = stationary_d2rho(name, rho, chain) if (ra and rb and slip != "no_d2pinf") else zero
    F = companion(name, rho)
    Fr = zero if slip == "no_dF" else companion_drho(name, rho)
    P = _prior(name, rho, p, n, vb)
    Pa, Pb, Pab = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    Pa[:p, :p], Pb[:p, :p], Pab[:p, :p] = Qa, Qb, Qab
    m, ma, mb, mab = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    hll, sprev, bprev = 0.0, None, -1
    for (s, band, _, r, s2) in ev:
        d = 0.0 if sprev is None else s - sprev
        if tb >= 0 and name == "OU" and sprev is not None and d == 0.0 and band != bprev:
            return math.nan
        # c_l = d lag / d tau_l: -[band = l] + [bprev = l], 0 at the first point
        ca = 0.0 if (ta < 0 or sprev is None) else -float(band == ta) + (0.0 if slip == "tau_one_lag" else float(bprev == ta))
        cb = 0.0 if (tb < 0 or sprev is None) else -float(band == tb) + (0.0 if slip == "tau_one_lag" else float(bprev == tb))
        sprev, bprev = s, band
        A = transition(name, d, rho)
        Aa = transition_drho(name, d, rho) if ra else (ca * (F @ A) if ca != 0.0 else zero)
        Ab = transition_drho(name, d, rho) if rb else (cb * (F @ A) if cb != 0.0 else zero)
        if ra and rb:
            Aab = transition_d2rho(name, d, rho, chain) if slip != "no_d2a" else zero
        elif ra and cb != 0.0:
            Aab = cb * (Fr @ A + F @ Aa)
        elif ca != 0.0 and cb != 0.0 and slip != "no_d2tau":
            Aab = (ca * cb) * (F @ (F @ A))
        else:
            Aab = zero
        X = slice(0, p)
        D, Da, Db, Dab = P[X, X] - Pinf, Pa[X, X] - Qa, Pb[X, X] - Qb, Pab[X, X] - Qab
        cross = zero if (slip == "no_cross" or (slip == "no_cross_tau" and tb >= 0)) else Aa @ D @ Ab.T + Ab @ D @ Aa.T
        mab[X] = Aab @ m[X] + Aa @ mb[X] + Ab @ ma[X] + A @ mab[X]
        Pab[X, X] = (Aab @ D @ A.T + A @ D @ Aab.T + cross + Aa @ Db @ A.T + A @ Db @ Aa.T + Ab @ Da @ A.T + A @ Da @ Ab.T
                     + A @ Dab @ A.T + Qab)
        Pab[X, p:] = Aab @ P[X, p:] + Aa @ Pb[X, p:] + Ab @ Pa[X, p:] + A @ Pab[X, p:]
        Pab[p:, X] = Pab[X, p:].T
        ma[X], mb[X] = Aa @ m[X] + A @ ma[X], Ab @ m[X] + A @ mb[X]
        Pa[X, X] = Aa @ D @ A.T + A @ Da @ A.T + A @ D @ Aa.T + Qa
        Pb[X, X] = Ab @ D @ A.T + A @ Db @ A.T + A @ D @ Ab.T + Qb
        Pa[X, p:], Pb[X, p:] = Aa @ P[X, p:] + A @ Pa[X, p:], Ab @ P[X, p:] + A @ Pb[X, p:]
        Pa[p:, X], Pb[p:, X] = Pa[X, p:].T, Pb[X, p:].T
        m[X] = A @ m[X]
        P[X, X] = A @ D @ A.T + Pinf
        P[X, p:] = A @ P[X, p:]
        P[p:, X] = P[X, p:].T

        h, ha, hb = np.zeros(n), np.zeros(n), np.zeros(n)
        h[0] = alpha[band]
        if n > p:
            h[p + band] = 1.0
        ha[0], hb[0] = float(band == a), float(band == b)
        Ph = P @ h
        Pha, Phb = Pa @ h + P @ ha, Pb @ h + P @ hb
        Phab = Pab @ h + Pa @ hb + Pb @ ha
        S = h @ Ph + s2
        if not (S > 0.0 and math.isfinite(S)):
            return math.nan
        Sa, Sb = ha @ Ph + h @ Pha, hb @ Ph + h @ Phb
        Sab = h @ Phab
        eps = r - h @ m
        ea, eb = -(ha @ m) - h @ ma, -(hb @ m) - h @ mb
        eab = -(h @ mab)
        if slip != "no_hahb":
            Sab += ha @ Phb + hb @ Pha
            eab -= ha @ mb + hb @ ma
        inv = 1.0 / S
        g = eps * inv
        ga, gb = (ea - g * Sa) * inv, (eb - g * Sb) * inv
        gab = (eab - ga * Sb - gb * Sa - g * Sab) * inv
        hll -= 0.5 * (Sab * inv - Sa * Sb * inv * inv + 2.0 * ea * eb * inv + 2.0 * g * eab - 2.0 * g * inv * (ea * Sb + eb * Sa)
                      - g * g * Sab + 2.0 * g * g * Sa * Sb * inv)
        k = Ph * inv
        ka, kb = Pha * inv - k * (inv * Sa), Phb * inv - k * (inv * Sb)
        kab = Phab * inv - Pha * (inv * inv * Sb) - Phb * (inv * inv * Sa) - k * (inv * Sab) + k * (2.0 * inv * inv * Sa * Sb)
        mab = mab + Phab * g + Pha * gb + Phb * ga + Ph * gab
        ma, mb = ma + Pha * g + Ph * ga, mb + Phb * g + Ph * gb
        m = m + Ph * g
        Pab = Pab - np.outer(kab, Ph) - np.outer(ka, Phb) - np.outer(kb, Pha) - np.outer(k, Phab)
        Pa = Pa - np.outer(ka, Ph) - np.outer(k, Pha)
        Pb = Pb - np.outer(kb, Ph) - np.outer(k, Phb)
        P = P - np.outer(k, Ph)
        P, Pa, Pb, Pab = (0.5 * (Z + Z.T) for Z in (P, Pa, Pb, Pab))
    return hll


def loglik_hess_hyper(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True, _slip=None):
    """(loglik, grad[2L+1], hess[L+1, L+1], info) of one (tau, alpha, rho): loglik()'s value and info, loglik_grad()'s full row and the
    Hessian over [alpha_1..alpha_L, rho] by the filter's second-order forward sensitivities, each pair computed once and mirrored:
    Objective.loglik_hess_hyper_markov_batch's row.  grad and hess are NaN where info != 0.
    _slip (tests only) injects one mistake: "no_d2a" (A_rhorho left out), "no_d2pinf" (Pinf_rhorho left out of the prior and the step),
    "no_cross" (the A_a D A_b' cross terms of the step left out), "no_hahb" (the h_a, h_b terms of S_ab and eps_ab left out), "chain_rho"
    (the (2 lambda / rho^2) d/dlambda term of the rho rho chain rule dropped)."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b,
                                                                       codes_first=True)
    ll, grad, info = loglik_grad(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b)
    hess = np.full((L + 1, L + 1), math.nan)
    if info:
        return ll, grad, hess, info
    for a in range(L + 1):
        for b in range(a, L + 1):
            hess[a, b] = hess[b, a] = _hess_pass(name, train, alpha, rho, p, n, vb, a, b, slip=_slip)
    return ll, grad, hess, 0


def loglik_hess_hyper_batch(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True):
    """loglik_hess_hyper over M rows -> (loglik[M], grad[M, 2L+1], hess[M, L+1, L+1], info[M]): Objective.loglik_hess_hyper_markov_batch's
    shape."""
    L = len(tarray)
    delays = np.asarray(delays, np.float64).reshape(-1, L)
    alpha = np.asarray(alpha, np.float64).reshape(-1, L)
    rho = np.asarray(rho, np.float64).reshape(-1)
    out = [loglik_hess_hyper(kernel, tarray, yarray, stdarray, delays[i], alpha[i], rho[i], marginalise_b) for i in range(len(rho))]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]).reshape(-1, 2 * L + 1),
            np.array([o[2] for o in out]).reshape(-1, L + 1, L + 1), np.array([o[3] for o in out], dtype=np.int32))


def loglik_hess(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True, _slip=None):
    """(loglik, grad[2L+1], hess[2L+1, 2L+1], info) of one (tau, alpha, rho): loglik_hess_hyper()'s value, gradient, info and leading
    (L+1) x (L+1) block, and the rows of tau by the same recursion, over [alpha_1..alpha_L, rho, tau_1..tau_L]:
    Objective.loglik_hess_markov_batch's row.  Each pair is computed once and mirrored.  grad and hess are NaN where info != 0.  On an
    OU row with a cross-band tie in shifted time every entry with a tau index is NaN and info stays 0 (no second derivative exists
    there: use the dense Hessian); with one band the tau entries are exact zeros.
    _slip (tests only) injects one mistake: "no_d2tau" (A_tautau left out), "no_dF" (the F_rho A term of A_rho,tau left out),
    "no_cross_tau" (the A_a D A_b' cross terms of the step left out when b is a tau), "tau_one_lag" (only the lag before a point of band
    l is differentiated, not the one after)."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b,
                                                                       codes_first=True)
    W = 2 * L + 1
    ll, grad, hyper, info = loglik_hess_hyper(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b)
    hess = np.full((W, W), math.nan)
    if info:
        return ll, grad, hess, info
    hess[:L + 1, :L + 1] = hyper
    for a in range(W):
        for b in range(max(a, L + 1), W):
            hess[a, b] = hess[b, a] = _hess_pass(name, train, alpha, rho, p, n, vb, a, b, slip=_slip)
    return ll, grad, hess, 0


def loglik_hess_batch(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True):
    """loglik_hess over M rows -> (loglik[M], grad[M, 2L+1], hess[M, 2L+1, 2L+1], info[M]): Objective.loglik_hess_markov_batch's shape."""
    L = len(tarray)
    W = 2 * L + 1
    delays = np.asarray(delays, np.float64).reshape(-1, L)
    alpha = np.asarray(alpha, np.float64).reshape(-1, L)
    rho = np.asarray(rho, np.float64).reshape(-1)
    out = [loglik_hess(kernel, tarray, yarray, stdarray, delays[i], alpha[i], rho[i], marginalise_b) for i in range(len(rho))]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]).reshape(-1, W),
            np.array([o[2] for o in out]).reshape(-1, W, W), np.array([o[3] for o in out], dtype=np.int32))


# ----------------------------------------------------------------------------------------------------------------------------------
# The Hessian under a noise model per row (csrc/gpcc_markov_noise_hess.hip.h, gpcc_loglik_hess_noise_markov_batch), the
# same algorithm in numpy, over theta = [alpha_1..alpha_L, rho, kappa_1..kappa_L, nu_1..nu_L], n = 3L + 1.  A pair of alpha and rho is
# _hess_pass on the mapped variances.  A pair with a noise parameter (_noise_hess_pass) is _hess_pass's recursion with _noise_pass's
# tangent in it: for kappa_l or nu_l the prior's, the transition's and the stationary tangent are zero and there is no h-tangent; at an
# observation of band l the variance moves by dvar = 2 kappa_l sigma_i^2 (kappa) or 1 (nu), and by d2var = 2 sigma_i^2 on the pair
# (kappa_l, kappa_l) alone:  S_a += dvar_a,  S_b += dvar_b,  S_ab += d2var,  and everything behind S, S_a, S_b, S_ab is _hess_pass's.
# A (rho, noise) pair forms A_rho and Pinf_rho only; a noise noise pair on two bands is not zero: the filter couples the bands.
# ----------------------------------------------------------------------------------------------------------------------------------
def _noise_hess_pass(name, ntrain, alpha, rho, p, n, vb, a, b, kappa, slip=None):
    """d2 loglik / d theta_a d theta_b for a <= b in 0..3L with b a noise parameter (b > L), over _noise_train's observations in
    merge_order()'s order.  slip: loglik_hess_noise()'s."""
    L = len(alpha)
    ev = sorted(ntrain, key=lambda e: e[:3])
    ra = a == L
    na = a > L

    def noise(q):       # (band, is_nu) of a noise index
        return ((q - L - 1) % L, q > 2 * L)

    (banda, nua) = noise(a) if na else (a if a < L else -1, False)
    bandb, nub = noise(b)
    zero = np.zeros((p, p))
    Pinf = stationary(name, rho)
    Qa = stationary_drho(name, rho) if ra else zero
    P = _prior(name, rho, p, n, vb)
    Pa, Pb, Pab = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    Pa[:p, :p] = Qa
    m, ma, mb, mab = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    kfac = 1.0 if slip == "kappa_linear" else 2.0
    hll, sprev = 0.0, None
    for (s, band, _, r, v, s2) in ev:
        d = 0.0 if sprev is None else s - sprev
        sprev = s
        A = transition(name, d, rho)
        Aa = transition_drho(name, d, rho) if (ra and slip != "rho_noise_no_dA") else zero
        X = slice(0, p)
        D, Da, Db, Dab = P[X, X] - Pinf, Pa[X, X] - Qa, Pb[X, X], Pab[X, X]
        # A_b = 0, A_ab = 0, Pinf_b = Pinf_ab = 0: _hess_pass's step without those terms
        mab[X] = Aa @ mb[X] + A @ mab[X]
        Pab[X, X] = Aa @ Db @ A.T + A @ Db @ Aa.T + A @ Dab @ A.T
        Pab[X, p:] = Aa @ Pb[X, p:] + A @ Pab[X, p:]
        Pab[p:, X] = Pab[X, p:].T
        ma[X], mb[X] = Aa @ m[X] + A @ ma[X], A @ mb[X]
        Pa[X, X] = Aa @ D @ A.T + A @ Da @ A.T + A @ D @ Aa.T + Qa
        Pb[X, X] = A @ Db @ A.T
        Pa[X, p:], Pb[X, p:] = Aa @ P[X, p:] + A @ Pa[X, p:], A @ Pb[X, p:]
        Pa[p:, X], Pb[p:, X] = Pa[X, p:].T, Pb[X, p:].T
        m[X] = A @ m[X]
        P[X, X] = A @ D @ A.T + Pinf
        P[X, p:] = A @ P[X, p:]
        P[p:, X] = P[X, p:].T

        h, ha = np.zeros(n), np.zeros(n)
        h[0] = alpha[band]
        if n > p:
            h[p + band] = 1.0
        ha[0] = float(a < L and band == a)
        dva = 0.0
        if na and band == banda:
            dva = 1.0 if nua else kfac * kappa[banda] * s2
        dvb = 0.0
        if band == bandb:
            dvb = 1.0 if nub else kfac * kappa[bandb] * s2
        d2v = 2.0 * s2 if (a == b and not nub and band == bandb and slip != "no_d2kappa") else 0.0
        Ph = P @ h
        Pha, Phb = Pa @ h + P @ ha, Pb @ h
        Phab = Pab @ h + Pb @ ha
        S = h @ Ph + v
        if not (S > 0.0 and math.isfinite(S)):
            return math.nan
        Sa, Sb = ha @ Ph + h @ Pha + dva, h @ Phb + dvb
        Sab = h @ Phab + ha @ Phb + d2v
        eps = r - h @ m
        ea, eb = -(ha @ m) - h @ ma, -(h @ mb)
        eab = -(h @ mab) - ha @ mb
        inv = 1.0 / S
        g = eps * inv
        ga, gb = (ea - g * Sa) * inv, (eb - g * Sb) * inv
        gab = (eab - ga * Sb - gb * Sa - g * Sab) * inv
        SaSb = (Sa - dva) * (Sb - dvb) if slip == "dvar_one_side" else Sa * Sb      # the S_a S_b cross terms of the second tangent
        hll -= 0.5 * (Sab * inv - SaSb * inv * inv + 2.0 * ea * eb * inv + 2.0 * g * eab - 2.0 * g * inv * (ea * Sb + eb * Sa)
                      - g * g * Sab + 2.0 * g * g * SaSb * inv)
        k = Ph * inv
        ka, kb = Pha * inv - k * (inv * Sa), Phb * inv - k * (inv * Sb)
        kab = Phab * inv - Pha * (inv * inv * Sb) - Phb * (inv * inv * Sa) - k * (inv * Sab) + k * (2.0 * inv * inv * SaSb)
        mab = mab + Phab * g + Pha * gb + Phb * ga + Ph * gab
        ma, mb = ma + Pha * g + Ph * ga, mb + Phb * g + Ph * gb
        m = m + Ph * g
        Pab = Pab - np.outer(kab, Ph) - np.outer(ka, Phb) - np.outer(kb, Pha) - np.outer(k, Phab)
        Pa = Pa - np.outer(ka, Ph) - np.outer(k, Pha)
        Pb = Pb - np.outer(kb, Ph) - np.outer(k, Phb)
        P = P - np.outer(k, Ph)
        P, Pa, Pb, Pab = (0.5 * (Z + Z.T) for Z in (P, Pa, Pb, Pab))
    return hll


def loglik_hess_noise(kernel, tarray, yarray, stdarray, delays, alpha, rho, kappa=None, nu=None, marginalise_b=True, _slip=None):
    """(loglik, grad[4L+1], hess[3L+1, 3L+1], info) of one (tau, alpha, rho, kappa, nu): loglik_grad_noise()'s value, row and info, and the
    Hessian over [alpha_1..alpha_L, rho, kappa_1..kappa_L, nu_1..nu_L] by the filter's second-order forward sensitivities with the
    variance's tangents, each pair computed once and mirrored: Objective.loglik_hess_markov_noise_batch's row.  The leading (L+1) x (L+1)
    block is loglik_hess_hyper()'s on the error bars sqrt(kappa_l^2 sigma_i^2 + nu_l).  grad and hess are NaN where info != 0.
    _slip (tests only) injects one mistake: "no_d2kappa" (the 2 sigma^2 term of (kappa_l, kappa_l) left out), "dvar_one_side" (dvar
    enters S_a, S_b but not the S_a S_b cross terms of the second tangent), "kappa_linear" (dvar = kappa sigma^2 instead of
    2 kappa sigma^2), "noise_noise_diag_only" (noise pairs on two bands set to zero), "rho_noise_no_dA" (the (rho, noise) pairs walked
    without A_rho)."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b,
                                                                       codes_first=True)
    W = 3 * L + 1
    ll, grad, info = loglik_grad_noise(kernel, tarray, yarray, stdarray, delays, alpha, rho, kappa, nu, marginalise_b)
    hess = np.full((W, W), math.nan)
    if info:
        return ll, grad, hess, info
    kappa, nu, _ = _noise_setup(L, kappa, nu)
    ntrain = _noise_train(train, kappa, nu)
    mapped = [e[:5] for e in ntrain]
    for a in range(W):
        for b in range(a, W):
            if b <= L:
                v = _hess_pass(name, mapped, alpha, rho, p, n, vb, a, b)
            elif _slip == "noise_noise_diag_only" and a > L and (a - L - 1) % L != (b - L - 1) % L:
                v = 0.0
            else:
                v = _noise_hess_pass(name, ntrain, alpha, rho, p, n, vb, a, b, kappa, slip=_slip)
            hess[a, b] = hess[b, a] = v
    return ll, grad, hess, 0


def loglik_hess_noise_batch(kernel, tarray, yarray, stdarray, delays, alpha, rho, kappa=None, nu=None, marginalise_b=True):
    """loglik_hess_noise over M rows -> (loglik[M], grad[M, 4L+1], hess[M, 3L+1, 3L+1], info[M]): Objective.loglik_hess_markov_noise_batch's
    shape."""
    L = len(tarray)
    W = 3 * L + 1
    delays = np.asarray(delays, np.float64).reshape(-1, L)
    alpha = np.asarray(alpha, np.float64).reshape(-1, L)
    rho = np.asarray(rho, np.float64).reshape(-1)
    kappa, nu = _noise_rows(L, len(rho), kappa), _noise_rows(L, len(rho), nu)
    out = [loglik_hess_noise(kernel, tarray, yarray, stdarray, delays[i], alpha[i], rho[i], kappa[i], nu[i], marginalise_b)
           for i in range(len(rho))]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]).reshape(-1, 4 * L + 1),
            np.array([o[2] for o in out]).reshape(-1, W, W), np.array([o[3] for o in out], dtype=np.int32))


# ----------------------------------------------------------------------------------------------------------------------------------
# The rows of tau of the Hessian under a noise model per row (csrc/gpcc_markov_noise_hess_tau.hip.h,
# gpcc_loglik_hess_full_noise_markov_batch), the same algorithm in numpy, over the gradient row's order
# theta = [alpha_1..alpha_L, rho, tau_1..tau_L, kappa_1..kappa_L, nu_1..nu_L], n = 4L + 1.  An (alpha, tau), (rho, tau) or (tau, tau)
# pair is _hess_pass on the mapped variances.  A (tau_l, noise) pair (_noise_tau_hess_pass) carries the noise tangent a of
# _noise_hess_pass (no tangent of A, of Pinf, of the prior or of h; dvar in S_a) and the tau tangent b of _hess_pass (A_b = c_l F A):
#   step     A_a = A_ab = 0, so  m_ab <- A_b m_a + A m_ab,  P_ab,xx <- A_b D_a A' + A D_a A_b' + A D_ab A',  P_ab,xb <- A_b P_a,xb + A P_ab,xb:
#            the second tangent moves as the tau tangent of the "state" (m_a, P_a) with a zero stationary part; no cross term
#   update   h_a = h_b = 0, S_a += dvar, nothing in S_b and S_ab
# On an OU row with a cross-band tie in shifted time the pair has no second derivative: NaN, as every pair with a tau.
# ----------------------------------------------------------------------------------------------------------------------------------
NOISE_HESS_FULL_SLIPS = ("tau_noise_no_dvar", "tau_noise_as_state", "plain_variance", "tau_noise_own_band")


def _noise_tau_hess_pass(name, ntrain, alpha, rho, p, n, vb, tl, q, kappa, slip=None):
    """d2 loglik / d tau_tl d theta_q for a noise parameter q of the 3L + 1 order of _noise_hess_pass (q > L: kappa_1..L, nu_1..L), over
    _noise_train's observations in merge_order()'s order.  NaN on an OU row with a cross-band tie.  slip: loglik_hess_full_noise()'s."""
    L = len(alpha)
    ev = sorted(ntrain, key=lambda e: e[:3])
    banda, nua = (q - L - 1) % L, q > 2 * L
    zero = np.zeros((p, p))
    Pinf = stationary(name, rho)
    F = companion(name, rho)
    P = _prior(name, rho, p, n, vb)
    Pa, Pb, Pab = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    m, ma, mb, mab = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    hll, sprev, bprev = 0.0, None, -1
    for (s, band, _, r, v, s2) in ev:
        d = 0.0 if sprev is None else s - sprev
        if name == "OU" and sprev is not None and d == 0.0 and band != bprev:
            return math.nan
        cb = 0.0 if sprev is None else -float(band == tl) + float(bprev == tl)
        sprev, bprev = s, band
        A = transition(name, d, rho)
        Ab = cb * (F @ A) if cb != 0.0 else zero
        X = slice(0, p)
        D, Da, Db, Dab = P[X, X] - Pinf, Pa[X, X], Pb[X, X], Pab[X, X]
        if slip == "tau_noise_as_state":      # the tau tangent of the state, not of (m_a, P_a)
            mab[X] = Ab @ m[X] + A @ mab[X]
            Pab[X, X] = Ab @ D @ A.T + A @ D @ Ab.T + A @ Dab @ A.T
            Pab[X, p:] = Ab @ P[X, p:] + A @ Pab[X, p:]
        else:
            mab[X] = Ab @ ma[X] + A @ mab[X]
            Pab[X, X] = Ab @ Da @ A.T + A @ Da @ Ab.T + A @ Dab @ A.T
            Pab[X, p:] = Ab @ Pa[X, p:] + A @ Pab[X, p:]
        Pab[p:, X] = Pab[X, p:].T
        ma[X], mb[X] = A @ ma[X], Ab @ m[X] + A @ mb[X]
        Pa[X, X] = A @ Da @ A.T
        Pb[X, X] = Ab @ D @ A.T + A @ Db @ A.T + A @ D @ Ab.T
        Pa[X, p:], Pb[X, p:] = A @ Pa[X, p:], Ab @ P[X, p:] + A @ Pb[X, p:]
        Pa[p:, X], Pb[p:, X] = Pa[X, p:].T, Pb[X, p:].T
        m[X] = A @ m[X]
        P[X, X] = A @ D @ A.T + Pinf
        P[X, p:] = A @ P[X, p:]
        P[p:, X] = P[X, p:].T

        h = np.zeros(n)
        h[0] = alpha[band]
        if n > p:
            h[p + band] = 1.0
        dva = 0.0
        if band == banda:
            dva = 1.0 if nua else 2.0 * kappa[banda] * s2
        Ph, Pha, Phb, Phab = P @ h, Pa @ h, Pb @ h, Pab @ h
        S = h @ Ph + v
        if not (S > 0.0 and math.isfinite(S)):
            return math.nan
        Sa1, Sb, Sab = h @ Pha + dva, h @ Phb, h @ Phab             # Sa1: the first-order update's S_a
        Sa = h @ Pha if slip == "tau_noise_no_dvar" else Sa1        # the second-order update's
        eps = r - h @ m
        ea, eb, eab = -(h @ ma), -(h @ mb), -(h @ mab)
        inv = 1.0 / S
        g = eps * inv
        ga, gb, ga1 = (ea - g * Sa) * inv, (eb - g * Sb) * inv, (ea - g * Sa1) * inv
        gab = (eab - ga * Sb - gb * Sa - g * Sab) * inv
        hll -= 0.5 * (Sab * inv - Sa * Sb * inv * inv + 2.0 * ea * eb * inv + 2.0 * g * eab - 2.0 * g * inv * (ea * Sb + eb * Sa)
                      - g * g * Sab + 2.0 * g * g * Sa * Sb * inv)
        k = Ph * inv
        ka, kb, ka1 = Pha * inv - k * (inv * Sa), Phb * inv - k * (inv * Sb), Pha * inv - k * (inv * Sa1)
        kab = Phab * inv - Pha * (inv * inv * Sb) - Phb * (inv * inv * Sa) - k * (inv * Sab) + k * (2.0 * inv * inv * Sa * Sb)
        mab = mab + Phab * g + Pha * gb + Phb * ga + Ph * gab
        ma, mb = ma + Pha * g + Ph * ga1, mb + Phb * g + Ph * gb
        m = m + Ph * g
        Pab = Pab - np.outer(kab, Ph) - np.outer(ka, Phb) - np.outer(kb, Pha) - np.outer(k, Phab)
        Pa = Pa - np.outer(ka1, Ph) - np.outer(k, Pha)
        Pb = Pb - np.outer(kb, Ph) - np.outer(k, Phb)
        P = P - np.outer(k, Ph)
        P, Pa, Pb, Pab = (0.5 * (Z + Z.T) for Z in (P, Pa, Pb, Pab))
    return hll


def loglik_hess_full_noise(kernel, tarray, yarray, stdarray, delays, alpha, rho, kappa=None, nu=None, marginalise_b=True, pairs=None,
                           _slip=None):
    """(loglik, grad[4L+1], hess[4L+1, 4L+1], info) of one (tau, alpha, rho, kappa, nu): loglik_grad_noise()'s value, row and info, and the
    full Hessian over the gradient row's order [alpha_1..L, rho, tau_1..L, kappa_1..L, nu_1..L], each pair computed once and mirrored:
    Objective.loglik_hess_full_markov_noise_batch's row.  The sub-block on the indices {0..L, 2L+1..4L} is loglik_hess_noise()'s exactly;
    the leading (2L+1) x (2L+1) block is loglik_hess()'s on the error bars sqrt(kappa_l^2 sigma_i^2 + nu_l).  grad and hess are NaN where
    info != 0.  On an OU row with a cross-band tie in shifted time every entry with a tau index is NaN and info stays 0; with one band
    the tau entries are exact zeros.  pairs: an iterable of (a, b) in the 4L+1 order that restricts the work to those entries (either
    order); the others come back NaN.
    _slip (tests only) injects one mistake: "tau_noise_no_dvar" (the noise tangent's dvar left out of the second-order update of a
    (tau, noise) pair), "tau_noise_as_state" (the (tau, noise) second tangent propagated from the state instead of from the noise
    tangent), "plain_variance" (the (alpha, tau), (rho, tau) and (tau, tau) pairs walked on sigma^2 instead of kappa^2 sigma^2 + nu),
    "tau_noise_own_band" (a (tau_l, noise_m) pair formed for l == m only, the others zero)."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b,
                                                                       codes_first=True)
    W, T, K = 4 * L + 1, L + 1, 2 * L + 1
    ll, grad, info = loglik_grad_noise(kernel, tarray, yarray, stdarray, delays, alpha, rho, kappa, nu, marginalise_b)
    hess = np.full((W, W), math.nan)
    if info:
        return ll, grad, hess, info
    kappa, nu, _ = _noise_setup(L, kappa, nu)
    ntrain = _noise_train(train, kappa, nu)
    mapped = [e[:5] for e in ntrain]
    want = None if pairs is None else {(min(a, b), max(a, b)) for (a, b) in pairs}
    for a in range(W):
        for b in range(a, W):
            if want is not None and (a, b) not in want:
                continue
            ta, tb = T <= a < K, T <= b < K
            if not ta and not tb:           # [alpha, rho, kappa, nu]: loglik_hess_noise()'s pair in its 3L + 1 order
                qa, qb = (a if a < T else a - L), (b if b < T else b - L)
                if qb <= L:
                    v = _hess_pass(name, mapped, alpha, rho, p, n, vb, qa, qb)
                else:
                    v = _noise_hess_pass(name, ntrain, alpha, rho, p, n, vb, qa, qb, kappa)
            elif b < K:                     # (alpha, tau), (rho, tau), (tau, tau): _hess_pass's order is this one's first 2L + 1
                v = _hess_pass(name, train if _slip == "plain_variance" else mapped, alpha, rho, p, n, vb, a, b)
            else:                           # (tau_l, noise): a is the tau
                if _slip == "tau_noise_own_band" and (a - T) != (b - K) % L:
                    v = 0.0
                else:
                    v = _noise_tau_hess_pass(name, ntrain, alpha, rho, p, n, vb, a - T, b - L, kappa, slip=_slip)
            hess[a, b] = hess[b, a] = v
    return ll, grad, hess, 0


def loglik_hess_full_noise_batch(kernel, tarray, yarray, stdarray, delays, alpha, rho, kappa=None, nu=None, marginalise_b=True, pairs=None):
    """loglik_hess_full_noise over M rows -> (loglik[M], grad[M, 4L+1], hess[M, 4L+1, 4L+1], info[M]):
    Objective.loglik_hess_full_markov_noise_batch's shape."""
    L = len(tarray)
    W = 4 * L + 1
    delays = np.asarray(delays, np.float64).reshape(-1, L)
    alpha = np.asarray(alpha, np.float64).reshape(-1, L)
    rho = np.asarray(rho, np.float64).reshape(-1)
    kappa, nu = _noise_rows(L, len(rho), kappa), _noise_rows(L, len(rho), nu)
    out = [loglik_hess_full_noise(kernel, tarray, yarray, stdarray, delays[i], alpha[i], rho[i], kappa[i], nu[i], marginalise_b, pairs)
           for i in range(len(rho))]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]).reshape(-1, W),
            np.array([o[2] for o in out]).reshape(-1, W, W), np.array([o[3] for o in out], dtype=np.int32))


# ----------------------------------------------------------------------------------------------------------------------------------
# The Fisher information in linear time (csrc/gpcc_markov_fisher.hip.h), the same algorithm in numpy.  The expectation
# of -l_ab over the data of the model at theta: the innovation eps_k is independent of the past with variance S_k, its tangent
# eps_a = -h_a'm - h'm_a depends on the past only, so
#
#   I_ab = sum_k [ S_a S_b / (2 S^2) + E[eps_a eps_b] / S ].
#
# No data enters: beside P, P_a, P_b (the gradient's tangents, _grad_pass's) the second moments of the means are carried, all n x n
# and zero at the start (the prior mean is 0): C_a = E[m_a m'], C_b = E[m_b m'], D = E[m_a m_b'].  Z = E[m m'] = Pi - P with Pi =
# blockdiag(Pinf, Sigma_b) the prior covariance: the state is stationary.  With Abar = blockdiag(A, I), Abar_a = blockdiag(A_a, 0):
#
#   predict   (Z before the step)  D <- Abar_a Z Abar_b' + Abar_a C_b' Abar' + Abar C_a Abar_b' + Abar D Abar',
#             C_a <- Abar_a Z Abar' + Abar C_a Abar',  then P_a, P_b, P as _grad_pass
#   update    (Z after the predict)  g = Ph / S,  g_a = (Ph)_a / S - Ph S_a / S^2,
#             u_a = E[eps_a m'] = -h_a'Z - h'C_a,  v_ab = E[eps_a m_b'] = -h_a'C_b' - h'D,  v_ba = -h_b'C_a' - h'D',
#             w = E[eps_a eps_b] = h_a'Z h_b + h_a'C_b'h + h'C_a h_b + h'D h:
#             I_ab += S_a S_b / (2 S^2) + w / S,
#             D += g v_ab + v_ba'g' + w g g' + S g_a g_b',  C_a += g u_a + S g_a g',  then P_a, P_b, P as _grad_pass
#
# The merged order is merge_order()'s, fixed.  The Matern kernels are C^1 at zero lag: exact, ties or not.  OU has a kink, the dense
# convention at an exact tie of two bands is the mean of the one-sided dK's and the Fisher information is bilinear in them, so on such
# a row every entry with a tau index is NaN (info stays 0, the (alpha, rho) block is exact): loglik_hess's contract.
# ----------------------------------------------------------------------------------------------------------------------------------
FISHER_SLIPS = ("no_innov", "prior_moment", "no_gain_tangent", "no_dh_moment", "tau_one_lag")


def _fisher_pass(name, train, alpha, rho, p, n, vb, a, b, slip=None):
    """I_ab (a <= b in 0..2L: alpha_1..alpha_L, rho, tau_1..tau_L) by the moment recursion over the training observations in
    merge_order()'s order; the residuals are not read.  A pair with a tau on an OU row with a cross-band tie: NaN.  slip: loglik_fisher()'s."""
    L = len(alpha)
    ev = sorted(train, key=lambda e: (e[0], e[1], e[2]))
    ra, rb = a == L, b == L
    ta, tb = a - L - 1, b - L - 1           # the band of a tau (negative: not a tau)
    X = slice(0, p)
    zero = np.zeros((p, p))
    Pinf = stationary(name, rho)
    Qa = stationary_drho(name, rho) if ra else zero
    Qb = stationary_drho(name, rho) if rb else zero
    F = companion(name, rho)
    Pi = _prior(name, rho, p, n, vb)
    P = Pi.copy()
    Pa, Pb = np.zeros((n, n)), np.zeros((n, n))
    Pa[X, X], Pb[X, X] = Qa, Qb
    Ca, Cb, D = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    Ab_, Aa_, Ab__ = np.eye(n), np.zeros((n, n)), np.zeros((n, n))      # Abar, Abar_a, Abar_b
    fish, sprev, bprev = 0.0, None, -1
    for (s, band, _, _, s2) in ev:
        d = 0.0 if sprev is None else s - sprev
        if tb >= 0 and name == "OU" and sprev is not None and d == 0.0 and band != bprev:
            return math.nan
        ca = 0.0 if (ta < 0 or sprev is None) else -float(band == ta) + (0.0 if slip == "tau_one_lag" else float(bprev == ta))
        cb = 0.0 if (tb < 0 or sprev is None) else -float(band == tb) + (0.0 if slip == "tau_one_lag" else float(bprev == tb))
        sprev, bprev = s, band
        A = transition(name, d, rho)
        Aa = transition_drho(name, d, rho) if ra else (ca * (F @ A) if ca != 0.0 else zero)
        Ab = transition_drho(name, d, rho) if rb else (cb * (F @ A) if cb != 0.0 else zero)
        Ab_[X, X], Aa_[X, X], Ab__[X, X] = A, Aa, Ab
        Z = Pi if slip == "prior_moment" else Pi - P
        D = Aa_ @ Z @ Ab__.T + Aa_ @ Cb.T @ Ab_.T + Ab_ @ Ca @ Ab__.T + Ab_ @ D @ Ab_.T
        Ca = Aa_ @ Z @ Ab_.T + Ab_ @ Ca @ Ab_.T
        Cb = Ab__ @ Z @ Ab_.T + Ab_ @ Cb @ Ab_.T
        D0, Da, Db = P[X, X] - Pinf, Pa[X, X] - Qa, Pb[X, X] - Qb
        Pa[X, X] = Aa @ D0 @ A.T + A @ Da @ A.T + A @ D0 @ Aa.T + Qa
        Pb[X, X] = Ab @ D0 @ A.T + A @ Db @ A.T + A @ D0 @ Ab.T + Qb
        Pa[X, p:], Pb[X, p:] = Aa @ P[X, p:] + A @ Pa[X, p:], Ab @ P[X, p:] + A @ Pb[X, p:]
        Pa[p:, X], Pb[p:, X] = Pa[X, p:].T, Pb[X, p:].T
        P[X, X] = A @ D0 @ A.T + Pinf
        P[X, p:] = A @ P[X, p:]
        P[p:, X] = P[X, p:].T

        h, ha, hb = np.zeros(n), np.zeros(n), np.zeros(n)
        h[0] = alpha[band]
        if n > p:
            h[p + band] = 1.0
        ha[0], hb[0] = float(band == a), float(band == b)
        Ph = P @ h
        Pha, Phb = Pa @ h + P @ ha, Pb @ h + P @ hb
        S = h @ Ph + s2
        if not (S > 0.0 and math.isfinite(S)):
            return math.nan
        Sa, Sb = ha @ Ph + h @ Pha, hb @ Ph + h @ Phb
        inv = 1.0 / S
        g = Ph * inv
        ga, gb = Pha * inv - g * (inv * Sa), Phb * inv - g * (inv * Sb)
        Z = Pi if slip == "prior_moment" else Pi - P
        ma, mb = (np.zeros(n), np.zeros(n)) if slip == "no_dh_moment" else (ha, hb)
        ua, ub = -(ma @ Z) - h @ Ca, -(mb @ Z) - h @ Cb
        vab, vba = -(ma @ Cb.T) - h @ D, -(mb @ Ca.T) - h @ D.T
        w = ma @ Z @ mb + ma @ Cb.T @ h + h @ Ca @ mb + h @ D @ h
        fish += 0.5 * Sa * Sb * inv * inv + (0.0 if slip == "no_innov" else w * inv)
        D = D + np.outer(g, vab) + np.outer(vba, g) + w * np.outer(g, g)
        Ca, Cb = Ca + np.outer(g, ua), Cb + np.outer(g, ub)
        if slip != "no_gain_tangent":
            D = D + S * np.outer(ga, gb)
            Ca, Cb = Ca + S * np.outer(ga, g), Cb + S * np.outer(gb, g)
        Pa = Pa - np.outer(ga, Ph) - np.outer(g, Pha)
        Pb = Pb - np.outer(gb, Ph) - np.outer(g, Phb)
        P = P - np.outer(g, Ph)
        P, Pa, Pb = (0.5 * (M_ + M_.T) for M_ in (P, Pa, Pb))
    return fish


def loglik_fisher(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True, pairs=None, _slip=None):
    """(loglik, grad[2L+1], fisher[2L+1, 2L+1], info) of one (tau, alpha, rho): loglik_grad()'s value, gradient and info, and the expected
    (Fisher) information over [alpha_1..alpha_L, rho, tau_1..tau_L] by the moment recursion above: Objective.loglik_fisher_markov_batch's
    row.  It depends on the fluxes through the offsets' prior variances only (not at all without marginalise_b), and is positive
    semi-definite at any point.  Each pair is computed once and mirrored; pairs (a list of (a, b)) restricts the work to those entries
    and leaves the others NaN.  grad and fisher are NaN where info != 0.  On an OU row with a cross-band tie in shifted time every entry
    with a tau index is NaN and info stays 0; with one band the tau entries are exact zeros.
    _slip (tests only) injects one mistake: "no_innov" (the E[eps_a eps_b] / S term left out), "prior_moment" (Z = Pi instead of Pi - P),
    "no_gain_tangent" (the S g_a terms of the moments' update left out), "no_dh_moment" (h_a, h_b left out of u, v and w), "tau_one_lag"
    (only the lag before a point of band l is differentiated, not the one after)."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b,
                                                                       codes_first=True)
    W = 2 * L + 1
    ll, grad, info = loglik_grad(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b)
    fisher = np.full((W, W), math.nan)
    if info:
        return ll, grad, fisher, info
    todo = [(a, b) for a in range(W) for b in range(a, W)] if pairs is None else sorted({(min(a, b), max(a, b)) for a, b in pairs})
    for a, b in todo:
        if not (0 <= a and b < W):
            raise ValueError("pair (%d, %d) outside 0..%d" % (a, b, W - 1))
        fisher[a, b] = fisher[b, a] = _fisher_pass(name, train, alpha, rho, p, n, vb, a, b, slip=_slip)
    return ll, grad, fisher, 0


def loglik_fisher_batch(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True, pairs=None):
    """loglik_fisher over M rows -> (loglik[M], grad[M, 2L+1], fisher[M, 2L+1, 2L+1], info[M]): Objective.loglik_fisher_markov_batch's shape."""
    L = len(tarray)
    W = 2 * L + 1
    delays = np.asarray(delays, np.float64).reshape(-1, L)
    alpha = np.asarray(alpha, np.float64).reshape(-1, L)
    rho = np.asarray(rho, np.float64).reshape(-1)
    out = [loglik_fisher(kernel, tarray, yarray, stdarray, delays[i], alpha[i], rho[i], marginalise_b, pairs) for i in range(len(rho))]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]).reshape(-1, W),
            np.array([o[2] for o in out]).reshape(-1, W, W), np.array([o[3] for o in out], dtype=np.int32))


JITTER = 1e-8   # added to every predictive variance and to sigma*^2 of a held-out point (gpcc_predict_batch's constant)


# ----------------------------------------------------------------------------------------------------------------------------------
# Linear-time predictions, held-out log-likelihoods and the offsets' posterior (csrc/gpcc_markov_pred.hip.h), the same
# algorithm in numpy.
#
#   predict   two filters and a combine.  The process is stationary, so reversed in time it is the same process with the odd
#             derivative negated: the identical filter over the points in DESCENDING shifted time with lags |d|, its state mapped by
#             D = diag(1, -1, 1)[:p] (+) I.  For a test point at s* = t* - tau_band: (m_f, P_f) = the forward filter after the training
#             points with s <= s*, propagated to s*; (m_b, P_b) = the backward filter after those with s > s*, propagated to s* (a
#             training point that ties with the test point is on the forward side only).  With P0 = blockdiag(Pinf, diag Sigma_b):
#             P_s = (P_f^-1 + P_b^-1 - P0^-1)^-1, m_s = P_s (P_f^-1 m_f + P_b^-1 m_b), mu* = h'm_s + mean(y_band), var* = h'P_s h +
#             JITTER; everything scaled by diag(P0)^-1/2 before the inversions.  The propagation works on a copy: the filter's own
#             chain is not split at test points, so the training log-likelihood is loglik()'s.
#   heldout   log p(y* | Y) = loglik(training U test) - loglik(training): the test points enter as observations with variance
#             sigma*^2 + JITTER and residual y* - mean(y_band of the TRAINING data); the offsets' priors from the training data.
#   postb     the offset block of the forward filter's final state: mu = m[p:] + mean(y_band), Sigma = P[p:, p:].
#
# _setup, _prior, _propagate and _pass are the module's one filter: loglik() above is _setup + _pass over the training points alone.
# ----------------------------------------------------------------------------------------------------------------------------------
def _prior(name, rho, p, n, vb):
    P0 = np.zeros((n, n))
    P0[:p, :p] = stationary(name, rho)
    for l in range(n - p):
        P0[p + l, p + l] = vb[l]
    return P0


def _propagate(name, m, P, Pinf, d, rho, p, no_q=False):
    """The state (m, P) a lag d later, on copies: m <- A m, P_xx <- A (P_xx - Pinf) A' + Pinf, P_xb <- A P_xb."""
    A = transition(name, d, rho)
    m = m.copy()
    P = P.copy()
    m[:p] = A @ m[:p]
    P[:p, :p] = A @ P[:p, :p] @ A.T if no_q else A @ (P[:p, :p] - Pinf) @ A.T + Pinf
    P[:p, p:] = A @ P[:p, p:]
    P[p:, :p] = P[:p, p:].T
    return m, P


def _pass(name, train, tests, alpha, rho, p, n, vb, reverse=False, tests_update=False, ties_first=False, slip=None):
    """One filter over the training observations `train` [(s, band, position, r, sigma^2)] and the test points `tests` [(s, band, index,
    r, sigma^2)].  reverse: descending s.  tests_update: the test points are observations too (held-out union) -- otherwise each is
    tapped: the state after the training points before it, propagated to it, kept in taps[index] (unflipped).  Ties in s: training
    points before test points going forward (or with ties_first), test points first going backward.  Among themselves the training
    points come by shifted time, then band, then position in the band: merge_order()'s order, which the device walks.  slip: loglik()'s.
    -> (loglik, info, final mean, final covariance, taps, index of the test point at which info was set or -1)."""
    sg = -1.0 if reverse else 1.0
    tr_kind = 0 if (not reverse or ties_first or tests_update) else 1
    ev = [(sg * s, tr_kind, b, sg * i, True, r, s2, i) for (s, b, i, r, s2) in train]
    ev += [(sg * s, 1 - tr_kind if not tests_update else 1, b, sg * i, False, r, s2, i) for (s, b, i, r, s2) in tests]
    ev.sort(key=lambda e: e[:4])
    if slip == "order":
        for j in range(len(ev) // 2, len(ev) - 1):
            if ev[j][0] != ev[j + 1][0]:
                ev[j], ev[j + 1] = ev[j + 1], ev[j]
                break
    Pinf = stationary(name, rho)
    P = _prior(name, rho, p, n, vb)
    m = np.zeros(n)
    ll, info, at, sprev, step, taps = 0.0, 0, -1, None, 0, {}
    for (key, _, b, _, is_train, r, s2, i) in ev:
        d = 0.0 if sprev is None else key - sprev
        if not is_train and not tests_update:
            taps[i] = _propagate(name, m, P, Pinf, d, rho, p)
            continue
        sprev = key
        step += 1
        m, P = _propagate(name, m, P, Pinf, d, rho, p, no_q=(slip == "no_q"))
        h = np.zeros(n)
        h[0] = alpha[b]
        if n > p and slip != "no_offset":
            h[p + b] = 1.0
        Ph = P @ h
        S = h @ Ph + s2
        if not (S > 0.0 and math.isfinite(S)):
            if info == 0:
                info, at = step, (-1 if is_train else i)
            return math.nan, info, m, P, taps, at
        eps = r - h @ m
        ll -= 0.5 * (LOG2PI + math.log(S) + eps * eps / S)
        m = m + Ph * (eps / S)
        P = P - np.outer(Ph, Ph) / S
        P = 0.5 * (P + P.T)
    return ll, info, m, P, taps, at


def _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b, codes_first=False):
    """The arguments as arrays, the argument code (-1: some alpha <= 0, -2: rho <= 0, else 0), what prepare() gives and the training
    observations for _pass.  More offset states than the device keeps raise, except (codes_first: loglik's precedence) beside a code."""
    name = _name(kernel)
    L = len(tarray)
    delays = np.asarray(delays, np.float64).reshape(L)
    alpha = np.asarray(alpha, np.float64).reshape(L)
    rho = float(rho)
    code = -1 if not np.all(alpha > 0.0) else (-2 if rho <= 0.0 else 0)
    if marginalise_b and L > MAX_OFFSET_BANDS and not (codes_first and code):
        raise ValueError("marginalise_b with %d bands: the linear-time solver keeps at most %d offset states" % (L, MAX_OFFSET_BANDS))
    ts, rs, s2, vb = prepare(tarray, yarray, stdarray, marginalise_b)
    means = np.array([np.asarray(y, np.float64).sum() / len(y) for y in yarray])
    p = _ORDER[name]
    n = p + (L if marginalise_b else 0)
    train = [(ts[l][i] - delays[l], l, i, rs[l][i], s2[l][i]) for l in range(L) for i in range(len(ts[l]))]
    return name, L, delays, alpha, rho, code, vb, means, p, n, train


def _spd_inverse(A):
    """inv(A) by Cholesky; None where a pivot is not positive and finite."""
    n = len(A)
    Lc = np.zeros((n, n))
    for j in range(n):
        d = A[j, j] - Lc[j, :j] @ Lc[j, :j]
        if not (d > 0.0 and math.isfinite(d)):
            return None
        Lc[j, j] = math.sqrt(d)
        for i in range(j + 1, n):
            Lc[i, j] = (A[i, j] - Lc[i, :j] @ Lc[j, :j]) / Lc[j, j]
    Li = np.linalg.solve(Lc, np.eye(n))
    return Li.T @ Li


def _test_list(L, ttest, delays):
    """The test points for _pass [(s*, band, index in the caller's flattened order, 0, 0)] and their bands."""
    tests, band_of = [], []
    for l in range(L):
        for v in np.asarray(ttest[l], np.float64).reshape(-1):
            tests.append((v - delays[l], l, len(tests), 0.0, 0.0))
            band_of.append(l)
    return tests, band_of


def _smooth(name, train, tests, band_of, alpha, rho, p, n, vb, slip=None):
    """Two filters over `train` and the combine at the test points -> (h'm_s[T], h'P_s h[T], loglik, info): predict()'s mean without the
    band mean and variance without JITTER.  Linear in the residuals of `train`; its covariances do not depend on them."""
    T, N = len(tests), len(train)
    nan = np.full(T, math.nan)
    ll, info, _, _, fw, _ = _pass(name, train, tests, alpha, rho, p, n, vb)
    if info:
        return nan, nan.copy(), math.nan, info
    _, _, _, _, bw, _ = _pass(name, train, tests, alpha, rho, p, n, vb, reverse=True, ties_first=(slip == "tie_both"))
    P0 = _prior(name, rho, p, n, vb)
    sc = 1.0 / np.sqrt(np.diag(P0))
    I0 = np.linalg.inv(sc[:, None] * P0 * sc[None, :])
    D = np.ones(n)
    if p >= 2 and slip != "no_flip":
        D[1] = -1.0
    mu, var = np.empty(T), np.empty(T)
    for j in range(T):
        mf, Pf = fw[j]
        mb, Pb = bw[j]
        mb, Pb = D * mb, D[:, None] * Pb * D[None, :]
        If = _spd_inverse(sc[:, None] * Pf * sc[None, :])
        Ib = _spd_inverse(sc[:, None] * Pb * sc[None, :])
        Ps = None
        if If is not None and Ib is not None:
            Ps = _spd_inverse(If + Ib - (0.0 if slip == "no_prior" else I0))
        if Ps is None:
            return nan, nan.copy(), ll, N + j + 1
        ms = Ps @ (If @ (sc * mf) + Ib @ (sc * mb))
        h = np.zeros(n)
        h[0] = alpha[band_of[j]]
        if n > p:
            h[p + band_of[j]] = 1.0
        h = h / sc
        mu[j] = h @ ms
        var[j] = h @ Ps @ h
    return mu, var, ll, 0


def _noise_apply(L, train, code, noise):
    """What a noise model does to _setup's results.  noise: None (nothing: the plain functions), or (kappa, nu, slip) of predict_noise
    and its siblings -> (the training observations on the mapped variances, _noise_train's; the code, -3 after -1 and -2; kappa^2 and
    the excess variance per band as the pass sees them, or None).  slip (tests only): "kappa_linear" (kappa sigma^2 + nu),
    "noise_all_bands" (every band under band 1's model)."""
    if noise is None:
        return train, code, None, None
    kappa, nu, ncode = _noise_setup(L, noise[0], noise[1])
    if code or ncode:
        return train, code or ncode, None, None
    if noise[2] == "kappa_linear":
        kappa = np.sqrt(kappa)
    if noise[2] == "noise_all_bands":
        kappa, nu = np.full(L, kappa[0]), np.full(L, nu[0])
    return [e[:5] for e in _noise_train(train, kappa, nu)], 0, kappa * kappa, nu


def predict(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, marginalise_b=True, _slip=None, _noise=None):
    """(mu[T], var[T], loglik, info) of one (tau, alpha, rho) at the test times ttest (a list of L arrays, any order; T = their total,
    flattened in band order): predictTest's per-band mean and variance (JITTER included) by two filters and a combine, and the training
    log-likelihood.  info: loglik()'s codes for the training filter (mu and var NaN then), else N + j for the first test point j
    (1-based, flattened order) whose combine meets a pivot that is not positive and finite (mu and var NaN), else 0.
    _slip (tests only): "no_flip" (D left out on the backward side), "tie_both" (a training point that ties with a test point used on
    both sides), "no_prior" (-P0^-1 dropped), "no_jitter"."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b)
    train, code, _, _ = _noise_apply(L, train, code, _noise)
    tests, band_of = _test_list(L, ttest, delays)
    if code:
        nan = np.full(len(tests), math.nan)
        return nan, nan.copy(), math.nan, code
    mu, var, ll, info = _smooth(name, train, tests, band_of, alpha, rho, p, n, vb, _slip)
    if info:
        return mu, var, ll, info
    return mu + means[band_of], var + (0.0 if _slip == "no_jitter" else JITTER), ll, 0


def heldout(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, ytest, sigmatest, marginalise_b=True, _slip=None, _noise=None):
    """(heldout, loglik, info) of one (tau, alpha, rho): log p(ytest | training) = loglik(training U test) - loglik(training), the
    reference's predictTest(ttest, ytest, sigmatest).  info: loglik()'s codes for the training filter, else N + j for the first test
    point j (1-based, flattened band order) whose predictive variance in the union filter is not positive and finite (heldout NaN).
    _slip (tests only): "no_jitter", "test_mean" (test residuals centred on the test set's own band means)."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b)
    train, code, k2, ex = _noise_apply(L, train, code, _noise)
    if code:
        return math.nan, math.nan, code
    if k2 is None or _noise[2] == "heldout_raw_sigmatest":
        k2, ex = np.ones(L), np.zeros(L)
    jit = 0.0 if _slip == "no_jitter" else JITTER
    tests = []
    for l in range(L):
        tt, yt, st = (np.asarray(a[l], np.float64).reshape(-1) for a in (ttest, ytest, sigmatest))
        centre = (yt.sum() / len(yt) if len(yt) else 0.0) if _slip == "test_mean" else means[l]
        for v, yv, sv in zip(tt, yt, st):
            tests.append((v - delays[l], l, len(tests), yv - centre, k2[l] * (sv * sv) + ex[l] + jit))
    ll, info, _, _, _, _ = _pass(name, train, [], alpha, rho, p, n, vb)
    if info:
        return math.nan, math.nan, info
    lu, uinfo, _, _, _, at = _pass(name, train, tests, alpha, rho, p, n, vb, tests_update=True)
    if uinfo:
        return math.nan, ll, len(train) + max(at, 0) + 1
    return lu - ll, ll, 0


def posterior_offsets(kernel, tarray, yarray, stdarray, delays, alpha, rho, _noise=None):
    """(mu_postb[L], Sigma_postb[L, L], loglik, info) of one (tau, alpha, rho) with marginalised offsets: the offset block of the
    forward filter's final state (marginaliseb.jl:244-250), NaN where the training filter fails."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, True)
    train, code, _, _ = _noise_apply(L, train, code, _noise)
    if code:
        return np.full(L, math.nan), np.full((L, L), math.nan), math.nan, code
    ll, info, m, P, _, _ = _pass(name, train, [], alpha, rho, p, n, vb)
    if info:
        return np.full(L, math.nan), np.full((L, L), math.nan), math.nan, info
    return m[p:] + means, P[p:, p:].copy(), ll, 0


# ----------------------------------------------------------------------------------------------------------------------------------
# Joint posterior draws in linear time (csrc/gpcc_markov_sample.hip.h), the same algorithm in numpy: Matheron's rule.
#
#   prior     the training and test points merged in ascending shifted time (training first on ties); the state x~ is simulated along
#             them: x~ = C(inf) xi at the first point, then x~ <- A(d) x~ + C xi, C C' = Q(d) = Pinf - A Pinf A' (_sim_factor: the
#             triangular factor of Q scaled by diag(Pinf)^-1/2 and evaluated without cancellation, process_noise_scaled; d = 0
#             gives Q = 0 and tied points share one state); offsets b~_l = sqrt(Sigma_b_l) xi.  Synthetic residual r~_i = alpha x~_1(s_i) + b~ + sigma_i xi,
#             prior value g~_j = alpha x~_1(s*_j) + b~
#   correct   c = _smooth() of r~ in place of r (no band mean): linear in r~
#   draw      f*_j = mu_j + g~_j - c_j + sqrt(JITTER + sigma*_j^2) xi  ~  N(mu_pred, Sigma_pred + JITTER I + diag sigma*^2)
#   normals   one block of four per POINT (rng.point_normals: training point e in gpcc_create's order, then test point j in the
#             caller's order, then the offsets): the first p drive the state into that point, the fourth is its noise
# ----------------------------------------------------------------------------------------------------------------------------------
SIM_SERIES_MAX = 1.0      # csrc/gpcc_markov_sample.hip.h: GPCC_MKS_SERIES_MAX, the largest x = lambda d that takes the series
SIM_SERIES_TERMS = 26     # ... GPCC_MKS_SERIES_TERMS: the tail after 26 terms at y = 2 is below 1e-20 of the sum


def _lower_gammas(K, y):
    """gamma(k + 1, y) = int_0^y v^k e^-v dv for k = 0 .. K without cancellation: the top one by the all-positive series
    y^(K+1) e^-y sum_m y^m / ((K + 1) ... (K + 1 + m)), the others by gamma(k, y) = (gamma(k + 1, y) + y^k e^-y) / k, a sum of positives."""
    e = math.exp(-y)
    term = 1.0 / (K + 1)
    acc = term
    for m in range(1, SIM_SERIES_TERMS):
        term = term * y / (K + 1 + m)
        acc += term
    g = [0.0] * (K + 1)
    g[K] = y ** (K + 1) * e * acc
    for k in range(K, 0, -1):
        g[k - 1] = (g[k] + y ** k * e) / k
    return g


def process_noise_scaled(kernel, d, rho):
    """Q(d) = Pinf - A(d) Pinf A(d)' in the units of diag(Pinf)^1/2.  Formed that way it is a cancellation from a unit diagonal: at a
    small lag x = lambda d its diagonal is ~x^5, x^3, x (Matern-5/2) and drowns in the rounding of A.  For x <= SIM_SERIES_MAX it is
    evaluated as what it is, Q = q int_0^d a(s) a(s)' ds with a(s) the last column of A(s) (the white noise enters the highest
    derivative; q = 2 lambda, 4 lambda^3, 16 lambda^5 / 3): scaled and with u = lambda s,
        OU           1 - e^-2x
        Matern-3/2   4 int b b' e^-2u du,        b = (u, 1 - u)
        Matern-5/2   16/3 int b b' e^-2u du,     b = (u^2 / 2, sqrt3 u (1 - u / 2), 1 - 2u + u^2 / 2)
    over 0 .. x, every integral int u^k e^-2u du = gamma(k + 1, 2x) / 2^(k+1) from _lower_gammas: each entry to a few eps of
    sqrt(Q_ii Q_jj).  Beyond, where Q is of the order of Pinf, by the difference."""
    name = _name(kernel)
    lam = rate(name, rho)
    x = lam * d
    if not x <= SIM_SERIES_MAX:
        Pinf = stationary(name, rho)
        A = transition(name, d, rho)
        sc = 1.0 / np.sqrt(np.diag(Pinf))
        Q = Pinf - A @ Pinf @ A.T
        return sc[:, None] * (0.5 * (Q + Q.T)) * sc[None, :]
    if name == "OU":
        return np.array([[-math.expm1(-2.0 * x)]])
    if name == "matern32":
        j = [g / 2.0 ** (k + 1) for k, g in enumerate(_lower_gammas(2, 2.0 * x))]
        q01 = 4.0 * (j[1] - j[2])
        return np.array([[4.0 * j[2], q01], [q01, 4.0 * (j[0] - 2.0 * j[1] + j[2])]])
    j = [g / 2.0 ** (k + 1) for k, g in enumerate(_lower_gammas(4, 2.0 * x))]
    c, s3 = 16.0 / 3.0, math.sqrt(3.0)
    q01 = c * (0.5 * s3) * (j[3] - 0.5 * j[4])
    q02 = c * (0.5 * j[2] - j[3] + 0.25 * j[4])
    q12 = c * s3 * (j[1] - 2.5 * j[2] + 1.5 * j[3] - 0.25 * j[4])
    return np.array([[c * 0.25 * j[4], q01, q02], [q01, c * 3.0 * (j[2] - j[3] + 0.25 * j[4]), q12],
                     [q02, q12, c * (j[0] - 4.0 * j[1] + 5.0 * j[2] - 2.0 * j[3] + 0.25 * j[4])]])


def _sim_factor(kernel, d, rho, _by_difference=False):
    """C with C C' = Q(d) (d None: Pinf, the stationary draw): the triangular factor of process_noise_scaled(), eliminated from the last
    component (the largest pivot) to the first, so C is upper triangular; a pivot that is not > 0 gives a zero column.  d = 0 gives
    C = 0: tied points share one state.  _by_difference (tests only): Q by the difference at every lag."""
    name = _name(kernel)
    Pinf = stationary(name, rho)
    p = len(Pinf)
    sc = 1.0 / np.sqrt(np.diag(Pinf))
    if d is None:
        Q = sc[:, None] * Pinf * sc[None, :]
    elif _by_difference:
        A = transition(name, d, rho)
        Q = Pinf - A @ Pinf @ A.T
        Q = sc[:, None] * (0.5 * (Q + Q.T)) * sc[None, :]
    else:
        Q = process_noise_scaled(name, d, rho)
    G = np.zeros((p, p))
    for j in range(p - 1, -1, -1):
        dj = Q[j, j] - sum(G[j, k] * G[j, k] for k in range(j + 1, p))
        if not (dj > 0.0 and math.isfinite(dj)):
            continue
        G[j, j] = math.sqrt(dj)
        for i in range(j):
            G[i, j] = (Q[i, j] - sum(G[i, k] * G[j, k] for k in range(j + 1, p))) / G[j, j]
    return G / sc[:, None]


def _draw_setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, sigmatest, marginalise_b, noise=None):
    """noise: None, or (kappa, nu, slip) of sample_noise (predict()'s _noise) -> `train` on the mapped variances, rv, the variance the
    synthetic residual's noise of training point (band, position) is drawn with (the filter's), and tv, the test noise's variance
    without JITTER: sigma*^2, mapped under a noise model, where sigmatest is given, zero (the latent curve: nu is not added) where it is
    None.  slip (tests only): _noise_apply's, and "draw_obs_noise_raw" (rv keeps sigma_i^2), "draw_test_noise_raw" (tv keeps sigma*^2)."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b)
    raw = train
    train, code, k2, ex = _noise_apply(L, train, code, noise)
    rv = {(e[1], e[2]): e[4] for e in (raw if noise is not None and noise[2] == "draw_obs_noise_raw" else train)}
    tests, band_of = _test_list(L, ttest, delays)
    # sorted position i of band l -> the point's index in gpcc_create's flattened order
    orig, off = {}, 0
    for l in range(L):
        perm = np.argsort(np.asarray(tarray[l], np.float64), kind="stable")
        for i, q in enumerate(perm):
            orig[(l, i)] = off + int(q)
        off += len(perm)
    if sigmatest is None:
        tv = np.zeros(len(tests))
    else:
        st = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in sigmatest]) if len(tests) else np.zeros(0)
        tv = st * st
        if k2 is not None and noise[2] != "draw_test_noise_raw":
            tv = k2[band_of] * tv + ex[band_of]
    return name, L, delays, alpha, rho, code, vb, means, p, n, train, tests, band_of, orig, tv, rv


def _prior_draw(name, alpha, rho, vb, p, n, train, tests, orig, tv, rv, xi, slip=None):
    """One prior draw from the normals xi (N + T + 1, 4) -> (r~ per entry of `train`, g~[T], noise[T]); tv, rv: _draw_setup's."""
    N, T = len(train), len(tests)
    ev = [(s, 0, b, i, True) for (s, b, i, _, _) in train] + [(s, 1, b, i, False) for (s, b, i, _, _) in tests]
    ev.sort(key=lambda e: e[:4])
    bt = np.zeros(len(alpha))
    if n > p and slip != "no_offset_draw":
        bt = np.sqrt(vb) * xi[N + T, :len(alpha)]
    rt, gt, noise = {}, np.empty(T), np.empty(T)
    x, sprev = None, None
    for pos, (s, _, b, i, is_train) in enumerate(ev):
        e = pos if slip == "merged_index" else (orig[(b, i)] if is_train else N + i)
        z = xi[e]
        if x is None:
            x = _sim_factor(name, None, rho) @ z[:p]
        else:
            x = transition(name, s - sprev, rho) @ x + _sim_factor(name, s - sprev, rho, slip == "q_by_difference") @ z[:p]
        sprev = s
        f = alpha[b] * x[0] + bt[b]
        if is_train:
            rt[(b, i)] = f + (0.0 if slip == "no_obs_noise" else math.sqrt(rv[(b, i)]) * z[3])
        else:
            gt[i] = f
            noise[i] = math.sqrt(JITTER + tv[i]) * z[3]
    return rt, gt, noise


def _normals_of(N, T, seed, s, m, normals):
    if normals is not None:
        xi = np.asarray(normals, np.float64)
        if xi.shape != (N + T + 1, 4):
            raise ValueError("normals must have shape (N + T + 1, 4) = (%d, 4)" % (N + T + 1))
        return xi
    from . import rng
    return rng.point_normals(seed, N + T + 1, [s], [m])[0]


def prior_draw(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, sigmatest=None, marginalise_b=True, seed=0, s=0, m=0,
               normals=None, _slip=None, _noise=None):
    """Step 1 of a linear-time draw -> (r~[N] in gpcc_create's flattened order, g~[T], noise[T] in the caller's flattened order): a draw
    of the prior at the training and test points, the synthetic residuals with their observation noise, and the JITTER / sigma* noise of
    the test points.  The normals are draw s of row m of `seed` (rng.point_normals; m = rng.MIXROW for a mixture draw) or `normals`,
    an array (N + T + 1, 4).  _slip (tests only): "no_obs_noise", "no_offset_draw", "merged_index", "q_by_difference" (_sim_factor's).
    _noise: predict()'s (kappa, nu, slip): the noises of r~ and of the test points under that model (_draw_setup)."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train, tests, band_of, orig, tv, rv = _draw_setup(
        kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, sigmatest, marginalise_b, _noise)
    if code:
        raise ValueError("prior_draw: alpha and rho must be positive, kappa and nu not negative")
    xi = _normals_of(len(train), len(tests), seed, s, m, normals)
    rt, gt, noise = _prior_draw(name, alpha, rho, vb, p, n, train, tests, orig, tv, rv, xi, _slip)
    out = np.empty(len(train))
    for key, v in rt.items():
        out[orig[key]] = v
    return out, gt, noise


def sample(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, sigmatest=None, marginalise_b=True, seed=0, s=0, m=0,
           normals=None, _slip=None, _noise=None):
    """(draw[T], loglik, info) of one (tau, alpha, rho): one joint posterior draw at the test times, distributed as
    N(mu_pred, Sigma_pred + JITTER I + diag sigmatest^2) -- gpcc_sample_batch's distribution -- by Matheron's rule: predict()'s mean
    plus a prior draw minus the smoother of the prior draw's synthetic data, plus the test noise.  loglik and info are predict()'s; a
    failed row's draw is NaN.  Normals as prior_draw.  _slip (tests only): predict()'s "no_flip", "tie_both", "no_prior" (in both the
    mean and the correction), prior_draw's, and "plus" (the correction added).  _noise: predict()'s (kappa, nu, slip) -- sample_noise."""
    name, L, delays, alpha, rho, code, vb, means, p, n, train, tests, band_of, orig, tv, rv = _draw_setup(
        kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, sigmatest, marginalise_b, _noise)
    T = len(tests)
    if code:
        return np.full(T, math.nan), math.nan, code
    pslip = _slip if _slip in ("no_flip", "tie_both", "no_prior") else None
    mu, _, ll, info = _smooth(name, train, tests, band_of, alpha, rho, p, n, vb, pslip)
    if info:
        return np.full(T, math.nan), ll, info
    xi = _normals_of(len(train), T, seed, s, m, normals)
    rt, gt, noise = _prior_draw(name, alpha, rho, vb, p, n, train, tests, orig, tv, rv, xi, _slip)
    synth = [(sv, b, i, rt[(b, i)], v) for (sv, b, i, _, v) in train]
    c, _, _, cinfo = _smooth(name, synth, tests, band_of, alpha, rho, p, n, vb, pslip)
    if cinfo:
        return np.full(T, math.nan), ll, cinfo
    return mu + means[band_of] + gt + (c if _slip == "plus" else -c) + noise, ll, 0


# ----------------------------------------------------------------------------------------------------------------------------------
# Exact leave-one-out predictive scores in linear time (csrc/gpcc_markov_loo.hip.h), the same algorithm in numpy.
#
#   taps      the forward filter walks the training points in merge_order()'s order (shifted time, then band, then position); at point i
#             the state propagated to s_i BEFORE the update with point i is kept.  The backward filter walks exactly the reverse order
#             (lags |d|) and keeps the same: every other point, tied with i or not, is then on exactly one side of i.
#   combine   predict()'s: P_s = (P_f^-1 + P_b^-1 - P0^-1)^-1, m_s = P_s (P_f^-1 m_f + P_b^-1 m_b), scaled by diag(P0)^-1/2, the
#             backward state mapped by D; with h of the point's band
#                 mu_i = h'm_s + mean(y_band),  var_i = h'P_s h + sigma_i^2,  lp_i = -(log 2 pi + log var_i + (y_i - mu_i)^2 / var_i) / 2
#             (no JITTER: p(y_i | y_-i) of the model the likelihood uses), reported in the caller's order.
#   mixture   with alpha and rho fixed per delay the exact LOO density of the delay mixture is the weighted HARMONIC mean of the rows'
#             densities: mix_lp_i = -log sum_m p_m exp(-lp_mi) (loo_mix).
# ----------------------------------------------------------------------------------------------------------------------------------
def _loo_taps(name, ev, alpha, rho, p, n, vb, reverse, after_update=False):
    """One filter over the events `ev` [(s, band, position, r, sigma^2)] in the order given (reverse: descending s, lags |d|) ->
    (loglik, info, {(band, position): (m, P) at the point before its update (after_update: after it)})."""
    Pinf = stationary(name, rho)
    P = _prior(name, rho, p, n, vb)
    m = np.zeros(n)
    ll, info, sprev, taps = 0.0, 0, None, {}
    for step, (s, b, i, r, s2) in enumerate(ev):
        d = 0.0 if sprev is None else (sprev - s if reverse else s - sprev)
        sprev = s
        m, P = _propagate(name, m, P, Pinf, d, rho, p)
        if not after_update:
            taps[(b, i)] = (m.copy(), P.copy())
        h = np.zeros(n)
        h[0] = alpha[b]
        if n > p:
            h[p + b] = 1.0
        Ph = P @ h
        S = h @ Ph + s2
        if not (S > 0.0 and math.isfinite(S)):
            return math.nan, step + 1, taps
        eps = r - h @ m
        ll -= 0.5 * (LOG2PI + math.log(S) + eps * eps / S)
        m = m + Ph * (eps / S)
        P = P - np.outer(Ph, Ph) / S
        P = 0.5 * (P + P.T)
        if after_update:
            taps[(b, i)] = (m.copy(), P.copy())
    return ll, info, taps


LOO_SLIPS = ("with_self", "tie_both", "no_sigma", "jitter", "sorted_order", "arith_mix")


def loo(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True, _slip=None, _noise=None):
    """(mu[N], var[N], lp[N], loo, loglik, info) of one (tau, alpha, rho): mean, variance and log-density of y_i given every other
    observation and their sum, Objective.loo_markov_batch's row, in the caller's order (band 1 as given, then band 2, ...).  info:
    loglik()'s codes for the filter, else N + i for the first point i (1-based, the caller's order) whose combine meets a pivot, or
    whose variance is, not positive and finite (mu, var, lp and loo NaN then, loglik valid), else 0.
    _slip (tests only) injects one mistake: "with_self" (the forward state AFTER the update with point i: the point is not left out),
    "tie_both" (the backward walk keeps the forward order among points that tie in shifted time, so a tied point is counted on both
    sides or on neither), "no_sigma" (the variance of the noiseless curve, without sigma_i^2), "jitter" (predictTest's 1e-8 added),
    "sorted_order" (outputs left in the order of the bands sorted by time); "arith_mix" acts in loo_mix()."""
    if _slip is not None and _slip not in LOO_SLIPS:
        raise ValueError("unknown slip %r" % (_slip,))
    name, L, delays, alpha, rho, code, vb, means, p, n, train = _setup(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b)
    raw = {(e[1], e[2]): e[4] for e in train}      # the reported sigma^2 (a noise model's slip "loo_var_raw" adds it in the combine)
    train, code, _, _ = _noise_apply(L, train, code, _noise)
    N = len(train)
    nan = np.full(N, math.nan)
    if code:
        return nan, nan.copy(), nan.copy(), math.nan, math.nan, code
    fwd = sorted(train, key=lambda e: e[:3])
    ll, info, fw = _loo_taps(name, fwd, alpha, rho, p, n, vb, False, after_update=(_slip == "with_self"))
    if info:
        return nan, nan.copy(), nan.copy(), math.nan, math.nan, info
    bwd = sorted(train, key=lambda e: (-e[0], e[1], e[2])) if _slip == "tie_both" else fwd[::-1]
    _, _, bw = _loo_taps(name, bwd, alpha, rho, p, n, vb, True)
    P0 = _prior(name, rho, p, n, vb)
    sc = 1.0 / np.sqrt(np.diag(P0))
    I0 = np.linalg.inv(sc[:, None] * P0 * sc[None, :])
    D = np.ones(n)
    if p >= 2:
        D[1] = -1.0
    # the caller's position of sorted point (band, position)
    off = np.concatenate([[0], np.cumsum([len(t) for t in tarray])])
    perms = [np.argsort(np.asarray(t, np.float64), kind="stable") for t in tarray]
    mu, var, lp = nan.copy(), nan.copy(), nan.copy()
    bad = N
    for (s, b, i, r, s2) in train:
        if _noise is not None and _noise[2] == "loo_var_raw":
            s2 = raw[(b, i)]
        o = int(off[b] + (i if _slip == "sorted_order" else perms[b][i]))
        Ps = None
        if (b, i) in bw:
            mf, Pf = fw[(b, i)]
            mb, Pb = bw[(b, i)]
            mb, Pb = D * mb, D[:, None] * Pb * D[None, :]
            If = _spd_inverse(sc[:, None] * Pf * sc[None, :])
            Ib = _spd_inverse(sc[:, None] * Pb * sc[None, :])
            if If is not None and Ib is not None:
                Ps = _spd_inverse(If + Ib - I0)
        v = math.nan
        if Ps is not None:
            ms = Ps @ (If @ (sc * mf) + Ib @ (sc * mb))
            h = np.zeros(n)
            h[0] = alpha[b]
            if n > p:
                h[p + b] = 1.0
            h = h / sc
            mean = h @ ms
            v = h @ Ps @ h + (0.0 if _slip == "no_sigma" else s2) + (JITTER if _slip == "jitter" else 0.0)
        if not (v > 0.0 and math.isfinite(v) and mean == mean):
            bad = min(bad, o)
            continue
        e = r - mean
        mu[o], var[o], lp[o] = mean + means[b], v, -0.5 * (LOG2PI + math.log(v) + e * e / v)
    if bad < N:
        return nan, nan.copy(), nan.copy(), math.nan, ll, N + bad + 1
    return mu, var, lp, float(np.sum(lp)), ll, 0


def loo_mix(lp, weights, _slip=None):
    """(mix_lp[N], mix_loo) of the rows' lp[M, N]: mix_lp_i = -log sum_m p_m exp(-lp_mi), p = w / sum w, the device's running
    max-shifted log-sum-exp per point in row order (zero-weight rows skipped; a failed row with weight makes it NaN; one row of weight 1
    returns its own bits), and mix_loo = sum_i mix_lp_i.  _slip "arith_mix": the arithmetic mean log sum_m p_m exp(lp_mi) instead."""
    lp = np.asarray(lp, np.float64)
    w = np.asarray(weights, np.float64)
    p = w / np.sum(w)
    sg = 1.0 if _slip == "arith_mix" else -1.0
    out = np.empty(lp.shape[1])
    for i in range(lp.shape[1]):
        mx, s, nan = -math.inf, 0.0, False
        for m_ in range(len(p)):
            if p[m_] == 0.0:
                continue
            x = sg * lp[m_, i]
            if x != x:
                nan = True
                continue
            lx = math.log(p[m_]) + x
            if lx == -math.inf:
                continue
            if s == 0.0:
                mx, s = lx, 1.0
            elif lx <= mx:
                s += math.exp(lx - mx)
            else:
                s = s * math.exp(mx - lx) + 1.0
                mx = lx
        out[i] = math.nan if nan else (sg * -math.inf if s == 0.0 else sg * (mx + math.log(s)))
    return out, float(np.sum(out))


def mix_moments(mu, var, weights):
    """The device's mixture over rows (gpcc_predict_batch's semantics): p = w / sum w, a running weighted mean and sum of squared
    deviations in row order; zero-weight rows skipped."""
    w = np.asarray(weights, np.float64)
    p = w / np.sum(w)
    T = np.shape(mu)[1]
    W, mean, S, V = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T)
    for m_ in range(len(p)):
        if p[m_] == 0.0:
            continue
        W = W + p[m_]
        d = mu[m_] - mean
        mean = mean + (p[m_] / W) * d
        S = S + p[m_] * d * (mu[m_] - mean)
        V = V + p[m_] * var[m_]
    return mean, (V + S) / W


def mix_logsumexp(values, weights):
    """log sum p_m exp(values_m), p = w / sum w, zero-weight rows skipped; NaN if a row with weight is NaN."""
    w = np.asarray(weights, np.float64)
    p = w / np.sum(w)
    keep = p > 0
    x = np.log(p[keep]) + np.asarray(values, np.float64)[keep]
    if np.any(np.isnan(x)):
        return math.nan
    mx = np.max(x)
    return float(mx + math.log(np.sum(np.exp(x - mx)))) if np.isfinite(mx) else float(mx)


# ----------------------------------------------------------------------------------------------------------------------------------
# Predictions, held-out scores, the offsets' posterior and leave-one-out scores under a noise model (csrc/gpcc_markov_noise_pred.hip.h,
# DESIGN.md 4.29), the same algorithm in numpy: predict(), heldout(), posterior_offsets() and loo() above, their passes unchanged, on
# _noise_train's mapped variances kappa_l^2 sigma_i^2 + nu_l (_noise_apply).  A held-out test point of band l has kappa_l^2 sigma*^2 +
# nu_l + JITTER; the leave-one-out variance adds the point's mapped variance.  At kappa = 1, nu = 0 these return the plain functions'
# numbers exactly.  Codes: the plain ones and, after -1 and -2, -3 (a kappa or nu negative or not finite).
# ----------------------------------------------------------------------------------------------------------------------------------
NOISE_PREDICT_SLIPS = ("heldout_raw_sigmatest", "loo_var_raw", "kappa_linear", "noise_all_bands")


def _noise_slip(slip):
    if slip is not None and slip not in NOISE_PREDICT_SLIPS:
        raise ValueError("unknown slip %r" % (slip,))
    return slip


def predict_noise(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, kappa=None, nu=None, marginalise_b=True, _slip=None):
    """predict() of one (tau, alpha, rho, kappa, nu): a row of Objective.predict_markov_noise_batch.  _slip (tests only): "kappa_linear"
    (the variance kappa sigma^2 + nu), "noise_all_bands" (every band under band 1's kappa, nu)."""
    return predict(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, marginalise_b, _noise=(kappa, nu, _noise_slip(_slip)))


def heldout_noise(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, ytest, sigmatest, kappa=None, nu=None, marginalise_b=True,
                  _slip=None):
    """heldout() of one (tau, alpha, rho, kappa, nu), the test error bars mapped by the same band's kappa, nu: a row of
    Objective.heldout_loglik_markov_noise_batch.  _slip (tests only): predict_noise's and "heldout_raw_sigmatest" (the test points keep
    sigma*^2)."""
    return heldout(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, ytest, sigmatest, marginalise_b,
                   _noise=(kappa, nu, _noise_slip(_slip)))


def posterior_offsets_noise(kernel, tarray, yarray, stdarray, delays, alpha, rho, kappa=None, nu=None, _slip=None):
    """posterior_offsets() of one (tau, alpha, rho, kappa, nu): a row of Objective.posterior_offsets_markov_noise_batch."""
    return posterior_offsets(kernel, tarray, yarray, stdarray, delays, alpha, rho, _noise=(kappa, nu, _noise_slip(_slip)))


def loo_noise(kernel, tarray, yarray, stdarray, delays, alpha, rho, kappa=None, nu=None, marginalise_b=True, _slip=None):
    """loo() of one (tau, alpha, rho, kappa, nu), var_i = h'P_s h + kappa_b^2 sigma_i^2 + nu_b: a row of
    Objective.loo_markov_noise_batch.  _slip (tests only): predict_noise's and "loo_var_raw" (the combine adds sigma_i^2 unmapped)."""
    return loo(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b, _noise=(kappa, nu, _noise_slip(_slip)))


# ----------------------------------------------------------------------------------------------------------------------------------
# Joint posterior draws under a noise model (csrc/gpcc_markov_noise_sample.hip.h), the same algorithm in numpy:
# prior_draw() and sample() above on _noise_train's mapped variances.  The synthetic residual's noise and the filter take the same
# v_i = kappa_l^2 sigma_i^2 + nu_l; with sigmatest a test point of band l has the noise variance JITTER + kappa_l^2 sigma*^2 + nu_l (a
# replicated observation under the fitted model), without it JITTER (the latent curve: nu is not added).  The normals are sample()'s.
# At kappa = 1, nu = 0 sample_noise returns sample()'s numbers exactly.
# ----------------------------------------------------------------------------------------------------------------------------------
NOISE_SAMPLE_SLIPS = ("draw_obs_noise_raw", "draw_test_noise_raw", "kappa_linear", "noise_all_bands")


def sample_noise(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, kappa=None, nu=None, sigmatest=None, marginalise_b=True,
                 seed=0, s=0, m=0, normals=None, _slip=None):
    """sample() of one (tau, alpha, rho, kappa, nu): a row of Objective.sample_markov_noise_batch -> (draw[T], loglik, info), info -3
    after -1 and -2.  _slip (tests only): "draw_obs_noise_raw" (the synthetic residual keeps sigma_i while the filter uses v_i),
    "draw_test_noise_raw" (the test noise keeps sigma*), "kappa_linear" (the variance kappa sigma^2 + nu), "noise_all_bands" (every band
    under band 1's kappa, nu)."""
    if _slip is not None and _slip not in NOISE_SAMPLE_SLIPS:
        raise ValueError("unknown slip %r" % (_slip,))
    return sample(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, sigmatest, marginalise_b, seed, s, m, normals,
                  _noise=(kappa, nu, _slip))


class MarkovObjective:
    """The CPU mirror with the methods gpcc_grid's `engine="python"` fit and the Markov predictors call (loglik_batch and
    loglik_markov_batch are the same filter here): gpcc_grid(..., objective=MarkovObjective(...), solver="markov") fits without a GPU."""

    def __init__(self, tarray, yarray, stdarray, kernel, marginalise_b=True):
        self.data = (tarray, yarray, stdarray)
        self.kernel, self.marginalise_b, self.L = _name(kernel), bool(marginalise_b), len(tarray)
        self.yflat = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in yarray])
        self.sflat = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in stdarray])

    def loglik_markov_batch(self, delays, alpha, rho):
        return loglik_batch(self.kernel, *self.data, delays, alpha, rho, self.marginalise_b)

    loglik_batch = loglik_markov_batch

    def loglik_markov_realisations(self, Y, delays, alpha, rho, center="own"):
        """Objective.loglik_markov_realisations' result: (loglik[M, R], info[M])."""
        if isinstance(center, str):
            if center not in ("own", "handle"):
                raise ValueError('center must be "own", "handle" or an (R, L) array')
            center = band_means(self.data[0], Y) if center == "own" else None
        return loglik_realisations(self.kernel, *self.data, Y, delays, alpha, rho, self.marginalise_b, mean=center)

    def loglik_markov_resampled(self, Y, delays, alpha, rho, real, counts=None, center="own", sigma_b="own"):
        """Objective.loglik_markov_resampled's result: (loglik[M], info[M])."""
        mean, vb = resample_arguments(self.data[0], Y, counts, center, sigma_b, self.marginalise_b)
        return loglik_resampled(self.kernel, *self.data, Y, counts, real, delays, alpha, rho, self.marginalise_b, mean=mean, sigma_b=vb)

    def loglik_grad_markov_resampled(self, Y, delays, alpha, rho, real, counts=None, center="own", sigma_b="own"):
        """Objective.loglik_grad_markov_resampled's result: (loglik[M], grad[M, 2L+1], info[M])."""
        mean, vb = resample_arguments(self.data[0], Y, counts, center, sigma_b, self.marginalise_b)
        return loglik_grad_resampled(self.kernel, *self.data, Y, counts, real, delays, alpha, rho, self.marginalise_b, mean=mean, sigma_b=vb)

    def loglik_markov_noise_batch(self, delays, alpha, rho, kappa=None, nu=None):
        """Objective.loglik_markov_noise_batch's result: (loglik[M], info[M])."""
        return loglik_noise_batch(self.kernel, *self.data, delays, alpha, rho, kappa, nu, self.marginalise_b)

    def loglik_grad_markov_noise_batch(self, delays, alpha, rho, kappa=None, nu=None):
        """Objective.loglik_grad_markov_noise_batch's result: (loglik[M], grad[M, 4L+1], info[M])."""
        return loglik_grad_noise_batch(self.kernel, *self.data, delays, alpha, rho, kappa, nu, self.marginalise_b)

    def loglik_hess_markov_noise_batch(self, delays, alpha, rho, kappa=None, nu=None):
        """Objective.loglik_hess_markov_noise_batch's result: (loglik[M], grad[M, 4L+1], hess[M, 3L+1, 3L+1], info[M])."""
        return loglik_hess_noise_batch(self.kernel, *self.data, delays, alpha, rho, kappa, nu, self.marginalise_b)

    def loglik_hess_full_markov_noise_batch(self, delays, alpha, rho, kappa=None, nu=None):
        """Objective.loglik_hess_full_markov_noise_batch's result: (loglik[M], grad[M, 4L+1], hess[M, 4L+1, 4L+1], info[M])."""
        return loglik_hess_full_noise_batch(self.kernel, *self.data, delays, alpha, rho, kappa, nu, self.marginalise_b)

    def loglik_hess_hyper_markov_batch(self, delays, alpha, rho):
        """Objective.loglik_hess_hyper_markov_batch's result: (loglik[M], grad[M, 2L+1], hess[M, L+1, L+1], info[M])."""
        return loglik_hess_hyper_batch(self.kernel, *self.data, delays, alpha, rho, self.marginalise_b)

    def loglik_hess_hyper_batch(self, delays, alpha, rho):
        """The same under the dense entry's name and shape (the Fisher information is loglik_fisher_markov_batch's: None here), so that
        laplace.laplace_evidence runs over this objective."""
        ll, grad, hess, info = self.loglik_hess_hyper_markov_batch(delays, alpha, rho)
        return ll, grad, hess, None, info

    def loglik_hess_markov_batch(self, delays, alpha, rho):
        """Objective.loglik_hess_markov_batch's result: (loglik[M], grad[M, 2L+1], hess[M, 2L+1, 2L+1], info[M])."""
        return loglik_hess_batch(self.kernel, *self.data, delays, alpha, rho, self.marginalise_b)

    def loglik_fisher_markov_batch(self, delays, alpha, rho):
        """Objective.loglik_fisher_markov_batch's result: (loglik[M], grad[M, 2L+1], fisher[M, 2L+1, 2L+1], info[M])."""
        return loglik_fisher_batch(self.kernel, *self.data, delays, alpha, rho, self.marginalise_b)

    def _rows(self, delays, alpha, rho):
        delays = np.asarray(delays, np.float64).reshape(-1, self.L)
        alpha = np.asarray(alpha, np.float64).reshape(-1, self.L)
        rho = np.asarray(rho, np.float64).reshape(-1)
        return delays, alpha, rho

    def _noise_of(self, M, noise):
        """Per row what predict() and its siblings take as _noise: None (a plain method), or (kappa[m], nu[m], None)."""
        if noise is None:
            return [None] * M
        kappa, nu = _noise_rows(self.L, M, noise[0]), _noise_rows(self.L, M, noise[1])
        return [(kappa[i], nu[i], None) for i in range(M)]

    def predict_markov_batch(self, delays, alpha, rho, ttest, weights=None, _noise=None):
        """Objective.predict_markov_batch's result: (mu[M, T], var[M, T], loglik[M], info[M], mix_mu, mix_var)."""
        delays, alpha, rho = self._rows(delays, alpha, rho)
        nz = self._noise_of(len(rho), _noise)
        out = [predict(self.kernel, *self.data, delays[i], alpha[i], rho[i], ttest, self.marginalise_b, _noise=nz[i])
               for i in range(len(rho))]
        mu, var = np.array([o[0] for o in out]), np.array([o[1] for o in out])
        mix = mix_moments(mu, var, weights) if weights is not None else (None, None)
        return mu, var, np.array([o[2] for o in out]), np.array([o[3] for o in out], dtype=np.int32), mix[0], mix[1]

    def heldout_loglik_markov_batch(self, delays, alpha, rho, ttest, ytest, sigmatest, weights=None, _noise=None):
        """Objective.heldout_loglik_markov_batch's result: (heldout[M], loglik[M], info[M], mix or None)."""
        delays, alpha, rho = self._rows(delays, alpha, rho)
        nz = self._noise_of(len(rho), _noise)
        out = [heldout(self.kernel, *self.data, delays[i], alpha[i], rho[i], ttest, ytest, sigmatest, self.marginalise_b, _noise=nz[i])
               for i in range(len(rho))]
        held = np.array([o[0] for o in out])
        mix = mix_logsumexp(held, weights) if weights is not None else None
        return held, np.array([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32), mix

    def loo_markov_batch(self, delays, alpha, rho, weights=None, outputs=None, _noise=None):
        """Objective.loo_markov_batch's result: LooResult(mu[M, N], var[M, N], lp[M, N], loo[M], loglik[M], info[M], mix_lp, mix_loo)
        (outputs is accepted and ignored: everything is computed)."""
        from .api import LooResult
        delays, alpha, rho = self._rows(delays, alpha, rho)
        nz = self._noise_of(len(rho), _noise)
        out = [loo(self.kernel, *self.data, delays[i], alpha[i], rho[i], self.marginalise_b, _noise=nz[i]) for i in range(len(rho))]
        lp = np.array([o[2] for o in out])
        mix = loo_mix(lp, weights) if weights is not None else (None, None)
        return LooResult(np.array([o[0] for o in out]), np.array([o[1] for o in out]), lp, np.array([o[3] for o in out]),
                         np.array([o[4] for o in out]), np.array([o[5] for o in out], dtype=np.int32), mix[0], mix[1])

    def posterior_offsets_markov_batch(self, delays, alpha, rho, _noise=None):
        """Objective.posterior_offsets_markov_batch's result: (mu_b[M, L], Sigma_b[M, L, L], loglik[M], info[M])."""
        if not self.marginalise_b:
            raise ValueError("posterior_offsets needs marginalise_b")
        delays, alpha, rho = self._rows(delays, alpha, rho)
        nz = self._noise_of(len(rho), _noise)
        out = [posterior_offsets(self.kernel, *self.data, delays[i], alpha[i], rho[i], _noise=nz[i]) for i in range(len(rho))]
        return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
                np.array([o[3] for o in out], dtype=np.int32))

    def predict_markov_noise_batch(self, delays, alpha, rho, ttest, kappa=None, nu=None, weights=None):
        """Objective.predict_markov_noise_batch's result: predict_markov_batch's tuple, every row under its own (kappa, nu)."""
        return self.predict_markov_batch(delays, alpha, rho, ttest, weights, _noise=(kappa, nu))

    def heldout_loglik_markov_noise_batch(self, delays, alpha, rho, ttest, ytest, sigmatest, kappa=None, nu=None, weights=None):
        """Objective.heldout_loglik_markov_noise_batch's result: heldout_loglik_markov_batch's tuple."""
        return self.heldout_loglik_markov_batch(delays, alpha, rho, ttest, ytest, sigmatest, weights, _noise=(kappa, nu))

    def posterior_offsets_markov_noise_batch(self, delays, alpha, rho, kappa=None, nu=None):
        """Objective.posterior_offsets_markov_noise_batch's result: posterior_offsets_markov_batch's tuple."""
        return self.posterior_offsets_markov_batch(delays, alpha, rho, _noise=(kappa, nu))

    def loo_markov_noise_batch(self, delays, alpha, rho, kappa=None, nu=None, weights=None, outputs=None):
        """Objective.loo_markov_noise_batch's result: loo_markov_batch's LooResult."""
        return self.loo_markov_batch(delays, alpha, rho, weights, outputs, _noise=(kappa, nu))

    def sample_markov_batch(self, delays, alpha, rho, ttest, S, seed, weights=None, sigmatest=None, _noise=None):
        """Objective.sample_markov_batch's result: (draws, draw_row, loglik[M], info[M])."""
        from . import rng
        delays, alpha, rho = self._rows(delays, alpha, rho)
        M, S = len(rho), int(S)
        nz = self._noise_of(M, _noise)
        if S < 1:
            raise ValueError("S=%d < 1" % S)
        T = sum(len(np.reshape(a, -1)) for a in ttest)
        if weights is not None:
            w = np.asarray(weights, np.float64).ravel()
            if w.shape != (M,) or not np.all(np.isfinite(w)) or np.any(w < 0) or not np.sum(w) > 0:
                raise ValueError("weights must be M finite non-negative values with a positive sum")
            draw_row = rng.pick_rows(seed, S, w)
            which = [(int(draw_row[s]), s, rng.MIXROW) for s in range(S)]
        else:
            draw_row = np.repeat(np.arange(M, dtype=np.int32), S)
            which = [(m, s, m) for m in range(M) for s in range(S)]
        draws = np.full((len(which), T), math.nan)
        ll, info = np.full(M, math.nan), np.full(M, -14, dtype=np.int32)          # GPCC_SAMPLE_NOT_DRAWN
        for o, (row, s, word) in enumerate(which):
            draws[o], ll[row], info[row] = sample(self.kernel, *self.data, delays[row], alpha[row], rho[row], ttest, sigmatest,
                                                  self.marginalise_b, seed=seed, s=s, m=word, _noise=nz[row])
        return draws, draw_row, ll, info

    def sample_markov_noise_batch(self, delays, alpha, rho, kappa, nu, ttest, S, seed, sigmatest=None, weights=None):
        """Objective.sample_markov_noise_batch's result: sample_markov_batch's tuple, every row under its own (kappa, nu)."""
        return self.sample_markov_batch(delays, alpha, rho, ttest, S, seed, weights, sigmatest, _noise=(kappa, nu))

    def close(self):
        pass
