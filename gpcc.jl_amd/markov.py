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
    name = _name(kernel)
    L = len(tarray)
    delays = np.asarray(delays, np.float64).reshape(L)
    alpha = np.asarray(alpha, np.float64).reshape(L)
    rho = float(rho)
    if not np.all(alpha > 0.0):
        return math.nan, -1
    if rho <= 0.0:
        return math.nan, -2
    if marginalise_b and L > MAX_OFFSET_BANDS:
        raise ValueError("marginalise_b with %d bands: the linear-time solver keeps at most %d offset states" % (L, MAX_OFFSET_BANDS))
    ts, rs, s2, vb = prepare(tarray, yarray, stdarray, marginalise_b)
    if _slip == "var_n":
        vb = vb * np.array([(len(t) - 1.0) / len(t) for t in ts])
    p = _ORDER[name]
    n = p + (L if marginalise_b else 0)
    Pinf = stationary(name, rho)
    P = np.zeros((n, n))
    P[:p, :p] = Pinf
    for l in range(n - p):
        P[p + l, p + l] = vb[l]
    m = np.zeros(n)
    seq = merge_order(ts, delays)
    if _slip == "order":
        for j in range(len(seq) // 2, len(seq) - 1):
            (b0, i0), (b1, i1) = seq[j], seq[j + 1]
            if ts[b0][i0] - delays[b0] != ts[b1][i1] - delays[b1]:
                seq[j], seq[j + 1] = seq[j + 1], seq[j]
                break
    ll = 0.0
    sprev = None
    for j, (b, i) in enumerate(seq):
        s = ts[b][i] - delays[b]
        d = 0.0 if sprev is None else s - sprev
        sprev = s
        A = transition(name, d, rho)
        m[:p] = A @ m[:p]
        if _slip == "no_q":
            P[:p, :p] = A @ P[:p, :p] @ A.T
        else:
            P[:p, :p] = A @ (P[:p, :p] - Pinf) @ A.T + Pinf
        P[:p, p:] = A @ P[:p, p:]
        P[p:, :p] = P[:p, p:].T
        h = np.zeros(n)
        h[0] = alpha[b]
        if n > p and _slip != "no_offset":
            h[p + b] = 1.0
        Ph = P @ h
        S = h @ Ph + s2[b][i]
        if not (S > 0.0 and math.isfinite(S)):
            return math.nan, j + 1
        eps = rs[b][i] - h @ m
        ll -= 0.5 * (LOG2PI + math.log(S) + eps * eps / S)
        m += Ph * (eps / S)
        P -= np.outer(Ph, Ph) / S
        P = 0.5 * (P + P.T)
    return ll, 0


def loglik_batch(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True):
    """loglik over M rows (delays and alpha M x L, rho M) -> (loglik[M], info[M]): Objective.loglik_markov_batch's shape."""
    L = len(tarray)
    delays = np.asarray(delays, np.float64).reshape(-1, L)
    alpha = np.asarray(alpha, np.float64).reshape(-1, L)
    rho = np.asarray(rho, np.float64).reshape(-1)
    out = [loglik(kernel, tarray, yarray, stdarray, delays[i], alpha[i], rho[i], marginalise_b) for i in range(len(rho))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32)


class MarkovObjective:
    """The CPU mirror with the two methods gpcc_grid's `engine="python"` fit calls (loglik_batch and loglik_markov_batch are the same
    filter here): gpcc_grid(..., objective=MarkovObjective(...), solver="markov") fits without a GPU."""

    def __init__(self, tarray, yarray, stdarray, kernel, marginalise_b=True):
        self.data = (tarray, yarray, stdarray)
        self.kernel, self.marginalise_b, self.L = _name(kernel), bool(marginalise_b), len(tarray)

    def loglik_markov_batch(self, delays, alpha, rho):
        return loglik_batch(self.kernel, *self.data, delays, alpha, rho, self.marginalise_b)

    loglik_batch = loglik_markov_batch

    def close(self):
        pass
