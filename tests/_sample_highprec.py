"""An extended-precision restatement of the joint posterior draws -- gpcc_sample_batch and gpcc_sample_markov_batch
(4.19) -- in numpy.longdouble on the CPU, their normals, and the comparator of tests/test_gpu_sample_highprec.py.  It checks itself in
tests/test_sample_highprec_cpu.py.  The model, the blocked Cholesky, err, Worst and report are _predict_highprec.py's.

Dense draws.  f* = mu + L zeta for normals zeta handed over as fp64: mu and S = cB + diag(sigma*^2 + JITTER) - V'V are
_predict_highprec.posterior_from's (with b marginalised by conditioning on b first; direct=True, the witness's algebra, for the fp64
runs), L the lower Cholesky factor of S in the caller's flattened test order.  sigmatest None is the latent curve.

Linear-time draws.  The reference is the dense Matheron draw  mu + g~ - kB*' K^-1 r~ + noise  of a prior draw restated from 4.19's
definition: the merged training and test points in ascending shifted time (training before test on ties; the training points among
themselves by band, then sorted position), one Philox block of four normals per POINT (training point e in the flattened order of
the handle, test point N + j in the caller's order, block N + T for the offsets); the stationary state C(inf) z at the first point,
then x <- A(d) x + C(d) z[:p] with C C' = Q(d) = Pinf - A Pinf A'; offsets sqrt(Sigma_b) xi; r~_i = alpha x_1 + b~ + sigma_i z_3,
g~_j = alpha x_1 + b~, noise_j = sqrt(JITTER + sigma*_j^2) z_3.  A, Pinf and Q are in longdouble.  Q, scaled by diag(Pinf)^-1/2, is a
combination of the integrals int_0^x u^k e^-2u du = gamma(k + 1, 2x) / 2^(k+1), each from the all-positive series of
markov._lower_gammas summed until its terms fall below the longdouble eps (x <= SERIES_MAX = 8; beyond, e^-2x < 2e-7 and the difference
cancels nothing); C is the factor eliminated from the last component, a triangular factor of a given Q being unique.  The draw is
linear in the normals: prior_map() walks once with the state as a p x 4 (N + T + 1) matrix and returns the maps of r~, g~ and the
noise, so a draw is mu + G xi, G = Gg - kB*' K^-1 Rt + Gn of shape T x 4 (N + T + 1).

The normals.  Box-Muller in longdouble from the same Philox words (rng.philox4x64), 2 pi to the working precision: box_muller().  An
fp64 evaluation z = r cos(theta), r = sqrt(-2 log u1), theta = fl(fl(2 pi) u2) < 8, is off by at most
    nu = 16 2^-53 max(r, 2^-53):   rounding theta (8 2^-53) + fl(2 pi) - 2 pi (2.2 2^-53) + cos / sin (2 2^-53), each times r, and r's own
                                   3 2^-53 relative (log, the product, sqrt) -- 15.2, derived and not measured.
gpcc_amd.rng.normals lands at most 0.40 nu from box_muller() on the CPU (2^20 normals of rng.normals, 2^18 of rng.point_normals;
tests/test_sample_highprec_cpu.py prints it).

The bar of one case -- one number, the largest over the case's draws and entries; every ingredient measured on the CPU, none on the
device, no cond term, no 1e-10 floor:
    bar = FACTOR max(e_witness, e_second, e_blocked, floor)  (+ sum_k |G_jk| nu_k per entry, linear-time only),      FACTOR = 16
  e_witness  the fp64 dense witness against the reference: _sample_witness.draws, _markov_sample_cases.matheron
  e_second   linear-time: the numpy mirror markov.sample(normals=...).  Dense: the mirror has no entry that takes zeta (its draw is a
             map of the point normals), so where it takes the case its predictive mean -- the draw of zeta = 0 -- is its part of the
             measurement, and the blocked run stands in for the rest, as it does for rbf and L > 4 offsets
  e_blocked  the witness's algebra (direct=True) in fp64 on the 16-blocked Cholesky, the device's own block
  floor      dense        (N + T) 2^-53 (|mu_j| + sum_k |L_jk zeta_k|)
             linear-time  (N + T) 2^-53 (|mu_j| + |g~_j| + |c_j| + |noise_j|),   c = kB*' K^-1 r~ as computed
The normals term stands outside FACTOR: the device's point normals are not visible (the entry has no return_noise), and within nu
of the reference's they move the draw by at most that sum.  The dense draws take the device's own zeta as input."""
from dataclasses import dataclass

import numpy as np

import _markov_predict_cases as PC
import _markov_sample_cases as SC
import _sample_witness as SW
from _grad_highprec import EXTENDED, LD, SKIP_REASON, cholesky_inverse  # noqa: F401
from _markov_cases import FACTOR
from _predict_highprec import (BLOCKED_NB, JITTER, NB, PI, U53, Worst, _factor, _flat, err, mirror_takes, model, posterior_from,  # noqa: F401
                               predict_from, report)
from gpcc_amd import markov, rng

SERIES_MAX = 8.0
_ORDER = {"OU": 1, "matern32": 2, "matern52": 3}
_cache = {}


# -- the normals --------------------------------------------------------------------------------------------------------------------
def words(seed, nb, draws, rows, stream):
    """The Philox words of blocks 0 .. nb-1 of the draws (s, m) of one stream -> uint64 (len(draws), nb, 4): rng._blocks' counters."""
    s = np.asarray(draws, dtype=np.uint64).ravel()
    m = np.broadcast_to(np.asarray(rows, dtype=np.uint64), s.shape)
    ctr = np.zeros((len(s), nb, 4), dtype=np.uint64)
    ctr[:, :, 0] = np.arange(nb, dtype=np.uint64)[None, :]
    ctr[:, :, 1] = s[:, None]
    ctr[:, :, 2] = m[:, None]
    ctr[:, :, 3] = stream
    return rng.philox4x64(ctr, np.array([seed, 0], dtype=np.uint64))


def box_muller(x):
    """(z, nu) of words x (..., 4): the four normals of each block in longdouble, and the bar nu of an fp64 evaluation of each."""
    z = np.empty(x.shape, dtype=LD)
    nu = np.empty(x.shape)
    for p in range(2):
        u1, u2 = rng.uniform53_open0(x[..., 2 * p]).astype(LD), rng.uniform53(x[..., 2 * p + 1]).astype(LD)
        r, th = np.sqrt(-2 * np.log(u1)), 2 * PI * u2
        z[..., 2 * p], z[..., 2 * p + 1] = r * np.cos(th), r * np.sin(th)
        nu[..., 2 * p] = nu[..., 2 * p + 1] = 16 * U53 * np.maximum(r.astype(np.float64), U53)
    return z, nu


def dense_normals(seed, T, draws, rows):
    """(zeta, nu) of rng.normals' draws, each (len(draws), T)."""
    nb = (int(T) + 3) // 4
    z, nu = box_muller(words(seed, nb, draws, rows, rng.STREAM_NORMALS))
    return z.reshape(len(z), 4 * nb)[:, :int(T)], nu.reshape(len(nu), 4 * nb)[:, :int(T)]


def point_normals(seed, points, draws, rows):
    """(xi, nu) of rng.point_normals' draws, each (len(draws), points, 4)."""
    return box_muller(words(seed, int(points), draws, rows, rng.STREAM_POINTS))


# -- dense draws --------------------------------------------------------------------------------------------------------------------
def _noise(m, sigmatest):
    """sigma* per test point in longdouble: None is the latent curve; a longdouble array is taken as it is (flattened)."""
    if isinstance(sigmatest, np.ndarray) and sigmatest.dtype == LD:
        return sigmatest
    return np.zeros(len(m.bs), dtype=LD) if sigmatest is None else _flat(sigmatest)


def dense_draws(m, sigmatest, zeta, dtype=LD, nb=NB, direct=False):
    """(draws (n, T), their terms |mu_j| + sum_k |L_jk zeta_k|, mu) of a Model for normals zeta (n, T), the algebra in `dtype`."""
    mu, S = posterior_from(m, _noise(m, sigmatest).astype(dtype), dtype, nb, direct)
    mu = mu + m.mean.astype(dtype)[m.bs]
    C, _ = _factor(S, nb)
    z = np.asarray(zeta, np.float64).astype(dtype)
    return mu[None, :] + z @ C.T, np.abs(mu)[None, :] + np.abs(z) @ np.abs(C).T, mu


@dataclass
class Reference:
    """The extended draws of one case, its bar and what went into it."""
    draws: np.ndarray = None           # longdouble (n, T)
    bar: object = None                 # one number (dense) or (n, T): the case's number plus each entry's normals term
    e_witness: float = 0.0
    e_second: float = 0.0
    e_blocked: float = 0.0
    floor: float = 0.0
    second: str = ""
    old_bar: float = 0.0               # _sample_witness.bar of the same draws, for the record
    G: np.ndarray = None               # linear-time: the map of the normals, T x 4 (N + T + 1)
    parts: dict = None                 # linear-time: mu, g, c, noise in longdouble

    @property
    def base(self):
        """The case's number: FACTOR max(e_witness, e_second, e_blocked, floor)."""
        return FACTOR * max(self.e_witness, self.e_second, self.e_blocked, self.floor)

    def ratio(self, got):
        """max |got - reference| / bar: <= 1 passes."""
        return float(np.max(err(got, self.draws) / self.bar))


def dense_reference(oracle, kernel, data, delays, alpha, rho, mb, ttest, sigmatest, zeta):
    """The Reference of the dense draws of one (tau, alpha, rho) for the fp64 normals zeta (n, T)."""
    t, y, s = data
    N, T, L = sum(len(a) for a in t), sum(len(a) for a in ttest), len(t)
    m = model(kernel, t, y, s, delays, alpha, rho, ttest, mb)
    draws, terms, mu = dense_draws(m, sigmatest, zeta)
    wit, cond = SW.draws(oracle, kernel, t, y, s, delays, alpha, rho, ttest, sigmatest, zeta, marginalise_b=mb)
    blk = dense_draws(m, sigmatest, zeta, np.float64, BLOCKED_NB, direct=True)[0]
    ref = Reference(draws=draws, e_witness=float(np.max(err(wit, draws))), e_blocked=float(np.max(err(blk, draws))),
                    floor=float((N + T) * U53 * np.max(terms)), second="blocked", old_bar=SW.bar(cond, wit))
    ref.e_second = ref.e_blocked
    if mirror_takes(kernel, L, mb):
        mmu, _, _, info = markov.predict(kernel, t, y, s, delays, alpha, rho, ttest, mb)
        assert info == 0
        ref.e_second, ref.second = max(ref.e_blocked, float(np.max(err(mmu, mu)))), "mirror's mean, blocked"
    ref.bar = ref.base
    return ref


# -- linear-time draws --------------------------------------------------------------------------------------------------------------
def rate(kernel, rho):
    return np.sqrt(LD({"OU": 1, "matern32": 3, "matern52": 5}[kernel])) / LD(np.float64(rho))


def stationary(kernel, lam):
    if kernel == "OU":
        return np.array([[1]], dtype=LD)
    if kernel == "matern32":
        return np.array([[1, 0], [0, lam * lam]], dtype=LD)
    kap = lam * lam / 3
    return np.array([[1, 0, -kap], [0, kap, 0], [-kap, 0, lam ** 4]], dtype=LD)


def transition(kernel, d, lam):
    """A(d) = expm(F d) in longdouble (markov.transition's formulas)."""
    d = LD(d)
    x, e = lam * d, np.exp(-lam * d)
    if kernel == "OU":
        return np.array([[e]], dtype=LD)
    if kernel == "matern32":
        return e * np.array([[1 + x, d], [-lam * lam * d, 1 - x]], dtype=LD)
    l2 = lam * lam
    return e * np.array([[1 + x + x * x / 2, d * (1 + x), d * d / 2], [-l2 * lam * d * d / 2, 1 + x - x * x, d * (1 - x / 2)],
                         [l2 * x * (x / 2 - 1), lam * x * (x - 3), 1 - 2 * x + x * x / 2]], dtype=LD)


def _gammas(K, y, perturb=None):
    """gamma(k + 1, y), k = 0 .. K, as markov._lower_gammas but summed until the terms fall below the longdouble eps."""
    e = np.exp(-y)
    term = LD(1) / (K + 1)
    acc, m = term, 1
    while term > np.finfo(LD).eps * acc / 64 and m < 400:
        term = term * y / (K + 1 + m)
        acc += term
        m += 1
    g = [LD(0)] * (K + 1)
    g[K] = y ** (K + 1) * e * acc
    for k in range(K, 0, -1):
        g[k - 1] = (g[k] + y ** k * e) / k
    return g


def process_noise_scaled(kernel, d, lam):
    """Q(d) = Pinf - A Pinf A' in the units of diag(Pinf)^1/2, in longdouble: markov.process_noise_scaled's integrals for
    x = lambda d <= SERIES_MAX, the difference beyond."""
    x = lam * LD(d)
    if not x <= SERIES_MAX:
        Pinf, A = stationary(kernel, lam), transition(kernel, d, lam)
        sc = 1 / np.sqrt(np.diagonal(Pinf))
        Q = Pinf - A @ Pinf @ A.T
        return sc[:, None] * ((Q + Q.T) / 2) * sc[None, :]
    if kernel == "OU":
        return np.array([[-np.expm1(-2 * x)]], dtype=LD)
    if kernel == "matern32":
        j = [g / LD(2) ** (k + 1) for k, g in enumerate(_gammas(2, 2 * x))]
        q01 = 4 * (j[1] - j[2])
        return np.array([[4 * j[2], q01], [q01, 4 * (j[0] - 2 * j[1] + j[2])]], dtype=LD)
    j = [g / LD(2) ** (k + 1) for k, g in enumerate(_gammas(4, 2 * x))]
    c, s3 = LD(16) / 3, np.sqrt(LD(3))
    q01 = c * (s3 / 2) * (j[3] - j[4] / 2)
    q02 = c * (j[2] / 2 - j[3] + j[4] / 4)
    q12 = c * s3 * (j[1] - 5 * j[2] / 2 + 3 * j[3] / 2 - j[4] / 4)
    return np.array([[c * j[4] / 4, q01, q02], [q01, c * 3 * (j[2] - j[3] + j[4] / 4), q12],
                     [q02, q12, c * (j[0] - 4 * j[1] + 5 * j[2] - 2 * j[3] + j[4] / 4)]], dtype=LD)


def sim_factor(kernel, d, lam):
    """C with C C' = Q(d) (d None: Pinf), upper triangular: the factor of the scaled Q eliminated from the last component to the
    first (markov._sim_factor's, the device's), unscaled."""
    Pinf = stationary(kernel, lam)
    p = len(Pinf)
    sc = 1 / np.sqrt(np.diagonal(Pinf))
    Q = sc[:, None] * Pinf * sc[None, :] if d is None else process_noise_scaled(kernel, d, lam)
    G = np.zeros((p, p), dtype=LD)
    for j in range(p - 1, -1, -1):
        dj = Q[j, j] - sum(G[j, k] * G[j, k] for k in range(j + 1, p))
        if not dj > 0:
            continue
        G[j, j] = np.sqrt(dj)
        for i in range(j):
            G[i, j] = (Q[i, j] - sum(G[i, k] * G[j, k] for k in range(j + 1, p))) / G[j, j]
    return G / sc[:, None]


def merged_points(tarray, ttest, delays):
    """[(shifted time, 0 training / 1 test, band, position, block e)] in the order of the walk."""
    tau = np.asarray(delays, np.float64).astype(LD)
    ev, off = [], 0
    for l, a in enumerate(tarray):
        a = np.asarray(a, np.float64).reshape(-1)
        for i, q in enumerate(np.argsort(a, kind="stable")):
            ev.append((LD(a[q]) - tau[l], 0, l, i, off + int(q)))
        off += len(a)
    j = 0
    for l, a in enumerate(ttest):
        for v in np.asarray(a, np.float64).reshape(-1):
            ev.append((LD(v) - tau[l], 1, l, j, off + j))
            j += 1
    ev.sort(key=lambda e: e[:4])
    return ev


def prior_map(kernel, data, delays, alpha, rho, ttest, sigmatest, m):
    """(Rt [N x K], Gg [T x K], Gn [T x K]), K = 4 (N + T + 1): r~ = Rt xi, g~ = Gg xi, noise = Gn xi for the point normals xi
    flattened (block e, component c) -> 4 e + c."""
    p, lam = _ORDER[kernel], rate(kernel, rho)
    N, T = len(m.r), len(m.bs)
    K = 4 * (N + T + 1)
    al, sd, st = np.asarray(alpha, np.float64).astype(LD), _flat(data[2]), _noise(m, sigmatest)
    Rt, Gg, Gn = (np.zeros((n, K), dtype=LD) for n in (N, T, T))
    X, sprev = None, None
    for (s, kind, b, _, e) in merged_points(data[0], ttest, delays):
        if X is None:
            X = np.zeros((p, K), dtype=LD)
            X[:, 4 * e:4 * e + p] = sim_factor(kernel, None, lam)
        elif s != sprev:
            X = transition(kernel, s - sprev, lam) @ X
            X[:, 4 * e:4 * e + p] += sim_factor(kernel, s - sprev, lam)
        sprev = s
        f = al[b] * X[0]
        if m.Sigb[b] != 0:                                            # (zero with fixed b)
            f[4 * (N + T) + b] += np.sqrt(m.Sigb[b])
        if kind == 0:
            Rt[e] = f
            Rt[e, 4 * e + 3] += sd[e]
        else:
            Gg[e - N] = f
            Gn[e - N, 4 * e + 3] = np.sqrt(LD(JITTER) + st[e - N] ** 2)
    return Rt, Gg, Gn


def smoother_weights(m):
    """W = kB*' K^-1 (T x N) of a Model in longdouble.  With b marginalised, by conditioning on b first as posterior_from does --
    W = V'X + (Q* - V'XQ) Sigma_p (XQ)'X on the matrices without Sigma_b, X = C0^-1, V = X kB0, Sigma_p = (Sigma_b^-1 + Q'K0^-1 Q)^-1 --
    in which no Sigma_b-sized terms cancel (the direct form costs tens of longdouble eps: tests/test_sample_highprec_cpu.py)."""
    if not np.any(m.Sigb):
        _, X = _factor(m.K, NB)
        return (X @ m.kB).T @ X
    L = len(m.Sigb)
    Q = (m.band[:, None] == np.arange(L)[None, :]).astype(LD)
    Qs = (m.bs[:, None] == np.arange(L)[None, :]).astype(LD)
    _, X = _factor(m.K0, NB)
    V, XQ = X @ m.kB0, X @ Q
    A = XQ.T @ XQ
    A[np.diag_indices(L)] += 1 / m.Sigb
    _, XA = _factor(A, NB)
    return V.T @ X + ((Qs - V.T @ XQ) @ (XA.T @ XA)) @ (XQ.T @ X)


def linear_map(kernel, data, delays, alpha, rho, mb, ttest, sigmatest):
    """(mu, Gg, C, Gn, the Model) in longdouble: a draw is mu + (Gg - C + Gn) xi, with C = kB*' K^-1 Rt."""
    m = model(kernel, *data, delays, alpha, rho, ttest, mb)
    Rt, Gg, Gn = prior_map(kernel, data, delays, alpha, rho, ttest, sigmatest, m)
    W = smoother_weights(m)
    return W @ m.r + m.mean[m.bs], Gg, W @ Rt, Gn, m


def linear_reference(oracle, case, seed, S, word):
    """The Reference of draws s = 0 .. S-1 of the linear-time entry for one case of the cases' form, counters (e, s, word, 2) under
    `seed` (cached)."""
    cid, kernel, data, delays, alpha, rho, mb, tests = case
    key = ("l", cid, seed, S, word)
    if key in _cache:
        return _cache[key]
    tt, st = tests[0], tests[2]
    N, T = SC.dims(case)
    mu, Gg, C, Gn, m = linear_map(kernel, data, delays, alpha, rho, mb, tt, st)
    G = Gg - C + Gn
    xi64 = rng.point_normals(seed, N + T + 1, range(S), [word] * S)
    xi = xi64.reshape(S, -1).astype(LD)
    _, nu = point_normals(seed, N + T + 1, range(S), [word] * S)
    parts = {"mu": mu, "g": xi @ Gg.T, "c": xi @ C.T, "noise": xi @ Gn.T}
    draws = mu[None, :] + xi @ G.T
    floor = (N + T) * U53 * (np.abs(mu)[None, :] + np.abs(parts["g"]) + np.abs(parts["c"]) + np.abs(parts["noise"]))
    bmu = predict_from(m, np.float64, BLOCKED_NB)[0]
    _, Xb = _factor(m.K.astype(np.float64), BLOCKED_NB)
    Vb = Xb @ m.kB.astype(np.float64)
    ew = es = eb = old = 0.0
    for s in range(S):
        rt, gt, noise = markov.prior_draw(kernel, *data, delays, alpha, rho, tt, st, mb, normals=xi64[s])
        wit, ob = SC.matheron(oracle, case, rt, gt, noise)
        mir, _, info = markov.sample(kernel, *data, delays, alpha, rho, tt, st, mb, normals=xi64[s])
        assert info == 0, cid
        blk = bmu + gt - Vb.T @ (Xb @ rt) + noise
        ew, es, eb = (max(a, float(np.max(err(v, draws[s])))) for a, v in ((ew, wit), (es, mir), (eb, blk)))
        old = max(old, ob)
    ref = Reference(draws=draws, e_witness=ew, e_second=es, e_blocked=eb, floor=float(np.max(floor)), second="mirror", old_bar=old,
                    G=G, parts=parts)
    ref.bar = ref.base + nu.reshape(S, -1) @ np.abs(G).astype(np.float64).T
    _cache[key] = ref
    return ref


# -- the cases ----------------------------------------------------------------------------------------------------------------------
def cases():
    """The 72 cases of the predictions (N = 110): test noise as given on the even-numbered ones, None (the latent curve) on the odd
    ones, which carry another id (the witnesses cache by id)."""
    out = []
    for idx, (cid, k, data, delays, alpha, rho, mb, (tt, yt, st)) in enumerate(PC.cpu_cases()):
        out.append((cid, k, data, delays, alpha, rho, mb, (tt, yt, st)) if idx % 2 == 0 else
                   (cid + "-latent", k, data, delays, alpha, rho, mb, (tt, yt, None)))
    return out


def branch_band(kernel, rho, mb):
    """One band of 12 training and 7 test points built for the process-noise branch of the walk (all lags between neighbouring merged
    points are exact in fp64): the two fp64 lags on either side of lambda d = 1 (fl(lambda d_lo) <= 1 < fl(lambda d_hi) in the
    device's own fp64 product), a lag of 2^-10, a tie inside the band, a test point on a training point, a lag of 40, test points in
    the gaps."""
    lam = markov.rate(kernel, rho)
    d_lo = 1.0 / lam
    while lam * d_lo > 1.0:
        d_lo = np.nextafter(d_lo, 0.0)
    while lam * np.nextafter(d_lo, np.inf) <= 1.0:
        d_lo = np.nextafter(d_lo, np.inf)
    d_hi = np.nextafter(d_lo, np.inf)
    g = 2.0 ** -10
    a = np.ceil(d_hi / g) * g + 2 * g                                 # the first grid point after d_hi, within 2 d_hi of it
    t = np.array([-d_lo - 40.0 * g, -d_lo, 0.0, d_hi, a, a + g, a + g, a + 0.5, a + 0.5 + g, a + 40.5 + g, a + 41.0, a + 41.0 + 3 * g])
    tt = np.array([-d_lo - 20.0 * g, a - g, a + 0.25, a + 0.5, a + 41.0 + g, a + 41.0 + 2 * g, a + 45.0])
    rg = np.random.default_rng(int(10 * rho) + _ORDER[kernel])
    perm = rg.permutation(len(t))
    y = (np.sin(0.3 * t) + 0.2 * rg.standard_normal(len(t)))[perm]
    s = (0.2 + 0.05 * rg.random(len(t)))[perm]
    st = 0.2 + 0.05 * rg.random(len(tt))
    cid = "branch-%s-b%d-rho%g" % (kernel, mb, rho)
    return (cid, kernel, ([t[perm]], [y], [s]), np.zeros(1), np.array([1.3]), rho, mb, ([tt[rg.permutation(len(tt))]], None, [st])), (d_lo, d_hi)
