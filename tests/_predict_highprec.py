"""An extended-precision restatement of the prediction family -- the per-row predictive mean and variance (gpcc_predict_batch,
gpcc_predict_markov_batch), the held-out log-likelihood (gpcc_heldout_loglik_batch, gpcc_heldout_loglik_markov_batch) and the offsets'
posterior (gpcc_posterior_offsets, gpcc_posterior_offsets_markov_batch) -- in numpy.longdouble (x87 80-bit: eps ~1.1e-19) on the CPU,
and the comparator of tests/test_gpu_predict_highprec.py.  It checks itself in tests/test_predict_highprec_cpu.py.  The kernels, the
blocked Cholesky and X = C^-1 are _grad_highprec.py's; the inputs are the fp64 values cast up, as _grad_highprec.evaluate does.

The model (all four kernels, both b-modes), with band p of training point i, band q of test point j, u = t - tau_band:
    K    = alpha_p alpha_p' k(u_i - u_i') + diag(sigma^2)  (+ Sigma_b_p on same-band pairs when b is marginalised)
    kB*  = alpha_p alpha_q k(u_i - u*_j)  (+ Sigma_b_p where p = q),      cdiag_j = alpha_q^2 + Sigma_b_q
    mean_l = mean(y_l),  Sigma_b_l = 100 var(y_l) (n - 1)  -- of the TRAINING fluxes, whatever the test set; Sigma_b = 0 with fixed b
and K = C C', X = C^-1, V = X kB*, w = X' X (y - mean):
    predict   mu_j = kB*_j' w + mean_q,        var_j = cdiag_j - |V_j|^2 + JITTER
    heldout   S = cB* + diag(sigma*^2 + JITTER) - V' V, symmetrised; l = log N(y* ; mu, S) by the Cholesky of S
    postb     K0 = K without the Sigma_b blocks, Q the N x L band indicator, Y the fluxes (not centred):
              Sigma = (Sigma_b^-1 + Q' K0^-1 Q)^-1,  mu = Sigma (Q' K0^-1 Y + Sigma_b^-1 mean)        (marginaliseb.jl:248-250)
Offsets apart.  With b marginalised S is a difference of Sigma_b-sized terms (100 var(y), about 50 here) that leaves sigma*^2-sized
pivots: a thousandfold cancellation that the terms of l below do not see, and that costs the direct form in longdouble a hundred eps
of them (measured against mpmath, tests/test_predict_highprec_cpu.py).  So heldout() conditions on b first -- the same S and mean,
    f* | Y, b ~ N(m0 + G b, S0),   m0 = kB0' K0^-1 r,  S0 = cB0 - kB0' K0^-1 kB0,  G = Q* - kB0' K0^-1 Q   (kB0, cB0: no Sigma_b; Q*: test bands)
    b | Y ~ N(mu_p, Sigma_p),      Sigma_p = (Sigma_b^-1 + Q' K0^-1 Q)^-1,  mu_p = Sigma_p Q' K0^-1 r
    S = S0 + G Sigma_p G' + noise,  mean = m0 + G mu_p + mean_q
-- in which only alpha^2-sized terms cancel and G Sigma_p G' is added.  direct=True keeps the first form (the witness's algebra).

A test time may equal a shifted training time (k(0) = 1 falls out of the lag), times may be repeated and in any order, a band may have
no test points.  JITTER and 2 pi are the device's fp64 constants cast up, respectively pi to the working precision.

Beside each value comes the size of the terms that were summed to give it -- what the rounding of an fp64 sum is relative to:
    mu    sum_i |kB*_ij w_i| + |mean_q|            var   cdiag_j + |V_j|^2
    l     z'z / 2 + sum |log pivot| + T log(2 pi) / 2   (z the whitened test residual, the pivots those of S)
    postb max |mu|, max |Sigma| (the bar of postb is per entry relative to the largest)

`dtype` and `nb` run the same algebra in another type and block size: with float64 and nb = 16 (the device's own block) it is the
blocked fp64 run of the bar, and the second evaluation of the cases that the numpy mirror (gpcc_amd.markov) does not take, rbf among them.

The bar of a quantity q of one case, every ingredient measured on the CPU and none on the device:
    bar(q) = FACTOR max(e_witness, e_second, e_blocked, n 2^-53 terms(q)),      FACTOR = _markov_cases.FACTOR (16, _hess_highprec's too)
e_witness = max |fp64 dense witness - extended| over the entries of q (_predict_witness.predict_row, _heldout_witness.heldout_row,
_markov_predict_cases.postb_reference), e_second the same for a second fp64 evaluation in another rounding order (OU and Matern: the
numpy mirror markov.predict / heldout / posterior_offsets; otherwise the blocked run, which follows), n = N for mu, var and postb
and N + T for the held-out value, terms(q) per entry for mu and var.  The errors are taken as the largest over q's entries and not
entry by entry: an fp64 evaluation's error at one entry is one draw of a rounding error and can land near zero there
(_hess_highprec.py's docstring has the measurement that taught this).  No cond term, no 1e-10 floor.

e_blocked: the witness's algebra (direct=True) in float64 on the 16-blocked Cholesky, the dense entries' own block.  Why a third run.
The dense held-out value goes through S = cB* - V'V, and with b marginalised that subtracts Sigma_b-sized terms (~50) to leave
pivots of the size of sigma*^2 (~0.05): whatever rounding V'V carries reaches log pivot a thousandfold, so the dense value's error is
~1e3 u times a sum over the factorisation's rounding -- one draw per ORDER of that factorisation's sums, and of the same scale for
every order.  The witness (LAPACK's order) is a single draw, and the mirror is no draw of it at all: the filter keeps the offsets as
states and never forms the difference.  Measured on the CPU alone over the 36 marginalised cases: the direct form in 16-blocks errs by
up to 26 x the larger of the witness's and the mirror's errors (matern32-L1-b1-rho20-before: 9.3e-15, 6.2e-14 and 1.6e-12; in 64-blocks
5.4e-12), and at matern52-L3-b1-rho20-ties (witness 1.1e-12, mirror 3.0e-12) by 2.5e-11, over half of a bar made from those two --
while conditioning on b first, in the same float64 and blocks, errs by 6.9e-13 there.  A bar from the first two is then 16 x a lucky
draw: the dense entry on the device, one more order of the same sums, came to 8.9e-11 at that case, 1.86 of that bar, and stayed under
0.6 of it in the 71 others.  So, as _hess_highprec.py does for the Hessian's mirror, the order of the factorisation is part of the
measurement: the 16-blocked run joins the maximum, for every quantity.  It is measured here, in numpy, and takes nothing from the
device."""
from dataclasses import dataclass

import numpy as np

from _grad_highprec import EXTENDED, LD, NB, SKIP_REASON, _kernel, cholesky_inverse  # noqa: F401
from _markov_cases import FACTOR

JITTER = np.float64(1e-8)
PI = LD(np.pi) + LD(1.2246467991473531772e-16)         # pi - fp64(pi), so that PI is pi to longdouble's precision
U53 = 2.0 ** -53
BLOCKED_NB = 16
_cache = {}


def _bands(arrays):
    return np.concatenate([np.full(len(a), l, dtype=int) for l, a in enumerate(arrays)]) if len(arrays) else np.zeros(0, int)


def _flat(arrays):
    return np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in arrays]).astype(LD)


@dataclass
class Model:
    """The matrices of one (tau, alpha, rho), in longdouble."""
    K: np.ndarray          # N x N, with the Sigma_b blocks when b is marginalised
    K0: np.ndarray         # N x N, without them
    r: np.ndarray          # y - mean_band
    y: np.ndarray
    kB: np.ndarray         # N x T
    cB: np.ndarray         # T x T, without noise and JITTER
    kB0: np.ndarray        # kB and cB without their Sigma_b terms
    cB0: np.ndarray
    cdiag: np.ndarray      # T
    mean: np.ndarray       # L
    Sigb: np.ndarray       # L (zeros with fixed b)
    band: np.ndarray
    bs: np.ndarray


def model(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, marginalise_b=True):
    L = len(tarray)
    band, bs = _bands(tarray), _bands(ttest)
    t, y, sd, ts = _flat(tarray), _flat(yarray), _flat(stdarray), _flat(ttest)
    tau = np.asarray(delays, np.float64).astype(LD)
    al = np.asarray(alpha, np.float64).astype(LD)
    mean = np.array([np.sum(np.asarray(a, np.float64).astype(LD)) / len(a) for a in yarray], dtype=LD)
    Sigb = np.zeros(L, dtype=LD)
    if marginalise_b:
        Sigb = np.array([100 * np.sum((np.asarray(a, np.float64).astype(LD) - m) ** 2) / (len(a) - 1) for a, m in zip(yarray, mean)],
                        dtype=LD)
    u, us = t - tau[band], ts - tau[bs]
    rho = np.float64(rho)
    K0 = al[band][:, None] * al[band][None, :] * _kernel(kernel, u[:, None] - u[None, :], rho)[0]
    K0[np.diag_indices(len(t))] += sd * sd
    K = K0 + Sigb[band][:, None] * (band[:, None] == band[None, :])
    kB0 = al[band][:, None] * al[bs][None, :] * _kernel(kernel, u[:, None] - us[None, :], rho)[0]
    kB = kB0 + Sigb[band][:, None] * (band[:, None] == bs[None, :])
    cB0 = al[bs][:, None] * al[bs][None, :] * _kernel(kernel, us[:, None] - us[None, :], rho)[0]
    cB = cB0 + Sigb[bs][:, None] * (bs[:, None] == bs[None, :])
    return Model(K=K, K0=K0, r=y - mean[band], y=y, kB=kB, cB=cB, kB0=kB0, cB0=cB0, cdiag=al[bs] ** 2 + Sigb[bs], mean=mean, Sigb=Sigb,
                 band=band, bs=bs)


def _factor(A, nb):
    C, X, info = cholesky_inverse(A, nb)
    assert info == 0, info
    return C, X


def predict_from(m, dtype=LD, nb=NB):
    """(mu[T], var[T], terms of mu[T], terms of var[T]) of a Model, the algebra in `dtype`."""
    K, kB, r, cdiag, mean = (a.astype(dtype) for a in (m.K, m.kB, m.r, m.cdiag, m.mean))
    _, X = _factor(K, nb)
    V = X @ kB
    w = X.T @ (X @ r)
    v2 = np.sum(V * V, axis=0)
    mu = kB.T @ w + mean[m.bs]
    var = cdiag - v2 + dtype(JITTER)
    return mu, var, np.sum(np.abs(kB * w[:, None]), axis=0) + np.abs(mean[m.bs]), cdiag + v2


def posterior_from(m, sigmatest, dtype=LD, nb=NB, direct=False):
    """(centred mean[T], S[T, T]) of a Model's test points under test noise sigmatest (flattened, in `dtype`): S = cB + diag(sigma*^2 +
    JITTER) - V'V symmetrised, the mean without the band means.  direct: both as the module's docstring (and the witness) writes them.
    Otherwise, with marginalised b, the same two by conditioning on b first (the docstring's "offsets apart").  heldout_from's first
    half, and what the joint draws factor (_sample_highprec.py)."""
    r, Sigb = m.r.astype(dtype), m.Sigb.astype(dtype)
    st = sigmatest
    T, L = len(st), len(Sigb)
    if direct or not np.any(m.Sigb):
        K, kB, S = m.K.astype(dtype), m.kB.astype(dtype), m.cB.astype(dtype)
        _, X = _factor(K, nb)
        V = X @ kB
        S = S - V.T @ V
        mu = V.T @ (X @ r)
    else:
        K0, kB0, S = m.K0.astype(dtype), m.kB0.astype(dtype), m.cB0.astype(dtype)
        Q = (m.band[:, None] == np.arange(L)[None, :]).astype(dtype)
        Qs = (m.bs[:, None] == np.arange(L)[None, :]).astype(dtype)
        _, X = _factor(K0, nb)
        V, z, XQ = X @ kB0, X @ r, X @ Q
        A = XQ.T @ XQ
        A[np.diag_indices(L)] += 1 / Sigb
        _, XA = _factor(A, nb)                         # Sigma_post = XA' XA
        G = Qs - V.T @ XQ
        W = XA @ G.T
        S = S - V.T @ V + W.T @ W
        mu = V.T @ z + W.T @ (XA @ (XQ.T @ z))
    S[np.diag_indices(T)] += st * st + dtype(JITTER)
    return mu, (S + S.T) / 2


def heldout_from(m, ytest, sigmatest, dtype=LD, nb=NB, direct=False):
    """(l, terms of l) of a Model and a test set, the algebra in `dtype`; direct: posterior_from's."""
    mean = m.mean.astype(dtype)
    yt, st = _flat(ytest).astype(dtype), _flat(sigmatest).astype(dtype)
    T = len(yt)
    mu, S = posterior_from(m, st, dtype, nb, direct)
    Cs, Xs = _factor(S, nb)
    z = Xs @ (yt - (mu + mean[m.bs]))
    quad, logs, const = (z @ z) / 2, np.log(np.diagonal(Cs)), T * np.log(2 * dtype(PI)) / 2
    return -quad - np.sum(logs) - const, quad + np.sum(np.abs(logs)) + const


def postb_from(m, dtype=LD, nb=NB):
    """(mu_b[L], Sigma_b[L, L]) of a Model built with marginalise_b=True, the algebra in `dtype`."""
    K0, y, mean, Sigb = (a.astype(dtype) for a in (m.K0, m.y, m.mean, m.Sigb))
    L = len(mean)
    Q = (m.band[:, None] == np.arange(L)[None, :]).astype(dtype)
    _, X = _factor(K0, nb)
    XQ = X @ Q
    A = XQ.T @ XQ
    A[np.diag_indices(L)] += 1 / Sigb
    _, XA = _factor(A, nb)
    Sig = XA.T @ XA
    return Sig @ (XQ.T @ (X @ y) + mean / Sigb), Sig


def predict(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, marginalise_b=True):
    """-> (mu[T], var[T], terms of mu[T], terms of var[T]) in longdouble."""
    return predict_from(model(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, marginalise_b))


def heldout(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, ytest, sigmatest, marginalise_b=True):
    """-> (l, terms of l) in longdouble."""
    return heldout_from(model(kernel, tarray, yarray, stdarray, delays, alpha, rho, ttest, marginalise_b), ytest, sigmatest)


def postb(kernel, tarray, yarray, stdarray, delays, alpha, rho):
    """-> (mu_b[L], Sigma_b[L, L]) in longdouble."""
    return postb_from(model(kernel, tarray, yarray, stdarray, delays, alpha, rho, [np.zeros(0)] * len(tarray), True))


# -- the comparator ---------------------------------------------------------------------------------------------------------------
def err(got, ref):
    """|got - ref| entry by entry as float64, the difference taken in longdouble; NaN counts as infinite."""
    e = np.abs(np.asarray(got, np.float64).astype(LD) - ref).astype(np.float64)
    return np.where(np.isnan(e), np.inf, e)


def bar(e_witness, e_second, e_blocked, n, terms):
    """The bar of the module's docstring; terms per entry or one number."""
    return FACTOR * np.maximum(max(float(e_witness), float(e_second), float(e_blocked)), n * U53 * np.asarray(terms, np.float64))


@dataclass
class Reference:
    """The extended values of one case, the bar of each and the two fp64 evaluations' errors that went into it."""
    mu: np.ndarray = None
    var: np.ndarray = None
    held: object = None
    pmu: np.ndarray = None
    pS: np.ndarray = None
    bar: dict = None                   # "mu", "var" [T]; "held"; "pmu", "pS" (one number each)
    e_witness: dict = None
    e_second: dict = None
    e_blocked: dict = None
    second: str = ""                   # "mirror" or "blocked" (the blocked run stands in where the mirror does not take the case)
    mean: np.ndarray = None            # float64 [L]: the training band means
    bs: np.ndarray = None              # band of each test point

    def ratio(self, what, got):
        """max |got - reference| / bar: <= 1 passes."""
        return float(np.max(err(got, getattr(self, what)) / self.bar[what]))


def mirror_takes(kernel, L, marginalise_b):
    """Whether the numpy mirror evaluates the case: a Markov kernel, and no more offset states than it keeps."""
    from gpcc_amd import markov
    return kernel in markov.KERNELS and not (marginalise_b and L > markov.MAX_OFFSET_BANDS)


def reference(oracle, kernel, data, delays, alpha, rho, marginalise_b, tests, want=("predict", "heldout", "postb")):
    """The Reference of one evaluation.  tests = (ttest, ytest, sigmatest); want: the quantities to compute (postb only with
    marginalise_b)."""
    import _heldout_witness as HW
    import _markov_predict_cases as PC
    import _predict_witness as PW
    from gpcc_amd import markov
    t, y, s = data
    N, T, L = sum(len(a) for a in t), sum(len(a) for a in tests[0]), len(t)
    m = model(kernel, t, y, s, delays, alpha, rho, tests[0], marginalise_b)
    use_mirror = mirror_takes(kernel, L, marginalise_b)
    ref = Reference(bar={}, e_witness={}, e_second={}, e_blocked={}, second="mirror" if use_mirror else "blocked", bs=m.bs,
                    mean=m.mean.astype(np.float64))

    def put(what, value, witness, second, blocked, n, terms):
        setattr(ref, what, value)
        ref.e_witness[what] = float(np.max(err(witness, value)))
        ref.e_second[what] = float(np.max(err(second, value)))
        ref.e_blocked[what] = float(np.max(err(blocked, value)))
        ref.bar[what] = bar(ref.e_witness[what], ref.e_second[what], ref.e_blocked[what], n, terms)

    if "predict" in want:
        mu, var, tmu, tvar = predict_from(m)
        wmu, wvar, _, _ = PW.predict_row(oracle, kernel, t, y, s, delays, alpha, rho, tests[0], marginalise_b)
        bmu, bvar, _, _ = predict_from(m, np.float64, BLOCKED_NB)
        smu, svar = bmu, bvar
        if use_mirror:
            smu, svar, _, info = markov.predict(kernel, t, y, s, delays, alpha, rho, tests[0], marginalise_b)
            assert info == 0
        put("mu", mu, wmu, smu, bmu, N, tmu)
        put("var", var, wvar, svar, bvar, N, tvar)
    if "heldout" in want:
        held, th = heldout_from(m, tests[1], tests[2])
        wh, _ = HW.heldout_row(oracle, kernel, t, y, s, delays, alpha, rho, *tests, marginalise_b)
        sh = bh = heldout_from(m, tests[1], tests[2], np.float64, BLOCKED_NB, direct=True)[0]
        if use_mirror:
            sh, _, info = markov.heldout(kernel, t, y, s, delays, alpha, rho, *tests, marginalise_b)
            assert info == 0
        put("held", held, wh, sh, bh, N + T, th)
    if "postb" in want and marginalise_b:
        pmu, pS = postb_from(m)
        wmu, wS = PC.postb_reference(oracle, kernel, t, y, s, delays, alpha, rho)
        bmu, bS = postb_from(m, np.float64, BLOCKED_NB)
        smu, sS = bmu, bS
        if use_mirror:
            smu, sS, _, info = markov.posterior_offsets(kernel, t, y, s, delays, alpha, rho)
            assert info == 0
        put("pmu", pmu, wmu, smu, bmu, N, float(np.max(np.abs(pmu))))
        put("pS", pS, wS, sS, bS, N, float(np.max(np.abs(pS))))
    return ref


def case_reference(oracle, case, kernel=None):
    """The Reference of a case of _markov_predict_cases.cpu_cases() (cached); kernel: another kernel on the same data (the rbf pass)."""
    cid, k, data, delays, alpha, rho, mb, tests = case
    k = kernel or k
    if (cid, k) not in _cache:
        _cache[(cid, k)] = reference(oracle, k, data, delays, alpha, rho, mb, tests)
    return _cache[(cid, k)]


class Worst:
    """The worst error / bar of a group."""

    def __init__(self, group):
        self.group, self.worst, self.where = group, 0.0, None

    def add(self, r, where):
        if r >= self.worst:
            self.worst, self.where = r, where

    def line(self):
        return "%s: worst error / bar %.3g (%s)" % (self.group, self.worst, self.where)


def report(groups):
    """Prints the line of every group, then asserts that every group passes (error / bar <= 1)."""
    groups = list(groups)
    for w in groups:
        print(w.line())
    missed = [w.line() for w in groups if not w.worst <= 1.0]
    assert not missed, missed
