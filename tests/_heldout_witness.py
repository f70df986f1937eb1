"""A numpy restatement of the per-row held-out log-likelihood of gpcc_heldout_loglik_batch (predictTest(ttest, ytest, sigmatest),
src/gpccfixdelay_marginaliseb.jl:311-325; the fixed-b variant src/gpccfixdelay.jl) on the oracle's matrices: K and Y - bbar from
oracle.model_matrix, the cross and test blocks from oracle.delayed_covariance, and the handle-independent constants mu_b (band means of
the training fluxes) and Sigma_b (100 x their sample variance, n - 1).

`slip` injects one of the mistakes the GPU tests' bar must catch: "no_jitter", "sigma_not_squared" (diag(sigma*) in place of
diag(sigma*^2)), "no_b_cross" (the B* term of kB* dropped), "wrong_band_mean" (the first test residual of band 0 centred on band 1's
mean), "padded_row" (one padded test row counted in T log 2pi)."""
import numpy as np

JITTER = 1e-8
LOG2PI = np.log(2.0 * np.pi)


def _bands(arrays):
    return np.concatenate([np.full(len(a), l, dtype=int) for l, a in enumerate(arrays)]) if len(arrays) else np.zeros(0, int)


def constants(y, marginalise_b=True):
    L = len(y)
    mub = np.array([np.mean(a) for a in y])
    Sigb = 100 * np.array([np.var(a, ddof=1) for a in y]) if marginalise_b else np.zeros(L)
    return mub, Sigb


def blocks(oracle, kname, t, y, s, delays, alpha, rho, ttest, stest, marginalise_b=True, slip=None):
    """-> (K, resid, kB, cB + JITTER + diag(sigma*^2), test bands, mu_b) of the union model."""
    mub, Sigb = constants(y, marginalise_b)
    K, resid = oracle.model_matrix(kname, t, y, s, delays, alpha, rho, marginalise_b)
    bt, bs = _bands(t), _bands(ttest)
    ttest = [np.asarray(a, dtype=np.float64) for a in ttest]
    kB = oracle.delayed_covariance(kname, alpha, delays, rho, t, ttest)
    if slip != "no_b_cross":
        kB = kB + (bt[:, None] == bs[None, :]) * Sigb[bt][:, None]
    cB = oracle.delayed_covariance(kname, alpha, delays, rho, ttest) + (bs[:, None] == bs[None, :]) * Sigb[bs][:, None]
    sv = np.concatenate([np.asarray(a, dtype=np.float64) for a in stest])
    C = cB + np.diag(sv if slip == "sigma_not_squared" else sv ** 2)
    if slip != "no_jitter":
        C = C + JITTER * np.eye(len(bs))
    return K, resid, kB, C, bs, mub


def _logpdf(S, r):
    Lc = np.linalg.cholesky(S)
    z = np.linalg.solve(Lc, r)
    return -0.5 * (len(r) * LOG2PI + 2.0 * np.sum(np.log(np.diag(Lc))) + z @ z)


def heldout_row(oracle, kname, t, y, s, delays, alpha, rho, ttest, ytest, stest, marginalise_b=True, slip=None):
    """-> (heldout, cond_1(K_aug)) at one (tau, alpha, rho)."""
    K, resid, kB, C, bs, mub = blocks(oracle, kname, t, y, s, delays, alpha, rho, ttest, stest, marginalise_b, slip)
    yv = np.concatenate([np.asarray(a, dtype=np.float64) for a in ytest])
    Kinv_kB = np.linalg.solve(K, kB)
    S = C - kB.T @ Kinv_kB
    S = 0.5 * (S + S.T)                                   # makematrixsymmetric!, :321
    centre = mub[bs].copy()
    if slip == "wrong_band_mean":
        centre[int(np.flatnonzero(bs == 0)[0])] = mub[1]
    mu = Kinv_kB.T @ resid + centre
    ll = _logpdf(S, yv - mu)
    if slip == "padded_row":
        ll -= 0.5 * LOG2PI
    Ka = np.block([[K, kB], [kB.T, C]])
    cond = np.linalg.norm(Ka, 1) * np.linalg.norm(np.linalg.inv(Ka), 1)
    return ll, cond


def union_identity(oracle, kname, t, y, s, delays, alpha, rho, ttest, ytest, stest, marginalise_b=True):
    """log p(y* | y) = log p([y; y*]) - log p(y) with scipy's multivariate normal on the union model (training constants, test noise
    sigma*^2 + JITTER): the conditional identity the witness must satisfy."""
    from scipy.stats import multivariate_normal
    K, resid, kB, C, bs, mub = blocks(oracle, kname, t, y, s, delays, alpha, rho, ttest, stest, marginalise_b)
    yv = np.concatenate([np.asarray(a, dtype=np.float64) for a in ytest])
    Ka = np.block([[K, kB], [kB.T, C]])
    ra = np.concatenate([resid, yv - mub[bs]])
    joint = multivariate_normal(mean=np.zeros(len(ra)), cov=Ka).logpdf(ra)
    train = multivariate_normal(mean=np.zeros(len(resid)), cov=K).logpdf(resid)
    return joint - train


def bar(cond, ref):
    """The parity bar: max(1e-10, 64 eps cond_1(K_aug)) * max(1, |l_ref|)."""
    return max(1e-10, 64 * np.finfo(np.float64).eps * cond) * max(1.0, abs(ref))
