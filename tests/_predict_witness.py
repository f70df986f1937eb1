"""A numpy restatement of the per-row predictive mean and variance of gpcc_predict_batch (src/gpccfixdelay_marginaliseb.jl:259-307; the
fixed-b variant src/gpccfixdelay.jl:244-266) on the oracle's matrices, and the two-pass mixture over rows.  It follows
tests/test_gpu_parity.py's _reference_predict, but returns the diagonal: var = diag(cB) - |L^-1 kB*|^2 + JITTER per column.

`slip` injects one of the mistakes the GPU tests' bar must catch: "no_jitter", "no_sigma_b_cross" (the Sigma_b term of kB* dropped),
"skip_tile_row" (the partial of training tile row 0 missed), "wrong_band" (the first test point of band 0 evaluated as band 1)."""
import numpy as np
from scipy.linalg import solve_triangular

JITTER = 1e-8
TILE = 128


def _bands(arrays):
    return np.concatenate([np.full(len(a), l, dtype=int) for l, a in enumerate(arrays)]) if len(arrays) else np.zeros(0, int)


def predict_row(oracle, kname, t, y, s, delays, alpha, rho, ttest, marginalise_b=True, slip=None):
    """-> (mu[T], var[T], cond_1(K), max diag(cB)) at one (tau, alpha, rho)."""
    L = len(t)
    K, resid = oracle.model_matrix(kname, t, y, s, delays, alpha, rho, marginalise_b)     # K (+ B), Y - bbar (Y - Qb)
    mub = np.array([np.mean(a) for a in y])
    Sigb = 100 * np.array([np.var(a, ddof=1) for a in y]) if marginalise_b else np.zeros(L)
    bt = _bands(t)
    bs = _bands(ttest)
    ttest = [np.asarray(a, dtype=np.float64) for a in ttest]
    kB = oracle.delayed_covariance(kname, alpha, delays, rho, t, ttest)
    if slip == "wrong_band":   # the first test point of band 0 evaluated as a point of band 1 (its time and position kept)
        j = int(np.flatnonzero(bs == 0)[0])
        one = [np.zeros(0) for _ in range(L)]
        one[1] = ttest[0][:1]
        kB[:, j] = oracle.delayed_covariance(kname, alpha, delays, rho, t, one)[:, 0]
        bs = bs.copy()
        bs[j] = 1
    if slip != "no_sigma_b_cross":
        kB = kB + (bt[:, None] == bs[None, :]) * Sigb[bt][:, None]
    cdiag = np.asarray(alpha, float)[bs] ** 2 + Sigb[bs]                    # alpha_q^2 k(0) (+ Sigma_b_q)
    Lc = np.linalg.cholesky(K)
    V = solve_triangular(Lc, kB, lower=True)
    if slip == "skip_tile_row":
        V = V[TILE:]
    var = cdiag - np.sum(V * V, axis=0) + (0.0 if slip == "no_jitter" else JITTER)
    mu = kB.T @ np.linalg.solve(K, resid) + mub[bs]
    cond = np.linalg.norm(K, 1) * np.linalg.norm(np.linalg.inv(K), 1)
    return mu, var, cond, float(np.max(cdiag)) if len(cdiag) else 0.0


def predict_rows(oracle, kname, t, y, s, delays, alpha, rho, ttest, marginalise_b=True, slip=None):
    """-> (mu[M, T], var[M, T], cond[M], cmax[M]) for M rows."""
    out = [predict_row(oracle, kname, t, y, s, delays[m], alpha[m], rho[m], ttest, marginalise_b, slip) for m in range(len(rho))]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
            np.array([o[3] for o in out]))


def mixture(mu, var, weights):
    """Two-pass mixture of rows: p = w / sum w, mix_mu = sum p mu, mix_var = sum p (var + (mu - mix_mu)^2); zero-weight rows skipped."""
    w = np.asarray(weights, dtype=np.float64)
    p = w / np.sum(w)
    keep = p > 0
    p, mu, var = p[keep], np.asarray(mu)[keep], np.asarray(var)[keep]
    mix_mu = np.sum(p[:, None] * mu, axis=0)
    mix_var = np.sum(p[:, None] * (var + (mu - mix_mu) ** 2), axis=0)
    return mix_mu, mix_var


def bar(cond, scale):
    """The parity bar: max(1e-10, 64 eps cond_1(K)) times a scale (max(1, max|mu_ref|) for mu, max diag(cB) for var)."""
    return max(1e-10, 64 * np.finfo(np.float64).eps * cond) * scale
