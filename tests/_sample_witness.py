"""A numpy restatement of one draw of gpcc_sample_batch on the oracle's matrices, through tests/_heldout_witness.blocks:
mu = bbar* + kB*' K^-1 (Y - bbar), C = cB + JITTER + diag(sigma*^2) - kB*' K^-1 kB* (the predictive covariance plus the test noise,
src/gpccfixdelay_marginaliseb.jl:259-289), and the draws mu + chol(C) zeta for given normals zeta (rows of the array).

`slip` injects one of the mistakes the GPU tests' bar must catch: "no_jitter" (JITTER left out), "transpose" (L22' used for L22),
"no_bbar" (bbar* left out of the mean), "shift" (zeta shifted by one test index), "no_b_cross" (the Sigma_b term of kB* dropped)."""
import numpy as np

import _heldout_witness as HW


def draws(oracle, kname, t, y, s, delays, alpha, rho, ttest, stest, zeta, marginalise_b=True, slip=None):
    """-> (draws (n, T), cond_1(K_aug)) for the normals zeta (n, T); stest None: the latent curve (sigma* = 0)."""
    if stest is None:
        stest = [np.zeros(len(a)) for a in ttest]
    hslip = slip if slip in ("no_jitter", "no_b_cross") else None
    K, resid, kB, C, bs, mub = HW.blocks(oracle, kname, t, y, s, delays, alpha, rho, ttest, stest, marginalise_b, hslip)
    Kinv_kB = np.linalg.solve(K, kB)
    S = C - kB.T @ Kinv_kB
    S = 0.5 * (S + S.T)
    mu = Kinv_kB.T @ resid
    if slip != "no_bbar":
        mu = mu + mub[bs]
    Lc = np.linalg.cholesky(S)
    if slip == "transpose":
        Lc = Lc.T
    z = np.asarray(zeta, dtype=np.float64)
    if slip == "shift":
        z = np.roll(z, 1, axis=1)
    Ka = np.block([[K, kB], [kB.T, C]])
    cond = np.linalg.norm(Ka, 1) * np.linalg.norm(np.linalg.inv(Ka), 1)
    return mu[None, :] + z @ Lc.T, cond


def bar(cond, ref):
    """The parity bar (the held-out one): max(1e-10, 64 eps cond_1(K_aug)) * max(1, max |f*|)."""
    return max(1e-10, 64 * np.finfo(np.float64).eps * cond) * max(1.0, float(np.max(np.abs(ref))) if np.size(ref) else 1.0)
