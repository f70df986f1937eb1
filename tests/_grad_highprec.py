"""An extended-precision restatement of objective(alpha, rho) and its gradient [d/dalpha_1..L, d/drho, d/dtau_1..L], in
numpy.longdouble (x87 80-bit on x86: eps ~1.1e-19), on the CPU.  It is the reference of the gradient's edge tests
(tests/test_gpu_gradient_edges.py) and checks itself against the fp64 torch witness, the CPU oracle and mpmath
(tests/test_grad_highprec_cpu.py).

The model is _grad_witness.py's: K = alpha_b alpha_b' k(s; rho) + diag(sigma^2), plus 100 var_b (sample variance, n - 1) on
same-band pairs when b is marginalised, s_ij = (t_i - tau_{b_i}) - (t_j - tau_{b_j}), r = y - mean_b.  The factorisation is a
blocked Cholesky (numpy.linalg does not take longdouble, matmul does), then z = C^-1 r by blocked forward substitution (all the
value needs: evaluate(value_only=True), the reference of tests/_loglik_highprec.py), X = C^-1, w = X' z, K^-1 = X' X,
G = w w' - K^-1, and every derivative is the trace formula  d loglik / d theta = 1/2 sum_ij G_ij dK_ij / d theta.

The kernels' derivatives, with r = |s|:
    OU        k = exp(-r/rho)                      dk/drho = r/rho^2 k            dk/ds = -sign(s) k / rho
    rbf       k = exp(-s^2/(4 rho))                dk/drho = s^2/(4 rho^2) k      dk/ds = -s/(2 rho) k
    matern32  k = (1 + a) e^-a, a = sqrt3 r/rho    dk/da = -a e^-a                da/drho = -a/rho, da/ds = sign(s) sqrt3/rho
    matern52  k = (1 + a + a^2/3) e^-a, a = sqrt5 r/rho    dk/da = -a (1 + a) e^-a / 3
OU's dk/ds at s = 0 is taken as 0 (the mean of the one-sided derivatives -1/rho and +1/rho): the convention of the device
(include/gpcc_hip.h) and of torch's abs'(0) = 0 in the witness.  The other three kernels are differentiable there.

`tile_gradient` recomputes the same gradient from per-(tile, tile, band, band) partial sums in the device's 128-point tiling,
and can inject the slips a tiled implementation can make; the self-checks use it to show that the comparator here rejects them."""
import math
from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble
EXTENDED = bool(np.finfo(LD).eps <= 1e-18)
SKIP_REASON = "numpy.longdouble is not an extended type here (eps %.2e > 1e-18)" % float(np.finfo(LD).eps)
EPS64 = float(np.finfo(np.float64).eps)
TILE = 128
NB = 64          # the Cholesky's block


def _kernel(name, S, rho):
    """k, dk/drho, dk/ds of one kernel over the matrix of lags S (longdouble)."""
    rho = LD(rho)
    r = np.abs(S)
    sg = np.sign(S)                      # sign(0) = 0: OU's dk/ds at s = 0 is 0 (see the module's docstring)
    if name == "OU":
        k = np.exp(-r / rho)
        return k, r / (rho * rho) * k, -sg * k / rho
    if name == "rbf":
        k = np.exp(-(S * S) / (4 * rho))
        return k, (S * S) / (4 * rho * rho) * k, -S / (2 * rho) * k
    if name == "matern32":
        c = np.sqrt(LD(3))
        a = c * r / rho
        e = np.exp(-a)
        dka = -a * e
        return (1 + a) * e, dka * (-a / rho), dka * (sg * c / rho)
    if name == "matern52":
        c = np.sqrt(LD(5))
        a = c * r / rho
        e = np.exp(-a)
        dka = -a * (1 + a) * e / 3
        return (1 + a + a * a / 3) * e, dka * (-a / rho), dka * (sg * c / rho)
    raise ValueError(name)


def _chol_unblocked(A, off):
    """Lower Cholesky factor of the small block A; (C, 0) or (None, order of the first non-positive pivot + off)."""
    n = A.shape[0]
    C = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - C[j, :j] @ C[j, :j]
        if not d > 0:
            return None, off + j + 1
        C[j, j] = np.sqrt(d)
        C[j + 1:, j] = (A[j + 1:, j] - C[j + 1:, :j] @ C[j, :j]) / C[j, j]
    return C, 0


def _tri_inv(C):
    """Inverse of a small lower-triangular block by forward substitution."""
    n = C.shape[0]
    X = np.zeros_like(C)
    for j in range(n):
        X[j, j] = 1 / C[j, j]
        for i in range(j + 1, n):
            X[i, j] = -(C[i, j:i] @ X[j:i, j]) / C[i, i]
    return X


def cholesky_blocked(K, nb=NB):
    """Blocked (right-looking by block column, blocks of nb) Cholesky K = C C' -> (C, [C_kk^-1 per diagonal block], info); info as
    LAPACK potrf."""
    N = K.shape[0]
    C = np.zeros_like(K)
    Xd = []
    for k in range(0, N, nb):
        e = min(k + nb, N)
        A = K[k:e, k:e] - C[k:e, :k] @ C[k:e, :k].T
        Ckk, info = _chol_unblocked(A, k)
        if info:
            return None, None, info
        C[k:e, k:e] = Ckk
        Xkk = _tri_inv(Ckk)
        Xd.append(Xkk)
        if e < N:
            C[e:, k:e] = (K[e:, k:e] - C[e:, :k] @ C[k:e, :k].T) @ Xkk.T
    return C, Xd, 0


def forward_solve(C, Xd, r, nb=NB):
    """z = C^-1 r by blocked forward substitution with the inverted diagonal blocks of cholesky_blocked."""
    z = np.zeros_like(r)
    for b, k in enumerate(range(0, C.shape[0], nb)):
        e = min(k + nb, C.shape[0])
        z[k:e] = Xd[b] @ (r[k:e] - C[k:e, :k] @ z[:k])
    return z


def cholesky_inverse(K, nb=NB):
    """cholesky_blocked and X = C^-1 -> (C, X, info)."""
    N = K.shape[0]
    C, Xd, info = cholesky_blocked(K, nb)
    if info:
        return None, None, info
    X = np.zeros_like(K)
    for b, k in enumerate(range(0, N, nb)):
        X[k:min(k + nb, N), k:min(k + nb, N)] = Xd[b]
    for k in range(nb, N, nb):            # block row k of X: X_k,<k = -X_kk C_k,<k X_<k,<k (X_<k,<k lower triangular)
        e = min(k + nb, N)
        T = np.empty((e - k, k), dtype=K.dtype)
        for j in range(0, k, nb):
            T[:, j:j + nb] = C[k:e, j:k] @ X[j:k, j:j + nb]
        X[k:e, :k] = -X[k:e, k:e] @ T
    return C, X, 0


def inverse_from_factor(X, nb=NB):
    """K^-1 = X' X for X = C^-1 lower triangular: the lower blocks (rows of X from the block's row on), mirrored."""
    N = X.shape[0]
    Kinv = np.empty_like(X)
    for i in range(0, N, nb):
        for j in range(0, i + 1, nb):
            B = X[i:, i:i + nb].T @ X[i:, j:j + nb]
            Kinv[i:i + nb, j:j + nb] = B
            Kinv[j:j + nb, i:i + nb] = B.T
    return Kinv


@dataclass
class Reference:
    loglik: float = math.nan
    grad: np.ndarray = None            # float64 [2L+1]
    grad_ld: np.ndarray = None         # longdouble [2L+1]
    scale: np.ndarray = None           # 1/2 sum_ij |G_ij dK_ij/dtheta| per theta: the size of the summed terms
    cond: float = math.inf             # 1-norm condition number of K
    info: int = 0                      # 0, or the order of the first non-positive pivot (extended precision)
    N: int = 0
    L: int = 0
    parts: dict = field(default_factory=dict, repr=False)


def evaluate(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True, keep=False, value_only=False):
    """The log-likelihood, its gradient, the terms' scale and cond_1(K) in extended precision.  keep=True keeps the matrices
    that tile_gradient needs.  value_only=True: the factor, z = C^-1 r by forward substitution and the log-determinant only -- the
    same loglik bit for bit, no gradient, and cond_1 of the fp64 rounding of K from LAPACK (it only scales a bar)."""
    L = len(tarray)
    band = np.concatenate([np.full(len(t), l) for l, t in enumerate(tarray)])
    t = np.concatenate([np.asarray(a, np.float64) for a in tarray]).astype(LD)
    y = np.concatenate([np.asarray(a, np.float64) for a in yarray]).astype(LD)
    sd = np.concatenate([np.asarray(a, np.float64) for a in stdarray]).astype(LD)
    N = len(t)
    tau = np.asarray(delays, np.float64).astype(LD)
    al = np.asarray(alpha, np.float64).astype(LD)
    mean = np.array([np.mean(np.asarray(a, np.float64).astype(LD)) for a in yarray], dtype=LD)
    u = t - tau[band]
    S = u[:, None] - u[None, :]
    k, dkr, dks = _kernel(kernel, S, np.float64(rho))
    ab = al[band]
    aa = ab[:, None] * ab[None, :]
    K = aa * k
    K[np.diag_indices(N)] += sd * sd
    same = band[:, None] == band[None, :]
    if marginalise_b:
        var = np.array([np.sum((np.asarray(a, np.float64).astype(LD) - m) ** 2) / (len(a) - 1) if len(a) > 1 else LD("nan")
                        for a, m in zip(yarray, mean)], dtype=LD)
        K = K + 100 * var[band][:, None] * same
    ref = Reference(N=N, L=L)
    r = y - mean[band]
    if value_only:
        C, Xd, info = cholesky_blocked(K)
        if info:
            ref.info = info
            return ref
        z = forward_solve(C, Xd, r)
        ref.loglik = float(-(z @ z) / 2 - np.sum(np.log(np.diagonal(C))) - N * np.log(2 * np.pi * LD(1)) / 2)
        ref.cond = float(np.linalg.cond(K.astype(np.float64), 1))
        return ref
    C, X, info = cholesky_inverse(K)
    if info:
        ref.info = info
        return ref
    z = forward_solve(C, [X[k:k + NB, k:k + NB] for k in range(0, N, NB)], r)   # (the value-only route's z, bit for bit)
    w = X.T @ z
    Kinv = inverse_from_factor(X)
    ref.loglik = float(-(z @ z) / 2 - np.sum(np.log(np.diagonal(C))) - N * np.log(2 * np.pi * LD(1)) / 2)
    ref.cond = float(np.max(np.sum(np.abs(K), 0)) * np.max(np.sum(np.abs(Kinv), 0)))
    G = w[:, None] * w[None, :] - Kinv
    g = np.zeros(2 * L + 1, dtype=LD)
    sc = np.zeros(2 * L + 1, dtype=LD)
    onehot = (band[:, None] == np.arange(L)[None, :]).astype(LD)     # N x L
    # d K_ij / d alpha_l = k_ij (delta(b_i, l) alpha_{b_j} + alpha_{b_i} delta(b_j, l))
    for l in range(L):
        dK = k * (onehot[:, l][:, None] * ab[None, :] + ab[:, None] * onehot[:, l][None, :])
        g[l] = np.sum(G * dK) / 2
        sc[l] = np.sum(np.abs(G * dK)) / 2
    # d K_ij / d rho = alpha_{b_i} alpha_{b_j} dk/drho
    dK = aa * dkr
    g[L] = np.sum(G * dK) / 2
    sc[L] = np.sum(np.abs(G * dK)) / 2
    # d s_ij / d tau_l = -delta(b_i, l) + delta(b_j, l)
    for l in range(L):
        dK = aa * dks * (onehot[:, l][None, :] - onehot[:, l][:, None])
        g[L + 1 + l] = np.sum(G * dK) / 2
        sc[L + 1 + l] = np.sum(np.abs(G * dK)) / 2
    ref.grad_ld = g
    ref.grad = g.astype(np.float64)
    ref.scale = sc.astype(np.float64)
    if keep:
        ref.parts = dict(G=G, X=X, w=w, k=k, dkr=dkr, dks=dks, al=al, band=band, u=u, rho=LD(np.float64(rho)), kernel=kernel)
    return ref


# -- the comparator of the device tests ------------------------------------------------------------------------------------------
def bar(ref):
    """The largest |device - reference| accepted for any component: 1e-11 relative to max(1, max|g|), raised to 64 eps64 cond_1(K)
    where K is ill-conditioned (an fp64 Cholesky's backward error is ~eps64 ||K||, so K^-1 and G carry up to ~eps64 cond(K) relative
    error).  Not relative to the size of the summed terms (ref.scale, up to 1e3 max|g| here): that would let a 1e-6 slip in
    dk/drho pass (test_grad_highprec_cpu.py's mutation check)."""
    return max(1e-11, 64 * EPS64 * ref.cond) * max(1.0, float(np.max(np.abs(ref.grad))))


def ratio(g, ref):
    """max |g - ref.grad| / bar(ref): <= 1 passes."""
    return float(np.max(np.abs(np.asarray(g, np.float64) - ref.grad))) / bar(ref)


# -- the gradient from tiled band-pair partials, with injectable slips ----------------------------------------------------------
def tile_gradient(ref, fault=None):
    """The gradient of `ref` (evaluated with keep=True) recomputed as a tiled implementation does: per tile pair (I, J) of the
    128-point tiling (padding to a whole tile), per band pair (p, q), the sums A = sum G k, R = sum G dk/drho, S = sum G dk/ds; the
    lower tiles with the transposed pair of an off-diagonal tile added (S: subtracted), then
        d/dalpha_l = sum_q alpha_q (A_lq + A_ql) / 2,  d/drho = 1/2 sum_pq alpha_p alpha_q R_pq,
        d/dtau_l = -alpha_l sum_q alpha_q (S_lq - S_ql) / 2.
    fault (for the self-checks): None, or one of
        ("drop_transpose", I, J)   the transposed pair of the off-diagonal tile (I, J), I > J, is not added
        ("flip_S", p, q)           S_pq enters with the wrong sign
        ("omit_kinv", I, J, Kt)    the term X_Kt,I' X_Kt,J of (K^-1)_IJ (Kt >= I) is left out of tile (I, J) (and its mirror)
        ("drho_scale", f)          dk/drho is f times too large
        ("pad_real",)              the first padded point is counted as a real point of the last band
    -> longdouble [2L+1]."""
    P = ref.parts
    G, k, dkr, dks, al, band, L = P["G"], P["k"], P["dkr"], P["dks"], P["al"], P["band"], ref.L
    N = ref.N
    nt = (N + TILE - 1) // TILE
    Np = nt * TILE
    bandp = np.full(Np, -1)
    bandp[:N] = band
    Gp = np.zeros((Np, Np), dtype=LD)
    Gp[:N, :N] = G
    kp, drp, dsp = (np.zeros((Np, Np), dtype=LD) for _ in range(3))
    kp[:N, :N], drp[:N, :N], dsp[:N, :N] = k, dkr, dks
    if fault and fault[0] == "pad_real":
        if N == Np:
            raise ValueError("no padded point")
        # a padded point: r = 0 and an identity row/column in the padded K, so w_pad = 0, (K^-1)_pad,pad = 1, G_pad,pad = -1
        Gp[N, N] = -1
        bandp[N] = L - 1
        kk, rr, ss = _kernel(P["kernel"], np.zeros((1, 1), dtype=LD), P["rho"])
        kp[N, N], drp[N, N], dsp[N, N] = kk[0, 0], rr[0, 0], ss[0, 0]
    if fault and fault[0] == "omit_kinv":
        _, I, J, Kt = fault
        X = np.zeros((Np, Np), dtype=LD)
        X[:N, :N] = P["X"]
        xi = X[Kt * TILE:(Kt + 1) * TILE, I * TILE:(I + 1) * TILE]
        xj = X[Kt * TILE:(Kt + 1) * TILE, J * TILE:(J + 1) * TILE]
        d = xi.T @ xj                                    # G = w w' - K^-1: leaving a term of K^-1 out adds it to G
        Gp[I * TILE:(I + 1) * TILE, J * TILE:(J + 1) * TILE] += d
        if I != J:
            Gp[J * TILE:(J + 1) * TILE, I * TILE:(I + 1) * TILE] += d.T
    if fault and fault[0] == "drho_scale":
        drp = drp * LD(fault[1])
    onehot = (bandp[:, None] == np.arange(L)[None, :]).astype(LD)
    tot = np.zeros((3, L, L), dtype=LD)
    for I in range(nt):
        for J in range(I + 1):
            si, sj = slice(I * TILE, (I + 1) * TILE), slice(J * TILE, (J + 1) * TILE)
            Ei, Ej = onehot[si], onehot[sj]
            part = np.stack([Ei.T @ (Gp[si, sj] * m[si, sj]) @ Ej for m in (kp, drp, dsp)])
            tot += part
            if I != J and not (fault and fault[0] == "drop_transpose" and fault[1:] == (I, J)):
                tot[0] += part[0].T
                tot[1] += part[1].T
                tot[2] -= part[2].T
    A, R, S = tot
    if fault and fault[0] == "flip_S":
        S = S.copy()
        S[fault[1], fault[2]] = -S[fault[1], fault[2]]
    g = np.zeros(2 * L + 1, dtype=LD)
    for l in range(L):
        g[l] = np.sum(al * (A[l, :] + A[:, l])) / 2
        g[L + 1 + l] = -al[l] * np.sum(al * (S[l, :] - S[:, l])) / 2
    g[L] = np.sum(al[:, None] * al[None, :] * R) / 2
    return g


def evaluate_job(args):
    """evaluate(*args): a top-level function, for a process pool."""
    return evaluate(*args)
