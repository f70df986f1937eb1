"""An extended-precision restatement of the Hessian and the Fisher information of objective(alpha, rho) over
theta = [alpha_1..alpha_L, rho, tau_1..tau_L] (P = 2L + 1), in numpy.longdouble (x87 80-bit: eps ~1.1e-19) on the CPU, and the
comparator of the Hessian's tests.  It builds on _grad_highprec.py (the model, the blocked Cholesky, X = C^-1, K^-1 = X' X).

With C = K^-1, w = C r, G = w w' - C and D_theta = dKd / dtheta,
    H = T1 - T2 + T3,   T1 = 1/2 sum_ij G_ij d2Kd_ij / dtheta dphi,   T2 = (D_theta w)' C (D_phi w),   T3 = 1/2 tr(C D_theta C D_phi) = F.
For i in band p, j in band q, s = (t_i - tau_p) - (t_j - tau_q), r = |s|, ir = 1 / rho:
    D_alpha_l = (d_pl alpha_q + d_ql alpha_p) k     D_rho = alpha_p alpha_q k_r     D_tau_l = alpha_p alpha_q (d_ql - d_pl) k_s
    OU        x = r ir, e = exp(-x):  k = e, k_r = x ir e, k_s = -sign(s) ir e, k_rr = e x ir^2 (x - 2), k_rs = sign(s) ir^2 e (1 - x),
              k_ss = ir^2 e
    rbf       u = s^2 ir / 4, e = exp(-u):  k = e, k_r = e u ir, k_s = -e s ir / 2, k_rr = e ir^2 u (u - 2), k_rs = s e ir^2 (1 - u) / 2,
              k_ss = -ir e (1 - 2u) / 2
    matern32  a = sqrt3 r ir, e = exp(-a):  k = (1 + a) e, k_r = a^2 e ir, k_s = -3 s ir^2 e, k_rr = e ir^2 a^2 (a - 3),
              k_rs = 3 s ir^3 e (2 - a), k_ss = -3 ir^2 e (1 - a)
    matern52  a = sqrt5 r ir, e = exp(-a):  k = (1 + a + a^2/3) e, k_r = a^2 (1 + a) e ir / 3, k_s = -5/3 s ir^2 (1 + a) e,
              k_rr = ir^2 e a^2 (a^2 - 3a - 3) / 3, k_rs = 5/3 s ir^3 e (2 + 2a - a^2), k_ss = -5/3 ir^2 e (1 + a - a^2)
OU at s = 0 follows the library (include/gpcc_hip.h): sign(0) = 0, so k_s = 0 and k_rs = 0, and k_ss = 1 / rho^2.  These are the
derivatives at 0 of cosh(s / rho), the mean of the kernel's two smooth branches exp(-s / rho) and exp(+s / rho)
(tests/test_hess_highprec_cpu.py checks the Hessian against mpmath with that reading).  Constants are formed in the working type.

The products M_theta = C D_theta use the band structure of D_theta: with Y = k diag(alpha_b), Ys = diag(alpha_b) k_s diag(alpha_b) and
E_l the indicator of band l,  D_alpha_l = E_l Y + Y' E_l  and  D_tau_l = Ys E_l - E_l Ys,  so three full products (C Y', C D_rho, C Ys) and
two band-restricted sets (C[:, l] Y[l, :], C[:, l] Ys[l, :]: one full product's work each) give every M_theta: 10 N^3 flops whatever L.

`tile_hessian` recomputes H and F the way the device does, can inject the slips such an implementation can make, and
with dtype=float64 is the fp64 mirror: the device's algorithm in the device's precision in another rounding order.

The comparator is per block (aa, ar, at, rr, rt, tt) and every ingredient of its bar comes from the CPU:
    bar_B = FACTOR max(e_mirror_B, e_witness_B, floor_B),      FACTOR = _markov_cases.FACTOR (16),
e_mirror_B = max over B of |fp64 mirror - extended| over the mirror's rounding orders (below), e_witness_B the same for the torch
witness (_hess_witness.hessian_and_fisher; left out for OU data with cross-band ties, where torch's abs''(0) = 0 is another convention), floor_B = N 2^-53 max over B of
(|T1| + |T2| + |T3|), the rounding of the sums themselves.

Why the mirror is several runs.  On an ill-conditioned K the mirror's error is one draw of a rounding error amplified by cond_1(K), and a
draw can land near zero in a block.  Measured on the CPU alone, over the 128 rows of the device tests' hyper-parameter envelope
(cond_1(K) up to 1.6e9): with bars made from the LAPACK mirror only, the same mirror with _grad_highprec's 64-blocked Cholesky
in place of LAPACK's -- the same algorithm and precision, another order of the factorisation's sums -- missed them in 9 rows, by up
to 23x (rr and tt of rbf, alpha = 100, rho = 300).  The device's 128-point tile Cholesky is a third such order.  So the order of the
factorisation is part of the mirror: e_mirror is the largest error of its fp64 runs (MIRRORS: LAPACK, 64-blocked, 16-blocked, LAPACK on
the points in the opposite order).  FACTOR and the floor are as they were.

Why one run has blocks of 16.  The device factorises and inverts in 16 x 16 blocks (gpcc_potf2_core): the off-diagonal blocks of
X = L^-1 are products with the inverted diagonal blocks, which on an ill-conditioned K carry more rounding than forward substitution
does.  A 64-blocked run has a single block at N = 40 and none of that.  On the CPU, the 16-blocked run exceeds bars made from the
other three runs in four of the eight rows at N = 40, sigma = 0.05, alpha = 100, rho = 300: rbf with b (rr 1.2 x), rbf without b
(rr 2.8 x, tt 7.1 x), Matern-3/2 with b (rr 5.4 x) and without (rt 1.8 x, tt 2.6 x); test_hess_highprec_cpu.py keeps the measurement.
The last three are the rows, and rr and tt the blocks, where the device exceeded those bars (rr 2.7, tt 3.3; rr 2.2; rr 1.2, tt 3.3),
and it exceeded them nowhere else in 396 rows.  So the mirror runs the device's block size too."""
import math
from dataclasses import dataclass, field

import numpy as np

import _grad_highprec as GH
from _grad_highprec import EPS64, EXTENDED, LD, SKIP_REASON, TILE, cholesky_inverse, inverse_from_factor  # noqa: F401
from _markov_cases import FACTOR

BLOCKS = ("aa", "ar", "at", "rr", "rt", "tt")
TABLES = ("A", "R", "S", "RR", "RS", "SS")      # sum G {k, k_r, k_s, k_rr, k_rs, k_ss} per band pair
ODD = (2, 4)                                    # S and RS are antisymmetric in the band pair


def derivatives(kernel, S, rho):
    """[k, k_r, k_s, k_rr, k_rs, k_ss] over the matrix of lags S, in S's type (see the module's docstring)."""
    T = S.dtype.type
    ir = T(1) / T(rho)
    r = np.abs(S)
    sg = np.sign(S)
    if kernel == "OU":
        x = r * ir
        e = np.exp(-x)
        return [e, x * ir * e, -sg * ir * e, e * x * ir * ir * (x - 2), sg * ir * ir * e * (1 - x), ir * ir * e]
    if kernel == "rbf":
        u = S * S * ir / 4
        e = np.exp(-u)
        return [e, e * u * ir, -e * S * ir / 2, e * ir * ir * u * (u - 2), S * e * ir * ir * (1 - u) / 2, -ir * e * (1 - 2 * u) / 2]
    if kernel == "matern32":
        a = np.sqrt(T(3)) * r * ir
        e = np.exp(-a)
        return [(1 + a) * e, a * a * e * ir, -3 * S * ir * ir * e, e * ir * ir * a * a * (a - 3), 3 * S * ir ** 3 * e * (2 - a),
                -3 * ir * ir * e * (1 - a)]
    if kernel == "matern52":
        a = np.sqrt(T(5)) * r * ir
        e = np.exp(-a)
        c = T(5) / T(3)
        return [(1 + a + a * a / 3) * e, a * a * (1 + a) * e * ir / 3, -c * S * ir * ir * (1 + a) * e,
                ir * ir * e * a * a * (a * a - 3 * a - 3) / 3, c * S * ir ** 3 * e * (2 + 2 * a - a * a), -c * ir * ir * e * (1 + a - a * a)]
    raise ValueError(kernel)


def _problem(kernel, tarray, yarray, stdarray, delays, alpha, rho, mb, T):
    """The model's pieces in the type T."""
    band = np.concatenate([np.full(len(t), l) for l, t in enumerate(tarray)])

    def cat(arrs):
        return np.concatenate([np.asarray(a, np.float64) for a in arrs]).astype(T)

    t, y, sd = cat(tarray), cat(yarray), cat(stdarray)
    ys = [np.asarray(a, np.float64).astype(T) for a in yarray]
    mean = np.array([np.sum(a) / T(len(a)) for a in ys], dtype=T)
    Kn = np.zeros((len(t), len(t)), dtype=T)
    Kn[np.diag_indices(len(t))] = sd * sd
    if mb:
        var = np.array([np.sum((a - m) ** 2) / T(len(a) - 1) if len(a) > 1 else T("nan") for a, m in zip(ys, mean)], dtype=T)
        Kn = Kn + 100 * var[band][:, None] * (band[:, None] == band[None, :])
    return dict(kernel=kernel, L=len(tarray), N=len(t), band=band, t=t, tau=np.asarray(delays, np.float64).astype(T),
                al=np.asarray(alpha, np.float64).astype(T), rho=T(np.float64(rho)), r=y - mean[band], Kn=Kn, T=T)


def _products(C, kd, ab, band, L):
    """[M_theta = C D_theta] from the band structure of D_theta (the module's docstring)."""
    Y = kd[0] * ab[None, :]
    Ys = ab[:, None] * kd[2] * ab[None, :]
    Z = C @ Y.T
    Zs = C @ Ys
    Ma, Mt = [], []
    for l in range(L):
        idx = np.flatnonzero(band == l)
        if len(idx) == len(band):     # one band: D_alpha = 2 k alpha, and D_tau is identically zero
            Ma.append(2 * Z)
            Mt.append(np.zeros_like(Z))
            continue
        m = C[:, idx] @ Y[idx, :]
        m[:, idx] += Z[:, idx]
        Ma.append(m)
        m = -(C[:, idx] @ Ys[idx, :])
        m[:, idx] += Zs[:, idx]
        Mt.append(m)
    return Ma + [C @ (ab[:, None] * kd[1] * ab[None, :])] + Mt


def _dmat(st, th):
    """D_theta written out element by element."""
    L, band, ab, kd = st["L"], st["band"], st["ab"], st["kd"]
    T = st["T"]
    if th == L:
        return ab[:, None] * ab[None, :] * kd[1]
    l = th if th < L else th - L - 1
    e = (band == l).astype(T)
    if th < L:
        return (e[:, None] * ab[None, :] + ab[:, None] * e[None, :]) * kd[0]
    return ab[:, None] * ab[None, :] * kd[2] * (e[None, :] - e[:, None])


def _reverse(p):
    """The same problem with its points in the opposite order (H and F do not depend on the order; their rounding does)."""
    q = dict(p)
    for k in ("band", "t", "r"):
        q[k] = p[k][::-1].copy()
    q["Kn"] = p["Kn"][::-1, ::-1].copy()
    return q


def _state(p, products=True, blocked=0):
    """Factorise and form what both the trace formula and the tiled recomputation need.  st["info"] != 0: K is not positive
    definite in this type (the order of the first non-positive pivot).  fp64: LAPACK's Cholesky and forward substitution, or (blocked = the
    block size) _grad_highprec's blocked Cholesky and blocked inverse."""
    st = dict(p)
    T = p["T"]
    u = p["t"] - p["tau"][p["band"]]
    st["S"] = S = u[:, None] - u[None, :]
    st["kd"] = kd = derivatives(p["kernel"], S, p["rho"])
    st["ab"] = ab = p["al"][p["band"]]
    K = ab[:, None] * ab[None, :] * kd[0] + p["Kn"]
    if T is LD or blocked:
        nb = blocked or GH.NB
        Cf, X, info = cholesky_inverse(K, nb)
        if not info:
            C = inverse_from_factor(X, nb)
    else:   # fp64 as on the device: its own Cholesky, X = L^-1, C = X' X
        from scipy.linalg import lapack, solve_triangular
        Cf, info = lapack.dpotrf(K, lower=1)
        if not info:
            Cf = np.tril(Cf)
            X = solve_triangular(Cf, np.eye(p["N"]), lower=True)
            C = X.T @ X
    st["info"] = int(info)
    if info:
        return st
    z = X @ p["r"]
    st["w"] = X.T @ z
    st["X"], st["C"] = X, C
    st["loglik"] = -(z @ z) / 2 - np.sum(np.log(np.diagonal(Cf))) - p["N"] * np.log(8 * np.arctan(T(1))) / 2
    st["cond"] = float(np.max(np.sum(np.abs(K), 0)) * np.max(np.sum(np.abs(C), 0)))
    if products:
        st["M"] = _products(C, kd, ab, p["band"], p["L"])
    return st


@dataclass
class Reference:
    loglik: float = math.nan
    grad: np.ndarray = None            # float64 [P]
    grad_ld: np.ndarray = None
    H: np.ndarray = None               # float64 [P, P] = T1 - T2 + T3
    F: np.ndarray = None               # float64 [P, P] = T3
    H_ld: np.ndarray = None
    F_ld: np.ndarray = None
    terms: np.ndarray = None           # longdouble [3, P, P]: T1, T2, T3 per entry
    cond: float = math.inf             # 1-norm condition number of K
    info: int = 0                      # 0, or the order of the first non-positive pivot (extended precision)
    N: int = 0
    L: int = 0
    ties: bool = False                 # cross-band pairs at the same shifted time
    bars: dict = None                  # {"H": {block: bar}, "F": {block: bar}} (add_bars)
    e_mirror: dict = None              # {"H": {block: error}, "F": ...}: the fp64 mirror against this reference
    e_witness: dict = None             # the same for the torch witness (None where it does not apply)
    floor: dict = None
    faulted: dict = None               # {fault: (H, F)} float64, where a job asked for them
    parts: dict = field(default_factory=dict, repr=False)


def _d2(st, a, b):
    """d2 Kd / dtheta_a dtheta_b element by element (a <= b)."""
    L, band, ab, kd, T = st["L"], st["band"], st["ab"], st["kd"], st["T"]

    def split(th):
        return (0, th) if th < L else (1, 0) if th == L else (2, th - L - 1)

    def e(l):
        return (band == l).astype(T)

    (ka, la), (kb, lb) = split(a), split(b)
    ap, aq = ab[:, None], ab[None, :]

    def da(l):
        return e(l)[:, None] * aq + ap * e(l)[None, :]

    def dt(l):
        return e(l)[None, :] - e(l)[:, None]

    if ka == 0 and kb == 0:
        return (e(la)[:, None] * e(lb)[None, :] + e(lb)[:, None] * e(la)[None, :]) * kd[0]
    if ka == 0 and kb == 1:
        return da(la) * kd[1]
    if ka == 0:
        return da(la) * dt(lb) * kd[2]
    if kb == 1:
        return ap * aq * kd[3]
    if ka == 1:
        return ap * aq * dt(lb) * kd[4]
    return ap * aq * dt(la) * dt(lb) * kd[5]


def evaluate(kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b=True, keep=False):
    """loglik, grad, H = T1 - T2 + T3, F = T3, the three terms per entry, cond_1(K) and info in extended precision, by the trace
    formulas.  keep=True keeps what tile_hessian needs."""
    args = (kernel, tarray, yarray, stdarray, delays, alpha, rho, marginalise_b)
    st = _state(_problem(*args, LD))
    L, N = st["L"], st["N"]
    ref = Reference(N=N, L=L, info=st["info"])
    if st["info"]:
        return ref
    P = 2 * L + 1
    C, w, M = st["C"], st["w"], st["M"]
    G = w[:, None] * w[None, :] - C
    cross = st["band"][:, None] != st["band"][None, :]
    ref.ties = bool(np.any((st["S"] == 0) & cross))
    g = np.zeros(P, dtype=LD)
    U = []
    for th in range(P):
        D = _dmat(st, th)
        g[th] = np.sum(G * D) / 2
        U.append(D @ w)
    Z = [C @ u for u in U]
    T = np.zeros((3, P, P), dtype=LD)
    for a in range(P):
        for b in range(a, P):
            T[0, a, b] = T[0, b, a] = np.sum(G * _d2(st, a, b)) / 2
            T[1, a, b] = T[1, b, a] = U[a] @ Z[b]
            T[2, a, b] = T[2, b, a] = np.sum(M[a] * M[b].T) / 2
    ref.loglik, ref.cond = float(st["loglik"]), st["cond"]
    ref.grad_ld, ref.grad = g, g.astype(np.float64)
    ref.terms = T
    ref.H_ld, ref.F_ld = T[0] - T[1] + T[2], T[2].copy()
    ref.H, ref.F = ref.H_ld.astype(np.float64), ref.F_ld.astype(np.float64)
    ref.parts = dict(args=args)
    if keep:
        ref.parts["st"] = st
    return ref


# -- the tiled recomputation, with injectable slips ----------------------------------------------------------------------------
def _extend_pad_point(st):
    """The first padded point counted as a real point of the last band: time 0, an identity row of K (so of C), w = 0."""
    T, N, L = st["T"], st["N"], st["L"]
    if N % TILE == 0:
        raise ValueError("no padded point")
    st = dict(st)
    st["N"] = N + 1
    st["band"] = np.append(st["band"], L - 1)
    st["t"] = np.append(st["t"], T(0))
    u = st["t"] - st["tau"][st["band"]]
    st["S"] = u[:, None] - u[None, :]
    st["kd"] = derivatives(st["kernel"], st["S"], st["rho"])
    st["ab"] = st["al"][st["band"]]
    C = np.zeros((N + 1, N + 1), dtype=T)
    C[:N, :N] = st["C"]
    C[N, N] = 1
    st["C"], st["w"] = C, np.append(st["w"], T(0))
    st["M"] = _products(C, st["kd"], st["ab"], st["band"], L)
    return st


MIRRORS = ("lapack", "blocked", "blocked16", "reversed")
BLOCKED = {"blocked": GH.NB, "blocked16": 16}     # 16: the device's pivot block (gpcc_potf2_core)


def tile_hessian(ref, fault=None, dtype=LD, Pa=None, mirror="lapack"):
    """H and F of `ref` (evaluated with keep=True) recomputed as the device does, in `dtype`, over the leading Pa
    parameters (block mode: Pa = L + 1) -> (H[Pa, Pa], F[Pa, Pa]) in dtype, or None if K does not factorise in dtype.
    mirror (fp64 only) chooses the rounding order of the factorisation and of the inverse: LAPACK's Cholesky with forward
    substitution, _grad_highprec's blocked Cholesky and blocked inverse in blocks of 64 or of 16, or LAPACK's on the points in the
    opposite order.
    128-point tiles; per lower tile (I, J) the six band-pair tables of G {k, k_r, k_s, k_rr, k_rs, k_ss}, the transposed pair of an
    off-diagonal tile added (negated for S and RS); u_theta = D_theta w, z_theta = C u_theta, T2 = 1/2 (u_theta.z_phi + u_phi.z_theta);
    M_theta = C D_theta and the trace per tile pair; the finish by the design's block formulas.  Padding contributes exact zeros, so
    the tiles are cut at N instead.
    fault (tests/test_hess_highprec_cpu.py places each one everywhere it can occur):
        ("drop_transpose", x, I, J)   table x: the transposed pair of the off-diagonal tile (I, J) is not added
        ("even_sign", x, I, J)        x in (S, RS): the transposed pair of tile (I, J) is added, not subtracted
        ("even_sign_tab", x)          x in (S, RS): the finished table is symmetrised, not antisymmetrised
        ("no_delta_at", l)            the delta_lm term of (alpha_l, tau_l) is left out
        ("no_delta_tt", l)            the delta_lm term of (tau_l, tau_l) is left out
        ("t2_one_product",)           T2 = 1/2 u_theta.z_phi: the second product is left out.  (u_theta.z_phi = u_phi.z_theta exactly,
                                      C being symmetric: an unsymmetrised T2 of the right size is no error, a forgotten product is.)
        ("t3_once", I, J)             the (i in J, j in I) half of tile pair (I, J), I > J, is left out of the trace
        ("omit_kinv", I, J, Kt)       the term X_Kt,I' X_Kt,J of C_IJ (Kt >= I) is left out of tile (I, J) of the dense C and its mirror
        ("pad_real",)                 the first padded point is counted as a real point of the last band
        ("k2_scale", x, f)            x in (3, 4, 5): k_rr, k_rs or k_ss is f times too large
        ("ou_kss0", v)                k_ss at s = 0 is v / rho^2 (the library: v = 1)
        ("pa_confusion", a)           block mode: the block's parameter a is read from the row of a tau"""
    args = ref.parts["args"]
    if dtype is LD:
        st = dict(ref.parts["st"])
    else:
        p = _problem(*args, dtype)
        st = _state(_reverse(p) if mirror == "reversed" else p, blocked=BLOCKED.get(mirror, 0))
        if st["info"]:
            return None
    T = st["T"]
    L = st["L"]
    P = 2 * L + 1
    Pa = P if Pa is None else Pa
    kind = fault[0] if fault else None
    if kind == "pad_real":
        st = _extend_pad_point(st)
    N, band, al = st["N"], st["band"], st["al"]
    C, w, M = st["C"], st["w"], st["M"]
    kd = list(st["kd"])
    if kind == "k2_scale":
        kd[fault[1]] = kd[fault[1]] * T(fault[2])
    if kind == "ou_kss0":
        kd[5] = np.where(st["S"] == 0, T(fault[1]) / (st["rho"] * st["rho"]), kd[5])
    st["kd"] = kd
    nt = (N + TILE - 1) // TILE
    sl = [slice(I * TILE, min((I + 1) * TILE, N)) for I in range(nt)]
    if kind == "omit_kinv":
        _, I, J, Kt = fault
        X = st["X"]
        d = X[sl[Kt], sl[I]].T @ X[sl[Kt], sl[J]]
        C = C.copy()
        C[sl[I], sl[J]] -= d
        if I != J:
            C[sl[J], sl[I]] -= d.T
        M = []
        for th in range(P):     # M_theta + (the change of C) D_theta: the change lives in two tiles
            D = _dmat(st, th)
            m = st["M"][th].copy()
            m[sl[I], :] -= d @ D[sl[J], :]
            if I != J:
                m[sl[J], :] -= d.T @ D[sl[I], :]
            M.append(m)
    params = list(range(Pa))
    if kind == "pa_confusion":
        params[fault[1]] = L + 1 + min(fault[1], L - 1)
    onehot = (band[:, None] == np.arange(L)[None, :]).astype(T)
    G = w[:, None] * w[None, :] - C
    tot = np.zeros((6, L, L), dtype=T)
    for I in range(nt):
        for J in range(I + 1):
            Ei, Ej = onehot[sl[I]], onehot[sl[J]]
            for x in range(6):
                part = Ei.T @ (G[sl[I], sl[J]] * kd[x][sl[I], sl[J]]) @ Ej
                tot[x] += part
                if I == J or fault == ("drop_transpose", x, I, J):
                    continue
                if x in ODD and fault != ("even_sign", x, I, J):
                    tot[x] -= part.T
                else:
                    tot[x] += part.T

    def tab(x, a, b):
        if x in ODD and fault != ("even_sign_tab", x):
            return (tot[x][a, b] - tot[x][b, a]) / 2
        return (tot[x][a, b] + tot[x][b, a]) / 2

    def asum(x, a):
        return sum(al[q] * tab(x, a, q) for q in range(L))

    def t1(th, ph):
        (k1, l), (k2, n) = [((0, v) if v < L else (1, 0) if v == L else (2, v - L - 1)) for v in (th, ph)]
        if k1 > k2:
            k1, l, k2, n = k2, n, k1, l
        if k1 == 0 and k2 == 0:
            return tab(0, l, n)
        if k1 == 0 and k2 == 1:
            return asum(1, l)
        if k1 == 0:
            return al[n] * tab(2, l, n) - (asum(2, l) if l == n and fault != ("no_delta_at", l) else 0)
        if k2 == 1:
            return sum(al[p] * asum(3, p) for p in range(L)) / 2
        if k1 == 1:
            return -al[n] * asum(4, n)
        if l == n and fault != ("no_delta_tt", l):      # (SS_ll cancels between the two terms and is never added, as on the device)
            return al[l] * sum(al[q] * tab(5, l, q) for q in range(L) if q != l)
        return -(al[l] * al[n] * tab(5, l, n))

    U = {th: _dmat(st, th) @ w for th in set(params)}
    Z = {th: C @ U[th] for th in U}
    H = np.zeros((Pa, Pa), dtype=T)
    F = np.zeros((Pa, Pa), dtype=T)
    for a in range(Pa):
        for b in range(a, Pa):
            th, ph = params[a], params[b]
            t2 = U[th] @ Z[ph] if kind == "t2_one_product" else U[th] @ Z[ph] + U[ph] @ Z[th]
            t3 = T(0)
            for I in range(nt):
                for J in range(I + 1):
                    t3 += np.sum(M[th][sl[I], sl[J]] * M[ph][sl[J], sl[I]].T)
                    if I != J and fault != ("t3_once", I, J):
                        t3 += np.sum(M[th][sl[J], sl[I]] * M[ph][sl[I], sl[J]].T)
            F[a, b] = F[b, a] = t3 / 2
            H[a, b] = H[b, a] = t1(th, ph) - t2 / 2 + t3 / 2
    return H, F


def all_faults(L=3, nt=3, ou=False):
    """Every structural fault of tile_hessian's list in every position it can occur with nt tiles and L bands (the derivative
    slips, which are per kernel, and the block-mode one are listed by the tests)."""
    low = [(I, J) for I in range(nt) for J in range(I)]
    f = [("drop_transpose", x, I, J) for x in range(6) for I, J in low]
    f += [("even_sign", x, I, J) for x in ODD for I, J in low] + [("even_sign_tab", x) for x in ODD]
    f += [("no_delta_at", l) for l in range(L)] + [("no_delta_tt", l) for l in range(L)]
    f += [("t2_one_product",)] + [("t3_once", I, J) for I, J in low]
    f += [("omit_kinv", I, J, Kt) for I in range(nt) for J in range(I + 1) for Kt in range(I, nt)]
    f += [("pad_real",)]
    return f


# -- the comparator -----------------------------------------------------------------------------------------------------------------
def block_masks(L, n=None):
    """{block: boolean [n, n] mask} over the leading n parameters (n = 2L + 1: all six; n = L + 1: aa, ar, rr)."""
    P = 2 * L + 1
    n = P if n is None else n
    kind = np.array([0] * L + [1] + [2] * L)[:n]
    out = {}
    for name, (a, b) in zip(BLOCKS, [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        m = (kind[:, None] == a) & (kind[None, :] == b)
        m = m | m.T
        if m.any():
            out[name] = m
    return out


def _block_max(A, L):
    return {b: float(np.max(np.abs(A[m]))) for b, m in block_masks(L).items()}


def mirror_errors(ref):
    """{mirror: {"H": {block: error}, "F": {block: error}}} of the fp64 mirror's runs that factorise, against `ref`."""
    out = {}
    for which in MIRRORS:
        m = tile_hessian(ref, dtype=np.float64, mirror=which)
        if m is not None:
            out[which] = {"H": _block_max(m[0].astype(LD) - ref.H_ld, ref.L), "F": _block_max(m[1].astype(LD) - ref.F_ld, ref.L)}
    return out


def add_bars(ref, witness=True):
    """The per-block bars of `ref` (evaluated with keep=True), from the fp64 mirror, the torch witness and the floor."""
    L, N = ref.L, ref.N
    ref.e_mirror = None
    for e in mirror_errors(ref).values():
        if ref.e_mirror is None:
            ref.e_mirror = e
        else:
            ref.e_mirror = {w: {b: max(v, e[w][b]) for b, v in ref.e_mirror[w].items()} for w in e}
    ref.e_witness = None
    if witness and not (ref.parts["args"][0] == "OU" and ref.ties):
        import _hess_witness as HW
        try:
            _, _, Hw, Fw = HW.hessian_and_fisher(*ref.parts["args"])
            if np.isfinite(Hw).all() and np.isfinite(Fw).all():
                ref.e_witness = {"H": _block_max(Hw.astype(LD) - ref.H_ld, L), "F": _block_max(Fw.astype(LD) - ref.F_ld, L)}
        except Exception:      # torch's fp64 Cholesky refuses K: no witness for this row
            pass
    size = np.abs(ref.terms[0]) + np.abs(ref.terms[1]) + np.abs(ref.terms[2])
    ref.floor = {"H": {b: N * 2.0 ** -53 * v for b, v in _block_max(size, L).items()},
                 "F": {b: N * 2.0 ** -53 * v for b, v in _block_max(ref.terms[2], L).items()}}
    ref.bars = {}
    for which in ("H", "F"):
        ref.bars[which] = {}
        for b in ref.floor[which]:
            e = [ref.floor[which][b]] + [src[which][b] for src in (ref.e_mirror, ref.e_witness) if src is not None]
            ref.bars[which][b] = FACTOR * max(e)
    return ref


def ratio_blocks(H, F, ref, against=None):
    """{block: error / bar}, the larger of H's and F's, for a full (P x P) or a hyper-block ((L+1) x (L+1)) result; F may be None.
    A block whose bar is 0 (every term exactly zero: the tau rows at L = 1) must be matched exactly.  against: another (H, F) to
    measure the distance to, with ref's bars (a faulted recomputation, in the device's mutation check)."""
    out = {}
    n = np.asarray(H).shape[0]
    wH, wF = (ref.H, ref.F) if against is None else against
    for which, got, want in (("H", H, wH), ("F", F, wF)):
        if got is None:
            continue
        err = np.abs(np.asarray(got, np.float64) - want[:n, :n])
        for b, m in block_masks(ref.L, n).items():
            e, bar = float(np.max(err[m])), ref.bars[which][b]
            r = e / bar if bar > 0 else (0.0 if e == 0 else math.inf)
            r = r if r == r else math.inf       # (NaN counts as a miss)
            out[b] = max(r, out.get(b, 0.0))
    return out


def worst(ratios):
    return max(ratios.values())


def value_bar(ref):
    """The gradient tests' bar of the value: conditioning-scaled, relative to max(1, |loglik|)."""
    return max(1e-11, 64 * EPS64 * ref.cond) * max(1.0, abs(ref.loglik))


def reference_job(job):
    """(kernel, t, y, s, delays, alpha, rho, mb[, faults]) -> the Reference with its bars, without the matrices: a top-level
    function for a process pool.  faults: tile_hessian's faults whose (H, F) are wanted too."""
    try:
        import torch
        torch.set_num_threads(2)
    except Exception:
        pass
    args, faults = job[:8], (job[8] if len(job) > 8 else ())
    ref = evaluate(*args, keep=True)
    if ref.info == 0:
        add_bars(ref)
        ref.faulted = {f: tuple(np.asarray(a, np.float64) for a in tile_hessian(ref, f)) for f in faults}
    ref.parts = {}
    return ref


def mutation_data(ties=False):
    """The mutation checks' case: N = 300 in bands of 100 / 110 / 90 (three tiles, bands crossing both tile edges, 84 padded points),
    tau = (0, 1.5, -2), alpha = (0.8, 1.3, 1.1), rho = 2.2.  ties=True: times on the 2^-10 grid and four points of each later band
    at the shifted time of a point of band 1 (cross-band pairs with s = 0 exactly: what OU's convention at 0 needs)."""
    import _grad_witness as W
    t, y, s = W.ragged_data([100, 110, 90], seed=21)
    delays, alpha, rho = np.array([0.0, 1.5, -2.0]), np.array([0.8, 1.3, 1.1]), 2.2
    if ties:
        t = [np.round(a * 1024) / 1024 for a in t]
        for l, pick in ((1, [3, 40, 77, 99]), (2, [10, 41, 60, 98])):
            t[l][[5, 30, 55, 80]] = t[0][pick] + delays[l]
            t[l] = np.sort(t[l])
    return (t, y, s), delays, alpha, rho
