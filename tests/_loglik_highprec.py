"""The value of gpcc_loglik_batch against extended precision: the cases, the value-only reference, the two bars and a tiled
restatement of the value that can make the slips a tiled factorisation can make.  The device tests are
tests/test_gpu_loglik_highprec.py; tests/test_loglik_highprec_cpu.py checks everything here on the CPU.

Reference.  _grad_highprec.evaluate(value_only=True): K in numpy.longdouble, the blocked Cholesky, z = C^-1 r by blocked forward
substitution, the log-determinant -- bit for bit the loglik of the full evaluate, at a quarter of its time.

Bars, both from the reference side only.
    outer   _hess_highprec.value_bar(ref) = max(1e-11, 64 eps64 cond_1(K)) max(1, |loglik|)          (the project's value bar)
    inner   FACTOR max(e_oracle, N 2^-53) |loglik| + U eps64 sens,  FACTOR = _markov_cases.FACTOR = 16  (_markov_cases.bar)
e_oracle is the relative error of the CPU oracle's fp64 value (oracle.loglik_batch) against the extended value of the same row:
the device is another summation order of the same fp64 factorisation.  sens = 1/2 sum_ij |G_ij K_ij|, G = w w' - K^-1, is what
one ulp of error on every element of K moves the value by, to first order, in units of eps64, and U = 1 the ulps allowed.

Why the second term.  e_oracle is ONE draw of a rounding error.  With b marginalised every same-band element carries
100 var_b ~ 50 beside a kernel value below alpha^2, cond_1(K) is 1e5 ... 2e6 and eps64 sens / |loglik| is 1e-11 ... 9e-11, while
the first term is ~1e-12.  Measured on the CPU: the fp64 tile_value below -- an honest factorisation in another order -- lands at
up to 1.2 of the first term alone on its own elements (three Matern-5/2 rows with b, N = 160, 385, 768), at up to 2.3 on the
oracle's own elements (rbf with b, N = 640), and moves by that much with the number of BLAS threads.  So the first term alone
rejects honest fp64 runs, as the issue foresaw for the device; the remedy it prescribes is this term.  U = 1 is not fitted:
an fp64 element carries half an ulp by being stored and the assembly (an exp, two or three products, the B term) the rest, and
a Cholesky's backward error is of the same form.  element_ulps measures the u of a set of elements as the value feels them;
the CPU test holds the oracle's and tile_value's elements to U on rows with b, the device test the device's
(gpcc_model_matrix), and both hold the elements' first-order displacement to the whole bar on every row measured.  Without b the
term is small beside the first (sens ~ N) and the bar is the issue's.

Cases (CASES): _grad_witness.ragged_data(Nl, seed=N), four kernels, both b-modes, and three reference rows per case (rows()):
random_params(L, 3, seed=N + 1) with row 1 at rho = 0.1 and row 2 at rho = 300, alpha = 2 on every band.  A group of M evaluations
(group()) carries them in its first row, its last row (row 1's parameters again) and its row 2, filler rows from
random_params(L, M, seed=N + 2) between them -- so a reference depends on (data, kernel, b-mode, row), never on the group size or
the path, and the position inside a group is exercised all the same.

tile_value restates the value the way the tiled path forms it: 128-point tiles padded to a whole tile (identity rows, r = 0), the
left-looking update T(I,k) = K(I,k) - sum_j L(I,j) L(k,j)', L(I,k) = T inv(L_kk)', z_I -= L(I,k) w_k, the log-determinant over the
real rows.  In fp64 it is one more summation order of the honest factorisation; with a fault it is what a slip would return."""
import math
from dataclasses import dataclass

import numpy as np

import _grad_highprec as GH
import _grad_witness as W
import _hess_highprec as HH
from _grad_highprec import EPS64, EXTENDED, LD, SKIP_REASON, TILE  # noqa: F401
from _markov_cases import FACTOR

KERNELS = ("OU", "rbf", "matern32", "matern52")
SEPARABLE = ("OU", "matern32", "matern52")      # exp(-c |x - y| / rho) = u_i v_j across a pair of sorted points
COND_MAX = 1e10
U = 1.0             # ulps of error on the elements of K that the inner bar allows for (the module's docstring)

# N -> band lengths (what each size exercises: DESIGN.md 4.6, "Accuracy of the value against extended precision")
CASES = {2: [2], 111: [60, 51], 160: [80, 80], 191: [64, 64, 63], 192: [100, 92], 383: [127, 128, 128], 384: [128, 128, 128],
         385: [129, 127, 129], 640: [256, 384], 641: [128, 384, 129], 768: [384, 384], 1025: [513, 512]}
ROWS = (0, 1, 2)


def data(N):
    return W.ragged_data(CASES[N], seed=N)


def modes(N):
    """The b-modes of a size: b is marginalised only where every band has two points or more."""
    return (True, False) if min(CASES[N]) >= 2 else (False,)


def rows(N):
    """(delays[3, L], alpha[3, L], rho[3]) of the three reference rows."""
    delays, alpha, rho = W.random_params(len(CASES[N]), 3, seed=N + 1)
    rho[1] = 0.1
    rho[2] = 300.0
    alpha[2, :] = 2.0
    return delays, alpha, rho


def group(N, M):
    """(delays[M, L], alpha[M, L], rho[M], {row of the group: reference row}) -- see the module's docstring."""
    d3, a3, r3 = rows(N)
    delays, alpha, rho = W.random_params(len(CASES[N]), M, seed=N + 2)
    which = {}
    for at, src in ((1, 1), (M - 1, 1), (2, 2), (0, 0)):
        if 0 <= at < M:
            delays[at], alpha[at], rho[at] = d3[src], a3[src], r3[src]
            which[at] = src
    if M >= 4:
        del which[1]          # (compared: the first row, the last row and row 2; at M = 3 the last row IS row 2)
    return delays, alpha, rho, which


def args_of(N, kernel, mb, row):
    d3, a3, r3 = rows(N)
    return (kernel, *data(N), d3[row], a3[row], r3[row], mb)


def all_keys(sizes=None):
    return [(N, k, mb, row) for N in (sizes or CASES) for k in KERNELS for mb in modes(N) for row in ROWS]


@dataclass
class Value:
    loglik: float = math.nan
    cond: float = math.inf
    info: int = 0
    N: int = 0
    oracle: float = math.nan        # the CPU oracle's fp64 value of the same row
    e_oracle: float = math.nan      # its relative error against loglik
    sens: float = math.nan          # 1/2 sum_ij |G_ij K_ij|, G = w w' - K^-1: what one ulp on every element moves the value by, / eps64
    seconds: float = 0.0            # the value-only reference's time


def reference(args):
    """The value-only extended reference of one row with the oracle's error beside it."""
    import time

    from oracle import oracle
    kernel, t, y, s, delays, alpha, rho, mb = args
    t0 = time.perf_counter()
    ref = GH.evaluate(*args, value_only=True)
    v = Value(loglik=ref.loglik, cond=ref.cond, info=ref.info, N=ref.N, seconds=time.perf_counter() - t0)
    if ref.info == 0:
        ll, info = oracle.loglik_batch(kernel, t, y, s, np.asarray(delays)[None, :], np.asarray(alpha)[None, :], [rho], mb)
        if info[0] == 0:
            v.oracle = float(ll[0])
            v.e_oracle = abs(v.oracle - v.loglik) / abs(v.loglik)
        K, r = oracle.model_matrix(kernel, t, y, s, delays, alpha, rho, mb)     # fp64: like cond, sens only scales a bar
        v.sens = sensitivity(K, r)
    return v


def _one_blas_thread():
    """A pool of processes with a BLAS thread pool each only gets in its own way."""
    try:
        import threadpoolctl
        threadpoolctl.threadpool_limits(1)
    except ImportError:
        pass


def sensitivity(K, r, dK=None):
    """1/2 sum_ij |G_ij| |dK_ij| with G = w w' - K^-1, w = K^-1 r: the first-order bound of what the element errors dK move the
    value by; dK = None: |K| itself (one unit of relative error on every element)."""
    Ki = np.linalg.inv(np.asarray(K, np.float64))
    w = Ki @ np.asarray(r, np.float64)
    G = np.abs(w[:, None] * w[None, :] - Ki)
    return float(np.sum(G * np.abs(K if dK is None else dK))) / 2


def job(key):
    """(N, kernel, mb, row) -> (key, Value): a top-level function for a process pool that never touches the GPU."""
    _one_blas_thread()
    return key, reference(args_of(*key))


def outer_bar(v):
    return HH.value_bar(v)


def inner_bar(v, u=None):
    """Absolute: the summation-order term and u ulps of element error to first order (u = None: U)."""
    return FACTOR * max(v.e_oracle, v.N * 2.0 ** -53) * abs(v.loglik) + (U if u is None else u) * EPS64 * v.sens


def ratios(x, v):
    """(error / inner bar, error / outer bar) of a value x; NaN counts as a miss."""
    e = abs(float(x) - v.loglik)
    e = e if e == e else math.inf
    return e / inner_bar(v), e / outer_bar(v)


# -- the tiled restatement, with injectable slips -------------------------------------------------------------------------------
def _kern(kernel, S, rho, e=None):
    """k over the lags S in S's type; e replaces exp(-c |s| / rho) where given (OU and Matern)."""
    T = S.dtype.type
    ir = T(1) / T(rho)
    if kernel == "rbf":
        return np.exp(-(S * S) * ir / 4)
    c = {"OU": T(1), "matern32": np.sqrt(T(3)), "matern52": np.sqrt(T(5))}[kernel]
    a = c * np.abs(S) * ir
    e = np.exp(-a) if e is None else e
    if kernel == "OU":
        return e
    if kernel == "matern32":
        return (1 + a) * e
    return (1 + a + a * a / 3) * e


def _fp32_mantissa(x):
    """x with its mantissa rounded to fp32's 24 bits, whatever its exponent (an fp32 factor scaled so that it neither overflows nor
    underflows)."""
    m, e = np.frexp(x)
    return np.ldexp(m.astype(np.float32).astype(x.dtype), e)


def prepare(args, T=np.float64):
    """The padded problem of tile_value in the type T: Kp (identity on the padded rows), rp, and what the element faults need."""
    p = HH._problem(*args, T)
    N = p["N"]
    u = p["t"] - p["tau"][p["band"]]
    ab = p["al"][p["band"]]
    K = ab[:, None] * ab[None, :] * _kern(p["kernel"], u[:, None] - u[None, :], p["rho"]) + p["Kn"]
    nt = (N + TILE - 1) // TILE
    Kp = np.eye(nt * TILE, dtype=T)
    Kp[:N, :N] = K
    rp = np.zeros(nt * TILE, dtype=T)
    rp[:N] = p["r"]
    sd = np.concatenate([np.asarray(a, np.float64) for a in args[3]]).astype(T)
    p.update(u=u, ab=ab, Kp=Kp, rp=rp, nt=nt, sd2=sd * sd, B=np.diagonal(p["Kn"]) - sd * sd)   # (B: 100 var_b per point, or 0)
    return p


def straddle(p):
    """(i, j, B of i's band): the first point i of a band and the last point j of the band before it, where that boundary lies
    inside a tile row; None where no boundary does or b is not marginalised (no B term to misplace)."""
    band = p["band"]
    for i in range(1, p["N"]):
        if band[i] != band[i - 1] and i % TILE != 0 and p["B"][i] != 0:
            return i, i - 1, p["B"][i]
    return None


def _chol_tile(A):
    """(lower factor, its inverse) of a diagonal tile, or (None, order of the first non-positive pivot)."""
    if A.dtype == np.float64:
        try:
            C = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return None, 1
        from scipy.linalg import solve_triangular
        return C, solve_triangular(C, np.eye(A.shape[0]), lower=True)
    C, info = GH._chol_unblocked(A, 0)
    if info:
        return None, info
    return C, GH._tri_inv(C)


def tile_value(p, fault=None):
    """The value of the problem p (prepare) as the tiled path forms it, in p's type -> loglik in that type (NaN where a diagonal
    tile does not factorise).  fault: None, or one of
        ("fp32_tile", I, J)        the assembled elements of tile (I, J), I >= J, are rounded to fp32
        ("drop_kslice", I, k, j)   the last 4 columns of the product L(I,j) L(k,j)', I >= k > j, are left out (one 16 x 16 x 4 step)
        ("z_skip", I, k, f)        the 16-row block f of z_I -= L(I,k) w_k, I > k, is omitted
        ("pad_logdet",)            the first padded diagonal entry counts with the last real row's sigma^2 instead of 1
        ("pad_rhs",)               the first padded entry of r is the last real residual instead of 0
        ("b_straddle",)            the cross-band pair that straddles a band boundary inside a tile row receives the B term
        ("sep_single", I, J)       tile (I, J), I > J (OU, Matern): the separable factors u, v are rounded to fp32 before their product
    A fault that does not exist on p (no padded row, no boundary inside a tile, rbf's factors) raises ValueError."""
    T, N, nt = p["T"], p["N"], p["nt"]
    kind = fault[0] if fault else None
    Kp, rp = p["Kp"], p["rp"]
    sl = [slice(I * TILE, (I + 1) * TILE) for I in range(nt)]
    nreal = N
    k0 = 0                  # the first tile column the fault touches: the columns before it are the clean run's
    if kind in ("fp32_tile", "sep_single", "pad_logdet", "b_straddle"):
        Kp = Kp.copy()
    if kind == "fp32_tile":
        _, I, J = fault
        Kp[sl[I], sl[J]] = Kp[sl[I], sl[J]].astype(np.float32).astype(T)
        k0 = J
    elif kind == "sep_single":
        _, I, J = fault
        if p["kernel"] not in SEPARABLE or I == J:
            raise ValueError("no separable factors")
        ri = np.arange(I * TILE, min((I + 1) * TILE, N))
        cj = np.arange(J * TILE, min((J + 1) * TILE, N))
        c = {"OU": T(1), "matern32": np.sqrt(T(3)), "matern52": np.sqrt(T(5))}[p["kernel"]] / p["rho"]
        x, y = p["u"][ri], p["u"][cj]
        mid = (np.min(np.concatenate([x, y])) + np.max(np.concatenate([x, y]))) / 2
        dn_x, up_x = _fp32_mantissa(np.exp(-(x - mid) * c)), _fp32_mantissa(np.exp((x - mid) * c))
        dn_y, up_y = _fp32_mantissa(np.exp(-(y - mid) * c)), _fp32_mantissa(np.exp((y - mid) * c))
        S = x[:, None] - y[None, :]
        e = np.where(S >= 0, dn_x[:, None] * up_y[None, :], up_x[:, None] * dn_y[None, :])
        blk = p["ab"][ri][:, None] * p["ab"][cj][None, :] * _kern(p["kernel"], S, p["rho"], e) + p["Kn"][np.ix_(ri, cj)]
        Kp[ri[0]:ri[-1] + 1, cj[0]:cj[-1] + 1] = blk
        k0 = J
    elif kind == "b_straddle":
        st = straddle(p)
        if st is None:
            raise ValueError("no band boundary inside a tile row with a B term")
        Kp[st[0], st[1]] += st[2]
        k0 = st[1] // TILE
    elif kind in ("pad_logdet", "pad_rhs"):
        if N == nt * TILE:
            raise ValueError("no padded row")
        k0 = nt - 1
        if kind == "pad_logdet":
            Kp[N, N] = p["sd2"][N - 1]
            nreal = N + 1
        else:
            rp = rp.copy()
            rp[N] = rp[N - 1]
    if kind in ("drop_kslice", "z_skip"):
        k0 = fault[2]
    if fault and "_clean" not in p:
        tile_value(p)
    zonly = kind in ("z_skip", "pad_rhs")      # the factor is the clean run's: only z is formed again
    if fault:
        Lf, z = p["_clean"][0] if zonly else p["_clean"][0].copy(), p["_clean"][1][k0].copy()
        z[N:] = rp[N:]       # (the padded rows of z are untouched before the last column)
    else:
        Lf, z, snaps, invs = np.zeros_like(Kp), rp.copy(), [], []
    for k in range(k0, nt):
        lo = k * TILE
        if not fault:
            snaps.append(z.copy())
        if zonly:
            w = p["_clean"][2][k] @ z[sl[k]]
            z[sl[k]] = w
            if k + 1 < nt:
                dz = Lf[lo + TILE:, sl[k]] @ w
                if kind == "z_skip" and fault[2] == k:
                    at = (fault[1] - k - 1) * TILE + 16 * fault[3]
                    dz[at:at + 16] = 0
                z[lo + TILE:] -= dz
            continue
        P = Kp[lo:, sl[k]] - Lf[lo:, :lo] @ Lf[sl[k], :lo].T          # the tiles (I, k), I >= k, minus their sums over j < k
        if kind == "drop_kslice" and fault[2] == k:
            _, I, _, j = fault
            cols = slice((j + 1) * TILE - 4, (j + 1) * TILE)
            P[(I - k) * TILE:(I - k + 1) * TILE] += Lf[sl[I], cols] @ Lf[sl[k], cols].T
        C, X = _chol_tile(np.tril(P[:TILE]) + np.tril(P[:TILE], -1).T)
        if C is None:
            return T(math.nan)
        Lf[sl[k], sl[k]] = C
        if not fault:
            invs.append(X)
        w = X @ z[sl[k]]
        z[sl[k]] = w
        if k + 1 < nt:
            Lf[lo + TILE:, sl[k]] = P[TILE:] @ X.T
            dz = Lf[lo + TILE:, sl[k]] @ w
            if kind == "z_skip" and fault[2] == k:
                _, I, _, f = fault
                at = (I - k - 1) * TILE + 16 * f
                dz[at:at + 16] = 0
            z[lo + TILE:] -= dz
    if not fault:
        p["_clean"] = (Lf, snaps, invs)
    d = np.diagonal(Lf)[:nreal]
    return -(z @ z) / 2 - np.sum(np.log(d)) - N * np.log(8 * np.arctan(T(1))) / 2


def faults(p):
    """Every fault of tile_value's list in every place it exists on p."""
    nt, N = p["nt"], p["N"]
    out = [("fp32_tile", I, J) for I in range(nt) for J in range(I + 1)]
    out += [("drop_kslice", I, k, j) for k in range(1, nt) for I in range(k, nt) for j in range(k)]
    out += [("z_skip", I, k, f) for k in range(nt) for I in range(k + 1, nt) for f in range(8) if I * TILE + 16 * f < N]
    if N % TILE:
        out += [("pad_logdet",), ("pad_rhs",)]
    if straddle(p) is not None:
        out += [("b_straddle",)]
    if p["kernel"] in SEPARABLE:
        out += [("sep_single", I, J) for I in range(nt) for J in range(I)]
    return out


def element_ulps(key, K):
    """The error of the fp64 elements K of the case `key` against the extended-precision elements, in ulps as the value feels them:
    u = sum |G_ij| |K_ij - Kext_ij| / (eps64 sum |G_ij Kext_ij|) -- the u of the inner bar's second term, so that an element of
    1e-300 that is 500 ulps off (exp of a large argument) weighs what it moves -- and the first-order bound itself,
    1/2 sum |G_ij| |K_ij - Kext_ij| -> (u, bound).  (The extended elements start from t - tau in extended precision: at
    rho = 0.1 the fp64 rounding of that difference alone is ~20 ulps of the elements it feeds.)"""
    q = prepare(args_of(*key), LD)
    N = q["N"]
    Kx = q["Kp"][:N, :N]
    dK = np.abs(np.asarray(K, np.float64).astype(LD) - Kx).astype(np.float64)
    K64, r = Kx.astype(np.float64), q["rp"][:N].astype(np.float64)
    return sensitivity(K64, r, dK) / (EPS64 * sensitivity(K64, r)), sensitivity(K64, r, dK)


def element_job(job_):
    """((N, kernel, mb, row), K) -> element_ulps: a top-level function for a process pool."""
    _one_blas_thread()
    return element_ulps(*job_)


def case_job(job_):
    """((N, kernel, mb), with_faults) -> (case, [Value per row], [error / inner bar of the fp64 tile_value per row], {fault: record}):
    a top-level function for a process pool.  A fault is tried on row 0, then, where that row does not reject it, on row 2 and on
    row 1; its record is (the row that rejected it or None, its relative error on row 0, the largest |faulted - clean| / inner bar
    over the rows tried)."""
    (N, kernel, mb), with_faults = job_
    _one_blas_thread()
    vals = [reference(args_of(N, kernel, mb, row)) for row in ROWS]
    clean, table = [], {}
    for row in (0, 2, 1):
        v = vals[row]
        if v.info:
            clean.append((row, math.inf))
            continue
        p = prepare(args_of(N, kernel, mb, row))
        x0 = float(tile_value(p))
        clean.append((row, ratios(x0, v)[0]))
        if not with_faults:
            continue
        for f in (faults(p) if row == 0 else [f for f, rec in table.items() if rec[0] is None]):
            try:
                x = float(tile_value(p, f))
            except ValueError:      # (a boundary inside a tile row is the same on every row; kept for safety)
                continue
            rel = abs(x - v.loglik) / abs(v.loglik) if x == x else math.inf
            moved = abs(x - x0) / inner_bar(v) if x == x else math.inf
            hit = row if ratios(x, v)[0] > 1.0 else None
            old = table.get(f)
            table[f] = (hit, rel, moved) if old is None else (hit, old[1], max(old[2], moved))
    return (N, kernel, mb), vals, [c for _, c in sorted(clean)], table
