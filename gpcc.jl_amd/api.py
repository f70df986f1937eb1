"""Host-side mirror of the reference's interface for the hot path (Python, because the image has
no Julia; INTEGRATION.md carries the Julia `ccall` shim over the same C ABI).

Names and argument meaning follow /root/reference/src:
  delayedCovariance(kernel, scale, delays, rho, x[, y])   src/delayedCovariance.jl:1-38
  getprobabilities(loglikel[, logpriorpdfvalues])         src/getprobabilities.jl:1-20
  Objective(tarray, yarray, stdarray; kernel)             the closure objective(alpha, rho) of
                                                          src/gpccfixdelay_marginaliseb.jl:133-141
                                                          (marginalise_b=False: src/gpccfixdelay.jl:131-139)
Every numeric result comes from libgpcc_hip.so (HIP kernels); nothing here computes on the CPU.
"""
import collections
import ctypes

import numpy as np

from . import _capi
from ._capi import GpccError, c_double_p, c_int_p


class Kernel:
    """Identity token for one of the reference's kernel functions (GPCC.OU, GPCC.rbf,
    GPCC.matern32, GPCC.matern52; src/util.jl:15-52).  The reference accepts any Julia callable;
    only these four have device implementations."""

    def __init__(self, name):
        self.name = name
        self.id = _capi.KERNEL_IDS[name]

    def __repr__(self):
        return "GPCC.%s" % self.name


OU = Kernel("OU")
rbf = Kernel("rbf")
matern32 = Kernel("matern32")
matern52 = Kernel("matern52")
KERNELS = {k.name: k for k in (OU, rbf, matern32, matern52)}


class PosDefException(np.linalg.LinAlgError):
    """Julia's LinearAlgebra.PosDefException(info): raised by Objective.__call__ like cholesky(K)
    does inside MvNormal(b, K) (marginaliseb.jl:139)."""

    def __init__(self, info):
        super().__init__("matrix is not positive definite; Cholesky factorization failed (info=%d)" % info)
        self.info = info


def _kernel(kernel):
    if isinstance(kernel, Kernel):
        return kernel
    if isinstance(kernel, str) and kernel in KERNELS:
        return KERNELS[kernel]
    raise TypeError("kernel must be one of gpcc_amd.OU / rbf / matern32 / matern52 (got %r); other callables "
                    "have no device implementation" % (kernel,))


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def _ip(a):
    return a.ctypes.data_as(c_int_p)


def _flatten(arrays):
    Nl = np.array([len(a) for a in arrays], dtype=np.int32)
    flat = _d(np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in arrays])) if len(arrays) else _d([])
    return Nl, flat


def _raise_reference_error(err):
    """Maps the C ABI's argument errors back to the exceptions the Julia code raises."""
    if "AssertionError" in err.message:
        raise AssertionError("all(scale .> 0)") from None    # @assert, delayedCovariance.jl:3
    if "is <= 0" in err.message:
        raise ValueError(err.message) from None               # error(...), delayedCovariance.jl:5-7
    raise err


def delayedCovariance(kernel, scale, delays, rho, x, y=None, device=0):
    """delayedCovariance(kernel, scale, delays, rho, x[, y]) -> (sum Nx, sum Ny) ndarray."""
    kernel = _kernel(kernel)
    if y is None:
        y = x
    scale, delays = _d(scale), _d(delays)
    L = len(scale)
    assert L == len(x) == len(y), "L == length(x) == length(y)"   # delayedCovariance.jl:11
    assert len(delays) == L
    Nx, fx = _flatten(x)
    Ny, fy = _flatten(y)
    out = np.empty((int(Ny.sum()), int(Nx.sum())), dtype=np.float64)  # column-major (Nx, Ny)
    try:
        _capi.check(_capi.load().gpcc_covariance(kernel.id, L, _dp(scale), _dp(delays), float(rho), _ip(Nx), _dp(fx),
                                                 _ip(Ny), _dp(fy), _dp(out), int(device)))
    except GpccError as e:
        _raise_reference_error(e)
    return out.T


def getprobabilities(loglikel, logpriorpdfvalues=None, device=0):
    """exp.(joint .- logsumexp(joint)), joint = loglikel .+ logprior; same shape as the input.
    The 1-argument form uses a log-prior of ones like the reference (getprobabilities.jl:3)."""
    ll = _d(loglikel)
    shape = ll.shape
    ll = ll.reshape(-1)
    lp = None
    if logpriorpdfvalues is not None:
        lpa = _d(logpriorpdfvalues)
        if lpa.shape != shape:
            raise ValueError("loglikel and logpriorpdfvalues differ in shape")
        lpa = lpa.reshape(-1)
        lp = _dp(lpa)
    out = np.empty_like(ll)
    _capi.check(_capi.load().gpcc_probabilities(len(ll), _dp(ll), lp, _dp(out), int(device)))
    return out.reshape(shape)


def mvnormal_logpdf(mu, Sigma, x, device=0):
    """logpdf(MvNormal(mu, Sigma), x) with an explicit covariance, on the device (marginaliseb.jl:325);
    raises PosDefException when the Cholesky factorisation fails."""
    Sigma = np.ascontiguousarray(np.asarray(Sigma, dtype=np.float64).T)   # column-major for the ABI
    n = Sigma.shape[0]
    mu, x = _d(mu), _d(x)
    assert Sigma.shape == (n, n) and mu.shape == (n,) and x.shape == (n,)
    ll, info = ctypes.c_double(0.0), ctypes.c_int(0)
    _capi.check(_capi.load().gpcc_mvnormal_logpdf(n, _dp(Sigma), _dp(mu), _dp(x), ctypes.byref(ll), ctypes.byref(info),
                                                  int(device)))
    if info.value > 0:
        raise PosDefException(info.value)
    return ll.value


LooResult = collections.namedtuple("LooResult", "mu var lp loo loglik info mix_lp mix_loo")


def logsumexp_rows(values, p):
    """log sum_m p_m exp(values_m) as gpcc_heldout_mix forms it: one running, max-shifted log-sum-exp over the rows in row order, rows
    with p_m = 0 skipped; NaN if a row with p_m > 0 is NaN; one row of weight 1 gives its own value bitwise."""
    mx, s, nan = -np.inf, 0.0, False
    for x, pm in zip(np.asarray(values, dtype=np.float64), np.asarray(p, dtype=np.float64)):
        if pm == 0.0:
            continue
        if x != x:
            nan = True
            continue
        lx = float(np.log(pm)) + float(x)
        if lx == -np.inf:
            continue
        if s == 0.0:
            mx, s = lx, 1.0
        elif lx <= mx:
            s += float(np.exp(lx - mx))
        else:
            s = s * float(np.exp(mx - lx)) + 1.0
            mx = lx
    if nan:
        return float("nan")
    return -np.inf if s == 0.0 else mx + float(np.log(s))


class Objective:
    """The marginal log-likelihood objective(alpha, rho) of gpccfixdelay, bound to one data set and
    living on one GPU -- or, with devices=[...], replicated on several GPUs of this process (gpcc_create_multi:
    batches are sharded in contiguous blocks, one all-gather collects them).  The delay vector is an argument
    (the reference captures tau in the closure; a grid sweep varies it), so one handle serves a whole delay grid."""

    def __init__(self, tarray, yarray, stdarray, kernel, marginalise_b=True, precision="fp64", device=0,
                 streams=None, slots_per_stream=None, devices=None):
        self._h = None
        self.kernel = _kernel(kernel)
        L = len(tarray)
        assert L == len(yarray) == len(stdarray), "L == length(yarray) == length(tarray) == length(stdarray)"
        Nl, t = _flatten(tarray)
        Ny, y = _flatten(yarray)
        Ns, s = _flatten(stdarray)
        assert np.array_equal(Nl, Ny) and np.array_equal(Nl, Ns), "band lengths differ between t, y, sigma"
        self.L, self.Nl, self.N = L, Nl.copy(), int(Nl.sum())
        self.yflat = y.copy()     # the fluxes in the order they were handed over (the leave-one-out residuals are taken against them)
        self.sflat = s.copy()     # the error bars in the same order (fit.gpcc_grid_noise scales the excess variance by their mean square)
        self.marginalise_b = bool(marginalise_b)
        self.device = int(device)
        lib = _capi.load()
        h = ctypes.c_void_p()
        if devices is None:
            _capi.check(lib.gpcc_create(ctypes.byref(h), L, _ip(Nl), _dp(t), _dp(y), _dp(s), self.kernel.id,
                                        int(self.marginalise_b), _capi.PRECISION_IDS[precision], self.device))
        else:
            devs = np.ascontiguousarray(devices, dtype=np.int32)
            self.device = int(devs[0]) if len(devs) else 0
            _capi.check(lib.gpcc_create_multi(ctypes.byref(h), L, _ip(Nl), _dp(t), _dp(y), _dp(s), self.kernel.id,
                                              int(self.marginalise_b), _capi.PRECISION_IDS[precision], _ip(devs), len(devs)))
        self._h = h
        for key, val in (("streams", streams), ("slots_per_stream", slots_per_stream)):
            if val is not None:
                self.set_option(key, int(val))

    # -- lifetime -------------------------------------------------------------------------------
    def close(self):
        if self._h is not None:
            _capi.load().gpcc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            raise GpccError(rc, _capi.last_error(self._h))

    def set_option(self, key, value):
        self._chk(_capi.load().gpcc_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        return _capi.load().gpcc_get_option(self._h, key.encode())

    def constants(self):
        """(mu_b, Sigma_b diagonal, Y - bbar) as precomputed at marginaliseb.jl:85-98."""
        mu, sb, r = np.empty(self.L), np.empty(self.L), np.empty(self.N)
        self._chk(_capi.load().gpcc_get_constants(self._h, _dp(mu), _dp(sb), _dp(r)))
        return mu, sb, r

    def conditioning(self, M):
        """fp32 handles: (M, 2) array [sum_i K_ii/d_i, max_i K_ii/d_i] of the last batch (gpcc_get_conditioning)."""
        out = np.empty((int(M), 2), dtype=np.float64)
        self._chk(_capi.load().gpcc_get_conditioning(self._h, int(M), _dp(out)))
        return out

    def gathered(self, which=0):
        """Multi-device handles: what the ONE all-gather of the last call left on device `which`.
        After loglik_batch: (loglik[n_devices, blk], info[n_devices, blk]) (padding: NaN / 0).
        After grid_loglik (the fit, sharded by delay): rows[n_devices, blk, L + 4] = [loglik, info, iterations, rho, alpha(L)] per
        fitted delay; device i's row j is delay j * n_devices + i of the grid (round-robin deal)."""
        blk = ctypes.c_long(0)
        self._chk(_capi.load().gpcc_multi_gathered(self._h, int(which), ctypes.byref(blk), None, 0))
        n = self.get_option("n_devices")
        w = self.get_option("gather_width")
        buf = np.empty(w * blk.value * n, dtype=np.float64)
        self._chk(_capi.load().gpcc_multi_gathered(self._h, int(which), ctypes.byref(blk), _dp(buf), buf.size))
        if w != 2:
            return buf.reshape(n, blk.value, w)
        buf = buf.reshape(n, 2, blk.value)
        return buf[:, 0, :], buf[:, 1, :].astype(np.int32)

    def multi_stats(self):
        """Multi-device handles: timing of the last loglik_batch -> (compute_ms per device, gather_ms, total_ms)."""
        n = self.get_option("n_devices")
        comp = np.empty(n, dtype=np.float64)
        g, tot = ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._chk(_capi.load().gpcc_multi_stats(self._h, _dp(comp), ctypes.byref(g), ctypes.byref(tot)))
        return comp, g.value, tot.value

    def chain_trace(self, evaluation=0):
        """Stamps of the last persistent few-evaluation launch (option "chain_trace" = 1): (nt, 80) microseconds (gpcc_chain_trace)."""
        nt = self.get_option("Np") // 128
        out = np.empty(80 * nt, dtype=np.float64)
        self._chk(_capi.load().gpcc_chain_trace(self._h, int(evaluation), _dp(out), out.size))
        return out.reshape(nt, 80)

    def chain_jobs_trace(self, capacity=32768):
        """The workers' jobs of the last persistent launch: (rows, 6) [kind, step, index, fetched, ready, done] (gpcc_chain_jobs_trace)."""
        out = np.empty(6 * capacity, dtype=np.float64)
        n = ctypes.c_long(0)
        self._chk(_capi.load().gpcc_chain_jobs_trace(self._h, _dp(out), capacity, ctypes.byref(n)))
        return out[:6 * n.value].reshape(n.value, 6)

    # -- the hot path ---------------------------------------------------------------------------
    def _params(self, delays, alpha, rho):
        rho = _d(np.atleast_1d(rho))
        M = len(rho)
        delays = _d(np.atleast_2d(delays))
        alpha = _d(np.atleast_2d(alpha))
        if delays.shape != (M, self.L) or alpha.shape != (M, self.L):
            raise ValueError("delays and alpha must be (M, L) = (%d, %d)" % (M, self.L))
        return M, delays, alpha, rho

    def _markov(self, symbol, delays, alpha, rho, shapes, noise=None):
        """The linear-time value or derivative entry `symbol` -> (loglik[M], one array (M,) + shape per shape of shapes, info[M]).
        noise: (kappa, nu) of a noise entry, which takes them behind rho (_noise); None for a plain entry."""
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        params = [delays, alpha, rho]
        if noise is not None:
            params += [self._noise(M, noise[0], "kappa"), self._noise(M, noise[1], "nu")]
        ll = np.empty(M, dtype=np.float64)
        out = [np.empty((M,) + shape, dtype=np.float64) for shape in shapes]
        info = np.zeros(M, dtype=np.int32)
        self._chk(getattr(_capi.load(), symbol)(self._h, M, *[_dp(x) if x is not None else None for x in params + [ll] + out], _ip(info)))
        return (ll, *out, info)

    def loglik_batch(self, delays, alpha, rho):
        """objective for M (tau, alpha, rho) triples -> (loglik[M], info[M]).  info follows LAPACK
        potrf (>0: not positive definite, loglik NaN); -1: alpha <= 0; -2: rho <= 0."""
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        ll = np.empty(M, dtype=np.float64)
        info = np.zeros(M, dtype=np.int32)
        self._chk(_capi.load().gpcc_loglik_batch(self._h, M, _dp(delays), _dp(alpha), _dp(rho), _dp(ll), _ip(info)))
        return ll, info

    def loglik_markov_batch(self, delays, alpha, rho):
        """The same objective in linear time (gpcc_loglik_markov_batch: a Kalman filter over the observations merged by shifted time;
        OU, matern32 and matern52 only) -> (loglik[M], info[M]).  info as loglik_batch, a positive value being the merged position of
        the first predictive variance that is not positive.  rbf, or marginalise_b with more than 4 bands: GpccError (unsupported)."""
        return self._markov("gpcc_loglik_markov_batch", delays, alpha, rho, [])

    def realisations(self, Y):
        """Y of loglik_markov_realisations as one (R, N) array: a list of L arrays (R, N_l) side by side, or the (R, N) array itself."""
        if isinstance(Y, (list, tuple)):
            if len(Y) != self.L:
                raise ValueError("Y must hold L = %d arrays (R, N_l)" % self.L)
            Y = np.concatenate([np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in Y], axis=1)
        Y = _d(np.atleast_2d(Y))
        if Y.shape[1] != self.N or Y.shape[0] < 1:
            raise ValueError("Y must be (R, N) = (R >= 1, %d)" % self.N)
        return Y

    def loglik_markov_realisations(self, Y, delays, alpha, rho, center="own"):
        """The linear-time objective of R flux realisations on this handle's cadence in one pass (gpcc_loglik_markov_multi_batch: per
        parameter row the filter's covariance recursion runs once and drives R means; OU, matern32 and matern52 only) ->
        (loglik[M, R], info[M]).  Y: a list of L arrays (R, N_l), or one (R, N) array, each row in the order the handle took y.
        The model is the handle's: times, sigma, kernel, b-mode and, with marginalise_b, the offsets' prior variances of the y the
        handle was created with.  center: "own" subtracts each realisation's own band means (without marginalise_b the value is then
        that of a fresh Objective on (t, Y_r, sigma)), "handle" the handle's band means, an (R, L) array is subtracted as given.
        info is loglik_markov_batch's and depends on the row only; a row with info != 0 is NaN throughout, a flux that is not finite
        makes its own column NaN.  Cell (m, r) is bitwise the same for any M, R and order; it is not bitwise loglik_markov_batch's.
        rbf, or marginalise_b with more than 4 bands: GpccError (unsupported)."""
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        Y = self.realisations(Y)
        R = Y.shape[0]
        if isinstance(center, str):
            if center not in ("own", "handle"):
                raise ValueError('center must be "own", "handle" or an (R, L) array')
            mean = None
            if center == "own":
                edges = np.concatenate([[0], np.cumsum(self.Nl)])
                mean = _d(np.stack([Y[:, edges[l]:edges[l + 1]].sum(axis=1) / self.Nl[l] for l in range(self.L)], axis=1))
        else:
            mean = _d(center)
            if mean.shape != (R, self.L):
                raise ValueError("center must be (R, L) = (%d, %d)" % (R, self.L))
        ll = np.empty((M, R), dtype=np.float64)
        info = np.zeros(M, dtype=np.int32)
        self._chk(_capi.load().gpcc_loglik_markov_multi_batch(self._h, M, _dp(delays), _dp(alpha), _dp(rho), R, _dp(Y),
                                                              _dp(mean) if mean is not None else None, _dp(ll), _ip(info)))
        return ll, info

    def loglik_markov_resampled(self, Y, delays, alpha, rho, real, counts=None, center="own", sigma_b="own"):
        """The linear-time objective of M rows that each carry their own (tau, alpha, rho) AND their own resampled data set on this
        handle's cadence (gpcc_loglik_markov_resampled_batch; OU, matern32 and matern52 only) -> (loglik[M], info[M]): flux
        randomisation with a refit per realisation, random subset selection, each realisation's own Sigma_b.  Y: the R realisations, a
        list of L arrays (R, N_l) or one (R, N) array, each row in the order the handle took y.  real[m] in [0, R): the realisation of
        row m.  counts: the multiplicities in Y's form (integers >= 0; 0 drops the point, n > 1 is the point once with sigma^2 / n), or
        None: all 1.  loglik[m] is the value of a fresh Objective on the kept points of realisation real[m] with error bars sigma /
        sqrt(count), when center and sigma_b are "own": each realisation's band means and 100 var (n - 1) over its distinct kept
        points (ValueError if a band keeps fewer than 2 while marginalise_b is on).  "handle": the handle's band means / prior
        variances; an (R, L) array is taken as given.  sigma_b is read with marginalise_b only.  A realisation that keeps no point
        gives (0.0, 0).  info is loglik_markov_batch's, a positive value counted among the kept points.  A flux that is not finite
        at a kept point makes the rows of that realisation NaN, and no other.  R is split across calls so that each fits option
        "markov_resample_bytes_max" (16 N bytes a realisation); a row's value does not depend on the split, on M, R or any order.
        ValueError: a real[m] outside [0, R), counts that are negative or of another shape.  rbf, or marginalise_b with more than
        4 bands: GpccError (unsupported)."""
        return self._markov_resampled(Y, delays, alpha, rho, real, counts, center, sigma_b, False)[::2]

    def loglik_grad_markov_resampled(self, Y, delays, alpha, rho, real, counts=None, center="own", sigma_b="own"):
        """loglik_markov_resampled and its exact gradient in linear time (gpcc_loglik_grad_markov_resampled_batch; OU, matern32 and
        matern52 only) -> (loglik[M], grad[M, 2L+1], info[M]), grad[m] = [d/dalpha_1..L, d/drho, d/dtau_1..L] of loglik[m]: the
        gradient a fresh Objective on the kept points of realisation real[m] returns from loglik_grad_markov_batch, the band means and
        Sigma_b being constants of the data.  The arguments, their handling, the split of R across calls and every ValueError are
        loglik_markov_resampled's; loglik and info are bitwise its results.  A row with info != 0 has a NaN gradient; a realisation
        that keeps no point gives 0.0 and a zero gradient; for OU an exact tie in shifted time between two kept points of different
        bands gives the mean of the one-sided derivatives (a tie with a dropped point is no tie)."""
        return self._markov_resampled(Y, delays, alpha, rho, real, counts, center, sigma_b, True)

    def _markov_resampled(self, Y, delays, alpha, rho, real, counts, center, sigma_b, want_grad):
        """loglik_markov_resampled's and loglik_grad_markov_resampled's argument handling and calls -> (loglik, grad or None, info)."""
        from . import markov
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        Y = self.realisations(Y)
        R = Y.shape[0]
        real = np.ascontiguousarray(np.atleast_1d(real), dtype=np.int32)
        if real.shape != (M,) or (M and (real.min() < 0 or real.max() >= R)):
            raise ValueError("real must hold one realisation in [0, R = %d) per row (M = %d)" % (R, M))
        shape = [np.empty(int(n)) for n in self.Nl]
        cnt = None
        if counts is not None:
            cnt = np.ascontiguousarray(np.concatenate(markov._counts(shape, counts, R), axis=1), dtype=np.int32)
        mean, vb = markov.resample_arguments(shape, Y, cnt, center, sigma_b, self.marginalise_b)
        W = 2 * self.L + 1
        ll = np.empty(M, dtype=np.float64)
        grad = np.empty((M, W), dtype=np.float64) if want_grad else None
        info = np.zeros(M, dtype=np.int32)
        per = max(1, int(self.get_option("markov_resample_bytes_max")) // (16 * self.N))
        for r0 in range(0, R, per):
            r1 = min(R, r0 + per)
            rows = np.arange(M) if per >= R else np.flatnonzero((real >= r0) & (real < r1))
            if not len(rows):
                continue
            d, a, rh, rl = _d(delays[rows]), _d(alpha[rows]), _d(rho[rows]), np.ascontiguousarray(real[rows] - r0, dtype=np.int32)
            yk = _d(Y[r0:r1])
            ck = np.ascontiguousarray(cnt[r0:r1]) if cnt is not None else None
            mk = _d(mean[r0:r1]) if mean is not None else None
            vk = _d(vb[r0:r1]) if vb is not None else None
            lk, ik = np.empty(len(rows), dtype=np.float64), np.zeros(len(rows), dtype=np.int32)
            args = (self._h, len(rows), _dp(d), _dp(a), _dp(rh), _ip(rl), r1 - r0, _dp(yk), _ip(ck) if ck is not None else None,
                    _dp(mk) if mk is not None else None, _dp(vk) if vk is not None else None, _dp(lk))
            if want_grad:
                gk = np.empty((len(rows), W), dtype=np.float64)
                self._chk(_capi.load().gpcc_loglik_grad_markov_resampled_batch(*args, _dp(gk), _ip(ik)))
                grad[rows] = gk
            else:
                self._chk(_capi.load().gpcc_loglik_markov_resampled_batch(*args, _ip(ik)))
            ll[rows], info[rows] = lk, ik
        return ll, grad, info

    def predict_markov_batch(self, delays, alpha, rho, ttest, weights=None):
        """predict_batch in linear time (gpcc_predict_markov_batch: two Kalman filters and a combine per row, O(N + T); OU, matern32 and
        matern52 only) -> (mu[M, T], var[M, T], loglik[M], info[M], mix_mu[T], mix_var[T]), what predict_batch returns.  ttest need not
        be sorted.  loglik and info are bitwise loglik_markov_batch's, except info = N + j where the combine of test point j failed;
        failed rows are NaN.  rbf, or marginalise_b with more than 4 bands: GpccError (unsupported)."""
        return self._predict_markov(delays, alpha, rho, ttest, weights, None)

    def _noise_args(self, M, noise):
        """What a noise entry takes behind rho: the pointers of kappa and nu (noise = (kappa, nu), _noise); nothing for a plain entry.
        -> (the arrays, kept alive by the caller; the pointers)."""
        if noise is None:
            return (), ()
        keep = (self._noise(M, noise[0], "kappa"), self._noise(M, noise[1], "nu"))
        return keep, tuple(_dp(x) if x is not None else None for x in keep)

    def _predict_markov(self, delays, alpha, rho, ttest, weights, noise):
        """predict_markov_batch (noise None) and predict_markov_noise_batch (noise = (kappa, nu))."""
        if len(ttest) != self.L:
            raise AssertionError("length(ttest) == L")
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        keep, nptr = self._noise_args(M, noise)
        entry = _capi.load().gpcc_predict_markov_batch if noise is None else _capi.load().gpcc_predict_noise_markov_batch
        Nt, tt = _flatten(ttest)
        T = int(Nt.sum())
        mu = np.empty((M, T), dtype=np.float64)
        var = np.empty((M, T), dtype=np.float64)
        ll = np.empty(M, dtype=np.float64)
        info = np.zeros(M, dtype=np.int32)
        w = mix_mu = mix_var = None
        if weights is not None:
            w = _d(np.asarray(weights, dtype=np.float64).ravel())
            if w.shape != (M,):
                raise ValueError("weights must have M = %d entries" % M)
            mix_mu = np.empty(T, dtype=np.float64)
            mix_var = np.empty(T, dtype=np.float64)
        try:
            self._chk(entry(self._h, M, _dp(delays), _dp(alpha), _dp(rho), *nptr, _ip(Nt), _dp(tt), _dp(w) if w is not None else None,
                            _dp(mu), _dp(var), _dp(mix_mu) if w is not None else None, _dp(mix_var) if w is not None else None,
                            _dp(ll), _ip(info)))
        except GpccError as e:
            _raise_reference_error(e)
        return mu, var, ll, info, mix_mu, mix_var

    def heldout_loglik_markov_batch(self, delays, alpha, rho, ttest, ytest, sigmatest, weights=None):
        """heldout_loglik_batch in linear time (gpcc_heldout_loglik_markov_batch: loglik(training U test) - loglik(training), two
        filters per row) -> (heldout[M], loglik[M], info[M], mix or None).  loglik and info are bitwise loglik_markov_batch's, except
        info = N + j where the predictive variance of test point j was not positive and finite (heldout NaN; there is no test block
        to repair, hence no fallback and no refit mask).  mix = log sum p_m exp(heldout_m), p = weights / sum(weights)."""
        return self._heldout_markov(delays, alpha, rho, ttest, ytest, sigmatest, weights, None)

    def _heldout_markov(self, delays, alpha, rho, ttest, ytest, sigmatest, weights, noise):
        """heldout_loglik_markov_batch (noise None) and heldout_loglik_markov_noise_batch (noise = (kappa, nu))."""
        if len(ttest) != self.L or len(ytest) != self.L or len(sigmatest) != self.L:
            raise AssertionError("length(ttest) == length(ytest) == length(sigmatest) == L")
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        keep, nptr = self._noise_args(M, noise)
        entry = _capi.load().gpcc_heldout_loglik_markov_batch if noise is None else _capi.load().gpcc_heldout_loglik_noise_markov_batch
        Nt, tt = _flatten(ttest)
        Ny, yt = _flatten(ytest)
        Ns, st = _flatten(sigmatest)
        if not (np.array_equal(Nt, Ny) and np.array_equal(Nt, Ns)):
            raise ValueError("band lengths differ between ttest, ytest and sigmatest")
        held = np.empty(M, dtype=np.float64)
        ll = np.empty(M, dtype=np.float64)
        info = np.zeros(M, dtype=np.int32)
        w = mix = None
        if weights is not None:
            w = _d(np.asarray(weights, dtype=np.float64).ravel())
            if w.shape != (M,):
                raise ValueError("weights must have M = %d entries" % M)
            mix = np.empty(1, dtype=np.float64)
        try:
            self._chk(entry(self._h, M, _dp(delays), _dp(alpha), _dp(rho), *nptr, _ip(Nt), _dp(tt), _dp(yt), _dp(st),
                            _dp(w) if w is not None else None, _dp(held), _dp(mix) if w is not None else None, _dp(ll), _ip(info)))
        except GpccError as e:
            _raise_reference_error(e)
        return held, ll, info, (float(mix[0]) if w is not None else None)

    def posterior_offsets_markov_batch(self, delays, alpha, rho):
        """posterior_offsets at M rows in linear time (gpcc_posterior_offsets_markov_batch: the offset block of the filter's final
        state) -> (mu_postb[M, L], Sigma_postb[M, L, L], loglik[M], info[M]); rows with info != 0 are NaN."""
        return self._postb_markov(delays, alpha, rho, None)

    def _postb_markov(self, delays, alpha, rho, noise):
        """posterior_offsets_markov_batch (noise None) and posterior_offsets_markov_noise_batch (noise = (kappa, nu))."""
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        keep, nptr = self._noise_args(M, noise)
        entry = _capi.load().gpcc_posterior_offsets_markov_batch if noise is None else _capi.load().gpcc_posterior_offsets_noise_markov_batch
        mu = np.empty((M, self.L), dtype=np.float64)
        Sig = np.empty((M, self.L, self.L), dtype=np.float64)
        ll = np.empty(M, dtype=np.float64)
        info = np.zeros(M, dtype=np.int32)
        try:
            self._chk(entry(self._h, M, _dp(delays), _dp(alpha), _dp(rho), *nptr, _dp(mu), _dp(Sig), _dp(ll), _ip(info)))
        except GpccError as e:
            _raise_reference_error(e)
        return mu, Sig, ll, info

    def __call__(self, alpha, rho, delays):
        """objective(alpha, rho) for one delay vector, raising what the reference raises."""
        ll, info = self.loglik_batch([delays], [alpha], [rho])
        if info[0] == -1:
            raise AssertionError("all(scale .> 0)")
        if info[0] == -2:
            raise ValueError("ρ=%.8f is <= 0" % rho)
        if info[0] > 0:
            raise PosDefException(int(info[0]))
        return float(ll[0])

    def loglik_grad_batch(self, delays, alpha, rho):
        """objective and its gradient for M (tau, alpha, rho) triples -> (loglik[M], grad[M, 2L+1], info[M]).
        A row of grad is [d/dalpha_1..alpha_L, d/drho, d/dtau_1..tau_L] in the reference's (constrained) parameters; NaN where
        info != 0 (info as loglik_batch).  Always fp64; a multi-device handle computes on its first device."""
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        ll = np.empty(M, dtype=np.float64)
        grad = np.empty((M, 2 * self.L + 1), dtype=np.float64)
        info = np.zeros(M, dtype=np.int32)
        self._chk(_capi.load().gpcc_loglik_grad_batch(self._h, M, _dp(delays), _dp(alpha), _dp(rho), _dp(ll), _dp(grad),
                                                      _ip(info)))
        return ll, grad, info

    def _loo(self, entry, delays, alpha, rho, weights, outputs, noise=None):
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        keep, nptr = self._noise_args(M, noise)
        N = self.N
        names = ("mu", "var", "lp", "loo", "mix_lp", "mix_loo", "loglik", "info")
        want = set(names if outputs is None else outputs)
        if not want <= set(names):
            raise ValueError("unknown outputs %r (of %r)" % (sorted(want - set(names)), names))
        w = None
        if weights is not None:
            w = _d(np.asarray(weights, dtype=np.float64).ravel())
            if w.shape != (M,):
                raise ValueError("weights must have M = %d entries" % M)
        elif outputs is None:
            want -= {"mix_lp", "mix_loo"}
        shapes = {"mu": (M, N), "var": (M, N), "lp": (M, N), "loo": (M,), "mix_lp": (N,), "mix_loo": (1,), "loglik": (M,)}
        buf = {k: np.empty(shapes[k], dtype=np.float64) for k in shapes if k in want}
        info = np.zeros(M, dtype=np.int32) if "info" in want else None
        ptr = {k: (_dp(buf[k]) if k in buf else None) for k in shapes}
        try:
            self._chk(entry(self._h, M, _dp(delays), _dp(alpha), _dp(rho), *nptr, _dp(w) if w is not None else None, ptr["mu"], ptr["var"],
                            ptr["lp"], ptr["loo"], ptr["mix_lp"], ptr["mix_loo"], ptr["loglik"], _ip(info) if info is not None else None))
        except GpccError as e:
            _raise_reference_error(e)
        return LooResult(buf.get("mu"), buf.get("var"), buf.get("lp"), buf.get("loo"), buf.get("loglik"), info, buf.get("mix_lp"),
                         float(buf["mix_loo"][0]) if "mix_loo" in buf else None)

    def loo_batch(self, delays, alpha, rho, weights=None, outputs=None):
        """Exact leave-one-out predictive scores at M rows (tau, alpha, rho) (gpcc_loo_batch) -> LooResult(mu[M, N], var[M, N],
        lp[M, N], loo[M], loglik[M], info[M], mix_lp[N], mix_loo).  Point i, in the order the light curves were handed over (band 1,
        then band 2, ...), has the mean mu, variance var and log-density lp of y_i given every other observation, under exactly the
        model of objective(alpha, rho) (no JITTER); loo = sum_i lp.  loglik and info are bitwise loglik_grad_batch's, except
        info = N + i for the first point whose variance is not positive and finite; failed rows are NaN.  With weights (M entries,
        p = weights / sum(weights), zero-weight rows skipped): mix_lp_i = -log sum_m p_m exp(-lp_mi), the exact LOO log-density of the
        delay mixture with alpha and rho fixed per delay, and mix_loo = sum_i mix_lp_i; None without weights.  outputs: the names to
        compute (default: all); the others come back as None and are never copied."""
        return self._loo(_capi.load().gpcc_loo_batch, delays, alpha, rho, weights, outputs)

    def loo_markov_batch(self, delays, alpha, rho, weights=None, outputs=None):
        """loo_batch in linear time (gpcc_loo_markov_batch: two Kalman filters tapped at every training point before its update, and
        the two-filter combine at the point; OU, matern32 and matern52 only) -> the same LooResult.  loglik and info are bitwise
        loglik_markov_batch's, except info = N + i for the first point (the caller's order) whose variance is not positive and finite.
        rbf, or marginalise_b with more than 4 bands: GpccError (unsupported)."""
        return self._loo(_capi.load().gpcc_loo_markov_batch, delays, alpha, rho, weights, outputs)

    def loglik_grad_markov_batch(self, delays, alpha, rho):
        """loglik_grad_batch in linear time (gpcc_loglik_grad_markov_batch: the Kalman filter's forward sensitivities, one lane per
        (row, parameter); OU, matern32 and matern52 only) -> (loglik[M], grad[M, 2L+1], info[M]).  loglik and info are bitwise
        loglik_markov_batch's; a row of grad is NaN where info != 0.  rbf, or marginalise_b with more than 4 bands: GpccError
        (unsupported)."""
        return self._markov("gpcc_loglik_grad_markov_batch", delays, alpha, rho, [(2 * self.L + 1,)])

    def _noise(self, M, x, name):
        """kappa or nu of the noise entries as a contiguous (M, L) array, or None: an (M, L) array, or (L,) broadcast over the rows."""
        if x is None:
            return None
        x = np.asarray(x, dtype=np.float64)
        if x.shape == (self.L,):
            x = np.broadcast_to(x, (M, self.L))
        if x.shape != (M, self.L):
            raise ValueError("%s must be (M, L) = (%d, %d), (L,) or None" % (name, M, self.L))
        return _d(x)

    def loglik_markov_noise_batch(self, delays, alpha, rho, kappa=None, nu=None):
        """The linear-time objective of M rows that each carry their own (tau, alpha, rho) AND their own noise model
        (gpcc_loglik_noise_markov_batch; OU, matern32 and matern52 only) -> (loglik[M], info[M]): point i of band l is observed with
        the variance kappa_l^2 sigma_i^2 + nu_l, kappa >= 0 the scale of the reported error bars, nu >= 0 an excess variance.  kappa,
        nu: (M, L), (L,) broadcast, or None (all 1 / all 0).  loglik[m] is the value of a fresh Objective on fit.effective_std(sigma,
        kappa[m], nu[m]); at kappa = 1, nu = 0 loglik and info are bitwise loglik_markov_batch's.  info as loglik_markov_batch and,
        after -1 and -2, -3: a kappa or nu of the row is negative or not finite.  rbf, or marginalise_b with more than 4 bands:
        GpccError (unsupported)."""
        return self._markov("gpcc_loglik_noise_markov_batch", delays, alpha, rho, [], noise=(kappa, nu))

    def loglik_grad_markov_noise_batch(self, delays, alpha, rho, kappa=None, nu=None):
        """loglik_markov_noise_batch and its gradient (gpcc_loglik_grad_noise_markov_batch: forward sensitivities, one lane per (row,
        parameter)) -> (loglik[M], grad[M, 4L+1], info[M]), a row of grad being [alpha_1..L, rho, tau_1..L, kappa_1..L, nu_1..L]: the
        first 2L+1 entries as loglik_grad_markov_batch, d/d kappa_l and d/d nu_l behind them.  loglik and info are
        loglik_markov_noise_batch's; a row of grad is NaN where info != 0."""
        return self._markov("gpcc_loglik_grad_noise_markov_batch", delays, alpha, rho, [(4 * self.L + 1,)], noise=(kappa, nu))

    def loglik_hess_markov_noise_batch(self, delays, alpha, rho, kappa=None, nu=None):
        """loglik_grad_markov_noise_batch and the Hessian over [alpha_1..L, rho, kappa_1..L, nu_1..L] in linear time
        (gpcc_loglik_hess_noise_markov_batch: second-order forward sensitivities with the variance's tangents, one lane per (row, pair
        of parameters)) -> (loglik[M], grad[M, 4L+1], hess[M, 3L+1, 3L+1], info[M]).  loglik, grad and info are bitwise
        loglik_grad_markov_noise_batch's; hess is bitwise symmetric and NaN where info != 0; the delays have no rows in it.  A row's
        leading (L+1) x (L+1) block is loglik_hess_hyper_markov_batch's of a fresh Objective on fit.effective_std(sigma, kappa[m],
        nu[m]).  rbf, marginalise_b with more than 4 bands, or matern52 with marginalise_b and 4 bands: GpccError (unsupported)."""
        n = 3 * self.L + 1
        return self._markov("gpcc_loglik_hess_noise_markov_batch", delays, alpha, rho, [(4 * self.L + 1,), (n, n)], noise=(kappa, nu))

    def loglik_hess_full_markov_noise_batch(self, delays, alpha, rho, kappa=None, nu=None):
        """loglik_grad_markov_noise_batch and the FULL Hessian, the delays included, over the gradient row's order [alpha_1..L, rho,
        tau_1..L, kappa_1..L, nu_1..L] in linear time (gpcc_loglik_hess_full_noise_markov_batch: the rows of tau by second-order forward
        sensitivities, one lane per (row, pair with a tau)) -> (loglik[M], grad[M, 4L+1], hess[M, 4L+1, 4L+1], info[M]).  loglik, grad
        and info are bitwise loglik_grad_markov_noise_batch's; the sub-block on the indices {0..L, 2L+1..4L} is bitwise
        loglik_hess_markov_noise_batch's; the leading (2L+1) x (2L+1) block is loglik_hess_markov_batch's of a fresh Objective on
        fit.effective_std(sigma, kappa[m], nu[m]).  hess is bitwise symmetric and NaN where info != 0.  On an OU row where two points of
        different bands have exactly equal shifted times every entry with a tau index is NaN and info stays 0; with one band the tau
        entries are exact zeros.  rbf, marginalise_b with more than 4 bands, or matern52 with marginalise_b and 4 bands: GpccError
        (unsupported)."""
        n = 4 * self.L + 1
        return self._markov("gpcc_loglik_hess_full_noise_markov_batch", delays, alpha, rho, [(n,), (n, n)], noise=(kappa, nu))

    def predict_markov_noise_batch(self, delays, alpha, rho, ttest, kappa=None, nu=None, weights=None):
        """predict_markov_batch of M rows that each carry their own noise model (gpcc_predict_noise_markov_batch) -> the same tuple
        (mu[M, T], var[M, T], loglik[M], info[M], mix_mu[T], mix_var[T]).  kappa, nu: (M, L), (L,) broadcast, or None (all 1 / all 0),
        as loglik_markov_noise_batch.  Row m is what a fresh Objective on fit.effective_std(sigma, kappa[m], nu[m]) returns: the
        latent curve's mean and variance (JITTER included), the noise model entering through the training points.  At kappa = 1,
        nu = 0 every output is bitwise predict_markov_batch's.  info: its codes and -3 (a kappa or nu negative or not finite: the
        row NaN, and the mixture NaN if the row has weight)."""
        return self._predict_markov(delays, alpha, rho, ttest, weights, (kappa, nu))

    def heldout_loglik_markov_noise_batch(self, delays, alpha, rho, ttest, ytest, sigmatest, kappa=None, nu=None, weights=None):
        """heldout_loglik_markov_batch under a per-row noise model (gpcc_heldout_loglik_noise_markov_batch) -> (heldout[M], loglik[M],
        info[M], mix or None).  A test point of band l is scored with the variance kappa_l^2 sigmatest^2 + nu_l (+ JITTER), the
        training points with theirs: row m is a fresh Objective on the effective error bars scoring test points with
        fit.effective_std(sigmatest, kappa[m], nu[m]).  Bitwise heldout_loglik_markov_batch's at kappa = 1, nu = 0; info -3 as above."""
        return self._heldout_markov(delays, alpha, rho, ttest, ytest, sigmatest, weights, (kappa, nu))

    def posterior_offsets_markov_noise_batch(self, delays, alpha, rho, kappa=None, nu=None):
        """posterior_offsets_markov_batch under a per-row noise model (gpcc_posterior_offsets_noise_markov_batch) -> (mu_postb[M, L],
        Sigma_postb[M, L, L], loglik[M], info[M]); bitwise the plain method's at kappa = 1, nu = 0; info -3 as above."""
        return self._postb_markov(delays, alpha, rho, (kappa, nu))

    def loo_markov_noise_batch(self, delays, alpha, rho, kappa=None, nu=None, weights=None, outputs=None):
        """loo_markov_batch under a per-row noise model (gpcc_loo_noise_markov_batch) -> the same LooResult: var_i = h'P_s h +
        kappa_b^2 sigma_i^2 + nu_b, so that (y - mu) / sqrt(var) is standardised by the FITTED error bars -- the check that kappa, nu
        have repaired them.  Row m is a fresh Objective on fit.effective_std(sigma, kappa[m], nu[m]); bitwise loo_markov_batch's at
        kappa = 1, nu = 0; info -3 as above; the mixture mixes rows with different noise models as it mixes any rows."""
        return self._loo(_capi.load().gpcc_loo_noise_markov_batch, delays, alpha, rho, weights, outputs, noise=(kappa, nu))

    def loglik_hess_batch(self, delays, alpha, rho):
        """objective, gradient, Hessian and expected (Fisher) information for M (tau, alpha, rho) triples -> (loglik[M],
        grad[M, P], hess[M, P, P], fisher[M, P, P], info[M]), P = 2L+1 in a gradient row's order [alpha_1..alpha_L, rho,
        tau_1..tau_L].  loglik and grad are bitwise loglik_grad_batch's; hess and fisher are bitwise symmetric; NaN where
        info != 0.  Always fp64; a multi-device handle computes on its first device."""
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        P = 2 * self.L + 1
        ll = np.empty(M, dtype=np.float64)
        grad = np.empty((M, P), dtype=np.float64)
        hess = np.empty((M, P, P), dtype=np.float64)
        fisher = np.empty((M, P, P), dtype=np.float64)
        info = np.zeros(M, dtype=np.int32)
        self._chk(_capi.load().gpcc_loglik_hess_batch(self._h, M, _dp(delays), _dp(alpha), _dp(rho), _dp(ll), _dp(grad),
                                                      _dp(hess), _dp(fisher), _ip(info)))
        return ll, grad, hess, fisher, info

    def loglik_hess_hyper_batch(self, delays, alpha, rho):
        """The hyper-parameter block of loglik_hess_batch -> (loglik[M], grad[M, P], hess[M, L+1, L+1], fisher[M, L+1, L+1], info[M]):
        loglik, grad and info bitwise loglik_grad_batch's, hess and fisher bitwise the leading [alpha_1..alpha_L, rho] block of
        loglik_hess_batch's (the kernels form only that block).  NaN blocks where info != 0."""
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        P, n = 2 * self.L + 1, self.L + 1
        ll = np.empty(M, dtype=np.float64)
        grad = np.empty((M, P), dtype=np.float64)
        hess = np.empty((M, n, n), dtype=np.float64)
        fisher = np.empty((M, n, n), dtype=np.float64)
        info = np.zeros(M, dtype=np.int32)
        self._chk(_capi.load().gpcc_loglik_hess_hyper_batch(self._h, M, _dp(delays), _dp(alpha), _dp(rho), _dp(ll), _dp(grad),
                                                            _dp(hess), _dp(fisher), _ip(info)))
        return ll, grad, hess, fisher, info

    def loglik_hess_hyper_markov_batch(self, delays, alpha, rho):
        """The hyper-parameter block of the Hessian in linear time (gpcc_loglik_hess_hyper_markov_batch: the Kalman filter's second-order
        forward sensitivities, one lane per (row, pair of parameters); OU, matern32 and matern52 only) -> (loglik[M], grad[M, 2L+1],
        hess[M, L+1, L+1], info[M]).  loglik, grad and info are bitwise loglik_grad_markov_batch's; hess is bitwise symmetric and NaN where
        info != 0.  The Fisher information in linear time: loglik_fisher_markov_batch.  The rows of tau: loglik_hess_markov_batch.
        rbf, or marginalise_b with more than 4 bands: GpccError (unsupported)."""
        P, n = 2 * self.L + 1, self.L + 1
        return self._markov("gpcc_loglik_hess_hyper_markov_batch", delays, alpha, rho, [(P,), (n, n)])

    def loglik_hess_markov_batch(self, delays, alpha, rho):
        """The full Hessian in linear time (gpcc_loglik_hess_markov_batch: loglik_hess_hyper_markov_batch's launches, and the rows of
        tau by the same second-order forward sensitivities, one lane per (row, pair); OU, matern32 and matern52 only) -> (loglik[M],
        grad[M, P], hess[M, P, P], info[M]), P = 2L+1 in loglik_hess_batch's order [alpha_1..alpha_L, rho, tau_1..tau_L].  loglik, grad
        and info are bitwise loglik_grad_markov_batch's and hess[:, :L+1, :L+1] bitwise loglik_hess_hyper_markov_batch's; hess is bitwise
        symmetric and NaN where info != 0.  OU has no second derivative by tau on a row where two points of different bands have
        exactly equal shifted times: there every entry with a tau index is NaN while info stays 0 and everything else is untouched --
        use loglik_hess_batch for OU on a grid of delays that collides with the cadence.  The Matern kernels are exact at ties.  The
        Fisher information in linear time: loglik_fisher_markov_batch.  rbf, marginalise_b with more than 4 bands, or matern52 with marginalise_b and 4 bands:
        GpccError (unsupported)."""
        P = 2 * self.L + 1
        return self._markov("gpcc_loglik_hess_markov_batch", delays, alpha, rho, [(P,), (P, P)])

    def loglik_fisher_markov_batch(self, delays, alpha, rho):
        """The expected (Fisher) information in linear time (gpcc_loglik_fisher_markov_batch: the Kalman filter carrying the second
        moments of its means and of their tangents, one lane per (row, pair); OU, matern32 and matern52 only) -> (loglik[M], grad[M, P],
        fisher[M, P, P], info[M]), P = 2L+1 in loglik_hess_batch's order [alpha_1..alpha_L, rho, tau_1..tau_L].  loglik, grad and info
        are bitwise loglik_grad_markov_batch's; fisher is bitwise symmetric, NaN where info != 0, positive semi-definite at any point,
        and depends on the fluxes through the offsets' prior variances only.  On an OU row where two points of different bands have
        exactly equal shifted times every entry with a tau index is NaN while info stays 0 and the (alpha, rho) block is exact -- use
        loglik_hess_batch's Fisher information there.  The Matern kernels are exact at ties.  rbf, marginalise_b with more than 4
        bands, or matern52 with marginalise_b and 4 bands: GpccError (unsupported)."""
        P = 2 * self.L + 1
        return self._markov("gpcc_loglik_fisher_markov_batch", delays, alpha, rho, [(P,), (P, P)])

    def laplace_evidence(self, delays, alpha0, rho0, rhomin=0.1, rhomax=20.0, max_rounds=50, g_tol=1e-6, solver="dense"):
        """The Laplace-marginalised evidence over alpha and rho per row of delays (G, L), from (alpha0[G, L], rho0[G]) (usually
        grid_loglik's output) -> (loglik[G], alpha[G, L], rho[G], log_evidence[G], cov[G, L+1, L+1], info[G], rounds[G],
        (evaluations, batches)).  Prior log-uniform in alpha and in rho on [rhomin, rhomax]: log_evidence is log Z(tau) up to one
        additive constant shared by all delays (getprobabilities(log_evidence) is the delay posterior).  cov: the posterior
        covariance of u = (log alpha, log rho).  info: 0, laplace.NOT_CONVERGED / NOT_MAXIMUM / ON_BOUND (NaN log_evidence), or
        the device's code of a start it could not evaluate.  solver "dense" (default): every Newton round is one
        loglik_hess_hyper_batch; "markov": one loglik_hess_hyper_markov_batch (option "laplace_markov", set around the call and
        restored; OU, matern32, matern52 -- DESIGN.md 4.18)."""
        if solver not in ("dense", "markov"):
            raise ValueError("solver must be 'dense' or 'markov', got %r" % (solver,))
        if solver == "markov":
            before = self.get_option("laplace_markov")
            self.set_option("laplace_markov", 1)
            try:
                return self._laplace_evidence(delays, alpha0, rho0, rhomin, rhomax, max_rounds, g_tol)
            finally:
                self.set_option("laplace_markov", before)
        return self._laplace_evidence(delays, alpha0, rho0, rhomin, rhomax, max_rounds, g_tol)

    def _laplace_evidence(self, delays, alpha0, rho0, rhomin, rhomax, max_rounds, g_tol):
        cand = np.ascontiguousarray(np.atleast_2d(delays), dtype=np.float64)
        G = cand.shape[0]
        if cand.shape[1] != self.L:
            raise ValueError("delays must be (G, %d)" % self.L)
        n = self.L + 1
        a0 = np.ascontiguousarray(np.asarray(alpha0, dtype=np.float64).reshape(G, self.L))
        r0 = np.ascontiguousarray(np.asarray(rho0, dtype=np.float64).reshape(G))
        ll = np.empty(G, dtype=np.float64)
        alpha = np.empty((G, self.L), dtype=np.float64)
        rho = np.empty(G, dtype=np.float64)
        logz = np.empty(G, dtype=np.float64)
        cov = np.empty((G, n, n), dtype=np.float64)
        info = np.empty(G, dtype=np.int32)
        rounds = np.empty(G, dtype=np.int32)
        stats = (ctypes.c_longlong * 2)()
        self._chk(_capi.load().gpcc_laplace_evidence(self._h, G, _dp(cand), _dp(a0), _dp(r0), float(rhomin), float(rhomax),
                                                     int(max_rounds), float(g_tol), _dp(ll), _dp(alpha), _dp(rho), _dp(logz),
                                                     _dp(cov), _ip(info), _ip(rounds), stats))
        return ll, alpha, rho, logz, cov, info, rounds, (int(stats[0]), int(stats[1]))

    def value_and_grad(self, alpha, rho, delays, solver="dense"):
        """(objective(alpha, rho), gradient) for one delay vector: the gradient is a dict {"alpha": (L,), "rho": float,
        "delays": (L,)}; raises what __call__ raises.  solver "dense" (default): loglik_grad_batch; "markov": the same in linear time
        (loglik_grad_markov_batch; OU, matern32, matern52)."""
        if solver not in ("dense", "markov"):
            raise ValueError("solver must be 'dense' or 'markov', got %r" % (solver,))
        ll, grad, info = (self.loglik_grad_markov_batch if solver == "markov" else self.loglik_grad_batch)([delays], [alpha], [rho])
        if info[0] == -1:
            raise AssertionError("all(scale .> 0)")
        if info[0] == -2:
            raise ValueError("ρ=%.8f is <= 0" % rho)
        if info[0] > 0:
            raise PosDefException(int(info[0]))
        g = grad[0]
        return float(ll[0]), {"alpha": g[:self.L].copy(), "rho": float(g[self.L]), "delays": g[self.L + 1:].copy()}

    def loglik_batch_device(self, delays, alpha, rho, out=None, info=None):
        """Same on torch CUDA tensors (float64, contiguous), asynchronous on torch's current stream."""
        import torch
        M = rho.numel()
        for tns in (delays, alpha, rho):
            assert tns.is_cuda and tns.dtype == torch.float64 and tns.is_contiguous()
        assert delays.numel() == M * self.L and alpha.numel() == M * self.L
        if out is None:
            out = torch.empty(M, dtype=torch.float64, device=rho.device)
        if info is None:
            info = torch.empty(M, dtype=torch.int32, device=rho.device)
        stream = torch.cuda.current_stream(rho.device).cuda_stream
        self._chk(_capi.load().gpcc_loglik_batch_device(self._h, M, delays.data_ptr(), alpha.data_ptr(),
                                                        rho.data_ptr(), out.data_ptr(), info.data_ptr(), stream))
        return out, info

    # -- dense views (prediction, tests) ------------------------------------------------------------
    def model_matrix(self, delays, alpha, rho):
        """K = delayedCovariance + Sobs + B (marginaliseb.jl:135), (N, N) ndarray."""
        delays, alpha = _d(delays), _d(alpha)
        K = np.empty((self.N, self.N), dtype=np.float64)
        try:
            self._chk(_capi.load().gpcc_model_matrix(self._h, _dp(delays), _dp(alpha), float(rho), _dp(K)))
        except GpccError as e:
            _raise_reference_error(e)
        return K.T

    def factor(self, delays, alpha, rho):
        """Lower Cholesky factor of K -> (L, info)."""
        delays, alpha = _d(delays), _d(alpha)
        Lf = np.empty((self.N, self.N), dtype=np.float64)
        info = ctypes.c_int(0)
        try:
            self._chk(_capi.load().gpcc_factor_dense(self._h, _dp(delays), _dp(alpha), float(rho), _dp(Lf),
                                                     ctypes.byref(info)))
        except GpccError as e:
            _raise_reference_error(e)
        return Lf.T, info.value

    # -- prediction / posterior of the offsets (reference: marginaliseb.jl:248-252, :259-343) ----------------
    def predict(self, delays, alpha, rho, ttest):
        """predictTest(ttest::Vector{Vector}) at (tau, alpha, rho): joint (mu_pred, Sigma_pred) for the test
        times ttest[l] of every band, Sigma_pred including JITTER*I (marginaliseb.jl:259-289)."""
        assert len(ttest) == self.L
        delays, alpha = _d(delays), _d(alpha)
        Nt, tt = _flatten(ttest)
        n = int(Nt.sum())
        mu = np.empty(n, dtype=np.float64)
        Sig = np.empty((n, n), dtype=np.float64)
        ll, info = ctypes.c_double(0.0), ctypes.c_int(0)
        try:
            self._chk(_capi.load().gpcc_predict(self._h, _dp(delays), _dp(alpha), float(rho), _ip(Nt), _dp(tt), _dp(mu),
                                                _dp(Sig), ctypes.byref(ll), ctypes.byref(info)))
        except GpccError as e:
            _raise_reference_error(e)
        if info.value > 0:
            raise PosDefException(info.value)
        return mu, Sig.T

    def predict_batch(self, delays, alpha, rho, ttest, weights=None):
        """The diagonal posterior predictive at M rows (tau, alpha, rho) on the test times ttest (a list of L arrays, shared by every row),
        and its average over the rows with weights -> (mu[M, T], var[M, T], loglik[M], info[M], mix_mu[T], mix_var[T]) (gpcc_predict_batch).
        Row m is predict()'s mu and diag(Sigma) at that row (JITTER included); loglik and info are bitwise loglik_grad_batch's, and
        failed rows (info != 0) are NaN.  mix_mu = sum p mu, mix_var = sum p (var + (mu - mix_mu)^2), p = weights / sum(weights);
        zero-weight rows are skipped; None without weights.  Always fp64; a multi-device handle computes on its first device."""
        if len(ttest) != self.L:
            raise AssertionError("length(ttest) == L")
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        Nt, tt = _flatten(ttest)
        T = int(Nt.sum())
        mu = np.empty((M, T), dtype=np.float64)
        var = np.empty((M, T), dtype=np.float64)
        ll = np.empty(M, dtype=np.float64)
        info = np.zeros(M, dtype=np.int32)
        w = mix_mu = mix_var = None
        if weights is not None:
            w = _d(np.asarray(weights, dtype=np.float64).ravel())
            if w.shape != (M,):
                raise ValueError("weights must have M = %d entries" % M)
            mix_mu = np.empty(T, dtype=np.float64)
            mix_var = np.empty(T, dtype=np.float64)
        try:
            self._chk(_capi.load().gpcc_predict_batch(self._h, M, _dp(delays), _dp(alpha), _dp(rho), _ip(Nt), _dp(tt),
                                                      _dp(w) if w is not None else None, _dp(mu), _dp(var),
                                                      _dp(mix_mu) if w is not None else None,
                                                      _dp(mix_var) if w is not None else None, _dp(ll), _ip(info)))
        except GpccError as e:
            _raise_reference_error(e)
        return mu, var, ll, info, mix_mu, mix_var

    def heldout_loglik_batch(self, delays, alpha, rho, ttest, ytest, sigmatest, weights=None, fallback=True):
        """The held-out log-likelihood of the test set (ttest, ytest, sigmatest: lists of L arrays, shared by every row) at M rows
        (tau, alpha, rho), and its average over the rows with weights -> (heldout[M], loglik[M], info[M], mix or None, refit_mask[M])
        (gpcc_heldout_loglik_batch).  Row m is predictTest(ttest, ytest, sigmatest) at that row (marginaliseb.jl:311-343); loglik and
        info are bitwise loglik_grad_batch's, except info = N + j where the j-th pivot of the test block Sigma_pred + JITTER I +
        diag(sigmatest^2) failed.  mix = log sum p_m exp(heldout_m), p = weights / sum(weights), zero-weight rows skipped.
        fallback: rows with info > N are recomputed by the reference's rule, the single-row Predictor form (nearestposdef(Sigma;
        minimumeigenvalue = 1e-6), retried once; :327-341), and flagged in refit_mask; if one of them has p > 0 the mixture is
        recomputed here from the final rows with the device's row-order log-sum-exp.  Always fp64; a multi-device handle computes on
        its first device."""
        if len(ttest) != self.L or len(ytest) != self.L or len(sigmatest) != self.L:
            raise AssertionError("length(ttest) == length(ytest) == length(sigmatest) == L")
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        Nt, tt = _flatten(ttest)
        Ny, yt = _flatten(ytest)
        Ns, st = _flatten(sigmatest)
        if not (np.array_equal(Nt, Ny) and np.array_equal(Nt, Ns)):
            raise ValueError("band lengths differ between ttest, ytest and sigmatest")
        held = np.empty(M, dtype=np.float64)
        ll = np.empty(M, dtype=np.float64)
        info = np.zeros(M, dtype=np.int32)
        w = mix = None
        if weights is not None:
            w = _d(np.asarray(weights, dtype=np.float64).ravel())
            if w.shape != (M,):
                raise ValueError("weights must have M = %d entries" % M)
            mix = np.empty(1, dtype=np.float64)
        try:
            self._chk(_capi.load().gpcc_heldout_loglik_batch(self._h, M, _dp(delays), _dp(alpha), _dp(rho), _ip(Nt), _dp(tt), _dp(yt),
                                                             _dp(st), _dp(w) if w is not None else None, _dp(held),
                                                             _dp(mix) if w is not None else None, _dp(ll), _ip(info)))
        except GpccError as e:
            _raise_reference_error(e)
        refit = np.zeros(M, dtype=bool)
        if fallback:
            from .fit import Predictor    # (fit imports this module)
            for m in np.flatnonzero(info > self.N):
                try:
                    held[m] = Predictor(self, delays[m], alpha[m], rho[m])(list(ttest), list(ytest), list(sigmatest))
                except PosDefException:
                    continue             # the retry failed too: the row stays NaN
                refit[m] = True
        mixv = None
        if w is not None:
            p = w / np.sum(w)
            mixv = logsumexp_rows(held, p) if np.any(refit & (p > 0)) else float(mix[0])
        return held, ll, info, mixv, refit

    def sample_batch(self, delays, alpha, rho, ttest, S, seed, weights=None, sigmatest=None, return_noise=False, fallback=True):
        """Joint posterior draws of the light curves at M rows (tau, alpha, rho) on the test times ttest (a list of L arrays, shared by
        every row) -> (draws, draw_row, loglik[M], info[M]) and, with return_noise, zeta (gpcc_sample_batch).  A draw of row m is
        mu_pred + chol(Sigma_pred + JITTER I + diag(sigmatest^2)) zeta with zeta ~ N(0, I_T) (marginaliseb.jl:259-289; sigmatest None:
        the latent curve, else a replicated observation).  Without weights: draws (M * S, T), draw s of row m at row m * S + s, draw_row
        its row.  With weights (M): S draws of the mixture, draw_row[s] the row each one used (rows without a draw: loglik NaN, info
        GPCC_SAMPLE_NOT_DRAWN = -14).  loglik and info of a drawn row are bitwise heldout_loglik_batch's (info = N + j: the j-th pivot
        of the test block failed).  seed: Philox4x64-10 key (gpcc_amd.rng mirrors it).  fallback: the draws of rows with info > N are
        redrawn here with the same zeta -- Objective.predict, nearestposdef(Sigma; minimumeigenvalue = 1e-6) (:327-341), a numpy
        Cholesky --; such rows keep info = N + j with finite draws (that is their flag), and stay NaN if that fails too.  zeta of the
        fallback: the device's with return_noise, else gpcc_amd.rng's (the same normals within 1e-15).  Always fp64; a multi-device
        handle computes on its first device."""
        if len(ttest) != self.L:
            raise AssertionError("length(ttest) == L")
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        Nt, tt = _flatten(ttest)
        T = int(Nt.sum())
        S = int(S)
        st = None
        if sigmatest is not None:
            if len(sigmatest) != self.L:
                raise AssertionError("length(sigmatest) == L")
            Ns, st = _flatten(sigmatest)
            if not np.array_equal(Nt, Ns):
                raise ValueError("band lengths differ between ttest and sigmatest")
        w = None
        if weights is not None:
            w = _d(np.asarray(weights, dtype=np.float64).ravel())
            if w.shape != (M,):
                raise ValueError("weights must have M = %d entries" % M)
        D = S if w is not None else M * S
        draws = np.empty((max(D, 0), T), dtype=np.float64)
        rows = np.empty(max(D, 0), dtype=np.int32)
        zeta = np.empty((max(D, 0), T), dtype=np.float64) if return_noise else None
        ll = np.empty(M, dtype=np.float64)
        info = np.zeros(M, dtype=np.int32)
        try:
            self._chk(_capi.load().gpcc_sample_batch(self._h, M, _dp(delays), _dp(alpha), _dp(rho), _ip(Nt), _dp(tt),
                                                     _dp(st) if st is not None else None, _dp(w) if w is not None else None, S,
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, _dp(draws), _ip(rows),
                                                     _dp(zeta) if zeta is not None else None, _dp(ll), _ip(info)))
        except GpccError as e:
            _raise_reference_error(e)
        if fallback:
            from . import rng
            from .fit import nearestposdef    # (fit imports this module)
            for m in np.flatnonzero(info > self.N):
                sel = np.flatnonzero(rows == m)
                mu, Sig = self.predict(delays[m], alpha[m], rho[m], list(ttest))
                if st is not None:
                    Sig = Sig + np.diag(st ** 2)
                try:
                    Lc = np.linalg.cholesky(nearestposdef(Sig, minimumeigenvalue=1e-6))
                except np.linalg.LinAlgError:
                    continue             # the row stays NaN
                if zeta is not None:
                    z = zeta[sel]
                else:
                    z = rng.normals(seed, T, sel if w is not None else sel - m * S, rng.MIXROW if w is not None else m)
                draws[sel] = mu[None, :] + z @ Lc.T
        out = (draws, rows, ll, info)
        return out + (zeta,) if return_noise else out

    def sample_markov_batch(self, delays, alpha, rho, ttest, S, seed, weights=None, sigmatest=None):
        """sample_batch in linear time (gpcc_sample_markov_batch: Matheron's rule over the Kalman filter, O(N + T) per draw; OU, matern32
        and matern52 only) -> (draws, draw_row, loglik[M], info[M]) in sample_batch's layouts and modes.  The draws have sample_batch's
        distribution N(mu_pred, Sigma_pred + JITTER I + diag(sigmatest^2)) exactly but are other draws (another linear map of other
        normals: 4 (N + T + 1) per draw, so there is no return_noise); draw_row is sample_batch's for the same seed and weights.  loglik
        and info of a drawn row are bitwise predict_markov_batch's; a failed row's draws are NaN (no test block to repair, hence no
        fallback); rows without a draw: loglik NaN, info GPCC_SAMPLE_NOT_DRAWN = -14.  seed: Philox4x64-10 key (gpcc_amd.rng.point_normals
        and gpcc_amd.markov.sample mirror it).  rbf, or marginalise_b with more than 4 bands: GpccError (unsupported)."""
        return self._sample_markov(delays, alpha, rho, ttest, S, seed, weights, sigmatest, None)

    def sample_markov_noise_batch(self, delays, alpha, rho, kappa, nu, ttest, S, seed, sigmatest=None, weights=None):
        """sample_markov_batch of M rows that each carry their own noise model (gpcc_sample_noise_markov_batch) -> the same tuple (draws,
        draw_row, loglik[M], info[M]).  kappa, nu: (M, L), (L,) broadcast, or None (all 1 / all 0), as loglik_markov_noise_batch.  Row
        m's draws are, to rounding, what a fresh Objective on fit.effective_std(sigma, kappa[m], nu[m]) draws with the SAME seed (the
        normals' counters name points) and sigmatest mapped the same way: with sigmatest a test point of band l is a replicated
        observation under the fitted model, noise variance JITTER + kappa_l^2 sigmatest^2 + nu_l; without it the latent curve, noise
        variance JITTER (nu is not added; sigmatest of zeros asks for the latent curve plus the excess variance).  draw_row is
        sample_markov_batch's for the same seed and weights.  At kappa = 1, nu = 0 every output is bitwise sample_markov_batch's.
        loglik and info of a drawn row are bitwise predict_markov_noise_batch's: info -3 (a kappa or nu negative or not finite) makes
        the row's draws NaN and touches no other row; a row without a draw is GPCC_SAMPLE_NOT_DRAWN whatever its kappa, nu.
        gpcc_amd.markov.sample_noise mirrors one row."""
        return self._sample_markov(delays, alpha, rho, ttest, S, seed, weights, sigmatest, (kappa, nu))

    def _sample_markov(self, delays, alpha, rho, ttest, S, seed, weights, sigmatest, noise):
        """sample_markov_batch (noise None) and sample_markov_noise_batch (noise = (kappa, nu))."""
        if len(ttest) != self.L:
            raise AssertionError("length(ttest) == L")
        M, delays, alpha, rho = self._params(delays, alpha, rho)
        keep, nptr = self._noise_args(M, noise)
        entry = _capi.load().gpcc_sample_markov_batch if noise is None else _capi.load().gpcc_sample_noise_markov_batch
        Nt, tt = _flatten(ttest)
        T = int(Nt.sum())
        S = int(S)
        st = None
        if sigmatest is not None:
            if len(sigmatest) != self.L:
                raise AssertionError("length(sigmatest) == L")
            Ns, st = _flatten(sigmatest)
            if not np.array_equal(Nt, Ns):
                raise ValueError("band lengths differ between ttest and sigmatest")
        w = None
        if weights is not None:
            w = _d(np.asarray(weights, dtype=np.float64).ravel())
            if w.shape != (M,):
                raise ValueError("weights must have M = %d entries" % M)
        D = S if w is not None else M * S
        draws = np.empty((max(D, 0), T), dtype=np.float64)
        rows = np.empty(max(D, 0), dtype=np.int32)
        ll = np.empty(M, dtype=np.float64)
        info = np.zeros(M, dtype=np.int32)
        try:
            self._chk(entry(self._h, M, _dp(delays), _dp(alpha), _dp(rho), *nptr, _ip(Nt), _dp(tt), _dp(st) if st is not None else None,
                            _dp(w) if w is not None else None, S, int(seed) & 0xFFFFFFFFFFFFFFFF, _dp(draws), _ip(rows), _dp(ll),
                            _ip(info)))
        except GpccError as e:
            _raise_reference_error(e)
        return draws, rows, ll, info

    def posterior_offsets(self, delays, alpha, rho):
        """(mu_postb, Sigma_postb) of marginaliseb.jl:248-252 (the reference wraps them in MvNormal)."""
        delays, alpha = _d(delays), _d(alpha)
        mu = np.empty(self.L, dtype=np.float64)
        Sig = np.empty((self.L, self.L), dtype=np.float64)
        info = ctypes.c_int(0)
        try:
            self._chk(_capi.load().gpcc_posterior_offsets(self._h, _dp(delays), _dp(alpha), float(rho), _dp(mu), _dp(Sig),
                                                          ctypes.byref(info)))
        except GpccError as e:
            _raise_reference_error(e)
        if info.value > 0:
            raise PosDefException(info.value)
        return mu, Sig.T

    # -- the per-delay fit over a grid (gpcc_grid_loglik) ---------------------------------------------
    def grid_loglik(self, candidatedelays, iterations, numberofrestarts=1, initialrandom=5, rhomin=0.1, rhomax=20.0,
                    seed=1, init_params=None):
        """Optimised log-likelihood per row of candidatedelays (G, L): README.md:172-174 as one native call.
        Returns (loglikel[G], alpha[G, L], rho[G], info[G], iterations[G], (f_calls, rounds))."""
        cand = np.ascontiguousarray(np.atleast_2d(candidatedelays), dtype=np.float64)
        G = cand.shape[0]
        if cand.shape[1] != self.L:
            raise ValueError("candidatedelays must be (G, %d)" % self.L)
        if init_params is not None:
            init_params = _d(init_params)
            if init_params.size != numberofrestarts * initialrandom * (self.L + 1):
                raise ValueError("init_params must be (numberofrestarts, initialrandom, L + 1)")
        ll = np.empty(G, dtype=np.float64)
        alpha = np.empty((G, self.L), dtype=np.float64)
        rho = np.empty(G, dtype=np.float64)
        info = np.empty(G, dtype=np.int32)
        its = np.empty(G, dtype=np.int32)
        stats = (ctypes.c_longlong * 2)()
        self._chk(_capi.load().gpcc_grid_loglik(self._h, G, _dp(cand), int(iterations), int(numberofrestarts),
                                                int(initialrandom), float(rhomin), float(rhomax), int(seed),
                                                _dp(init_params) if init_params is not None else None, _dp(ll),
                                                _dp(alpha), _dp(rho), _ip(info), _ip(its), stats))
        return ll, alpha, rho, info, its, (int(stats[0]), int(stats[1]))

    def initial_params(self, numberofrestarts=1, initialrandom=5, rhomin=0.1, rhomax=20.0, seed=1):
        out = np.empty((numberofrestarts, initialrandom, self.L + 1), dtype=np.float64)
        self._chk(_capi.load().gpcc_initial_params(self._h, int(numberofrestarts), int(initialrandom), float(rhomin),
                                                   float(rhomax), int(seed), _dp(out)))
        return out

    # -- profiling (bench.py) ------------------------------------------------------------------------
    def profile(self, on):
        self._chk(_capi.load().gpcc_profile_enable(self._h, int(bool(on))))

    def profile_reset(self):
        self._chk(_capi.load().gpcc_profile_reset(self._h))

    def profile_get(self):
        """{kernel: (launches, total_ms)} measured with HIP events on the launching stream."""
        out = {}
        for i, name in enumerate(_capi.PROF_NAMES):
            n, ms = ctypes.c_long(0), ctypes.c_double(0.0)
            self._chk(_capi.load().gpcc_profile_get(self._h, i, ctypes.byref(n), ctypes.byref(ms)))
            out[name] = (n.value, ms.value)
        return out


def unpack_params(X, L, rhomin, rhomax):
    """`unpack` of marginaliseb.jl:112-126 through the library (host arithmetic, no device needed)."""
    X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.float64)
    M = X.shape[0]
    alpha = np.empty((M, L), dtype=np.float64)
    rho = np.empty(M, dtype=np.float64)
    _capi.check(_capi.load().gpcc_unpack_params(M, int(L), _dp(X), float(rhomin), float(rhomax), _dp(alpha), _dp(rho)))
    return alpha, rho


def selftest(device=0, rate=True):
    """f64 MFMA fragment-map check (+ measured fp64 MFMA TFLOP/s)."""
    tf = ctypes.c_double(0.0)
    _capi.check(_capi.load().gpcc_selftest(int(device), ctypes.byref(tf) if rate else None))
    return tf.value


def build_info():
    """What the loaded library was built from: "src=<hash of its sources> defines=[...]" (gpcc_build_info)."""
    return _capi.load().gpcc_build_info().decode()
