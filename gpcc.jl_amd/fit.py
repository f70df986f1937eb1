"""gpcc(): the per-delay model fit of the reference (src/gpccfixdelay_marginaliseb.jl:46-53, :56-352),
host logic in Python over the device objective.  A whole grid of candidate delays is fitted in
lock-step (neldermead.BatchedNelderMead): every optimiser round is ONE gpcc_loglik_batch call.

Restated from the reference: parameter packing `unpack` (:112-126), initial rho values (:160-176),
`sampleα` (:188), `sampleunconstrainedsolution` (:195-196), `getsolution` (:203-215: the best of
`initialrandom` random candidates starts Nelder-Mead), restarts (:222-226), returned value
`-result.minimum` (:351).

Not reproducible here (no Julia): MersenneTwister's stream (numpy's PCG64 is used; like the reference,
every delay of a grid sees the SAME random draws because each gpcc call seeds its own generator with
`seed`), Optim's exact trajectory, and MiscUtil's transforms, whose source is not under
/root/reference: `makepositive` is taken to be softplus and `transformbetween(x, a, b)` to be
a + (b - a) * logistic(x), the package's documented purpose; `safewrapper` is taken to turn exceptions
(PosDefException) into +Inf of the negative objective."""
import collections

import numpy as np

from . import laplace
from .api import Objective, PosDefException, getprobabilities, mvnormal_logpdf
from .bfgs import BatchedBFGS
from .neldermead import BatchedNelderMead


def makepositive(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x > 30.0, x, np.log1p(np.exp(np.minimum(x, 30.0))))


def invmakepositive(y):
    y = np.asarray(y, dtype=np.float64)
    return np.where(y > 30.0, y, np.log(np.expm1(np.minimum(y, 30.0))))


def transformbetween(x, a, b):
    x = np.asarray(x, dtype=np.float64)
    return a + (b - a) / (1.0 + np.exp(-x))


def invtransformbetween(y, a, b):
    u = (np.asarray(y, dtype=np.float64) - a) / (b - a)
    return np.log(u) - np.log1p(-u)


def unpack_grad(X, grad, L, rhomin, rhomax):
    """Chain rule through `unpack` (marginaliseb.jl:112-126): X (..., L+1) unconstrained vectors, grad (..., L+1 or 2L+1) the
    gradient in the constrained parameters [alpha_1..alpha_L, rho(, tau_1..tau_L)] (Objective.loglik_grad_batch) -> the same
    gradient in the optimiser's coordinates.  alpha = makepositive(x) + 1e-8: times makepositive'(x) = logistic(x) (1 where
    makepositive is the identity, x > 30); rho = transformbetween(x, a, b): times (b - a) s (1 - s), s = logistic(x).  The delays
    are not transformed: their columns pass through."""
    X = np.asarray(X, dtype=np.float64)
    out = np.array(grad, dtype=np.float64, copy=True)
    xa, xr = X[..., :L], X[..., L]
    out[..., :L] *= np.where(xa > 30.0, 1.0, 1.0 / (1.0 + np.exp(-np.minimum(xa, 30.0))))
    sr = 1.0 / (1.0 + np.exp(-xr))
    out[..., L] *= (rhomax - rhomin) * sr * (1.0 - sr)
    return out


def unpack_hessian(X, grad, hess, L, rhomin, rhomax):
    """Second-order chain rule through `unpack`, the companion of unpack_grad: X (..., L+1) unconstrained vectors, grad (..., n) and
    hess (..., n, n) in the constrained parameters (n = L+1, or 2L+1 with the delays: Objective.loglik_hess_batch) -> the Hessian in
    the optimiser's coordinates, J' H J + diag(grad * x''), with J = diag(x') over alpha and rho and the identity over the delays.
    alpha = makepositive(x) + 1e-8: x' = s, x'' = s (1 - s), s = logistic(x) (x' = 1, x'' = 0 where makepositive is the identity,
    x > 30); rho = transformbetween(x, a, b): x' = (b - a) s (1 - s), x'' = (b - a) s (1 - s) (1 - 2 s)."""
    X = np.asarray(X, dtype=np.float64)
    g = np.asarray(grad, dtype=np.float64)
    H = np.array(hess, dtype=np.float64, copy=True)
    n = H.shape[-1]
    xa, xr = X[..., :L], X[..., L]
    sa = 1.0 / (1.0 + np.exp(-np.minimum(xa, 30.0)))
    big = xa > 30.0
    d1 = np.ones(X.shape[:-1] + (n,))
    d2 = np.zeros(X.shape[:-1] + (n,))
    d1[..., :L] = np.where(big, 1.0, sa)
    d2[..., :L] = np.where(big, 0.0, sa * (1.0 - sa))
    sr = 1.0 / (1.0 + np.exp(-xr))
    d1[..., L] = (rhomax - rhomin) * sr * (1.0 - sr)
    d2[..., L] = (rhomax - rhomin) * sr * (1.0 - sr) * (1.0 - 2.0 * sr)
    H *= d1[..., :, None] * d1[..., None, :]
    idx = np.arange(n)
    H[..., idx, idx] += g[..., :n] * d2
    return H


def laplace_covariance(H, free, L=None):
    """(-H_ff)^-1, the Laplace (normal) approximation's covariance over the parameters `free` (indices, or a boolean mask, into a
    Hessian in [alpha_1..alpha_L, rho, tau_1..tau_L] order; L defaults to (n - 1) / 2) -> (cov, ok).  The likelihood does not
    change when every delay shifts together, so `free` must leave out at least one delay (ValueError otherwise).  ok is False and
    cov all NaN when -H_ff is not positive definite (not a maximum, or numerically singular): never a silent result."""
    H = np.asarray(H, dtype=np.float64)
    n = H.shape[0]
    if H.shape != (n, n):
        raise ValueError("H must be square, got %s" % (H.shape,))
    free = np.asarray(free)
    idx = np.flatnonzero(free) if free.dtype == bool else free.astype(int).ravel()
    if L is None:
        L = (n - 1) // 2
    delays = set(range(L + 1, 2 * L + 1)) if n == 2 * L + 1 else set()
    if delays and delays <= set(idx.tolist()):
        raise ValueError("free holds every delay: a common shift of all delays leaves the likelihood unchanged, fix at least one")
    A = -H[np.ix_(idx, idx)]
    A = 0.5 * (A + A.T)
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return np.full((len(idx), len(idx)), np.nan), False
    Li = np.linalg.solve(Lc, np.eye(len(idx)))
    cov = Li.T @ Li
    if not np.all(np.isfinite(cov)):
        return np.full((len(idx), len(idx)), np.nan), False
    return cov, True


def delay_covariance(objective, delays, alpha, rho, free=None, solver="dense", curvature="hessian", kappa=None, nu=None, noise_free=None):
    """The Laplace covariance of the delays (and hyper-parameters) at one point (delays[L], alpha[L], rho): one Hessian call over
    [alpha_1..alpha_L, rho, tau_1..tau_L] -- objective.loglik_hess_batch (solver "dense") or objective.loglik_hess_markov_batch (solver
    "markov": linear time, OU / matern32 / matern52; Objective's or markov.MarkovObjective's) -- then
    laplace_covariance over `free` -> (cov, ok).  free defaults to every alpha, rho and tau_2..tau_L (the first delay fixed: a common
    shift of all delays leaves the likelihood unchanged).  ok is False and cov all NaN when the point cannot be evaluated (info != 0),
    when a needed entry of the Hessian is NaN (solver "markov" with OU at a delay that makes two bands' shifted times collide: use
    "dense" there) or when -H_ff is not positive definite.  ValueError for another solver, or for a `free` that holds every delay.
    curvature="fisher": the expected (Fisher) information I in place of -H, cov = (I_ff)^-1 -- positive semi-definite at any point, not
    only at a maximum, and independent of the fluxes (a cadence's forecast) -- from objective.loglik_hess_batch's Fisher matrix (solver
    "dense") or objective.loglik_fisher_markov_batch (solver "markov"); the same ok rules.
    kappa, nu (each (L,) or None; both None: everything above, unchanged): the point carries a noise model, point i of band l observed
    with the variance kappa_l^2 sigma_i^2 + nu_l (None beside a given one: ones / zeros).  The Hessian is then
    objective.loglik_hess_full_markov_noise_batch's over [alpha_1..L, rho, tau_1..L, kappa_1..L, nu_1..L], so the delay's
    variance carries the (tau, kappa) and (tau, nu) couplings that a noise model frozen into the error bars drops; solver must be
    "markov" and curvature "hessian" (ValueError otherwise: the Fisher information in kappa, nu does not exist yet).  `free` indexes that
    4L+1 order and defaults to every alpha, rho, tau_2..tau_L and the noise parameters of `noise_free`, a boolean mask of 2L
    (kappa_1..L, nu_1..L) whose default is kappa_l > 0 and nu_l > 0: a parameter on its lower bound is not at an interior maximum and
    is left out, the way laplace.BatchedNewton pins it.  The same ok rules and the same ValueError for a `free` that holds every delay.
    At a stationary point the delay block of cov does not depend on how the nuisance parameters are parametrised (kappa or log kappa,
    nu or sqrt(nu): the Hessian transforms as J'HJ there, and the block of the inverse over the untransformed delays is unchanged)."""
    noise = kappa is not None or nu is not None
    if noise and solver != "markov":
        raise ValueError("kappa / nu need solver='markov', got %r: the dense path has no noise model (the Fisher information in kappa, nu "
                         "does not exist yet either)" % (solver,))
    if noise and curvature != "hessian":
        raise ValueError("kappa / nu need curvature='hessian', got %r: the Fisher information in kappa, nu does not exist yet" % (curvature,))
    if solver not in ("dense", "markov"):
        raise ValueError("solver must be 'dense' or 'markov', got %r" % (solver,))
    if curvature not in ("hessian", "fisher"):
        raise ValueError("curvature must be 'hessian' or 'fisher', got %r" % (curvature,))
    delays = np.asarray(delays, dtype=np.float64).reshape(1, -1)
    L = delays.shape[1]
    alpha = np.asarray(alpha, dtype=np.float64).reshape(1, L)
    rho = np.asarray(rho, dtype=np.float64).reshape(1)
    if noise:
        kappa = np.ones((1, L)) if kappa is None else np.asarray(kappa, dtype=np.float64).reshape(1, L)
        nu = np.zeros((1, L)) if nu is None else np.asarray(nu, dtype=np.float64).reshape(1, L)
        if free is None:
            if noise_free is None:
                noise_free = np.concatenate([kappa[0] > 0.0, nu[0] > 0.0])
            noise_free = np.asarray(noise_free, dtype=bool).reshape(2 * L)
            free = list(range(L + 1)) + list(range(L + 2, 2 * L + 1)) + [2 * L + 1 + int(k) for k in np.flatnonzero(noise_free)]
    if free is None:
        free = list(range(L + 1)) + list(range(L + 2, 2 * L + 1))
    free = np.asarray(free)
    idx = np.flatnonzero(free) if free.dtype == bool else free.astype(int).ravel()
    if set(range(L + 1, 2 * L + 1)) <= set(idx.tolist()):
        raise ValueError("free holds every delay: a common shift of all delays leaves the likelihood unchanged, fix at least one")
    if noise:
        _, _, hess, info = objective.loglik_hess_full_markov_noise_batch(delays, alpha, rho, kappa, nu)
    elif curvature == "fisher":
        if solver == "markov":
            _, _, fisher, info = objective.loglik_fisher_markov_batch(delays, alpha, rho)
        else:
            _, _, _, fisher, info = objective.loglik_hess_batch(delays, alpha, rho)
        hess = -np.asarray(fisher, dtype=np.float64)
    elif solver == "markov":
        _, _, hess, info = objective.loglik_hess_markov_batch(delays, alpha, rho)
    else:
        _, _, hess, _, info = objective.loglik_hess_batch(delays, alpha, rho)
    H = np.asarray(hess, dtype=np.float64)[0]
    if info[0] != 0 or not np.all(np.isfinite(H[np.ix_(idx, idx)])):
        return np.full((len(idx), len(idx)), np.nan), False
    return laplace_covariance(H, idx, L)


def nearestposdef(A, minimumeigenvalue=1e-6):
    """MiscUtil.nearestposdef(A; minimumeigenvalue) as used at marginaliseb.jl:331 -- MiscUtil's source is not
    available (unregistered dependency), so this is the assumed definition: symmetrise, eigendecompose, lift every
    eigenvalue below `minimumeigenvalue` up to it, recompose, symmetrise.  Host-side like the reference's (it only
    runs after a PosDefException on an Ntest x Ntest predictive covariance, never on the delay-grid path)."""
    A = np.asarray(A, dtype=np.float64)
    S = 0.5 * (A + A.T)
    w, V = np.linalg.eigh(S)
    R = (V * np.maximum(w, minimumeigenvalue)) @ V.T
    return 0.5 * (R + R.T)


class UniformDelayPrior:
    """Uniform(0, upper) over the delay, with the log-density vector getprobabilities takes as its second argument."""

    def __init__(self, upper):
        self.lower, self.upper = 0.0, float(upper)

    def logpdf(self, delays):
        d = np.asarray(delays, dtype=np.float64)
        return np.where((d >= self.lower) & (d <= self.upper), -np.log(self.upper - self.lower), -np.inf)


def uniformpriordelay(*, L, z):
    """src/uniformpriordelay.jl:10-16: Uniform(0, 10^1.559 (L 1e-44)^0.549 (1+z)); L luminosity, z redshift."""
    return UniformDelayPrior(10.0 ** 1.559 * (L * 1e-44) ** 0.549 * (1.0 + z))


def logrange(a, b, n):
    return np.exp(np.linspace(np.log(a), np.log(b), n))


class GridFit:
    """Result of gpcc_grid: loglikel[G] (= -minimum, what README.md:172-174 feeds to
    getprobabilities), alpha[G, L], rho[G], f_calls, rounds.  With evidence="laplace" also log_evidence[G] (the
    Laplace-marginalised evidence over alpha and rho, up to one constant shared by all delays: feed it to getprobabilities),
    hyper_cov[G, L+1, L+1] (posterior covariance of (log alpha, log rho)), laplace_info[G] and laplace_rounds[G]
    (DESIGN.md 4.11); None otherwise."""

    def __init__(self, loglikel, alpha, rho, f_calls, rounds, iterations_done):
        self.loglikel, self.alpha, self.rho = loglikel, alpha, rho
        self.f_calls, self.rounds, self.iterations_done = f_calls, rounds, iterations_done
        self.log_evidence = self.hyper_cov = self.laplace_info = self.laplace_rounds = None


def gpcc_grid(tarray, yarray, stdarray, *, kernel, candidatedelays, iterations, seed=1, numberofrestarts=1,
              initialrandom=5, rhomin=0.1, rhomax=20.0, objective=None, device=0, marginalise_b=True, engine=None,
              unpack=None, evidence=None, laplace_rounds=50, laplace_g_tol=1e-6, solver="dense", evidence_solver=None):
    """Fits the GPCC model for each row of candidatedelays (G, L): the README's
    `map(delay -> gpcc(...; delays = [0; delay])[1], candidatedelays)` as one lock-step batch.

    engine "native" (default with a device Objective): the whole fit is one gpcc_grid_loglik call, the random
    candidates drawn here (numpy) and handed over as init_params.  engine "python" (default when another
    objective is injected): the same algorithm in numpy (neldermead.py) over objective.loglik_batch; `unpack`
    may replace the numpy parameter transforms (api.unpack_params = the library's own).

    solver "dense" (default): every optimiser round is a batch of dense Cholesky factorisations (loglik_batch).  solver "markov": the
    rounds evaluate the same likelihood in linear time (loglik_markov_batch: OU, matern32, matern52; option "fit_markov" of the native
    engine) -- the values agree with the dense ones to rounding, so the fit follows the same trajectory up to that; rbf, or more than 4
    bands with marginalise_b, raise.  Every prediction stays dense, and so does the evidence unless evidence_solver says otherwise.

    evidence "laplace": after the fit, the Laplace-marginalised evidence over alpha and rho at every delay, from the fitted
    (alpha, rho) (Objective.laplace_evidence with the native engine, laplace.laplace_evidence otherwise) -> GridFit.log_evidence,
    .hyper_cov, .laplace_info, .laplace_rounds.  None (default): the profile likelihood only, as before.  evidence_solver None
    (default) or "dense": the Newton rounds of the evidence take the dense Hessian block whatever `solver` is; "markov": the block in
    linear time (loglik_hess_hyper_markov_batch; the same kernels and limits as solver "markov")."""
    if evidence_solver not in (None, "dense", "markov"):
        raise ValueError("evidence_solver must be None, 'dense' or 'markov', got %r" % (evidence_solver,))
    esolver = evidence_solver or "dense"
    if evidence not in (None, "laplace"):
        raise ValueError("evidence must be None or 'laplace', got %r" % (evidence,))
    if solver not in ("dense", "markov"):
        raise ValueError("solver must be 'dense' or 'markov', got %r" % (solver,))
    cand = np.ascontiguousarray(np.atleast_2d(candidatedelays), dtype=np.float64)
    G, L = cand.shape
    assert L == len(tarray) == len(yarray) == len(stdarray)          # marginaliseb.jl:78
    own = objective is None
    obj = objective if objective is not None else Objective(tarray, yarray, stdarray, kernel,
                                                            marginalise_b=marginalise_b, device=device)
    try:
        R = int(numberofrestarts)
        rg = np.random.default_rng(seed)
        if R in (1, 2):                                                  # :160-176
            rho0 = rg.uniform(rhomin + 1e-3, rhomax - 1e-3, R)
        else:
            rho0 = logrange(rhomin + 1e-3, rhomax - 1e-3, R)
        vary = np.array([np.var(np.asarray(y, dtype=np.float64), ddof=1) for y in yarray])
        # the same candidates for every delay (each reference call re-seeds): (R, initialrandom, L+1)
        cands = np.empty((R, initialrandom, L + 1))
        for i in range(R):
            for c in range(initialrandom):
                cands[i, c, :L] = invmakepositive(vary * (rg.random(L) * (1.2 - 0.8) + 0.8))   # sampleα, :188
                cands[i, c, L] = invtransformbetween(rho0[i], rhomin, rhomax)
        P = G * R                                                        # problem p = (delay p // R, restart p % R)
        if engine is None:
            engine = "native" if isinstance(obj, Objective) else "python"
        if engine == "native":
            before = obj.get_option("fit_markov")
            obj.set_option("fit_markov", int(solver == "markov"))
            try:
                ll, alpha, rho, info, its, (f_calls, rounds) = obj.grid_loglik(
                    cand, iterations, numberofrestarts=R, initialrandom=initialrandom, rhomin=rhomin, rhomax=rhomax,
                    seed=seed, init_params=cands)
            finally:
                obj.set_option("fit_markov", before)
            return _with_evidence(GridFit(ll, alpha, rho, f_calls, rounds, its.astype(np.int64)), obj, cand, engine, evidence,
                                  rhomin, rhomax, laplace_rounds, laplace_g_tol, esolver)

        def negobj(pidx, X):
            if unpack is not None:
                alpha, rho = unpack(X, L, rhomin, rhomax)
            else:
                alpha = makepositive(X[:, :L]) + 1e-8                    # makeα, :112
                rho = transformbetween(X[:, L], rhomin, rhomax)          # makeρ, :114
            ll, info = (obj.loglik_markov_batch if solver == "markov" else obj.loglik_batch)(cand[pidx // R], alpha, rho)
            return np.where(info == 0, -ll, np.inf)                      # safewrapper(negativeobjective), :149-153

        # argmin over the random candidates (:209)
        pid = np.repeat(np.arange(P), initialrandom)
        Xc = cands[np.tile(np.repeat(np.arange(R), initialrandom), G), np.tile(np.arange(initialrandom), P)]
        f0 = negobj(pid, Xc).reshape(P, initialrandom)
        best = np.argmin(f0, axis=1)
        x0 = Xc.reshape(P, initialrandom, L + 1)[np.arange(P), best]
        nm = BatchedNelderMead(x0, negobj, iterations=iterations, g_tol=1e-6)   # Optim.Options(g_tol = 1e-6), :205
        xmin, fmin = nm.run()
        fmin = fmin.reshape(G, R)
        pick = np.argmin(fmin, axis=1)                                   # best restart, :224
        xsel = xmin.reshape(G, R, L + 1)[np.arange(G), pick]
        a_sel, r_sel = (unpack(xsel, L, rhomin, rhomax) if unpack is not None else
                        (makepositive(xsel[:, :L]) + 1e-8, transformbetween(xsel[:, L], rhomin, rhomax)))
        return _with_evidence(GridFit(-fmin[np.arange(G), pick], a_sel, r_sel, nm.f_calls + P * initialrandom, nm.rounds + 1,
                                      nm.iterations_done.reshape(G, R)[np.arange(G), pick]), obj, cand, engine, evidence,
                              rhomin, rhomax, laplace_rounds, laplace_g_tol, esolver)
    finally:
        if own:
            obj.close()


class RealisationDelays(collections.namedtuple("RealisationDelays", "prob map_index mean_delay")):
    """realisation_delays' result: prob[R, G] (each realisation's getprobabilities over the grid), map_index[R] (its most probable
    grid point) and mean_delay[R, L] (its posterior-mean delay, prob @ candidatedelays)."""


def realisation_delays(objective, candidatedelays, alpha, rho, Y, logprior=None, center="own", probabilities=getprobabilities):
    """The delay posterior of every flux realisation in Y over the grid candidatedelays (G, L), in ONE linear-time pass
    (objective.loglik_markov_realisations) -> RealisationDelays(prob[R, G], map_index[R], mean_delay[R, L]).

    alpha (G, L) and rho (G) are the per-delay fitted hyper-parameters of a GridFit of the ORIGINAL data (res.alpha, res.rho).  They are
    FROZEN: nothing is refitted per realisation, and with marginalise_b the offsets' prior variances stay the original data's.  Row r of
    prob is getprobabilities(loglik[:, r], logprior) of realisation r under the fitted model at each delay.  So with Y =
    synthetic.flux_randomise(yarray, stdarray, R, seed) the scatter of mean_delay (or of candidatedelays[map_index]) is the
    flux-randomisation scatter of the delay UNDER THE FITTED MODEL; it leaves out the scatter of the hyper-parameters' own fit, which a
    refit per realisation (one gpcc_grid each) would add.  With parametric-bootstrap or null light curves as Y the same call gives a
    false-alarm rate.  center: loglik_markov_realisations' ("own": each realisation's band means).  logprior: getprobabilities' second
    argument (G).  probabilities: the function applied per realisation (default: getprobabilities)."""
    cand = np.asarray(candidatedelays, np.float64)
    cand = cand.reshape(len(cand), -1)
    ll, info = objective.loglik_markov_realisations(Y, cand, alpha, rho, center=center)
    if (np.asarray(info) != 0).any():
        bad = int(np.flatnonzero(np.asarray(info) != 0)[0])
        raise ValueError("realisation_delays: grid point %d has info = %d (loglik_markov_batch's codes)" % (bad, int(info[bad])))
    R = ll.shape[1]
    prob = np.stack([probabilities(ll[:, r]) if logprior is None else probabilities(ll[:, r], logprior) for r in range(R)])
    return RealisationDelays(prob, np.argmax(prob, axis=1), prob @ cand)


class RealisationRefits(collections.namedtuple("RealisationRefits", "loglikel alpha rho f_calls rounds delays start_loglikel")):
    """realisation_refits' result: loglikel[R, G] (each realisation's refitted profile likelihood over the grid), alpha[R, G, L],
    rho[R, G], f_calls, rounds, delays (the RealisationDelays of loglikel) and start_loglikel[R, G] (the value at the warm start as the
    optimiser holds it, loglikel >= it; None with start=None).  Beside the fields, two attributes that realisation_refits sets on its
    result (copies made through the tuple, _replace or pickle fall back to None): x[R, G, L + 1], the returned cells in the
    optimiser's coordinates, alpha = makepositive(x[..., :L]) + 1e-8 and rho = transformbetween(x[..., L], rhomin, rhomax), what
    unpack_grad takes; converged[R, G], with optimiser="bfgs" whether the gradient of the cell's run fell to g_tol, None with
    "neldermead", which has no such test."""
    x = None
    converged = None


def realisation_refits(objective, candidatedelays, Y, counts=None, *, iterations, start=None, seed=1, numberofrestarts=1,
                       initialrandom=5, rhomin=0.1, rhomax=20.0, logprior=None, probabilities=getprobabilities, optimiser="neldermead"):
    """FR/RSS with a REFIT PER REALISATION: fits (alpha, rho) at every row of candidatedelays (G, L) for every resampled data set
    (Y, counts) on objective's cadence (synthetic.resample's result; counts None: all 1) -> RealisationRefits.  The lock-step
    BatchedNelderMead of gpcc_grid's python engine runs over the problems (realisation, delay, restart); every optimiser round is ONE
    objective.loglik_markov_resampled call (linear time: OU, matern32, matern52), each realisation under its own band means and, with
    marginalise_b, its own offsets' prior variances.  objective: an Objective, or a markov.MarkovObjective (no GPU).

    start=None: the reference's random candidates exactly as gpcc_grid draws them -- the same seed and the same draws for every
    realisation and delay, scaled by each realisation's own band variances -- so that realisation r's result is that of
    gpcc_grid(engine="python", solver="markov") on its reduced data set.  start=(alpha[G, L], rho[G]), usually a GridFit of the
    original data (res.alpha, res.rho): every realisation starts Nelder-Mead at delay g from (alpha[g], rho[g]), with one restart and
    no random candidates; rho is clipped into (rhomin, rhomax).  delays: getprobabilities per realisation over its refitted likelihoods
    (logprior, probabilities: realisation_delays').  realisation_delays is the frozen route, one pass and no refit.

    optimiser "neldermead" (default): as above.  "bfgs": the same problems from the same starting points by the lock-step
    bfgs.BatchedBFGS (g_tol 1e-6 on the gradient in the optimiser's coordinates), every round ONE
    objective.loglik_grad_markov_resampled call, whose gradient unpack_grad takes to the optimiser's coordinates; `iterations` bounds
    the accepted steps of a problem.  The fields of the result are the same (start_loglikel: the value at the optimiser's first
    point); its attributes x and converged are RealisationRefits'."""
    from . import markov
    if optimiser not in ("neldermead", "bfgs"):
        raise ValueError("optimiser must be 'neldermead' or 'bfgs', got %r" % (optimiser,))
    cand = np.ascontiguousarray(np.asarray(candidatedelays, np.float64).reshape(len(candidatedelays), -1))
    G, L = cand.shape
    shape = [np.empty(int(n)) for n in objective.Nl] if hasattr(objective, "Nl") else objective.data[0]
    Yb = markov._bands(shape, Y)
    R = Yb[0].shape[0]
    cb = markov._counts(shape, counts, R)
    mb = bool(objective.marginalise_b)
    mean, vb = markov.resample_constants(shape, Yb, cb, mb)
    Yf = np.ascontiguousarray(np.concatenate(Yb, axis=1))
    cf = None if counts is None else np.ascontiguousarray(np.concatenate(cb, axis=1))
    if start is None:
        K = int(numberofrestarts)
        rg = np.random.default_rng(seed)
        rho0 = rg.uniform(rhomin + 1e-3, rhomax - 1e-3, K) if K in (1, 2) else logrange(rhomin + 1e-3, rhomax - 1e-3, K)
        vary = np.array([[np.var(Yb[l][r][cb[l][r] > 0], ddof=1) for l in range(L)] for r in range(R)])
        cands = np.empty((R, K, initialrandom, L + 1))
        for i in range(K):
            for c in range(initialrandom):
                u = rg.random(L) * (1.2 - 0.8) + 0.8
                for r in range(R):
                    cands[r, i, c, :L] = invmakepositive(vary[r] * u)
                cands[:, i, c, L] = invtransformbetween(rho0[i], rhomin, rhomax)
    else:
        K = 1
        a0 = np.asarray(start[0], np.float64).reshape(G, L)
        r0 = np.clip(np.asarray(start[1], np.float64).reshape(G), rhomin + 1e-9 * (rhomax - rhomin), rhomax - 1e-9 * (rhomax - rhomin))
        xs = np.concatenate([invmakepositive(np.maximum(a0 - 1e-8, 1e-300)), invtransformbetween(r0, rhomin, rhomax)[:, None]], axis=1)
    P = R * G * K                                                        # problem p = (realisation, delay, restart), realisation-major

    def unpack(X):
        return makepositive(X[:, :L]) + 1e-8, transformbetween(X[:, L], rhomin, rhomax)

    def negobj(pidx, X):
        alpha, rho = unpack(X)
        ll, info = objective.loglik_markov_resampled(Yf, cand[(pidx // K) % G], alpha, rho, pidx // (G * K), counts=cf, center=mean,
                                                     sigma_b=vb)
        return np.where(info == 0, -ll, np.inf)

    def negfg(pidx, X):
        with np.errstate(over="ignore"):                                 # (a long trial step: exp(-x) overflows to a rho on its bound)
            alpha, rho = unpack(X)
            ll, grad, info = objective.loglik_grad_markov_resampled(Yf, cand[(pidx // K) % G], alpha, rho, pidx // (G * K), counts=cf,
                                                                    center=mean, sigma_b=vb)
            bad = info != 0
            return np.where(bad, np.inf, -ll), np.where(bad[:, None], 0.0, -unpack_grad(X, grad[:, :L + 1], L, rhomin, rhomax))

    extra_calls, extra_rounds, f_start = 0, 0, None
    if start is None:
        pid = np.repeat(np.arange(P), initialrandom)
        Xc = cands[pid // (G * K), pid % K, np.tile(np.arange(initialrandom), P)]
        f0 = negobj(pid, Xc).reshape(P, initialrandom)                   # argmin over the random candidates (:209)
        x0 = Xc.reshape(P, initialrandom, L + 1)[np.arange(P), np.argmin(f0, axis=1)]
        extra_calls, extra_rounds = P * initialrandom, 1
    else:
        x0 = np.tile(xs, (R, 1))
        if optimiser == "neldermead":
            f_start = -negobj(np.arange(P), x0).reshape(R, G)
    if optimiser == "bfgs":
        nm = BatchedBFGS(x0, negfg, iterations=iterations, g_tol=1e-6)
        xmin, fmin = nm.run()
        if start is not None:
            f_start = -nm.f_start.reshape(R, G)
    else:
        nm = BatchedNelderMead(x0, negobj, iterations=iterations, g_tol=1e-6)
        xmin, fmin = nm.run()
    fmin = fmin.reshape(R * G, K)
    pick = np.argmin(fmin, axis=1)
    a_sel, r_sel = unpack(xmin.reshape(R * G, K, L + 1)[np.arange(R * G), pick])
    ll = -fmin[np.arange(R * G), pick].reshape(R, G)
    prob = np.stack([probabilities(ll[r]) if logprior is None else probabilities(ll[r], logprior) for r in range(R)])
    out = RealisationRefits(ll, a_sel.reshape(R, G, L), r_sel.reshape(R, G), nm.f_calls + extra_calls, nm.rounds + extra_rounds,
                            RealisationDelays(prob, np.argmax(prob, axis=1), prob @ cand), f_start)
    out.x = xmin.reshape(R * G, K, L + 1)[np.arange(R * G), pick].reshape(R, G, L + 1)   # (attributes beside the fields, which stay as they are)
    if optimiser == "bfgs":
        out.converged = nm.converged.reshape(R * G, K)[np.arange(R * G), pick].reshape(R, G)
    return out


class RealisationPeaks(collections.namedtuple("RealisationPeaks", "delays alpha rho loglikel start_loglikel converged f_calls rounds")):
    """realisation_peaks' result: delays[R, L] (each realisation's delay as a continuous number), alpha[R, L], rho[R], loglikel[R] (the
    value there), start_loglikel[R] (the value at the grid cell it started from, loglikel >= it), converged[R] (the gradient in the
    optimiser's coordinates fell to g_tol), f_calls, rounds.  Beside the fields the attribute x[R, L + 1 + F] that realisation_peaks
    sets: the returned points in the optimiser's coordinates -- alpha and rho as RealisationRefits.x holds them, then the F free delays,
    tau_l = transformbetween(x, min, max of column l of the grid); a realisation that kept its cell has the cell's own delays and the
    coordinates of its start."""
    x = None


def realisation_peaks(objective, candidatedelays, Y, counts=None, *, start, iterations, free_delays=None, rhomin=0.1, rhomax=20.0,
                      g_tol=1e-6, logprior=None, probabilities=getprobabilities):
    """EACH REALISATION'S DELAY AS A CONTINUOUS NUMBER: for every resampled data set (Y, counts) on objective's cadence, takes its most
    probable cell of the grid candidatedelays (G, L) and from there maximises the log-likelihood JOINTLY over (alpha, rho) and the free
    delays with the lock-step bfgs.BatchedBFGS -> RealisationPeaks.  That is R problems of 1 + L + len(free_delays) parameters per round,
    not R x G, every round ONE objective.loglik_grad_markov_resampled call (linear time: OU, matern32, matern52), each realisation
    under its own band means and, with marginalise_b, its own offsets' prior variances.  The scatter of delays[:, l] is the FR/RSS
    scatter of the peak, no longer quantised to the grid's spacing.

    start: a RealisationRefits of the same (candidatedelays, Y, counts) -- realisation r starts at its cell start.delays.map_index[r]
    with the refitted (alpha, rho) of that cell -- or (alpha[G, L], rho[G]), the per-delay hyper-parameters of a GridFit of the
    original data: the cell is then the most probable one under those frozen hyper-parameters (realisation_delays; with counts, one
    loglik_markov_resampled pass over the R x G cells and getprobabilities per realisation; logprior, probabilities:
    realisation_delays').  free_delays: the bands (0-based) whose
    delay moves; None: all but the first.  A free delay tau_l = transformbetween(x, min, max) of column l of the grid, so it stays inside
    the grid's range; a start on the edge of that range is moved inside by 1e-3 of its width, where the transform still has a slope.  rho
    stays in (rhomin, rhomax) and alpha positive as in the fit.  The other delays stay the cell's.  If no accepted step betters the
    cell itself, the cell is returned (converged False unless its own gradient is below g_tol).

    For OU the likelihood has kinks in tau wherever two shifted times of different bands cross; there the gradient is the mean of the
    one-sided derivatives, the line search may stall on the kink, and such a realisation ends with converged = False at its best
    point.  That is reported, not raised; the Matern kernels are C^1 in tau."""
    from . import markov
    cand = np.ascontiguousarray(np.asarray(candidatedelays, np.float64).reshape(len(candidatedelays), -1))
    G, L = cand.shape
    shape = [np.empty(int(n)) for n in objective.Nl] if hasattr(objective, "Nl") else objective.data[0]
    Yb = markov._bands(shape, Y)
    R = Yb[0].shape[0]
    cb = markov._counts(shape, counts, R)
    mean, vb = markov.resample_constants(shape, Yb, cb, bool(objective.marginalise_b))
    Yf = np.ascontiguousarray(np.concatenate(Yb, axis=1))
    cf = None if counts is None else np.ascontiguousarray(np.concatenate(cb, axis=1))
    free = np.arange(1, L) if free_delays is None else np.unique(np.asarray(free_delays, dtype=np.int64).reshape(-1))
    if len(free) and (free.min() < 0 or free.max() >= L):
        raise ValueError("free_delays must be bands in [0, %d)" % L)
    lo, hi = cand[:, free].min(axis=0), cand[:, free].max(axis=0)
    if (hi <= lo).any():
        raise ValueError("free_delays: band %d has one delay in the grid, no range to move in" % int(free[np.argmax(hi <= lo)]))
    real = np.arange(R)
    if isinstance(start, RealisationRefits):
        cell = np.asarray(start.delays.map_index, dtype=np.int64).reshape(R)
        a0, r0 = np.asarray(start.alpha, np.float64)[real, cell], np.asarray(start.rho, np.float64)[real, cell]
    else:
        ag, rg = np.asarray(start[0], np.float64).reshape(G, L), np.asarray(start[1], np.float64).reshape(G)
        if counts is None:
            cell = np.asarray(realisation_delays(objective, cand, ag, rg, Yb, logprior=logprior, probabilities=probabilities).map_index,
                              dtype=np.int64)
        else:
            ll, info = objective.loglik_markov_resampled(Yf, np.tile(cand, (R, 1)), np.tile(ag, (R, 1)), np.tile(rg, R), np.repeat(real, G),
                                                         counts=cf, center=mean, sigma_b=vb)
            if (np.asarray(info) != 0).any():
                bad = int(np.flatnonzero(np.asarray(info) != 0)[0])
                raise ValueError("realisation_peaks: realisation %d at grid point %d has info = %d" % (bad // G, bad % G, int(info[bad])))
            ll = ll.reshape(R, G)
            cell = np.array([int(np.argmax(probabilities(ll[r]) if logprior is None else probabilities(ll[r], logprior))) for r in range(R)],
                            dtype=np.int64)
        a0, r0 = ag[cell], rg[cell]
    r0 = np.clip(r0, rhomin + 1e-9 * (rhomax - rhomin), rhomax - 1e-9 * (rhomax - rhomin))
    tau0 = cand[cell]
    tf0 = np.clip(tau0[:, free], lo + 1e-3 * (hi - lo), hi - 1e-3 * (hi - lo))
    x0 = np.concatenate([invmakepositive(np.maximum(a0 - 1e-8, 1e-300)), invtransformbetween(r0, rhomin, rhomax)[:, None],
                         invtransformbetween(tf0, lo, hi)], axis=1)

    def negfg(pidx, X, at_cell=False):
        with np.errstate(over="ignore"):                                 # (a long trial step: exp(-x) overflows to a bound)
            alpha, rho = makepositive(X[:, :L]) + 1e-8, transformbetween(X[:, L], rhomin, rhomax)
            tau = tau0[pidx].copy()
            if not at_cell:
                tau[:, free] = transformbetween(X[:, L + 1:], lo, hi)
            ll, grad, info = objective.loglik_grad_markov_resampled(Yf, tau, alpha, rho, pidx, counts=cf, center=mean, sigma_b=vb)
            g = unpack_grad(X[:, :L + 1], grad[:, :L + 1], L, rhomin, rhomax)
            st = 1.0 / (1.0 + np.exp(-X[:, L + 1:]))
            g = np.concatenate([g, grad[:, L + 1 + free] * ((hi - lo) * st * (1.0 - st))], axis=1)
            bad = info != 0
            return np.where(bad, np.inf, -ll), np.where(bad[:, None], 0.0, -g)

    # the cell itself, with (alpha, rho) as the optimiser's coordinates hold them and the grid's own delays: the value to better
    fc, gc = negfg(real, x0, at_cell=True)
    opt = BatchedBFGS(x0, negfg, iterations=iterations, g_tol=g_tol)
    xmin, fmin = opt.run()
    keep = ~(fmin <= fc)                                                 # no step bettered the cell (or the run never had a finite value)
    alpha, rho = makepositive(xmin[:, :L]) + 1e-8, transformbetween(xmin[:, L], rhomin, rhomax)
    tau = tau0.copy()
    tau[:, free] = transformbetween(xmin[:, L + 1:], lo, hi)
    a_cell, r_cell = makepositive(x0[:, :L]) + 1e-8, transformbetween(x0[:, L], rhomin, rhomax)
    alpha[keep], rho[keep], tau[keep] = a_cell[keep], r_cell[keep], tau0[keep]
    with np.errstate(invalid="ignore"):
        conv = np.where(keep, np.isfinite(fc) & (np.abs(gc).max(axis=1, initial=0.0) <= g_tol), opt.converged)
    out = RealisationPeaks(tau, alpha, rho, -np.where(keep, fc, fmin), -fc, conv, opt.f_calls + R, opt.rounds + 1)
    out.x = np.where(keep[:, None], x0, xmin)
    return out


def effective_std(stdarray, kappa, nu):
    """The error bars sqrt(kappa_l^2 sigma_l^2 + nu_l) of the noise model of Objective.loglik_markov_noise_batch, as a list of L
    arrays: kappa and nu scalars or (L,).  A fresh Objective or Predictor on them is the route to joint predictions, the dense path
    and draws under a fitted noise model (its loglik_markov_batch is loglik_markov_noise_batch's value); per-band predictions, held-out
    scores and leave-one-out scores take the model directly (Predictor(..., kappa=, nu=), noise_predictor)."""
    L = len(stdarray)
    kappa = np.broadcast_to(np.asarray(kappa, np.float64), (L,))
    nu = np.broadcast_to(np.asarray(nu, np.float64), (L,))
    return [np.sqrt(kappa[l] ** 2 * np.asarray(stdarray[l], np.float64) ** 2 + nu[l]) for l in range(L)]


class NoiseGridFit(collections.namedtuple("NoiseGridFit", "loglikel alpha rho kappa nu f_calls rounds start_loglikel")):
    """gpcc_grid_noise's result: loglikel[G] (the profile likelihood over the grid with the noise model fitted beside alpha and rho),
    alpha[G, L], rho[G], kappa[G, L], nu[G, L], f_calls, rounds and start_loglikel[G] (the value at the warm start as the optimiser
    holds it, loglikel >= it; None with start=None)."""


def gpcc_grid_noise(objective, candidatedelays, *, iterations, noise="both", shared=False, start=None, seed=1, numberofrestarts=1,
                    initialrandom=5, rhomin=0.1, rhomax=20.0, kappa=1.0, nu=0.0):
    """gpcc_grid with a NOISE MODEL fitted beside (alpha, rho) at every row of candidatedelays (G, L): point i of band l has the
    variance kappa_l^2 sigma_i^2 + nu_l -> NoiseGridFit.  Built like realisation_refits: the lock-step
    BatchedNelderMead over the problems (delay, restart), every optimiser round ONE objective.loglik_markov_noise_batch call (linear
    time: OU, matern32, matern52).  objective: an Objective, or a markov.MarkovObjective (no GPU).

    noise: "scale" fits kappa, "excess" fits nu, "both" both; the part not fitted stays at the `kappa` / `nu` argument (a scalar or
    (L,)).  shared=True fits one kappa and / or one nu for all bands.  kappa=0.0, noise="excess", shared=True is the model of the
    reference's unused src/UNUSED/gpccfixdelay_globalnoiseterm.jl, up to the scale of nu.  The optimiser's variables: kappa =
    makepositive(x); nu_l = makepositive(x) mean(sigma_l^2), so that x is dimensionless.

    start=None: the random candidates -- alpha and rho exactly gpcc_grid's draws (the same seed gives the same ones), kappa from
    U(0.8, 1.2) and nu from U(0, 1) mean(sigma_l^2), drawn after them.  start=(alpha[G, L], rho[G]), usually a GridFit of the plain
    model: Nelder-Mead starts at delay g from (alpha[g], rho[g], kappa = 1, nu = 0.1 mean(sigma_l^2)) with one restart and no
    candidates; rho is clipped into (rhomin, rhomax)."""
    if noise not in ("scale", "excess", "both"):
        raise ValueError('noise must be "scale", "excess" or "both", got %r' % (noise,))
    cand = np.ascontiguousarray(np.asarray(candidatedelays, np.float64).reshape(len(candidatedelays), -1))
    G, L = cand.shape
    edges = np.concatenate([[0], np.cumsum(objective.Nl if hasattr(objective, "Nl") else [len(t) for t in objective.data[0]])])
    vary = np.array([np.var(objective.yflat[edges[l]:edges[l + 1]], ddof=1) for l in range(L)])
    ms2 = np.array([np.mean(objective.sflat[edges[l]:edges[l + 1]] ** 2) for l in range(L)])
    kfix = np.broadcast_to(np.asarray(kappa, np.float64), (L,))
    vfix = np.broadcast_to(np.asarray(nu, np.float64), (L,))
    nk = 0 if noise == "excess" else (1 if shared else L)                # the optimiser's kappa and nu variables
    nv = 0 if noise == "scale" else (1 if shared else L)
    n = L + 1 + nk + nv

    def unpack(X):
        kap = np.broadcast_to(makepositive(X[:, L + 1:L + 1 + nk]), (len(X), L)) if nk else np.tile(kfix, (len(X), 1))
        exc = np.broadcast_to(makepositive(X[:, L + 1 + nk:]), (len(X), L)) * ms2 if nv else np.tile(vfix, (len(X), 1))
        return makepositive(X[:, :L]) + 1e-8, transformbetween(X[:, L], rhomin, rhomax), kap, exc

    if start is None:
        K = int(numberofrestarts)
        rg = np.random.default_rng(seed)
        rho0 = rg.uniform(rhomin + 1e-3, rhomax - 1e-3, K) if K in (1, 2) else logrange(rhomin + 1e-3, rhomax - 1e-3, K)
        cands = np.empty((K, initialrandom, n))
        for i in range(K):
            for c in range(initialrandom):
                cands[i, c, :L] = invmakepositive(vary * (rg.random(L) * (1.2 - 0.8) + 0.8))
                cands[i, c, L] = invtransformbetween(rho0[i], rhomin, rhomax)
        for i in range(K):                                               # after gpcc_grid's draws, so that those stay gpcc_grid's
            for c in range(initialrandom):
                cands[i, c, L + 1:L + 1 + nk] = invmakepositive(rg.random(nk) * (1.2 - 0.8) + 0.8)
                cands[i, c, L + 1 + nk:] = invmakepositive(np.maximum(rg.random(nv), 1e-12))
    else:
        K = 1
        a0 = np.asarray(start[0], np.float64).reshape(G, L)
        r0 = np.clip(np.asarray(start[1], np.float64).reshape(G), rhomin + 1e-9 * (rhomax - rhomin), rhomax - 1e-9 * (rhomax - rhomin))
        xs = np.concatenate([invmakepositive(np.maximum(a0 - 1e-8, 1e-300)), invtransformbetween(r0, rhomin, rhomax)[:, None],
                             np.full((G, nk), float(invmakepositive(1.0))), np.full((G, nv), float(invmakepositive(0.1)))], axis=1)
    P = G * K                                                            # problem p = (delay p // K, restart p % K)

    def negobj(pidx, X):
        alpha, rho, kap, exc = unpack(X)
        ll, info = objective.loglik_markov_noise_batch(cand[pidx // K], alpha, rho, kap, exc)
        return np.where(info == 0, -ll, np.inf)

    extra_calls, extra_rounds, f_start = 0, 0, None
    if start is None:
        pid = np.repeat(np.arange(P), initialrandom)
        Xc = cands[np.tile(np.repeat(np.arange(K), initialrandom), G), np.tile(np.arange(initialrandom), P)]
        f0 = negobj(pid, Xc).reshape(P, initialrandom)                   # argmin over the random candidates
        x0 = Xc.reshape(P, initialrandom, n)[np.arange(P), np.argmin(f0, axis=1)]
        extra_calls, extra_rounds = P * initialrandom, 1
    else:
        x0 = xs
        f_start = -negobj(np.arange(P), x0)
    nm = BatchedNelderMead(x0, negobj, iterations=iterations, g_tol=1e-6)
    xmin, fmin = nm.run()
    fmin = fmin.reshape(G, K)
    pick = np.argmin(fmin, axis=1)
    a_sel, r_sel, k_sel, v_sel = unpack(xmin.reshape(G, K, n)[np.arange(G), pick])
    return NoiseGridFit(-fmin[np.arange(G), pick], a_sel, r_sel, np.array(k_sel), np.array(v_sel), nm.f_calls + extra_calls,
                        nm.rounds + extra_rounds, f_start)


class NoiseEvidence(collections.namedtuple("NoiseEvidence", "loglik alpha rho kappa nu log_evidence cov info rounds pinned")):
    """noise_evidence's result: the mode at every delay (loglik[G], alpha[G, L], rho[G], kappa[G, L], nu[G, L]), log_evidence[G] up to
    one constant shared by all delays, cov[G, n, n] in the variables u of laplace.laplace_evidence_noise, info[G] (0, or laplace's
    codes), rounds[G] and pinned[G, n]: the one-sided variables (kappa, w) that ended on a bound with the gradient pointing out."""


def noise_evidence(objective, candidatedelays, noisefit, *, noise="both", shared=False, kappa=1.0, nu=0.0, rhomin=0.1, rhomax=20.0,
                   max_rounds=50, g_tol=1e-6, **bounds):
    """The Laplace-marginalised evidence over (alpha, rho, kappa, nu) at every row of candidatedelays, started at a NoiseGridFit
    (gpcc_grid_noise's result, with the same noise, shared, kappa, nu, rhomin and rhomax) -> NoiseEvidence: laplace.laplace_evidence_noise
    with the fit as the start.  getprobabilities(result.log_evidence) is the delay posterior with the hyper-parameters AND the noise
    model integrated out, where the fit's profile likelihood only maximises over them.  objective: an Objective (the rounds are
    gpcc_loglik_hess_noise_markov_batch calls) or a markov.MarkovObjective (no GPU).  The part of the noise model that is not fitted
    stays at `kappa` / `nu`.  bounds: kappamin, kappamax, wmin, wmax of laplace_evidence_noise."""
    cand = np.ascontiguousarray(np.asarray(candidatedelays, np.float64).reshape(len(candidatedelays), -1))
    G, L = cand.shape
    kap0 = np.asarray(noisefit.kappa, np.float64).reshape(G, L) if noise != "excess" else np.broadcast_to(np.asarray(kappa, np.float64), (G, L))
    exc0 = np.asarray(noisefit.nu, np.float64).reshape(G, L) if noise != "scale" else np.broadcast_to(np.asarray(nu, np.float64), (G, L))
    return NoiseEvidence(*laplace.laplace_evidence_noise(objective, cand, noisefit.alpha, noisefit.rho, kap0, exc0, noise=noise,
                                                         shared=shared, rhomin=rhomin, rhomax=rhomax, max_rounds=max_rounds,
                                                         g_tol=g_tol, **bounds))


def _with_evidence(res, obj, cand, engine, evidence, rhomin, rhomax, max_rounds, g_tol, solver="dense"):
    if evidence is None:
        return res
    ok = np.all(np.isfinite(res.alpha), axis=1) & np.isfinite(res.rho) & np.all(res.alpha > 0, axis=1) & (res.rho > 0)
    G, n = cand.shape[0], cand.shape[1] + 1
    a0 = np.where(ok[:, None], res.alpha, 1.0)     # a delay whose fit found no valid point: a placeholder start, info set below
    r0 = np.where(ok, res.rho, np.sqrt(rhomin * rhomax))
    if engine == "native":
        _, _, _, logz, cov, info, rounds, _ = obj.laplace_evidence(cand, a0, r0, rhomin=rhomin, rhomax=rhomax, max_rounds=max_rounds,
                                                                   g_tol=g_tol, solver=solver)
    else:
        _, _, _, logz, cov, info, rounds = laplace.laplace_evidence(obj, cand, a0, r0, rhomin=rhomin, rhomax=rhomax,
                                                                    max_rounds=max_rounds, g_tol=g_tol, solver=solver)
    info = np.where(ok, info, laplace.BAD_START).astype(np.int32)
    res.log_evidence = np.where(ok, logz, np.nan)
    res.hyper_cov = np.where(ok[:, None, None], cov, np.nan).reshape(G, n, n)
    res.laplace_info, res.laplace_rounds = info, rounds
    return res


def _sample_bands(L, ttest):
    """ttest as Predictor's call forms take it: a list of L arrays (each band's own times) or one array (the same times in every band)."""
    if isinstance(ttest, (list, tuple)) and len(ttest) == L and all(np.ndim(a) == 1 for a in ttest):
        return [np.asarray(a, dtype=np.float64) for a in ttest]
    return [np.asarray(ttest, dtype=np.float64).ravel()] * L


def _check_sample_solver(solver):
    if solver not in (None, "dense", "markov"):
        raise ValueError("sample: solver must be None, 'dense' or 'markov', got %r" % (solver,))


def _split_bands(draws, bands):
    off = np.concatenate([[0], np.cumsum([len(b) for b in bands])]).astype(int)
    return [draws[:, off[l]:off[l + 1]] for l in range(len(bands))]


class LooScores(collections.namedtuple("LooScores", "mu sigma lp z total")):
    """Leave-one-out predictive scores of the training points, in the order the light curves were handed over: mean mu, standard
    deviation sigma and log-density lp of y_i given every other observation, the standardised residual z = (y - mu) / sigma (a large
    |z| flags a bad epoch or an underestimated error bar) and total = sum(lp), the score that compares kernels or delays."""


def _loo_entry(obj, solver):
    if solver not in ("dense", "markov"):
        raise ValueError("solver must be 'dense' or 'markov', got %r" % (solver,))
    return obj.loo_markov_batch if solver == "markov" else obj.loo_batch


_NOISE_ROUTE = ("is not available under a noise model (kappa=, nu=): build the predictor on a fresh Objective with the error bars "
                "fit.effective_std(stdarray, kappa, nu)")


def _noise_model(L, G, kappa, nu, solver):
    """kappa=, nu= of the predictors -> None (neither given: the plain entries) or (kappa[G, L], nu[G, L]) for the noise entries; each
    may be (L,), (G, L) or None (ones / zeros).  A noise model needs solver="markov"."""
    if kappa is None and nu is None:
        return None
    if solver != "markov":
        raise ValueError("kappa= and nu= need solver='markov' (the noise model runs in the linear-time entries only)")
    out = []
    for name, x, fill in (("kappa", kappa, 1.0), ("nu", nu, 0.0)):
        x = np.full((G, L), fill) if x is None else np.asarray(x, dtype=np.float64)
        if x.shape == (L,):
            x = np.broadcast_to(x, (G, L))
        if x.shape != (G, L):
            raise ValueError("%s must be (L,) = (%d,), (G, L) = (%d, %d) or None" % (name, L, G, L))
        out.append(np.ascontiguousarray(x))
    return tuple(out)


class Predictor:
    """The `predictTest` closure returned by gpcc() (marginaliseb.jl:259-343), three call forms:
      pred(ttest)                       ttest = list of L arrays  -> (mu_pred, Sigma_pred), joint    (:259-289)
      pred(ttest)                       ttest = one array / range -> (mu per band, sigma per band)   (:293-307)
      pred(ttest, ytest, sigmatest)     lists of L arrays         -> test log-likelihood             (:311-343)
    All linear algebra runs on the device (Objective.predict / mvnormal_logpdf).
    solver "dense" (default): every form factorises the N x N matrix.  solver "markov" (OU, matern32, matern52): the per-band form and
    the three-argument form run in linear time (Objective.predict_markov_batch / heldout_loglik_markov_batch, one row; a test point
    whose combine or predictive variance fails raises PosDefException, there being no test block for nearestposdef to repair); the
    JOINT form (Sigma_pred is T x T) stays dense, and so does sample() unless it is called with solver="markov".
    kappa=, nu= ((L,) each, or None: 1 / 0; solver "markov" only): a fitted noise model, every observation of band l having the variance
    kappa_l^2 sigma^2 + nu_l (Objective.predict_markov_noise_batch / heldout_loglik_markov_noise_batch / loo_markov_noise_batch): the
    per-band form, the three-argument form (sigmatest mapped by the same band's kappa, nu) and loo(), whose z is then standardised by
    the fitted variance, are those of a predictor on a fresh Objective with the error bars effective_std(stdarray, kappa, nu), and so,
    with the same seed, are the draws of sample(..., solver="markov") (Objective.sample_markov_noise_batch).  The joint form, and
    sample() with solver None or "dense" (the dense path has no noise model), raise NotImplementedError under a noise model: that fresh
    Objective is their route."""

    def __init__(self, objective, delays, alpha, rho, solver="dense", kappa=None, nu=None):
        if solver not in ("dense", "markov"):
            raise ValueError("solver must be 'dense' or 'markov', got %r" % (solver,))
        self.obj, self.delays, self.alpha, self.rho = objective, np.array(delays, float), np.array(alpha, float), float(rho)
        self.solver = solver
        self.noise = _noise_model(objective.L, 1, kappa, nu, solver)

    def __call__(self, ttest, ytest=None, sigmatest=None):
        L = self.obj.L
        joint = isinstance(ttest, (list, tuple)) and len(ttest) == L and all(np.ndim(a) == 1 for a in ttest)
        if self.noise is not None:
            if ytest is not None:
                held, _, info, _ = self.obj.heldout_loglik_markov_noise_batch(self.delays[None, :], self.alpha[None, :], [self.rho],
                                                                              list(ttest), list(ytest), list(sigmatest), *self.noise)
                if info[0] > 0:
                    raise PosDefException(int(info[0]))
                return float(held[0])
            if joint:
                raise NotImplementedError("the joint form " + _NOISE_ROUTE)
            tt = np.asarray(ttest, dtype=np.float64).ravel()
            n = len(tt)
            mu, var, _, info, _, _ = self.obj.predict_markov_noise_batch(self.delays[None, :], self.alpha[None, :], [self.rho], [tt] * L,
                                                                         *self.noise)
            if info[0] > 0:
                raise PosDefException(int(info[0]))
            return ([mu[0, l * n:(l + 1) * n] for l in range(L)],
                    [np.sqrt(np.maximum(var[0, l * n:(l + 1) * n], 1e-6)) for l in range(L)])      # :301-303
        if self.solver == "markov" and ytest is not None:
            held, _, info, _ = self.obj.heldout_loglik_markov_batch(self.delays[None, :], self.alpha[None, :], [self.rho], list(ttest),
                                                                    list(ytest), list(sigmatest))
            if info[0] > 0:
                raise PosDefException(int(info[0]))
            return float(held[0])
        if self.solver == "markov" and not joint:
            tt = np.asarray(ttest, dtype=np.float64).ravel()
            n = len(tt)
            mu, var, _, info, _, _ = self.obj.predict_markov_batch(self.delays[None, :], self.alpha[None, :], [self.rho], [tt] * L)
            if info[0] > 0:
                raise PosDefException(int(info[0]))
            return ([mu[0, l * n:(l + 1) * n] for l in range(L)],
                    [np.sqrt(np.maximum(var[0, l * n:(l + 1) * n], 1e-6)) for l in range(L)])      # :301-303
        if ytest is not None:
            mu, Sig = self.obj.predict(self.delays, self.alpha, self.rho, ttest)
            s2 = np.concatenate([np.asarray(a, dtype=np.float64) for a in sigmatest]) ** 2
            Sig = Sig + np.diag(s2)                                       # + Sobs*, :317-319
            yv = np.concatenate([np.asarray(a, dtype=np.float64) for a in ytest])
            try:
                return mvnormal_logpdf(mu, Sig, yv, device=self.obj.device)
            except PosDefException:
                # :327-341 -- retry once on nearestposdef(Sigma; minimumeigenvalue = 1e-6); a second
                # PosDefException propagates, as in the reference
                return mvnormal_logpdf(mu, nearestposdef(Sig, minimumeigenvalue=1e-6), yv, device=self.obj.device)
        if joint:
            return self.obj.predict(self.delays, self.alpha, self.rho, [np.asarray(a, dtype=np.float64) for a in ttest])
        tt = np.asarray(ttest, dtype=np.float64).ravel()
        n = len(tt)
        mu, Sig = self.obj.predict(self.delays, self.alpha, self.rho, [tt] * L)
        d = np.diag(Sig)
        return ([mu[l * n:(l + 1) * n] for l in range(L)],
                [np.sqrt(np.maximum(d[l * n:(l + 1) * n], 1e-6)) for l in range(L)])      # :301-303

    def loo(self, solver=None):
        """Exact leave-one-out scores of the training points under this fit -> LooScores (Objective.loo_batch, one row; no refit and
        no JITTER: p(y_i | y_-i) of the model the likelihood uses).  solver None: the predictor's own; "dense" or "markov" (OU,
        matern32, matern52: linear time).  A failed row raises PosDefException."""
        if self.noise is not None:
            if solver not in (None, "markov"):
                raise ValueError("loo under a noise model (kappa=, nu=) needs solver='markov'")
            res = self.obj.loo_markov_noise_batch(self.delays[None, :], self.alpha[None, :], [self.rho], *self.noise)
        else:
            res = _loo_entry(self.obj, solver or self.solver)(self.delays[None, :], self.alpha[None, :], [self.rho])
        if res.info[0] > 0:
            raise PosDefException(int(res.info[0]))
        sigma = np.sqrt(res.var[0])
        return LooScores(res.mu[0], sigma, res.lp[0], (self.obj.yflat - res.mu[0]) / sigma, float(res.loo[0]))

    def sample(self, ttest, S, seed, sigmatest=None, solver=None):
        """S joint draws of the light curves at ttest (Predictor's forms: a list of L arrays or one array for every band) -> per-band
        arrays (S, Ntest_l): mu_pred + chol(Sigma_pred + diag(sigmatest^2)) zeta, the latent curve without sigmatest (Sigma_pred holds
        JITTER), a replicated observation with it (Objective.sample_batch, one row).  solver None (default) or "dense": those dense
        draws, whatever the predictor's own solver.  solver "markov" (OU, matern32, matern52): draws of the same distribution in linear
        time (Objective.sample_markov_batch; other normals, so other draws); a failed filter or combine raises
        PosDefException.  Under kappa=, nu=: solver "markov" draws under the fitted noise model
        (Objective.sample_markov_noise_batch, one row: with sigmatest replicated observations of variance kappa_l^2 sigmatest^2 + nu_l
        around the curve, without it the latent curve); None or "dense" raise NotImplementedError."""
        _check_sample_solver(solver)
        if self.noise is not None and solver != "markov":
            raise NotImplementedError("sample() with solver=%r " % (solver,) + _NOISE_ROUTE + ", or call sample(..., solver='markov')")
        bands = _sample_bands(self.obj.L, ttest)
        st = None if sigmatest is None else _sample_bands(self.obj.L, sigmatest)
        if self.noise is not None:
            draws, _, _, info = self.obj.sample_markov_noise_batch(self.delays[None, :], self.alpha[None, :], [self.rho], *self.noise, bands,
                                                                   S, seed, sigmatest=st)
            if info[0] > 0:
                raise PosDefException(int(info[0]))
            return _split_bands(draws, bands)
        if solver == "markov":
            draws, _, _, info = self.obj.sample_markov_batch(self.delays[None, :], self.alpha[None, :], [self.rho], bands, S, seed,
                                                             sigmatest=st)
            if info[0] > 0:
                raise PosDefException(int(info[0]))
            return _split_bands(draws, bands)
        draws, _, _, info = self.obj.sample_batch(self.delays[None, :], self.alpha[None, :], [self.rho], bands, S, seed, sigmatest=st)
        if 0 < info[0] <= self.obj.N:
            raise PosDefException(int(info[0]))
        return _split_bands(draws, bands)


class DelayAveragedPredictor:
    """Light-curve predictions averaged over a posterior of delays: the mixture over the rows (delays[g], alpha[g], rho[g]) with
    weights[g] of the per-row posterior predictives, all rows in one batched device call (Objective.predict_batch).  delays (G, L),
    alpha (G, L) and rho (G) are typically the candidate grid and a GridFit's fitted values; weights typically
    getprobabilities(res.log_evidence) or getprobabilities(res.loglikel).  Call forms, as Predictor's per-band form (:293-307):
      pred(ttest)    ttest = one array / range  -> (mu per band, sigma per band) at those times in every band
      pred(ttest)    ttest = list of L arrays   -> the same per-band lists at each band's own times
    mu = sum p mu_g and sigma = sqrt(max(var, 1e-6)) with var = sum p (var_g + (mu_g - mu)^2), the mixture's mean and variance.
    A mixture of Gaussians has no single joint Gaussian to return, so its joint uncertainty comes as draws instead:
    sample(ttest, S, seed) returns S joint draws of the mixture, each from a row picked by the weights (Objective.sample_batch).  Its
    held-out density is well defined too: loglik(ttest, ytest, sigmatest) = log sum_g p_g N(ytest; mu_g, Sigma_g)
    (Objective.heldout_loglik_batch).
    solver "markov" (OU, matern32, matern52): __call__ and loglik run in linear time (Objective.predict_markov_batch /
    heldout_loglik_markov_batch); sample() stays dense unless it is called with solver="markov".
    kappa=, nu= ((L,) or (G, L) each, or None: 1 / 0; solver "markov" only): a noise model per row, e.g. a NoiseGridFit's (noise_predictor
    builds that predictor): __call__, loglik, loo() and sample(..., solver="markov") mix the rows of the noise entries in one call each,
    as Predictor's kappa=, nu=; sample() with solver None or "dense" raises NotImplementedError."""

    def __init__(self, objective, delays, alpha, rho, weights, solver="dense", kappa=None, nu=None):
        if solver not in ("dense", "markov"):
            raise ValueError("solver must be 'dense' or 'markov', got %r" % (solver,))
        self.obj = objective
        self.solver = solver
        self.delays = np.atleast_2d(np.asarray(delays, dtype=np.float64))
        self.alpha = np.atleast_2d(np.asarray(alpha, dtype=np.float64))
        self.rho = np.atleast_1d(np.asarray(rho, dtype=np.float64))
        self.weights = np.atleast_1d(np.asarray(weights, dtype=np.float64))
        G, L = len(self.rho), objective.L
        if self.delays.shape != (G, L) or self.alpha.shape != (G, L) or self.weights.shape != (G,):
            raise ValueError("delays and alpha must be (G, L) = (%d, %d) and weights (G,)" % (G, L))
        if not np.all(np.isfinite(self.weights)) or np.any(self.weights < 0) or not self.weights.sum() > 0:
            raise ValueError("weights must be finite, >= 0 and not all zero")
        self.noise = _noise_model(L, G, kappa, nu, solver)

    def __call__(self, ttest):
        L = self.obj.L
        if isinstance(ttest, (list, tuple)) and len(ttest) == L and all(np.ndim(a) == 1 for a in ttest):
            bands = [np.asarray(a, dtype=np.float64) for a in ttest]
        else:
            bands = [np.asarray(ttest, dtype=np.float64).ravel()] * L
        if self.noise is not None:
            _, _, _, _, mu, var = self.obj.predict_markov_noise_batch(self.delays, self.alpha, self.rho, bands, *self.noise,
                                                                      weights=self.weights)
        else:
            predict = self.obj.predict_markov_batch if self.solver == "markov" else self.obj.predict_batch
            _, _, _, _, mu, var = predict(self.delays, self.alpha, self.rho, bands, weights=self.weights)
        off = np.concatenate([[0], np.cumsum([len(b) for b in bands])])
        return ([mu[off[l]:off[l + 1]] for l in range(L)],
                [np.sqrt(np.maximum(var[off[l]:off[l + 1]], 1e-6)) for l in range(L)])      # :301-303

    def loglik(self, ttest, ytest, sigmatest):
        """The mixture's held-out log density log sum_g p_g N(ytest; mu_g, Sigma_g + diag(sigmatest^2)) of the test set (lists of L
        arrays), every row scored as Predictor(ttest, ytest, sigmatest) scores it (marginaliseb.jl:311-343)."""
        if self.noise is not None:
            return self.obj.heldout_loglik_markov_noise_batch(self.delays, self.alpha, self.rho, ttest, ytest, sigmatest, *self.noise,
                                                              weights=self.weights)[3]
        if self.solver == "markov":
            return self.obj.heldout_loglik_markov_batch(self.delays, self.alpha, self.rho, ttest, ytest, sigmatest, weights=self.weights)[3]
        return self.obj.heldout_loglik_batch(self.delays, self.alpha, self.rho, ttest, ytest, sigmatest, weights=self.weights)[3]

    def loo(self, solver=None):
        """Exact leave-one-out scores of the delay mixture, alpha and rho fixed per delay -> LooScores.  lp_i = -log sum_g p_g
        exp(-lp_gi) (the weighted harmonic mean of the rows' densities: Objective.loo_batch's mix_lp) and total = sum(lp).  Given
        y_-i the mixture's weights are q_gi proportional to p_g exp(-lp_gi); mu and sigma are the mean and the standard deviation of
        that mixture of the rows' Gaussians, z = (y - mu) / sigma.  Rows of weight 0 are left out; a failed row with weight makes
        everything NaN.  solver as Predictor.loo."""
        if self.noise is not None:
            if solver not in (None, "markov"):
                raise ValueError("loo under a noise model (kappa=, nu=) needs solver='markov'")
            res = self.obj.loo_markov_noise_batch(self.delays, self.alpha, self.rho, *self.noise, weights=self.weights)
        else:
            res = _loo_entry(self.obj, solver or self.solver)(self.delays, self.alpha, self.rho, weights=self.weights)
        keep = self.weights > 0
        p = self.weights[keep] / self.weights[keep].sum()
        x = np.log(p)[:, None] - res.lp[keep]
        q = np.exp(x - x.max(axis=0))
        q = q / q.sum(axis=0)
        mu = np.sum(q * res.mu[keep], axis=0)
        sigma = np.sqrt(np.sum(q * (res.var[keep] + (res.mu[keep] - mu) ** 2), axis=0))
        return LooScores(mu, sigma, res.mix_lp, (self.obj.yflat - mu) / sigma, float(res.mix_loo))

    def sample(self, ttest, S, seed, sigmatest=None, solver=None):
        """S joint draws of the delay-averaged light curves -> (per-band arrays (S, Ntest_l), row[S]): draw s comes from the row
        row[s], picked with probability weights[row] / sum(weights), so (self.delays[row[s]], draws[.][s]) are joint (tau, f*)
        samples.  ttest and sigmatest take Predictor's forms; without sigmatest the latent curves, with it replicated observations.
        solver None (default) or "dense": Objective.sample_batch whatever the predictor's own solver; "markov": the same mixture drawn in
        linear time (Objective.sample_markov_batch; the same rows for the same seed and weights, other normals).  Under kappa=, nu=:
        solver "markov" draws every row under its own noise model in one call (Objective.sample_markov_noise_batch; the same rows again);
        None or "dense" raise NotImplementedError."""
        _check_sample_solver(solver)
        if self.noise is not None and solver != "markov":
            raise NotImplementedError("sample() with solver=%r " % (solver,) + _NOISE_ROUTE + ", or call sample(..., solver='markov')")
        bands = _sample_bands(self.obj.L, ttest)
        st = None if sigmatest is None else _sample_bands(self.obj.L, sigmatest)
        if self.noise is not None:
            draws, rows, _, _ = self.obj.sample_markov_noise_batch(self.delays, self.alpha, self.rho, *self.noise, bands, S, seed,
                                                                   sigmatest=st, weights=self.weights)
            return _split_bands(draws, bands), rows
        if solver == "markov":
            draws, rows, _, _ = self.obj.sample_markov_batch(self.delays, self.alpha, self.rho, bands, S, seed, weights=self.weights,
                                                             sigmatest=st)
            return _split_bands(draws, bands), rows
        draws, rows, _, _ = self.obj.sample_batch(self.delays, self.alpha, self.rho, bands, S, seed, weights=self.weights, sigmatest=st)
        return _split_bands(draws, bands), rows


def noise_predictor(objective, candidatedelays, noisefit, weights=None):
    """The DelayAveragedPredictor of a NoiseGridFit (gpcc_grid_noise): the rows (candidatedelays[g], noisefit.alpha[g], noisefit.rho[g])
    each under its own fitted noise model (noisefit.kappa[g], noisefit.nu[g]), in linear time.  weights: (G,), default
    getprobabilities(noisefit.loglikel).  Its predictions, held-out density and leave-one-out scores are one device call each, where a
    fresh Objective on effective_std per candidate delay was G of them; so are its joint (tau, f*) draws, by sample(ttest, S, seed,
    solver="markov") -> (per-band draws, row): the posterior light curves of the noise fit, or with sigmatest replicated observations
    for a posterior-predictive check (sample() with the default solver raises: the dense path has no noise model)."""
    delays = np.atleast_2d(np.asarray(candidatedelays, dtype=np.float64))
    if weights is None:
        weights = getprobabilities(np.asarray(noisefit.loglikel, dtype=np.float64))
    return DelayAveragedPredictor(objective, delays, noisefit.alpha, noisefit.rho, weights, solver="markov", kappa=noisefit.kappa,
                                  nu=noisefit.nu)


def gpcc(tarray, yarray, stdarray, *, kernel, delays, iterations, seed=1, numberofrestarts=1, initialrandom=5,
         rhomin=0.1, rhomax, device=0, solver="dense"):
    """loglikel, pred, (alpha, postb, rho) = gpcc(tarray, yarray, stdarray; kernel, delays, iterations, ...)
    -- src/gpccfixdelay_marginaliseb.jl:46-53.  postb is returned as (mu_postb, Sigma_postb), the
    parameters of the reference's MvNormal (:252).  solver: gpcc_grid's; with "markov" the fit, postb (the filter's final state) and the
    returned Predictor's per-band and held-out forms are all linear-time (its joint form and sample() stay dense)."""
    delays = np.asarray(delays, dtype=np.float64)
    assert len(delays) == len(tarray) == len(yarray) == len(stdarray)              # :78
    obj = Objective(tarray, yarray, stdarray, kernel, marginalise_b=True, device=device)
    res = gpcc_grid(tarray, yarray, stdarray, kernel=kernel, candidatedelays=delays[None, :], iterations=iterations,
                    seed=seed, numberofrestarts=numberofrestarts, initialrandom=initialrandom, rhomin=rhomin,
                    rhomax=rhomax, objective=obj, solver=solver)
    alpha, rho = res.alpha[0], float(res.rho[0])
    if solver == "markov":
        mu_b, Sig_b, _, info = obj.posterior_offsets_markov_batch(delays[None, :], alpha[None, :], [rho])
        if info[0] > 0:
            raise PosDefException(int(info[0]))
        postb = (mu_b[0], Sig_b[0])
    else:
        postb = obj.posterior_offsets(delays, alpha, rho)
    return float(res.loglikel[0]), Predictor(obj, delays, alpha, rho, solver=solver), (alpha, postb, rho)


def singlegp(tobs, yobs, sigmaobs, *, kernel, iterations, seed=1, numberofrestarts=1, initialrandom=5, rhomin=0.1,
             rhomax, device=0):
    """src/util.jl:95-99: one band, delay [0.0] -- gpccfixdelay([tobs], [yobs], [sigmaobs]; tau = [0.0], ...)."""
    return gpcc([tobs], [yobs], [sigmaobs], kernel=kernel, delays=[0.0], iterations=iterations, seed=seed,
                numberofrestarts=numberofrestarts, initialrandom=initialrandom, rhomin=rhomin, rhomax=rhomax, device=device)


# ------------------------------------------------------------------------------------------
# Cross-validation (src/UNUSED/performcv.jl)
# ------------------------------------------------------------------------------------------
def cvindices(Nl, numberoffolds, seed):
    """The folds of performcv.jl:59: per band b (1-based) a partition of range(Nl[b-1]) into `numberoffolds` test folds (sorted index
    arrays) whose sizes differ by at most 1, drawn from numpy.random.default_rng(seed + b) -- the reference's `seedcv + b`.  A band with
    fewer points than folds leaves some folds empty.  MiscUtil's CVindices and Julia's random stream are not available here, so these
    folds are this project's own (as the random starts of gpcc_grid_loglik are), not the reference's."""
    F = int(numberoffolds)
    if F < 2:
        raise ValueError("numberoffolds must be >= 2, got %d" % F)
    out = []
    for b, n in enumerate(Nl, start=1):
        perm = np.random.default_rng(int(seed) + b).permutation(int(n))
        out.append([np.sort(f) for f in np.array_split(perm, F)])
    return out


def _split(tobs, yobs, sobs, folds, f):
    """(train, test) of fold f: each a triple of per-band lists."""
    L = len(tobs)
    tr, te = ([], [], []), ([], [], [])
    for b in range(L):
        n = len(tobs[b])
        test = folds[b][f]
        train = np.setdiff1d(np.arange(n), test)
        for k, arr in enumerate((tobs, yobs, sobs)):
            a = np.asarray(arr[b], dtype=np.float64)
            tr[k].append(a[train])
            te[k].append(a[test])
    return tr, te


def _check_folds(tobs, yobs, sobs, folds, F):
    for b in range(len(tobs)):
        if not len(tobs[b]) == len(yobs[b]) == len(sobs[b]):
            raise AssertionError("length(tobs[i]) == length(yobs[i]) == length(σobs[i])")
        for f in range(F):
            ntrain = len(tobs[b]) - len(folds[b][f])
            if ntrain < 2:
                raise ValueError("fold %d leaves band %d with %d training point(s): the marginalised offset needs at least 2 per band "
                                 "(sample variance)" % (f + 1, b + 1, ntrain))
    for f in range(F):
        if sum(len(folds[b][f]) for b in range(len(tobs))) == 0:
            raise ValueError("fold %d has no test points in any band" % (f + 1))


def performcv(tobs, yobs, σobs, *, delays, kernel, iterations=1, seedcv=1, numberofrestarts=1, initialrandom=1, numberoffolds=5,
              rhomin=0.1, rhomax=20.0, device=0):
    """fitness[F] = performcv(tobs, yobs, σobs; delays, kernel, ...) -- src/UNUSED/performcv.jl with its defaults: per fold, gpcc() on
    the training split (seed = seedcv), then the Predictor's test log-likelihood of the held-out split.  Folds: cvindices(.., seedcv)."""
    assert len(tobs) == len(yobs) == len(σobs)
    F = int(numberoffolds)
    folds = cvindices([len(a) for a in tobs], F, seedcv)
    _check_folds(tobs, yobs, σobs, folds, F)
    fitness = np.zeros(F)
    for f in range(F):
        (ttr, ytr, str_), (tte, yte, ste) = _split(tobs, yobs, σobs, folds, f)
        _, pred, _ = gpcc(ttr, ytr, str_, kernel=kernel, delays=delays, numberofrestarts=numberofrestarts, initialrandom=initialrandom,
                          iterations=iterations, seed=seedcv, rhomin=rhomin, rhomax=rhomax, device=device)
        fitness[f] = pred(tte, yte, ste)
        pred.obj.close()
    return fitness


class CVGrid:
    """Result of performcv_grid: heldout[F, G] and info[F, G] (Objective.heldout_loglik_batch per fold and delay), fits[F] (the folds'
    GridFits), weights[F, G] (each fold's own delay posterior), mix[F] (the delay-averaged held-out score per fold), cv_score[G] =
    heldout.sum(0) and probabilities = getprobabilities(cv_score)."""

    def __init__(self, heldout, info, fits, weights, mix, refit):
        self.heldout, self.info, self.fits, self.weights, self.mix, self.refit = heldout, info, fits, weights, mix, refit
        self.cv_score = heldout.sum(0)
        ok = np.isfinite(self.cv_score)
        self.probabilities = getprobabilities(np.where(ok, self.cv_score, -np.inf)) if ok.any() else np.full_like(self.cv_score, np.nan)


def performcv_grid(tobs, yobs, σobs, *, candidatedelays, kernel, iterations=1, seedcv=1, numberofrestarts=1, initialrandom=1,
                   numberoffolds=5, rhomin=0.1, rhomax=20.0, evidence=None, device=0, solver="dense"):
    """performcv over a whole grid of candidate delays (G, L): per fold ONE Objective on the training split, ONE gpcc_grid fit over all
    G delays (seed = seedcv, as performcv's gpcc calls) and ONE heldout_loglik_batch over the G rows, weighted by the fold's own delay
    posterior (getprobabilities(loglikel), or of log_evidence with evidence="laplace") -> CVGrid.  heldout[:, g] is what performcv
    returns at delay g.  Compare kernels by performcv_grid(...).mix.sum().  solver: gpcc_grid's; with "markov" the folds' fits AND their
    held-out scores are linear-time (heldout_loglik_markov_batch: no nearestposdef retry, refit stays False)."""
    cand = np.ascontiguousarray(np.atleast_2d(candidatedelays), dtype=np.float64)
    G, L = cand.shape
    assert L == len(tobs) == len(yobs) == len(σobs)
    F = int(numberoffolds)
    folds = cvindices([len(a) for a in tobs], F, seedcv)
    _check_folds(tobs, yobs, σobs, folds, F)
    held = np.empty((F, G))
    info = np.zeros((F, G), dtype=np.int32)
    wts = np.empty((F, G))
    mix = np.empty(F)
    refit = np.zeros((F, G), dtype=bool)
    fits = []
    for f in range(F):
        (ttr, ytr, str_), (tte, yte, ste) = _split(tobs, yobs, σobs, folds, f)
        with Objective(ttr, ytr, str_, kernel, marginalise_b=True, device=device) as obj:
            res = gpcc_grid(ttr, ytr, str_, kernel=kernel, candidatedelays=cand, iterations=iterations, seed=seedcv,
                            numberofrestarts=numberofrestarts, initialrandom=initialrandom, rhomin=rhomin, rhomax=rhomax, objective=obj,
                            evidence=evidence, solver=solver)
            score = res.log_evidence if evidence == "laplace" else res.loglikel
            score = np.where(np.isfinite(score), score, -np.inf)
            w = getprobabilities(score)
            a = np.where(np.isfinite(res.alpha), res.alpha, 1.0)   # (a delay without a fit: a placeholder row of weight 0)
            r = np.where(np.isfinite(res.rho), res.rho, 1.0)
            if solver == "markov":
                held[f], _, info[f], mix[f] = obj.heldout_loglik_markov_batch(cand, a, r, tte, yte, ste, weights=w)
            else:
                held[f], _, info[f], mix[f], refit[f] = obj.heldout_loglik_batch(cand, a, r, tte, yte, ste, weights=w)
            held[f][~(np.all(np.isfinite(res.alpha), axis=1) & np.isfinite(res.rho))] = np.nan
            wts[f] = w
            fits.append(res)
    return CVGrid(held, info, fits, wts, mix, refit)
