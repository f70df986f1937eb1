"""Synthetic irregularly-sampled light curves (numpy only, host side).

Restates the statistical recipe of the reference's generator
(/root/reference/src/simulatedata.jl:96-162) at arbitrary size, as SURVEY.md section 8(d)
prescribes: per band, times ~ U(0, T) i.i.d. and UNSORTED with T = N_l/3 days (the reference
has 60 observations on [0, 20], simulatedata.jl:119-121); a latent OU process with rho = 3.5
drawn exactly by its AR(1) recursion on the merged, delay-shifted, sorted time axis (instead of
the reference's O(N^3) MvNormal draw, :128-145); y_l = alpha_l^2 f(t_l - tau_l) + b_l + sigma eps
(alpha enters twice in the reference: inside C at :128 and again at :153);
alpha = (1, 1.5, 2), b = (6, 15, 25), true delays (0, 2, 4), sigma = 0.75 (:105-111, :153-159).
The reference's MersenneTwister stream cannot be reproduced without Julia; numpy's PCG64 is used.
"""
import numpy as np

TRUE_DELAYS = (0.0, 2.0, 4.0)
ALPHAS = (1.0, 1.5, 2.0)
OFFSETS = (6.0, 15.0, 25.0)
RHO_TRUE = 3.5


def simulate_lightcurves(Nl, seed=1, sigma=0.75, rho=RHO_TRUE, gap_band=None, span=None):
    """Returns (tarray, yarray, stdarray, truedelays) as lists of float64 arrays, band order kept.

    gap_band: optional band index that gets the reference's mid-gap pattern
    (half the points in [0, 0.4T], half in [0.6T, T]; simulatedata.jl:121).
    """
    Nl = [int(n) for n in Nl]
    L = len(Nl)
    if L < 1 or L > len(TRUE_DELAYS):
        raise ValueError("1 <= number of bands <= %d" % len(TRUE_DELAYS))
    rng = np.random.default_rng(seed)
    tarray = []
    for l, n in enumerate(Nl):
        T = span if span is not None else n / 3.0
        if gap_band is not None and l == gap_band:
            h = n // 2
            t = np.concatenate([rng.random(h) * 0.4 * T, 0.6 * T + rng.random(n - h) * 0.4 * T])
        else:
            t = rng.random(n) * T
        tarray.append(t)
    # latent OU on the merged shifted axis, exact AR(1): f(s_k) = phi f(s_{k-1}) + sqrt(1-phi^2) e
    u = np.concatenate([tarray[l] - TRUE_DELAYS[l] for l in range(L)])
    order = np.argsort(u, kind="stable")
    us = u[order]
    e = rng.standard_normal(len(us))
    f_sorted = np.empty_like(us)
    f_sorted[0] = e[0]
    phi = np.exp(-np.diff(us) / rho)
    sd = np.sqrt(np.maximum(0.0, 1.0 - phi * phi))
    for k in range(1, len(us)):
        f_sorted[k] = phi[k - 1] * f_sorted[k - 1] + sd[k - 1] * e[k]
    f = np.empty_like(us)
    f[order] = f_sorted
    yarray, stdarray = [], []
    off = 0
    for l, n in enumerate(Nl):
        fl = f[off:off + n]
        off += n
        y = ALPHAS[l] ** 2 * fl + OFFSETS[l] + sigma * rng.standard_normal(n)
        yarray.append(y)
        stdarray.append(np.full(n, sigma))
    return tarray, yarray, stdarray, list(TRUE_DELAYS[:L])


def default_hyperparameters(yarray):
    """Fixed hyper-parameters for fixed-hyper sweeps: alpha_l = var(y_l)
    (centre of sampleα, gpccfixdelay_marginaliseb.jl:188), rho = 3.5."""
    return np.array([np.var(y, ddof=1) for y in yarray]), RHO_TRUE


def flux_randomise(yarray, stdarray, R, seed):
    """R flux-randomised realisations of a data set on its own cadence: per band an (R, N_l) array y_l + sigma_l z, z standard normal,
    every flux redrawn within its error bar (reverberation mapping's "flux randomisation").  Reproducible from the seed (numpy's PCG64;
    the bands are drawn one after the other from one generator).  What Objective.loglik_markov_realisations and
    fit.realisation_delays take as Y."""
    R = int(R)
    if R < 1:
        raise ValueError("R >= 1")
    rng = np.random.default_rng(seed)
    out = []
    for y, sd in zip(yarray, stdarray):
        y, sd = np.asarray(y, np.float64).reshape(-1), np.asarray(sd, np.float64).reshape(-1)
        out.append(y[None, :] + sd[None, :] * rng.standard_normal((R, len(y))))
    return out


def resample(yarray, stdarray, R, seed, flux=True, subset=True):
    """R resampled realisations of a data set on its own cadence, reverberation mapping's FR/RSS -> (Y, counts): per band an (R, N_l)
    array of fluxes and an (R, N_l) integer array of multiplicities.  flux: flux_randomise's recipe, y_l + sigma_l z with z standard
    normal (False: y_l unchanged).  subset: random subset selection -- per band N_l indices drawn with replacement, counts their
    multiplicities (each band's counts sum to N_l; a point not drawn has count 0, a point drawn n times stands for error bar
    sigma / sqrt n); a draw that leaves a band fewer than 2 distinct points is redrawn, so every band keeps at least 2 (False: counts
    of 1).  Realisation r is drawn from its own generator (numpy's PCG64 seeded with (seed, r); per band first the fluxes, then the
    indices): reproducible from the seed and the same in any R.  What Objective.loglik_markov_resampled and fit.realisation_refits
    take as Y and counts."""
    R = int(R)
    if R < 1:
        raise ValueError("R >= 1")
    ys = [np.asarray(y, np.float64).reshape(-1) for y in yarray]
    sds = [np.asarray(sd, np.float64).reshape(-1) for sd in stdarray]
    if subset and any(len(y) < 2 for y in ys):
        raise ValueError("random subset selection keeps at least 2 distinct points per band: a band has fewer")
    Y = [np.empty((R, len(y))) for y in ys]
    counts = [np.ones((R, len(y)), dtype=np.int64) for y in ys]
    for r in range(R):
        rng = np.random.default_rng([int(seed), r])
        for l, (y, sd) in enumerate(zip(ys, sds)):
            Y[l][r] = y + sd * rng.standard_normal(len(y)) if flux else y
            while subset:
                c = np.bincount(rng.integers(0, len(y), len(y)), minlength=len(y))
                if np.count_nonzero(c) >= 2:
                    counts[l][r] = c
                    break
    return Y, counts
