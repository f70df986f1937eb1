"""The entries that take a per-row noise model or a per-row data set over tests/_markov_regime_cases.py (RC), whose cases, order and seeds
stay as they are (tests/test_markov_regime_noise_cpu.py, tests/test_gpu_markov_regime_noise.py): lambda x lag down to 5e-8, rho up to 3e5,
4 and 8 bands with three or more bands tied on one shifted time.

Noise model of a regime case: drawn from one default_rng(SEED) in RC.cases()' order, kappa_l uniform in [0.5, 2], nu_l uniform in
[0, 0.05]; on every second case band 0 gets kappa = 0, nu = 0.01; on every third case the last band gets kappa = 1, nu = 0 exactly.  The
times are compressed by 2^-k, y and sigma are not, so the same ranges serve every tier.  A noise case is RC's tuple with (kappa, nu)
appended: _markov_noise_cases' form.

OU twins without ties: every OU case of the N <= 120 shapes (L = 2, 4, 8; four k tiers: 12) again with the delays
delays[l] + l 2^-14 2^-k -- exact, and with every time on the 2^-10 2^-k grid no two bands share a shifted time any more (asserted from
the data: RC.shared_times is empty, _markov_hess_full_cases.tie_rows is False); ties inside a band stay.  The new lags, 2^-14 2^-k, are
smaller than any of the tier: intended, the e_mirror rule covers it.  A twin has its case's noise model, tier and k.

Resampled cells: per N <= 120 case R = 4 realisations as _markov_resample_cases.realisations builds them (own y, flux, subset, flux +
subset), per N = 370 case the "flux + subset" one.  y and sigma are those of the shape, whatever the kernel and the tier, so a shape has
one set of realisations; its seed is the first of seed0, seed0 + 3, ... (seed0 = 100 N + L) at which, for L >= 3, the "subset" and the
"flux + subset" realisation both keep a shifted time shared by >= 3 bands and a kept point on a cross-band tie with count >= 2
(subset_condition, from the data; counted again by the CPU test for every case).  No case is filtered out.

References and bars are the families' own, from the reference side: _markov_noise_cases.reference_job, value_bar and noise_bar,
_grad_highprec.bar for the first 2L + 1 gradient entries; _markov_noise_hess_full_cases.reference_job with its block bars, scale and
_markov_hess_full_cases.device_limit -- its blocks aa, ar, rr, an, rn, nn are _markov_noise_hess_cases' (the same trace formulas over the
same entries, so one reference serves both Hessian entries); _markov_cases.reference_and_bar on the reduced fresh data set of a cell.
RC's rule on top: outside the control tier max(existing bar, FACTOR x e_mirror), e_mirror = |numpy mirror - extended| of
markov.loglik_grad_noise, loglik_hess_full_noise (whose [alpha, rho, kappa, nu] sub-block is loglik_hess_noise's exactly),
loglik_resampled and loglik_realisations, measured on the CPU and never from the device."""
import numpy as np

import _grad_highprec as H
import _markov_cases as MC
import _markov_hess_full_cases as FC
import _markov_noise_cases as NC
import _markov_noise_hess_full_cases as NF
import _markov_regime_cases as RC
import _markov_resample_cases as SC
from gpcc_amd import markov

FACTOR = RC.FACTOR
SEED = 11
R = SC.R
ROWS = 65
TWIN_SHIFT = 2.0 ** -14
SUBSET_CELLS = (2, 3)
_noise, _twins, _real, _seed = {}, [], {}, {}


# ---- the noise model -------------------------------------------------------------------------------------------------------------------
def noise_of(cid):
    """(kappa[L], nu[L]) of a regime case (a twin: its case's)."""
    if not _noise:
        rg = np.random.default_rng(SEED)
        for idx, c in enumerate(RC.cases()):
            L = len(c[4])
            kappa, nu = rg.uniform(0.5, 2.0, L), rg.uniform(0.0, 0.05, L)
            if idx % 2 == 1:
                kappa[0], nu[0] = 0.0, 0.01
            if idx % 3 == 2:
                kappa[L - 1], nu[L - 1] = 1.0, 0.0
            _noise[c[0]] = (kappa, nu)
    return _noise[cid[:-len("-twin")] if cid.endswith("-twin") else cid]


def noise_case(case):
    return tuple(case[:8]) + noise_of(case[0])


def cases(tier=None, kernel=None, small=None):
    """The regime cases (of a tier, a kernel, the N <= 120 shapes or the others) with their noise models."""
    return [noise_case(c) for c in RC.cases() if (tier is None or RC.TIER[c[0]] == tier) and (kernel is None or c[1] == kernel)
            and (small is None or (c[7] <= RC.SMALL) == small)]


def twins(tier=None):
    """The 12 OU twins without cross-band ties (of a tier), with their noise models."""
    if not _twins:
        for c in RC.small_cases():
            cid, kernel, data, delays, alpha, rho, mb, N = c
            if kernel != "OU":
                continue
            k = RC.K_OF[cid]
            d = delays + np.arange(len(delays)) * TWIN_SHIFT * 2.0 ** -k
            assert np.array_equal((d - delays) * 2.0 ** (14 + k), np.arange(len(delays)))                 # exact
            assert not RC.shared_times(data[0], d) and not FC.tie_rows(data[0], d)[0], cid
            tid = cid + "-twin"
            RC.TIER[tid], RC.K_OF[tid] = RC.TIER[cid], k
            _twins.append(noise_case((tid, kernel, data, d, alpha, rho, mb, N)))
        assert len(_twins) == 12 and sorted({len(c[4]) for c in _twins}) == [2, 4, 8]
    return [c for c in _twins if tier is None or RC.TIER[c[0]] == tier]


def batch(case, seed):
    """(delays, alpha, rho, kappa, nu) of 65 rows, every row with its own, the case's row last: alone in a second, ragged wave."""
    cid, k, data, delays, alpha, rho, mb, N, kappa, nu = case
    L = len(alpha)
    rg = np.random.default_rng(seed)
    M = ROWS - 1
    d = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 45.0, (M, L - 1)))], 1) * 2.0 ** -RC.K_OF[cid]
    a, r = rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))
    kap, exc = rg.uniform(0.5, 2.0, (M, L)), rg.uniform(0.0, 0.05, (M, L))
    return (np.concatenate([d, delays[None, :]]), np.concatenate([a, alpha[None, :]]), np.concatenate([r, [rho]]),
            np.concatenate([kap, kappa[None, :]]), np.concatenate([exc, nu[None, :]]))


# ---- value and gradient under the noise model ---------------------------------------------------------------------------------------
def grad_job(job):
    """(what, noise case) -> "ref": _markov_noise_cases.reference_job's (Reference on the effective error bars, g_kappa, g_nu), info == 0
    asserted; "mirror": markov.loglik_grad_noise's (value, gradient[4L + 1]).  A top-level function, for a process pool."""
    what, case = job
    cid, kernel, data, delays, alpha, rho, mb, N, kappa, nu = case
    if what == "ref":
        out = NC.reference_job(NC.job(case))
        assert out[0].info == 0, cid
        return out
    ll, g, info = markov.loglik_grad_noise(kernel, *data, delays, alpha, rho, kappa, nu, mb)
    assert info == 0, cid
    return ll, g


def grad_references(pool, cases):
    """{case id: GradBars' job} of noise cases."""
    res = list(pool.map(grad_job, [(w, c) for c in cases for w in ("ref", "mirror")]))
    return {c[0]: res[2 * i] + res[2 * i + 1] for i, c in enumerate(cases)}


class GradBars:
    """The existing bars of a noise case's value (relative), first 2L + 1 gradient entries and 2L noise entries (absolute), and the
    mirror's error of each."""

    def __init__(self, oracle, case, job):
        self.ref, self.gk, self.gv, self.mirror_ll, self.mirror_grad = job
        self.case, self.L = case, len(case[4])
        self.want_noise = np.concatenate([self.gk, self.gv])
        self.existing = {"value": NC.value_bar(oracle, case, self.ref)[0], "grad": H.bar(self.ref), "noise": NC.noise_bar(self.ref, self.gk, self.gv)}
        self.e_mirror = self.errors(self.mirror_ll, self.mirror_grad)

    def errors(self, ll, grad):
        """{quantity: error} of a row (value, gradient[4L + 1]); a NaN is an infinite error."""
        K = 2 * self.L + 1
        grad = np.asarray(grad, np.float64)
        e = {"value": abs(ll - self.ref.loglik) / abs(self.ref.loglik), "grad": np.max(np.abs(grad[:K] - self.ref.grad)),
             "noise": np.max(np.abs(grad[K:] - self.want_noise))}
        return {q: float(v) if v == v else np.inf for q, v in e.items()}

    def add(self, worst, ll, grad, show=True):
        """A row's three pairs into {quantity: RC.Worst}.  -> {quantity: error / bar}"""
        e = self.errors(ll, grad)
        return {q: RC.add_pair(worst[q], self.case[0], q, e[q], self.existing[q], self.e_mirror[q], show) for q in ("value", "grad", "noise")}


# ---- the Hessians under the noise model ---------------------------------------------------------------------------------------------
def ships_hessian(case):
    return RC.ships_hessian(case[:8])


def hess_job(job):
    """(what, noise case, part) -> "ref": _markov_noise_hess_full_cases.reference_job's NoiseReference over 4L + 1 with the ten blocks'
    bars, info == 0 asserted; "mirror": markov.loglik_hess_full_noise's matrix (NaN in the tau entries of an OU row with a cross-band
    tie) restricted to the pairs of _pairs(L)[part] (pairs=: each pair is a pass of its own, so the parts put together are the whole
    call's matrix bit for bit), NaN elsewhere."""
    what, case, part = job
    cid, kernel, data, delays, alpha, rho, mb, N, kappa, nu = case
    if what == "ref":
        try:
            import torch
            torch.set_num_threads(2)
        except Exception:
            pass
        ref = NF.reference_job(NF.job(case))
        assert ref.info == 0, cid
        return ref
    out = markov.loglik_hess_full_noise(kernel, *data, delays, alpha, rho, kappa, nu, mb, pairs=_pairs(len(alpha))[part])
    assert out[3] == 0, cid
    return out[2]


def _pairs(L):
    """The (4L + 1)(4L + 2) / 2 pairs dealt into 1 (L <= 2), 3 (L <= 4) or 8 parts, every part a mix of all blocks: the mirror walks one
    pair at a time, 561 of them at L = 8, and a pool shares the parts."""
    n = 4 * L + 1
    pairs = [(a, b) for a in range(n) for b in range(a, n)]
    parts = 1 if L <= 2 else (3 if L <= 4 else 8)
    return [pairs[i::parts] for i in range(parts)]


def hess_references(pool, cases):
    """{case id: (NoiseReference, the mirror's full matrix)} of the noise cases that ship."""
    cases = [c for c in cases if ships_hessian(c)]
    jobs = [("ref", c, 0) for c in cases] + [("mirror", c, i) for c in cases for i in range(len(_pairs(len(c[4]))))]
    res = list(pool.map(hess_job, jobs))
    out, k = {}, len(cases)
    for i, c in enumerate(cases):
        parts = _pairs(len(c[4]))
        H = np.full((4 * len(c[4]) + 1,) * 2, np.nan)
        for pairs in parts:
            for a, b in pairs:
                H[a, b] = H[b, a] = res[k][a, b]
            k += 1
        out[c[0]] = (res[i], H)
    return out


def tied(case):
    """Whether the case's own row is an OU row with a cross-band tie: NaN in the tau entries by contract."""
    return case[1] == "OU" and bool(FC.tie_rows(case[2][0], case[3])[0])


def hess_pairs(ref, case, got, mirror, blocks, index=None):
    """[(quantity, error, existing bar, e_mirror)] per block of a matrix over the indices `index` of the 4L + 1 order (default: all), the
    existing bar being the one of _markov_noise_hess_full_cases.ratios, bar_B / scale, times _markov_hess_full_cases.device_limit.  On a
    tied OU row the tau blocks are left out (the NaN contract is the caller's)."""
    L = ref.L
    index = list(range(4 * L + 1)) if index is None else list(index)
    ix = np.ix_(index, index)
    want = ref.H[ix]
    out = []
    for b, m in NF.block_masks(L).items():
        m = m[ix]
        if b not in blocks or not m.any() or (b in NF.TAU_BLOCKS and tied(case)):
            continue
        e = np.abs(np.asarray(got, np.float64) - want)[m]
        em = np.abs(np.asarray(mirror, np.float64)[ix] - want)[m]
        assert np.isfinite(em).all(), (case[0], b)
        out.append((b, float(np.max(np.where(np.isnan(e), np.inf, e))), ref.bars[b] / NF.scale(case) * FC.device_limit(case[:8]), float(np.max(em))))
    return out


def tau_pairs_distinct(H, L, bar):
    """Whether the L (L - 1) / 2 off-diagonal (tau_l, tau_m) entries of a reference matrix (2L + 1 or 4L + 1 order) differ pairwise by
    more than bar: then no wrong decoding of a pair's slot passes by a symmetry of the data.  -> (smallest difference, bar)"""
    v = np.array([H[L + 1 + l, L + 1 + m] for l in range(L) for m in range(l + 1, L)], np.float64)
    d = np.abs(v[:, None] - v[None, :])[np.triu_indices(len(v), 1)]
    return float(np.min(d)), float(bar)


# ---- the per-row data sets ------------------------------------------------------------------------------------------------------------
def subset_condition(t, delays, counts, r):
    """(a shifted time is shared by >= 3 bands among the kept points of realisation r, a kept point on a cross-band tie has count >= 2)."""
    kept = [np.asarray(t[l], np.float64)[np.asarray(counts[l][r]) > 0] for l in range(len(t))]
    sh = RC.shared_times(kept, delays)
    twice = any(float(u - delays[l]) in sh for l in range(len(t)) for u in np.asarray(t[l], np.float64)[np.asarray(counts[l][r]) >= 2])
    return any(len(b) >= 3 for b in sh.values()), twice


def _build(y, s, seed):
    from gpcc_amd import synthetic
    Yf, _ = synthetic.resample(y, s, 1, seed, flux=True, subset=False)
    _, cs = synthetic.resample(y, s, 1, seed + 1, flux=False, subset=True)
    Yb, cb = synthetic.resample(y, s, 1, seed + 2, flux=True, subset=True)
    Y, counts = [], []
    for l in range(len(y)):
        yl = np.asarray(y[l], np.float64)[None, :]
        Y.append(np.concatenate([yl, Yf[l], yl, Yb[l]], axis=0))
        counts.append(np.concatenate([np.ones_like(cs[l]), np.ones_like(cs[l]), cs[l], cb[l]], axis=0))
    return Y, counts


def realisations(case):
    """(Y, counts) of a case: lists of L arrays (4, N_l), SC.KINDS in this order; one set per shape (N, L), at the shape's seed."""
    cid, _, (t, y, s), delays = case[:4]
    key = (case[7], len(t))
    if key not in _real:
        seed = 100 * key[0] + key[1]
        while True:
            Y, counts = _build(y, s, seed)
            if len(t) < 3 or all(all(subset_condition(t, delays, counts, r)) for r in SUBSET_CELLS):
                break
            seed += 3
        _real[key], _seed[key] = (Y, counts), seed
    return _real[key]


def cells(case):
    """The realisations of a case that are checked: all four at the N <= 120 shapes, "flux + subset" at N = 370."""
    return tuple(range(R)) if case[7] <= RC.SMALL else (3,)


def resample_cases(tier):
    """The cases of the resampled entries' test in a tier: the N <= 120 cases of a k tier, the N = 370 cases of a rho tier."""
    return [c for c in RC.tier(tier) if c[7] <= RC.SMALL or c[7] == 370]


def reduced_case(case, r):
    """Realisation r of a case as a case of _markov_cases.py: its reduced fresh data set, N = the kept points."""
    cid, kernel, data, delays, alpha, rho, mb, _ = case[:8]
    Y, counts = realisations(case)
    red = SC.reduced(data, Y, counts, r)
    return ("%s/regime%d" % (cid, r), kernel, red, delays, alpha, rho, mb, sum(len(a) for a in red[0]))


def same_model(case, r):
    """Whether loglik_markov_realisations' cell r (each realisation's own band means, the HANDLE's offset prior variances) is the value
    of the reduced fresh data set: no subset, and either the handle's own y or no marginalised offsets."""
    return r < 2 and (r == 0 or not case[6])


def cell_job(job):
    """(case, r) -> (reference, existing relative bar, the mirror's loglik_resampled value, its loglik_realisations value or None) of
    a cell: _markov_cases.reference_and_bar on the reduced fresh data set; info == 0 asserted on all sides."""
    case, r = job
    cid, kernel, (t, y, s), delays, alpha, rho, mb, N = case[:8]
    o = RC._oracle()
    ref, bar, _ = MC.reference_and_bar(o, reduced_case(case, r))
    Y, counts = realisations(case)
    mean, vb = markov.resample_constants(t, Y, counts, mb)
    ll, info = markov.loglik_resampled(kernel, t, y, s, Y, counts, [r], delays, alpha, rho, mb, mean, vb)
    assert info[0] == 0, (cid, r)
    multi = None
    if same_model(case, r):
        m, minfo = markov.loglik_realisations(kernel, t, y, s, Y, delays, alpha, rho, mb, mean=mean)
        assert minfo[0] == 0, (cid, r)
        multi = float(m[0][r])
    return ref, bar, float(ll[0]), multi


def cell_references(pool, cases):
    """{(case id, r): cell_job's} of the checked cells of the cases."""
    jobs = [(c, r) for c in cases for r in cells(c)]
    return {(c[0], r): v for (c, r), v in zip(jobs, pool.map(cell_job, jobs))}


# ---- slips: what the bars have to catch -------------------------------------------------------------------------------------------------
RESAMPLE_SLIPS = ("count_as_one", "dropped_kept")


def grad_slip_job(job):
    """(noise case, slip of _markov_noise_cases.SLIPS) -> markov.loglik_grad_noise's (value, gradient) with the slip."""
    case, slip = job
    cid, kernel, data, delays, alpha, rho, mb, N, kappa, nu = case
    ll, g, info = markov.loglik_grad_noise(kernel, *data, delays, alpha, rho, kappa, nu, mb, _slip=slip)
    assert info == 0, (cid, slip)
    return ll, g


def resample_slip_job(job):
    """(case, r, slip) -> the mirror's loglik_resampled value of the cell with a mistake in what a count means (the mirror has no slips
    of its own here, so the mistake is made in its input): "count_as_one": a point drawn n times keeps sigma^2 instead of sigma^2 / n;
    "dropped_kept": a point with count 0 stays in the merge with count 1.  Means and prior variances are the cell's own."""
    case, r, slip = job
    cid, kernel, (t, y, s), delays, alpha, rho, mb, N = case[:8]
    Y, counts = realisations(case)
    mean, vb = markov.resample_constants(t, Y, counts, mb)
    bad = [np.minimum(c, 1) if slip == "count_as_one" else np.maximum(c, 1) for c in counts]
    ll, info = markov.loglik_resampled(kernel, t, y, s, Y, bad, [r], delays, alpha, rho, mb, mean, vb)
    assert info[0] == 0, (cid, r, slip)
    return float(ll[0])


def rel(x, ref):
    e = abs(x - ref) / abs(ref)
    return e if e == e else np.inf


twins()      # RC.TIER and RC.K_OF hold the twins from the import on: a pool's workers look a case up by its id
