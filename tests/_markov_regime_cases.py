"""Cases of the linear-time path's two regimes that tests/_markov_cases.py never reaches (tests/test_markov_regime_cpu.py,
tests/test_gpu_markov_regime.py): lambda x lag far below 1e-3, and 4 and 8 bands with three or more bands tied on one shifted time.

A case is _markov_cases.cpu_cases()'s tuple (id, kernel, data, delays, alpha, rho, marginalise_b, N); TIER[id] names its tier and TESTS[id]
holds the test points (ttest, ytest, sigmatest) of the N <= 120 shapes.

Light curves: _markov_cases.lightcurves(kind="ties") and then multi_ties(): with three or more bands, two shifted times are shared by
>= 3 bands (bands 0, 1, 2 -- band 1 holding that time twice -- and a second one by >= 4 bands where L >= 4), every time and delay a
multiple of 2^-10, so a tie is a tie.  alpha = default_rng(L).uniform(0.5, 2, L).

Tiers by compression, "k0", "k7", "k14", "k21": times, delays and test times multiplied by 2^-k (exact) at rho = 3, over SHAPES; k0 is the
control tier.  Tiers by rho, "rho3000", "rho30000", "rho300000": times uncompressed, [150, 120, 100] for all kernels and both b-modes,
[300, 200, 267] for the fixed subset RHO_767.  DECADE[tier] is the decade that the tier's median lambda x lag (the median over the
cases of the median over a case's merged lags) has to lie in; checked by check_tiers().

The bar of a quantity ("accuracy at small lags"): the family's existing bar, computed from the reference side as the
family's own tests compute it; outside the control tier max(existing bar, FACTOR x e_mirror), e_mirror = max |numpy mirror - extended|
over the quantity's entries, measured on the CPU and never from the device.  FACTOR = _markov_cases.FACTOR: the project's margin for
another rounding order of the same sums, the rule of _predict_highprec.py's e_second.  The control tier takes no e_mirror term."""
import numpy as np

import _grad_highprec as H
import _markov_cases as MC
import _markov_predict_cases as PC
from gpcc_amd import markov

FACTOR = MC.FACTOR
RHO0 = 3.0
KS = (0, 7, 14, 21)
SHAPES = (([60, 50], True), ([35, 30, 25, 30], True), ([20, 15, 12, 18, 14, 16, 13, 12], False), ([100, 90, 80, 98], True),
          ([50, 45, 40, 48, 44, 46, 47, 48], False))
SMALL = 120                                   # the O(N^3)-per-entry families run at N <= SMALL
RHOS = (3e3, 3e4, 3e5)
RHO_370, RHO_767 = [150, 120, 100], [300, 200, 267]
RHO_767_SUBSET = (("matern52", 3e4, True), ("matern52", 3e4, False), ("matern32", 3e4, False), ("OU", 3e4, False), ("matern52", 3e5, True),
                  ("matern32", 3e3, True))
CONTROL = "k0"
TIERS = tuple("k%d" % k for k in KS) + tuple("rho%g" % r for r in RHOS)
DECADE = {"k0": (3e-2, 3e-1), "k7": (3e-4, 3e-3), "k14": (2e-6, 2e-5), "k21": (1.5e-8, 1.5e-7),
          "rho3000": (1e-5, 1e-4), "rho30000": (1e-6, 1e-5), "rho300000": (1e-7, 1e-6)}
TIER, TESTS, K_OF = {}, {}, {}
_cases = []


def shared_times(t, delays):
    """{shifted time: {band: count}} of the shifted times that two or more bands share."""
    seen = {}
    for l, tl in enumerate(t):
        for u in np.asarray(tl) - delays[l]:
            seen.setdefault(float(u), {}).setdefault(l, 0)
            seen[float(u)][l] += 1
    return {u: b for u, b in seen.items() if len(b) >= 2}


def multi_ties(t, y, s, delays, seed):
    """Puts two shifted times of band 0 into three or more bands (in place): the first into bands 1 (twice) and 2, the second into bands 1, 2, 3 (L = 4) or every
    second band and the last (L > 4): >= 4 bands where L >= 4.  The overwritten entries keep their flux and error bar."""
    L = len(t)
    if L < 3:
        return
    rg = np.random.default_rng(seed)
    taken = shared_times(t, delays)
    free = [u for u in t[0] if float(u) not in taken and np.count_nonzero(t[0] == u) == 1]
    u1, u2 = rg.choice(free, 2, replace=False)
    groups = ((u1, [1, 1, 2]), (u2, [1, 2, 3] if L == 4 else sorted(set(range(2, L, 2)) | {L - 1}) if L > 4 else [1, 2]))
    used = {l: set() for l in range(L)}
    for u, bands in groups:
        for l in bands:
            idle = [i for i in range(len(t[l])) if i not in used[l] and float(t[l][i] - delays[l]) not in taken]
            i = int(rg.choice(idle))
            used[l].add(i)
            t[l][i] = u + delays[l]
    for a in t:
        assert np.array_equal(a, MC.snap(a))


def check_ties(t, delays):
    """The tie structure that multi_ties() promises, counted from the data."""
    L = len(t)
    if L < 3:
        return
    sh = shared_times(t, delays)
    three = [b for b in sh.values() if len(b) >= 3]
    assert len(three) >= 2, three
    assert any(max(b.values()) >= 2 for b in three), three            # one of them holds a time repeated inside a band
    if L >= 4:
        assert any(len(b) >= 4 for b in three), three


def scaled(x, k):
    return [np.asarray(a, np.float64) * 2.0 ** -k for a in x]


def _make(Nl, seed):
    t, y, s, delays = MC.lightcurves(Nl, seed=seed, kind="ties")
    multi_ties(t, y, s, delays, seed)
    check_ties(t, delays)
    return t, y, s, delays


def cases():
    """Every case, in a fixed order (built once)."""
    if _cases:
        return _cases
    for si, (Nl, mb) in enumerate(SHAPES):
        L, N = len(Nl), sum(Nl)
        t, y, s, delays = _make(Nl, 5000 + si)
        alpha = np.random.default_rng(L).uniform(0.5, 2.0, L)
        tests = PC.test_points(t, delays, 6000 + si, si % L if si % 2 == 0 and L > 1 else -1) if N <= SMALL else None
        for kernel in MC.KERNELS:
            for k in KS:
                cid = "%s-N%d-L%d-b%d-k%d" % (kernel, N, L, mb, k)
                _cases.append((cid, kernel, (scaled(t, k), y, s), delays * 2.0 ** -k, alpha, RHO0, mb, N))
                TIER[cid], K_OF[cid] = "k%d" % k, k
                if tests is not None:
                    TESTS[cid] = (scaled(tests[0], k), tests[1], tests[2])
    for Nl in (RHO_370, RHO_767):
        L, N = 3, sum(Nl)
        t, y, s, delays = _make(Nl, 5100 + N)
        alpha = np.random.default_rng(L).uniform(0.5, 2.0, L)
        for kernel in MC.KERNELS:
            for mb in (True, False):
                for rho in RHOS:
                    if N == 767 and (kernel, rho, mb) not in RHO_767_SUBSET:
                        continue
                    cid = "%s-N%d-L%d-b%d-rho%g" % (kernel, N, L, mb, rho)
                    _cases.append((cid, kernel, (t, y, s), delays, alpha, rho, mb, N))
                    TIER[cid], K_OF[cid] = "rho%g" % rho, 0
    assert len(_cases) == len(SHAPES) * 3 * len(KS) + 18 + len(RHO_767_SUBSET) and len(TIER) == len(_cases)
    return _cases


def tier(name, kernel=None, small=None):
    return [c for c in cases() if TIER[c[0]] == name and (kernel is None or c[1] == kernel) and (small is None or (c[7] <= SMALL) == small)]


def small_cases(name=None):
    return [c for c in cases() if c[7] <= SMALL and (name is None or TIER[c[0]] == name)]


def median_lambda_lag(case):
    cid, kernel, (t, y, s), delays, alpha, rho, mb, N = case
    u = np.sort(np.concatenate([np.asarray(a) - delays[l] for l, a in enumerate(t)]))
    lag = np.diff(u)
    return float(markov.rate(kernel, rho)) * float(np.median(lag[lag > 0]))


def check_tiers():
    """Every tier's median lambda x lag lies in its decade.  -> {tier: median}"""
    out = {}
    for name in TIERS:
        m = float(np.median([median_lambda_lag(c) for c in tier(name)]))
        lo, hi = DECADE[name]
        assert abs(hi / lo - 10.0) < 1e-9 and lo <= m < hi, (name, m, lo, hi)
        out[name] = m
    return out


# ---- value and gradient: the reference, the mirror's error and the bars -----------------------------------------------------------
def value_grad_job(case):
    """(extended Reference, mirror value, mirror gradient) of a case: a top-level function, for a process pool.  Asserts, from the
    reference side, info == 0."""
    cid, kernel, data, delays, alpha, rho, mb, N = case
    ref = H.evaluate(kernel, *data, delays, alpha, rho, mb)
    assert ref.info == 0, cid
    ll, g, info = markov.loglik_grad(kernel, *data, delays, alpha, rho, mb)
    assert info == 0, cid
    return ref, ll, g


class Bars:
    """The bars of one case's value (relative to |reference|) and gradient (absolute), with what went into them."""

    def __init__(self, oracle, case, job):
        cid, kernel, data, delays, alpha, rho, mb, N = case
        self.ref, self.mirror_ll, self.mirror_grad = job
        ref = self.ref
        d, info = oracle.loglik_batch(kernel, *data, delays[None, :], alpha[None, :], [rho], mb)
        assert info[0] == 0, cid
        self.e_dense = abs(float(d[0]) - ref.loglik) / abs(ref.loglik)
        self.value_existing = MC.bar(self.e_dense, N, MC.factor(alpha, data[2]))
        self.grad_existing = H.bar(ref)
        self.e_mirror_value = abs(self.mirror_ll - ref.loglik) / abs(ref.loglik)
        self.e_mirror_grad = float(np.max(np.abs(self.mirror_grad - ref.grad)))
        control = TIER[cid] == CONTROL
        self.value = self.value_existing if control else max(self.value_existing, FACTOR * self.e_mirror_value)
        self.grad = self.grad_existing if control else max(self.grad_existing, FACTOR * self.e_mirror_grad)
        self.value_active, self.grad_active = self.value > self.value_existing, self.grad > self.grad_existing

    def value_ratio(self, ll):
        return abs(ll - self.ref.loglik) / abs(self.ref.loglik) / self.value

    def grad_ratio(self, g):
        e = np.abs(np.asarray(g, np.float64) - self.ref.grad)
        return float(np.max(np.where(np.isnan(e), np.inf, e))) / self.grad


def regime_bar(existing, e_mirror, cid):
    """(bar, whether the e_mirror term is active) of any family's quantity: per entry or one number."""
    existing = np.asarray(existing, np.float64)
    if TIER[cid] == CONTROL:
        return existing, False
    b = np.maximum(existing, FACTOR * float(e_mirror))
    return b, bool(np.any(b > existing))


class Worst:
    """The worst error / bar of a group, and how many (case, quantity) pairs had the e_mirror term active."""

    def __init__(self, group):
        self.group, self.worst, self.where, self.active, self.pairs, self.control_active = group, 0.0, None, 0, 0, 0

    def add(self, ratio, where, active=False):
        self.pairs += 1
        self.active += bool(active)
        self.control_active += bool(active) and TIER[where.split(" ")[0]] == CONTROL
        if not ratio < self.worst:
            self.worst, self.where = ratio, where

    def line(self):
        return "%s: worst error / bar %.3g (%s); e_mirror term active in %d of %d pairs" % (self.group, self.worst, self.where, self.active,
                                                                                           self.pairs)


def report(groups):
    """Prints every group's line, then asserts that no control pair took the e_mirror term and that every group passes.  -> the lines"""
    groups = list(groups)
    lines = [w.line() for w in groups]
    for line in lines:
        print(line)
    assert not any(w.control_active for w in groups)
    missed = [w.line() for w in groups if not w.worst <= 1.0]
    assert not missed, missed
    return lines


# ---- the O(N^3)-per-entry families at the N <= SMALL shapes: references and the mirror's runs, for a process pool ----------------
def _oracle():
    """The CPU oracle inside a pool's worker (the test's oracle fixture has built it), on one BLAS thread: the workers' own thread
    pools only get in each other's way."""
    from _loglik_highprec import _one_blas_thread
    from oracle import oracle as o
    _one_blas_thread()
    return o


def ships_hessian(case):
    """Whether the Hessian and Fisher kernels ship the case's <P, NOFF>: everything but <3, 4> (Matern-5/2, 4 marginalised offsets)."""
    return not (case[1] == "matern52" and case[6] and len(case[4]) == 4)


def hess_job(job):
    """(what, case) -> one third of a case's Hessian work, so that a pool shares it: "ref": (the Reference with the bars of
    _markov_hess_full_cases.reference_job, the leading block's bars of _hess_highprec.reference_job); "hess" and "fisher": the mirror's
    full Hessian (whose leading block is its loglik_hess_hyper: the same passes) and Fisher matrix."""
    what, case = job
    cid, kernel, data, delays, alpha, rho, mb, N = case
    if what == "ref":
        import _hess_highprec as HH
        try:
            import torch
            torch.set_num_threads(2)
        except Exception:
            pass
        ref = HH.evaluate(kernel, *data, delays, alpha, rho, mb, keep=True)
        assert ref.info == 0, cid
        HH.add_bars(ref)
        hyper_bars = {b: v for b, v in ref.bars["H"].items() if b in ("aa", "ar", "rr")}
        HH.add_bars(ref, witness=not ref.ties)
        ref.parts = {}
        return ref, hyper_bars
    out = (markov.loglik_hess if what == "hess" else markov.loglik_fisher)(kernel, *data, delays, alpha, rho, mb)
    assert out[3] == 0, cid
    return out[2]


def hess_references(pool, cases):
    """{case id: (Reference, hyper bars, mirror Hessian, mirror Fisher)} of the cases that ship."""
    cases = [c for c in cases if ships_hessian(c)]
    jobs = [(w, c) for c in cases for w in ("ref", "hess", "fisher")]
    res = list(pool.map(hess_job, jobs))
    return {c[0]: res[3 * i] + (res[3 * i + 1], res[3 * i + 2]) for i, c in enumerate(cases)}


def predict_case(case):
    """The case in _markov_predict_cases' form: the test points in place of N."""
    return case[:7] + (TESTS[case[0]],)


def predict_job(case):
    """_predict_highprec.reference of a case: mu, var, the held-out value and postb with their bars (e_second is the mirror's error)."""
    import _predict_highprec as PH
    cid, kernel, data, delays, alpha, rho, mb, N = case
    return PH.reference(_oracle(), kernel, data, delays, alpha, rho, mb, TESTS[cid])


def loo_case(case):
    """The case in _loo_highprec's form: a second row (the later bands' delays moved by 2^-4 2^-k, alpha x 1.25, rho x 0.8)."""
    cid, kernel, data, delays, alpha, rho, mb, N = case
    d2 = delays.copy()
    d2[1:] += 2.0 ** (-4 - K_OF[cid])
    return (cid, kernel, data, np.stack([delays, d2]), np.stack([alpha, 1.25 * alpha]), np.array([rho, 0.8 * rho]), mb, N)


def loo_job(case):
    """(_loo_highprec.reference of loo_case(case), the mirror's {quantity: value})."""
    import _loo_highprec as LH
    _oracle()
    cid, k, data, delays, alpha, rho, mb, N = lc = loo_case(case)
    ref = LH.reference(lc)
    rows = [markov.loo(k, *data, delays[m], alpha[m], rho[m], mb) for m in range(2)]
    assert all(r[5] == 0 for r in rows), cid
    mir = {"mu": np.stack([r[0] for r in rows]), "var": np.stack([r[1] for r in rows]), "lp": np.stack([r[2] for r in rows]),
           "loo": np.array([r[3] for r in rows])}
    mir["mix_lp"], mir["mix_loo"] = markov.loo_mix(mir["lp"], LH.WEIGHTS)
    return ref, mir


SAMPLE_DRAWS = 3


def sample_job(args):
    """(case, seed, word) -> _sample_highprec.linear_reference of SAMPLE_DRAWS draws (e_second is the mirror's error), without the map."""
    import _sample_highprec as SH
    case, seed, word = args
    ref = SH.linear_reference(_oracle(), predict_case(case), seed, SAMPLE_DRAWS, word)
    ref.G = None
    return ref


def hess_pairs(ref, hyper_bars, case, which, got, mirror):
    """[(quantity, error, existing bar, e_mirror)] per block of one matrix: which = "hyper" (leading block, _markov_hess_cases.ratio's
    bar), "H" or "F" (all six blocks, _markov_hess_full_cases.ratios' / _markov_fisher_cases.ratios' bars).  On an OU row with a
    cross-band tie the tau entries are NaN by contract and only the (alpha, rho) blocks are compared."""
    import _hess_highprec as HH
    import _markov_hess_cases as HC
    L = ref.L
    n = L + 1 if which == "hyper" else 2 * L + 1
    want = (ref.F if which == "F" else ref.H)[:n, :n]
    bars = hyper_bars if which == "hyper" else ref.bars[which]
    out = []
    for b, m in HH.block_masks(L, n).items():
        if case[1] == "OU" and ref.ties and b in ("at", "rt", "tt"):
            continue
        e = np.abs(np.asarray(got, np.float64)[:n, :n] - want)[m]
        em = np.abs(np.asarray(mirror, np.float64)[:n, :n] - want)[m]
        e = float(np.max(np.where(np.isnan(e), np.inf, e)))
        out.append(("%s %s" % (which, b), e, bars[b] / HC.scale(case), float(np.max(em))))
    return out


def add_pair(worst, cid, quantity, err, existing, e_mirror, show=True):
    """One (case, quantity) pair into a Worst: err and existing per entry or one number each; the bar is regime_bar's.  -> error / bar"""
    err = np.asarray(err, np.float64)
    err = np.where(np.isnan(err), np.inf, err)
    b, active = regime_bar(existing, e_mirror, cid)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = float(np.max(np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))))
        r0 = float(np.max(np.where(np.asarray(existing) > 0, err / existing, np.where(err == 0, 0.0, np.inf))))
    if show:
        print("%-26s %-10s error %.3g existing bar %.3g ratio %.3g e_mirror %.3g%s"
              % (cid, quantity, float(np.max(err)), float(np.min(existing)), r0, float(e_mirror), "  (16 e_mirror active)" if active else ""))
    worst.add(r, "%s %s" % (cid, quantity), active)
    return r


def slip_table(rows, need):
    """rows: [(family, slip, case id, error / bar, bar's e_mirror term active)]; a slip is caught where its error is at least twice the
    bar of a quantity it touches.  Prints the table -- a slip that a tier's e_mirror term has swallowed is named -- and asserts that every
    family has a slip caught on every case id prefix of `need`."""
    missed = []
    for family, slip, cid, ratio, active in rows:
        caught = ratio >= 2.0
        print("%-14s slip %-20s %-32s error / bar %-9.3g %s" % (family, slip, cid, ratio, "caught" if caught else
                                                               "NOT CAUGHT" + (": swallowed by the e_mirror term" if active else "")))
    for family in sorted({r[0] for r in rows}):
        for want in need:
            if not any(r[0] == family and want in r[2] and r[3] >= 2.0 for r in rows):
                missed.append((family, want))
    assert not missed, missed


cases()          # TIER, TESTS and K_OF are filled on import: a pool's workers look a case up by its id
check_tiers()    # ... and every tier's median lambda x lag lies in its decade
