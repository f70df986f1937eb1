"""gpcc_predict_noise_markov_batch, gpcc_heldout_loglik_noise_markov_batch, gpcc_posterior_offsets_noise_markov_batch and
gpcc_loo_noise_markov_batch on the device: every quantity against the extended-precision references on the effective
error bars (tests/_markov_noise_predict_cases.py); bitwise the plain entries at kappa = 1, nu = 0 in every shipped <P, NOFF>; the
contract -- a row is a fresh handle's on effective_std; info = -3; rows that do not depend on M, the row order, the chunking and the
launch shape; the unstaged path; memory.  The worst error / bar of each group is printed."""
import numpy as np
import pytest

import _loo_highprec as LH
import _markov_cases as MC
import _markov_noise_cases as NC
import _markov_noise_predict_cases as C
import _markov_predict_cases as PC
import _predict_highprec as PH
import gpcc_amd
from gpcc_amd import fit, markov

pytestmark = pytest.mark.gpu

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
extended = pytest.mark.skipif(not PH.EXTENDED, reason=PH.SKIP_REASON)
LOO_FIELDS = ("mu", "var", "lp", "loo", "loglik", "info", "mix_lp", "mix_loo")


def _noise(obj, d, a, r, tests, mb, kappa, nu, w=None):
    """Every output of the four noise entries, in one flat list (the mixtures with weights w)."""
    out = list(obj.predict_markov_noise_batch(d, a, r, tests[0], kappa, nu, weights=w))
    out += list(obj.heldout_loglik_markov_noise_batch(d, a, r, *tests, kappa, nu, weights=w))
    if mb:
        out += list(obj.posterior_offsets_markov_noise_batch(d, a, r, kappa, nu))
    res = obj.loo_markov_noise_batch(d, a, r, kappa, nu, weights=w)
    return out + [getattr(res, f) for f in LOO_FIELDS]


def _plain(obj, d, a, r, tests, mb, w=None):
    out = list(obj.predict_markov_batch(d, a, r, tests[0], weights=w))
    out += list(obj.heldout_loglik_markov_batch(d, a, r, *tests, weights=w))
    if mb:
        out += list(obj.posterior_offsets_markov_batch(d, a, r))
    res = obj.loo_markov_batch(d, a, r, weights=w)
    return out + [getattr(res, f) for f in LOO_FIELDS]


def _eq(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---- 1. accuracy -------------------------------------------------------------------------------------------------------------------
@extended
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_accuracy_cpu_cases(oracle, kernel):
    worst = {q: PH.Worst("device noise %s %s" % (q, kernel)) for q in ("mu", "var", "held", "pmu", "pS")}
    lworst = {q: LH.Worst("device noise loo %s %s" % (q, kernel)) for q in LH.QUANTITIES}
    print("build: %s" % gpcc_amd.build_info())
    n = 0
    for pentry, lentry in zip(C.predict_cases(), C.loo_cases()):
        (cid, k, data, delays, alpha, rho, mb, tests), kappa, nu = pentry
        if k != kernel:
            continue
        n += 1
        ref = C.predict_reference(oracle, pentry)
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            mu, var, ll, info, _, _ = obj.predict_markov_noise_batch([delays], [alpha], [rho], tests[0], kappa, nu)
            held, llh, infoh, _ = obj.heldout_loglik_markov_noise_batch([delays], [alpha], [rho], *tests, kappa, nu)
            vl, vinfo = obj.loglik_markov_noise_batch([delays], [alpha], [rho], kappa, nu)
            assert info[0] == 0 and infoh[0] == 0 and vinfo[0] == 0 and ll[0] == vl[0] == llh[0], cid     # the taps do not split the chain
            got = {"mu": mu[0], "var": var[0], "held": held[0]}
            if mb:
                pmu, pS, llp, infop = obj.posterior_offsets_markov_noise_batch([delays], [alpha], [rho], kappa, nu)
                assert infop[0] == 0 and llp[0] == vl[0], cid
                got["pmu"], got["pS"] = pmu[0], pS[0]
        (lcase, lk, lnu) = lentry                                         # (the leave-one-out cases have their own light curves)
        assert lcase[1] == k and lcase[6] == mb
        with gpcc_amd.Objective(*lcase[2], KERN[k], marginalise_b=mb) as lobj:
            res = lobj.loo_markov_noise_batch(lcase[3], lcase[4], lcase[5], lk, lnu, weights=LH.WEIGHTS)
        assert (res.info == 0).all(), lcase[0]
        for q, v in got.items():
            worst[q].add(ref.ratio(q, v), cid)
        for q, r_ in C.loo_ratios(C.loo_reference(lentry), res).items():
            lworst[q].add(r_, lcase[0])
    assert n == 24
    PH.report(list(worst.values()) + list(lworst.values()))


# ---- 2. bitwise at kappa = 1, nu = 0 -------------------------------------------------------------------------------------------------
def _batch(L, M, seed):
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 45.0, (M, L - 1)))], 1)
    return delays, rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))


@pytest.mark.parametrize("noff", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_unit_noise_is_bitwise_the_plain_entries(kernel, noff):
    """<P, NOFF> = <order of the kernel, noff>: 130 rows, refused and failing ones among them (weight 0 on those, so that the mixtures are
    numbers).  Every output of each noise entry -- loglik, info and the mixtures included -- with explicit arrays and with None equals
    the plain entry's.  The held-out value is bitwise too: the rounded sigma*^2 plus JITTER on the lane is the host's sum."""
    Nl = [13, 11, 9, 8][:noff] if noff else [13, 11]
    L, M, mb = len(Nl), 130, noff > 0
    t, y, s, d0 = MC.lightcurves(Nl, seed=40 + noff, kind="ties" if L > 1 else "plain")
    tests = PC.test_points(t, d0, 50 + noff, -1)
    delays, alpha, rho = _batch(L, M, seed=noff)
    delays[0] = d0
    alpha[5, L - 1] = 0.0
    rho[70] = -1.0
    rho[99] = np.nan
    w = np.random.default_rng(3).uniform(0.1, 1.0, M)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        first = _plain(obj, delays, alpha, rho, tests, mb)
        w[(first[3] != 0) | (first[8] != 0) | (first[-3] != 0)] = 0.0       # whatever fails in one of the entries has no weight
        plain = _plain(obj, delays, alpha, rho, tests, mb, w)
        info = plain[3]
        assert list(info[[5, 70]]) == [-1, -2] and info[99] != 0 and np.count_nonzero(w) >= 120
        assert np.isfinite(plain[4]).all() and np.isfinite(plain[9]) and np.isfinite(plain[-1])            # mix_mu, mix_heldout, mix_loo
        for kappa, nu in ((None, None), (np.ones((M, L)), np.zeros((M, L))), (np.ones(L), None)):
            got = _noise(obj, delays, alpha, rho, tests, mb, kappa, nu, w)
            assert len(got) == len(plain)
            for i, (a, b) in enumerate(zip(got, plain)):
                assert _eq(a, b), (kernel, noff, i)


# ---- 3. the contract -----------------------------------------------------------------------------------------------------------------
@extended
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_rows_are_a_fresh_handles_on_effective_std(oracle, kernel):
    """Three cases per kernel, kappa = 0 on one band among them (the odd places of the list) and both b-modes: the noise entries on the
    handle against the plain entries on a fresh handle created on effective_std, each quantity within the bar of its reference
    (section 4.25's form: the bar of the value, nothing invented here)."""
    mine = [(p, l) for p, l in zip(C.predict_cases(), C.loo_cases()) if p[0][1] == kernel]
    pick = [mine[i] for i in (1, 10, 21)]
    assert any(p[1][0] == 0.0 for p, _ in pick) and {bool(p[0][6]) for p, _ in pick} == {True, False}
    for pentry, lentry in pick:
        (cid, k, (t, y, s), delays, alpha, rho, mb, tests), kappa, nu = pentry
        ref = C.predict_reference(oracle, pentry)
        with gpcc_amd.Objective(t, y, s, KERN[k], marginalise_b=mb) as obj:
            got = _noise(obj, [delays], [alpha], [rho], tests, mb, kappa, nu)
        with gpcc_amd.Objective(t, y, fit.effective_std(s, kappa, nu), KERN[k], marginalise_b=mb) as fresh:
            want = _plain(fresh, [delays], [alpha], [rho], C.mapped_tests(tests, kappa, nu), mb)
        assert got[3][0] == 0 and want[3][0] == 0, cid
        names = ["mu", "var", None, None, None, None, "held", None, None, None] + (["pmu", "pS", None, None] if mb else [])
        for q, a, b in zip(names, got, want):
            if q is not None:
                e = float(np.max(np.abs(np.asarray(a[0]) - np.asarray(b[0])) / ref.bar[q]))
                print("%s %s: against the fresh handle %.3g of the reference's bar" % (cid, q, e))
                assert e <= 1.0, (cid, q)
        (lcase, lk, lnu) = lentry
        lref = C.loo_reference(lentry)
        with gpcc_amd.Objective(*lcase[2], KERN[k], marginalise_b=mb) as obj:
            res = obj.loo_markov_noise_batch(lcase[3], lcase[4], lcase[5], lk, lnu)
        for m in range(2):
            with gpcc_amd.Objective(lcase[2][0], lcase[2][1], fit.effective_std(lcase[2][2], lk[m], lnu[m]), KERN[k], marginalise_b=mb) as fresh:
                fr = fresh.loo_markov_batch(lcase[3][m:m + 1], lcase[4][m:m + 1], lcase[5][m:m + 1])
            assert res.info[m] == 0 and fr.info[0] == 0
            for q in ("mu", "var", "lp", "loo"):
                b = lref.bar[q][m]
                e = float(np.max(np.abs(np.asarray(getattr(res, q)[m]) - np.asarray(getattr(fr, q)[0])) / b))
                assert e <= 1.0, (lcase[0], m, q, e)


# ---- 4. info = -3 ----------------------------------------------------------------------------------------------------------------------
def test_info_minus_three():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="ties")
    tests = PC.test_points(t, d0, 12, -1)
    M, L, N = 9, 2, 110
    rg = np.random.default_rng(5)
    d, a, r = np.tile(d0, (M, 1)), rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.5), np.log(30.0), M))
    kappa, nu = rg.uniform(0.5, 2.0, (M, L)), rg.uniform(0.0, 0.05, (M, L))
    a2, r2, k2, v2 = a.copy(), r.copy(), kappa.copy(), nu.copy()
    a2[1, 0], k2[1, 1] = 0.0, -1.0      # -1 before -3
    r2[2], v2[2, 0] = 0.0, -0.5         # -2 before -3
    k2[3, 0] = -1e-300                  # a negative kappa
    v2[4, 1] = np.nan                   # a NaN nu
    k2[5, 1] = np.inf                   # an infinite kappa
    v2[6, 0] = -1e-300
    want = [0, -1, -2, -3, -3, -3, -3, 0, 0]
    bad = np.array([c != 0 for c in want])
    w_pos, w_zero = np.ones(M), np.where(bad, 0.0, 1.0)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        good = _noise(obj, d, a, r, tests, True, kappa, nu, w_zero)
        assert all((x == 0).all() for x in (good[3], good[8], good[13], good[19]))
        for w in (w_pos, w_zero):
            got = _noise(obj, d, a2, r2, tests, True, k2, v2, w)
            for info in (got[3], got[8], got[13], got[19]):                  # predict, held-out, postb, leave-one-out
                assert list(info) == want
            for i in (0, 1, 2, 6, 7, 10, 11, 12, 14, 15, 16, 17, 18):         # the per-row outputs: the row NaN, the others bitwise unchanged
                assert np.isnan(np.asarray(got[i])[bad]).all(), i
                assert np.array_equal(np.asarray(got[i])[~bad], np.asarray(good[i])[~bad]), i
            mixes = (got[4], got[5], got[9], got[20], got[21])               # mix_mu, mix_var, mix_heldout, mix_lp, mix_loo
            if w is w_pos:
                assert all(np.isnan(np.asarray(x)).all() for x in mixes)     # a failed row with weight: NaN, as today
            else:
                assert all(_eq(x, g) for x, g in zip(mixes, (good[4], good[5], good[9], good[20], good[21])))      # weight 0: untouched
        hm = markov.predict_noise("matern32", t, y, s, d[3], a2[3], r2[3], tests[0], k2[3], v2[3])
        assert hm[3] == -3
        with pytest.raises(ValueError):
            obj.predict_markov_noise_batch(d, a, r, tests[0], np.ones((M, L + 1)))
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        for call in (lambda: obj.predict_markov_noise_batch(d, a, r, tests[0], kappa, nu), lambda: obj.loo_markov_noise_batch(d, a, r, kappa, nu),
                     lambda: obj.heldout_loglik_markov_noise_batch(d, a, r, *tests, kappa, nu),
                     lambda: obj.posterior_offsets_markov_noise_batch(d, a, r, kappa, nu)):
            with pytest.raises(gpcc_amd.GpccError) as ei:
                call()
            assert ei.value.code == -3 and "rbf" in ei.value.message


# ---- 5. independence -------------------------------------------------------------------------------------------------------------------
def _same(got, full, rows, M):
    for a, b in zip(got, full):
        if a is None or np.ndim(b) == 0 or np.shape(b)[0] != M:
            continue
        if not np.array_equal(np.asarray(a), np.asarray(b)[rows], equal_nan=True):
            return False
    return True


@pytest.mark.parametrize("kernel,Nl,mb", [("matern52", [30, 20, 27], True), ("OU", [60, 50], False)])
def test_rows_do_not_depend_on_the_batch(kernel, Nl, mb):
    """M = 1 / 63 / 64 / 65 / 257, permuted rows, markov_chunk_rows 7 / 64 / 100: bitwise (the per-row outputs; the mixtures run over
    other rows)."""
    t, y, s, d0 = MC.lightcurves(Nl, seed=7, kind="ties")
    L, M = len(Nl), 257
    tests = PC.test_points(t, d0, 8, -1)
    delays, alpha, rho = _batch(L, M, seed=L)
    delays[0] = d0
    rg = np.random.default_rng(L)
    kappa, nu = rg.uniform(0.0, 2.0, (M, L)), rg.uniform(0.001, 0.05, (M, L))
    kappa[200, 0] = -0.5                                                  # one row fails (-3)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        full = _noise(obj, delays, alpha, rho, tests, mb, kappa, nu)
        assert full[3][200] == -3 and (np.delete(full[3], 200) == 0).all()
        for m in (1, 63, 64, 65):
            assert _same(_noise(obj, delays[:m], alpha[:m], rho[:m], tests, mb, kappa[:m], nu[:m]), full, slice(0, m), M), m
        perm = np.random.default_rng(1).permutation(M)
        assert _same(_noise(obj, delays[perm], alpha[perm], rho[perm], tests, mb, kappa[perm], nu[perm]), full, perm, M)
        try:
            for chunk in (7, 64, 100):
                obj.set_option("markov_chunk_rows", chunk)
                assert _same(_noise(obj, delays, alpha, rho, tests, mb, kappa, nu), full, slice(None), M), chunk
        finally:
            obj.set_option("markov_chunk_rows", 0)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, precision="fp32") as o32:      # an fp32 handle, on its fp64 twin
        assert _same(_noise(o32, delays[:65], alpha[:65], rho[:65], tests, mb, kappa[:65], nu[:65]), full, slice(0, 65), M)


def test_rows_do_not_depend_on_the_launch_shape():
    """Two lanes per row: a batch whose waves number between the chip's CUs and twice that runs two waves per workgroup, a call of up
    to 64 rows one; the rows are the same bits."""
    import torch
    C_ = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = (3 * C_ // 2) // 2
    blocks -= 1 - blocks % 2
    M = 64 * (blocks - 1) + 1
    assert C_ < (M + 63) // 64 * 2 <= 2 * C_
    t, y, s, d0 = MC.lightcurves([7, 5], seed=33, kind="plain")
    tests = ([np.array([1.0, 31.0, -2.0]), np.array([12.5])], [np.array([0.1, 0.2, 0.3]), np.array([0.4])], [np.full(3, 0.2), np.full(1, 0.25)])
    rg = np.random.default_rng(M)
    delays = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 8.0, (M, 1)))], 1)
    alpha, rho = rg.uniform(0.4, 2.0, (M, 2)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))
    kappa, nu = rg.uniform(0.0, 2.0, (M, 2)), rg.uniform(0.001, 0.05, (M, 2))
    kappa[M - 1, 1] = -0.5                                                # the last row fails (-3), alone in the last workgroup
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        assert obj.get_option("markov_chunk_rows") == 0                   # (the tap scratch holds all M rows of these few points: one launch)
        full = _noise(obj, delays, alpha, rho, tests, True, kappa, nu)
        assert full[3][M - 1] == -3 and (full[3][:M - 1] == 0).all()
        for r0, n in ((0, 64), (M - 65, 64), (M - 1, 1), (128 - 32, 64)):
            sl = slice(r0, r0 + n)
            assert _same(_noise(obj, delays[sl], alpha[sl], rho[sl], tests, True, kappa[sl], nu[sl]), full, sl, M), r0


# ---- 6. the unstaged path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [6600, 110])
def test_unstaged_and_staged_against_the_mirror(N):
    """One band, Matern-5/2, three rows that differ in (kappa, nu) alone, T = 64.  N = 6600: 24 N bytes beside 56 (44) bytes a lane
    exceed the 156 KiB a workgroup may take, so the light curves come through the caches; N = 110: staged.  Against the numpy mirror
    under section 4.25's bar of that test, the value's bar with e_dense at its floor, F (N + T) 2^-53 with F of the row's effective error
    bars, relative to the size of each quantity: max(1, max|mu|) for a mean, alpha^2 + Sigma_b (the prior variance of a band's curve) for
    the latent variance, the largest variance for the leave-one-out variance, max(1, |.|) for a log-density and for a sum of them."""
    rg = np.random.default_rng(N)
    t = [np.sort(MC.snap(rg.uniform(0.0, 30.0 * N / 110, N)))]
    y = [np.sin(0.4 * t[0]) + 0.2 * rg.standard_normal(N)]
    s = [0.2 + 0.05 * rg.random(N)]
    T = 64
    tt = [MC.snap(rg.uniform(-2.0, 30.0 * N / 110 + 2.0, T))]
    tt[0][:4] = t[0][[0, 5, N // 2, N - 1]]                               # on training points
    tests = (tt, [np.sin(0.4 * tt[0]) + 0.2 * rg.standard_normal(T)], [0.2 + 0.05 * rg.random(T)])
    alpha0, rho0 = 1.3, 2.5
    kappa, nu = np.array([[0.6], [1.7], [0.0]]), np.array([[0.004], [0.03], [0.05]])
    d, a, r = np.zeros((3, 1)), np.full((3, 1), alpha0), np.full(3, rho0)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        mu, var, ll, info, _, _ = obj.predict_markov_noise_batch(d, a, r, tt, kappa, nu)
        held, _, infoh, _ = obj.heldout_loglik_markov_noise_batch(d, a, r, *tests, kappa, nu)
        pmu, pS, _, infop = obj.posterior_offsets_markov_noise_batch(d, a, r, kappa, nu)
        res = obj.loo_markov_noise_batch(d, a, r, kappa, nu)
        vl, _ = obj.loglik_markov_noise_batch(d, a, r, kappa, nu)
    assert (info == 0).all() and (infoh == 0).all() and (infop == 0).all() and (res.info == 0).all()
    assert np.array_equal(ll, vl) and np.array_equal(res.loglik, vl)
    cmax = alpha0 ** 2 + 100.0 * float(np.var(y[0], ddof=1))
    for m in range(3):
        b = MC.bar(0.0, N + T, MC.factor([alpha0], NC.effective(s, kappa[m], nu[m])))
        hmu, hvar, hll, hinfo = markov.predict_noise("matern52", t, y, s, d[m], a[m], r[m], tt, kappa[m], nu[m])
        hheld = markov.heldout_noise("matern52", t, y, s, d[m], a[m], r[m], *tests, kappa[m], nu[m])[0]
        hp = markov.posterior_offsets_noise("matern52", t, y, s, d[m], a[m], r[m], kappa[m], nu[m])
        lo = markov.loo_noise("matern52", t, y, s, d[m], a[m], r[m], kappa[m], nu[m])
        assert hinfo == 0 and lo[5] == 0
        e = {"loglik": abs(ll[m] - hll) / abs(hll),
             "mu": np.max(np.abs(mu[m] - hmu)) / max(1.0, np.max(np.abs(hmu))), "var": np.max(np.abs(var[m] - hvar)) / cmax,
             "held": abs(held[m] - hheld) / max(1.0, abs(hheld)),
             "postb mu": np.max(np.abs(pmu[m] - hp[0])) / max(1.0, np.max(np.abs(hp[0]))), "postb Sigma": np.max(np.abs(pS[m] - hp[1])) / cmax,
             "loo mu": np.max(np.abs(res.mu[m] - lo[0])) / max(1.0, np.max(np.abs(lo[0]))), "loo var": np.max(np.abs(res.var[m] - lo[1])) / np.max(lo[1]),
             "loo lp": np.max(np.abs(res.lp[m] - lo[2])) / max(1.0, np.max(np.abs(lo[2]))), "loo": abs(res.loo[m] - lo[3]) / max(1.0, abs(lo[3]))}
        print("N = %d row %d (bar %.3g): %s" % (N, m, b, ", ".join("%s %.3g" % (q, v / b) for q, v in e.items())))
        assert all(v <= b for v in e.values()), (N, m, e, b)


# ---- 7. memory -------------------------------------------------------------------------------------------------------------------------
def test_memory():
    """N = 16384, Matern-5/2, T = 2 x 512, 64 rows with their own noise model, the first calls of a handle: it grows by the plain
    entries' documented buffers (tests/test_gpu_markov_predict.py: the tap scratch, mu and var; the leave-one-out entry's taps are N
    points for T and share the scratch) plus 16 M L bytes for kappa | nu, within that test's allowance of 4 MiB, and none of the N^2
    workspace appears."""
    import torch
    from gpcc_amd import synthetic
    Nl = [8192, 8192]
    N, M, L = 16384, 64, 2
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=3)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    delays = np.stack([np.zeros(M), np.linspace(0.0, 12.6, M)], 1)
    alpha, rho = np.tile(alpha0, (M, 1)), np.full(M, rho0)
    rg = np.random.default_rng(5)
    kappa, nu = rg.uniform(0.5, 2.0, (M, L)), rg.uniform(0.0, 0.05, (M, L)) * np.array([np.mean(a ** 2) for a in s])
    hi = max(np.max(a) for a in t)
    tt = [rg.uniform(-0.02 * hi, 1.02 * hi, 512) for _ in range(2)]
    yt = [np.mean(y[l]) + np.std(y[l]) * rg.standard_normal(512) for l in range(2)]
    st = [np.full(512, float(np.mean(s[l]))) for l in range(2)]
    T, nrec = 1024, 5 + 15
    torch.cuda.synchronize()
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        free0, _ = torch.cuda.mem_get_info(0)
        mu, var, ll, info, _, _ = obj.predict_markov_noise_batch(delays, alpha, rho, tt, kappa, nu)
        held, _, infoh, _ = obj.heldout_loglik_markov_noise_batch(delays, alpha, rho, tt, yt, st, kappa, nu)
        pmu, pS, _, infop = obj.posterior_offsets_markov_noise_batch(delays, alpha, rho, kappa, nu)
        free1, _ = torch.cuda.mem_get_info(0)
        assert obj.get_option("workspace_slots") == obj.get_option("slots_per_stream")     # (never built)
        assert obj.get_option("markov_tap_bytes") == 16 * T * nrec * M
        documented = 16 * T * nrec * M + 16 * T * M + 16 * M * L
        res = obj.loo_markov_noise_batch(delays[:8], alpha[:8], rho[:8], kappa[:8], nu[:8], outputs=("loo", "loglik", "info"))
        free2, _ = torch.cuda.mem_get_info(0)
        assert obj.get_option("workspace_slots") == obj.get_option("slots_per_stream")
        chunk = min(8, (128 << 20) // (16 * N * nrec))                    # the rows of a chunk of the leave-one-out entry here
        loo_documented = max(0, 16 * N * nrec * chunk - 16 * T * nrec * M) + 24 * N * chunk + 8 * N + 8 * 8
        vl, vinfo = obj.loglik_markov_noise_batch(delays, alpha, rho, kappa, nu)
    print("N = 16384 noise-model predictions: %.2f MiB of growth (documented %.2f MiB); leave-one-out, 8 rows: %.2f MiB more (documented %.2f MiB)"
          % ((free0 - free1) / 2.0 ** 20, documented / 2.0 ** 20, (free1 - free2) / 2.0 ** 20, loo_documented / 2.0 ** 20))
    assert free0 - free1 < documented + 4 * 2 ** 20
    assert free1 - free2 < loo_documented + 4 * 2 ** 20
    assert (info == 0).all() and (infoh == 0).all() and (infop == 0).all() and (res.info == 0).all() and (vinfo == 0).all()
    assert np.array_equal(ll, vl) and np.array_equal(res.loglik, vl[:8]) and np.isfinite(held).all() and np.isfinite(res.loo).all()
    assert np.isfinite(mu).all() and (var > 0).all() and np.isfinite(pmu).all()
