"""The linear-time entries on the device over tests/_markov_regime_cases.py: lambda x lag down to 5e-8 (times compressed by 2^-k), rho up
to 3e5, 4 and 8 bands with three or more bands tied on one shifted time.  Value and gradient of every case, and the other families at
the N <= 120 shapes, against the extended-precision references under max(the family's existing bar, 16 e_mirror) -- no e_mirror term in
the control tier (k = 0); the identities with the plain entry at L = 4 and 8.  Every call carries the case's row as the last of a batch
of 65 (a second, ragged wave): all rows info 0, and the case's row bitwise the same row sent alone.  The references and the mirror's
errors are computed in a pool of CPU processes that never touch the GPU; the worst error / bar of each group is printed with the number
of (case, quantity) pairs in which the e_mirror term was active."""
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _grad_highprec as H
import _loo_highprec as LH
import _markov_cases as MC
import _markov_hess_full_cases as FC
import _markov_regime_cases as RC
import _predict_highprec as PH
import gpcc_amd
from gpcc_amd import synthetic

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)]

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
UNSUPPORTED = -3
ROWS = 65


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


def _batch(L, M, seed, k=0):
    """M rows like the siblings' _batch, the delays on the 2^-10 grid and then scaled by 2^-k."""
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 45.0, (M, L - 1)))], 1) * 2.0 ** -k
    return delays, rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))


def rows_of(case, seed=None):
    """(delays, alpha, rho) of 65 rows, the case's own row last."""
    cid, k, data, delays, alpha, rho, mb, N = case
    L = len(alpha)
    d, a, r = _batch(L, ROWS - 1, L if seed is None else seed, RC.K_OF[cid])
    return np.concatenate([d, delays[None, :]]), np.concatenate([a, alpha[None, :]]), np.concatenate([r, [rho]])


def alone(x):
    return tuple(v[-1:] for v in x)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- value and gradient, every case ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", RC.TIERS)
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_value_and_gradient(oracle, pool, kernel, tier):
    cases = RC.tier(tier, kernel)
    assert len(cases) == (5 if tier.startswith("k") else len([s for s in RC.RHO_767_SUBSET if s[0] == kernel and "rho%g" % s[1] == tier]) + 2)
    jobs = list(pool.map(RC.value_grad_job, cases))
    wv, wg = RC.Worst("device value %s, tier %s" % (kernel, tier)), RC.Worst("device gradient %s, tier %s" % (kernel, tier))
    for case, job in zip(cases, jobs):
        cid, k, data, delays, alpha, rho, mb, N = case
        b = RC.Bars(oracle, case, job)
        d, a, r = rows_of(case)
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll, info = obj.loglik_markov_batch(d, a, r)
            gl, grad, ginfo = obj.loglik_grad_markov_batch(d, a, r)
            l1, i1 = obj.loglik_markov_batch(*alone((d, a, r)))
            g1l, g1, g1i = obj.loglik_grad_markov_batch(*alone((d, a, r)))
        assert (info == 0).all() and (ginfo == 0).all() and np.isfinite(ll).all() and np.isfinite(grad).all(), cid
        assert same(gl, ll) and l1[0] == ll[-1] and g1l[0] == ll[-1] and i1[0] == 0 and g1i[0] == 0 and same(g1[0], grad[-1]), cid
        ev, eg, gmax = abs(ll[-1] - b.ref.loglik) / abs(b.ref.loglik), float(np.max(np.abs(grad[-1] - b.ref.grad))), float(np.max(np.abs(b.ref.grad)))
        print("%-30s value: device %.3g mirror %.3g bar %.3g | gradient of max|g|: device %.3g mirror %.3g bar %.3g"
              % (cid, ev, b.e_mirror_value, b.value, eg / gmax, b.e_mirror_grad / gmax, b.grad / gmax))
        wv.add(b.value_ratio(ll[-1]), cid, b.value_active)
        wg.add(b.grad_ratio(grad[-1]), cid, b.grad_active)
    RC.report([wv, wg])


# ---- the identities with the plain entry at L = 4 and 8 ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 14])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_identities_with_the_plain_entry(kernel, k):
    """loglik_markov_resampled on the handle's own data and the noise entries at kappa = 1, nu = 0 return loglik_markov_batch's value and
    info bit for bit; loglik_markov_realisations' column of the handle's own fluxes is that value within twice the value's smallest
    bar, F N 2^-53 (api.py: "not bitwise loglik_markov_batch's", another statement order; tests/test_gpu_markov_realisations.py's
    assertion) -- whether it is bitwise is printed."""
    cases = [c for c in RC.tier("k%d" % k, kernel) if len(c[4]) in (4, 8)]
    assert len(cases) == 4
    for case in cases:
        cid, kn, (t, y, s), delays, alpha, rho, mb, N = case
        L = len(alpha)
        d, a, r = rows_of(case, seed=100 + L)
        Y = np.concatenate(synthetic.flux_randomise(y, s, 3, seed=1), axis=1)
        Y[0] = np.concatenate(y)
        with gpcc_amd.Objective(t, y, s, KERN[kn], marginalise_b=mb) as obj:
            ll, info = obj.loglik_markov_batch(d, a, r)
            multi, minfo = obj.loglik_markov_realisations(Y, d, a, r, center="handle")
            res, rinfo = obj.loglik_markov_resampled(Y, d, a, r, np.zeros(ROWS, np.int32), center="handle", sigma_b="handle")
            noise = [obj.loglik_markov_noise_batch(d, a, r), obj.loglik_markov_noise_batch(d, a, r, np.ones((ROWS, L)), np.zeros((ROWS, L)))]
            nl, ng, ninfo = obj.loglik_grad_markov_noise_batch(d, a, r)
            m1, _ = obj.loglik_markov_realisations(Y, *alone((d, a, r)), center="handle")
        assert (info == 0).all() and np.isfinite(ll).all(), cid
        assert same(res, ll) and same(rinfo, info), cid
        for vl, vinfo in noise + [(nl, ninfo)]:
            assert same(vl, ll) and same(vinfo, info), cid
        assert np.isfinite(ng).all() and ng.shape == (ROWS, 4 * L + 1)
        assert same(minfo, info) and multi.shape == (ROWS, 3) and np.isfinite(multi).all() and same(m1[0], multi[-1]), cid
        tol = 2 * np.array([MC.bar(0.0, N, MC.factor(a[m], s)) for m in range(ROWS)])
        rel = np.abs(multi[:, 0] - ll) / np.abs(ll)
        print("%-26s realisation 0 against the plain value: worst %.3g of 2 F N 2^-53, %d of %d rows bitwise"
              % (cid, float(np.max(rel / tol)), int(np.sum(multi[:, 0] == ll)), ROWS))
        assert (rel <= tol).all(), cid


# ---- the other families at the N <= 120 shapes, every compression tier ------------------------------------------------------------
SMALL_TIERS = RC.TIERS[:4]


@pytest.mark.parametrize("tier", SMALL_TIERS)
def test_hessians_and_fisher(pool, tier):
    """loglik_hess_hyper_markov_batch, loglik_hess_markov_batch and loglik_fisher_markov_batch per block; <3, 4> is refused by all three;
    OU rows with a cross-band tie (the case's own row always, with three and more bands tied): NaN in the tau entries and only there."""
    cases = RC.small_cases(tier)
    refs = RC.hess_references(pool, cases)
    assert len(cases) == 9 and len(refs) == 8
    worst = {w: RC.Worst("device %s, tier %s" % (n, tier)) for w, n in (("hyper", "Hessian block"), ("H", "full Hessian"), ("F", "Fisher"))}
    for case in cases:
        cid, k, data, delays, alpha, rho, mb, N = case
        L = len(alpha)
        d, a, r = rows_of(case, seed=200 + L)
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            entries = (obj.loglik_hess_hyper_markov_batch, obj.loglik_hess_markov_batch, obj.loglik_fisher_markov_batch)
            if not RC.ships_hessian(case):
                for entry in entries:
                    with pytest.raises(gpcc_amd.GpccError) as ei:
                        entry(d, a, r)
                    assert ei.value.code == UNSUPPORTED, cid
                continue
            gl, gg, ginfo = obj.loglik_grad_markov_batch(d, a, r)
            out = [entry(d, a, r) for entry in entries]
            one = [entry(*alone((d, a, r))) for entry in entries]
        ref, hyper_bars, mh, mf = refs[cid]
        tau = FC.tau_mask(L)
        tied = FC.tie_rows(data[0], d) if k == "OU" else np.zeros(ROWS, bool)
        assert ref.ties and (ginfo == 0).all() and (tied[-1] or k != "OU"), cid
        for (ll, grad, mat, info), (l1, g1, m1, i1), full in zip(out, one, (False, True, True)):
            assert same(ll, gl) and same(grad, gg) and same(info, ginfo), cid                      # bitwise the gradient entry's
            assert same(m1[0], mat[-1]) and l1[0] == ll[-1] and same(g1[0], grad[-1]) and i1[0] == 0, cid
            assert same(mat, np.swapaxes(mat, 1, 2)), cid
            if full:
                assert np.array_equal(np.isnan(mat), tied[:, None, None] & tau[None, :, :]), cid
            else:
                assert np.isfinite(mat).all() and same(mat, out[1][2][:, :L + 1, :L + 1]), cid
        for which, got, mirror in (("hyper", out[0][2][-1], mh[:L + 1, :L + 1]), ("H", out[1][2][-1], mh), ("F", out[2][2][-1], mf)):
            for q, e, existing, em in RC.hess_pairs(ref, hyper_bars, case, which, got, mirror):
                RC.add_pair(worst[which], cid, q, e, existing, em)
    RC.report(worst.values())


@pytest.mark.parametrize("tier", SMALL_TIERS)
def test_predict_heldout_and_postb(oracle, pool, tier):
    """predict_markov_batch, heldout_loglik_markov_batch and posterior_offsets_markov_batch (marginalised b) under _predict_highprec's
    bars, which hold the mirror's error already (e_second)."""
    cases = RC.small_cases(tier)
    refs = list(pool.map(RC.predict_job, cases))
    worst = {w: RC.Worst("device %s, tier %s" % (w, tier)) for w in ("predict", "held-out", "postb")}
    group = {"mu": "predict", "var": "predict", "held": "held-out", "pmu": "postb", "pS": "postb"}
    for case, ref in zip(cases, refs):
        cid, k, data, delays, alpha, rho, mb, N = case
        tests = RC.TESTS[cid]
        d, a, r = rows_of(case, seed=300 + len(alpha))
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            vl, vinfo = obj.loglik_markov_batch(d, a, r)
            mu, var, pl, pinfo, _, _ = obj.predict_markov_batch(d, a, r, tests[0])
            held, hl, hinfo, _ = obj.heldout_loglik_markov_batch(d, a, r, *tests)
            mu1, var1, _, _, _, _ = obj.predict_markov_batch(*alone((d, a, r)), tests[0])
            held1 = obj.heldout_loglik_markov_batch(*alone((d, a, r)), *tests)[0]
            got = {"mu": mu[-1], "var": var[-1], "held": held[-1]}
            assert (vinfo == 0).all() and same(pinfo, vinfo) and same(hinfo, vinfo) and same(pl, vl) and same(hl, vl), cid
            assert same(mu1[0], mu[-1]) and same(var1[0], var[-1]) and held1[0] == held[-1], cid
            assert np.isfinite(mu).all() and np.isfinite(var).all() and np.isfinite(held).all(), cid
            if mb:
                pmu, pS, bl, binfo = obj.posterior_offsets_markov_batch(d, a, r)
                p1 = obj.posterior_offsets_markov_batch(*alone((d, a, r)))
                assert same(binfo, vinfo) and same(bl, vl) and same(p1[0][0], pmu[-1]) and same(p1[1][0], pS[-1]), cid
                got["pmu"], got["pS"] = pmu[-1], pS[-1]
        assert set(got) == set(ref.bar) and ref.second == "mirror", cid
        for q, value in got.items():
            RC.add_pair(worst[group[q]], cid, q, PH.err(value, getattr(ref, q)), ref.bar[q], ref.e_second[q])
    RC.report(worst.values())


@pytest.mark.parametrize("tier", SMALL_TIERS)
def test_leave_one_out(pool, tier):
    """loo_markov_batch: the case's row and its second row (weights 0.75, 0.25) behind 63 rows of weight 0, under _loo_highprec's bar
    times the filter's factor; the two rows sent alone give the same bits, the mixture included."""
    cases = RC.small_cases(tier)
    refs = list(pool.map(RC.loo_job, cases))
    worst = RC.Worst("device leave-one-out, tier %s" % tier)
    for case, (ref, mir) in zip(cases, refs):
        cid, k, data, delays, alpha, rho, mb, N = RC.loo_case(case)
        L = alpha.shape[1]
        d, a, r = _batch(L, ROWS - 2, 400 + L, RC.K_OF[cid])
        d, a, r = np.concatenate([d, delays]), np.concatenate([a, alpha]), np.concatenate([r, rho])
        w = np.concatenate([np.zeros(ROWS - 2), LH.WEIGHTS])
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            vl, vinfo = obj.loglik_markov_batch(d, a, r)
            res = obj.loo_markov_batch(d, a, r, weights=w)
            two = obj.loo_markov_batch(d[-2:], a[-2:], r[-2:], weights=LH.WEIGHTS)
        assert (vinfo == 0).all() and same(res.info, vinfo) and same(res.loglik, vl), cid
        got = {"mu": res.mu[-2:], "var": res.var[-2:], "lp": res.lp[-2:], "loo": res.loo[-2:], "mix_lp": res.mix_lp, "mix_loo": res.mix_loo}
        alone2 = {"mu": two.mu, "var": two.var, "lp": two.lp, "loo": two.loo, "mix_lp": two.mix_lp, "mix_loo": two.mix_loo}
        for q in LH.QUANTITIES:
            assert same(np.asarray(got[q]), np.asarray(alone2[q])), (cid, q)
            RC.add_pair(worst, cid, "loo " + q, PH.err(got[q], getattr(ref, q)), ref.bar[q] * ref.scale,
                        float(np.max(PH.err(mir[q], getattr(ref, q)))))
    RC.report([worst])


@pytest.mark.parametrize("tier", SMALL_TIERS)
def test_draws(oracle, pool, tier):
    """sample_markov_batch, 3 draws of every row: the case's row is row 64, so its normals are those of (seed, row 64) -- the reference is
    built for that row, and a row sent alone (row 0, other normals) is another draw.  loglik and info are the value entry's."""
    cases = RC.small_cases(tier)
    refs = list(pool.map(RC.sample_job, [(c, 700 + i, ROWS - 1) for i, c in enumerate(cases)]))
    worst = RC.Worst("device draws, tier %s" % tier)
    S = RC.SAMPLE_DRAWS
    for i, (case, ref) in enumerate(zip(cases, refs)):
        cid, k, data, delays, alpha, rho, mb, N = case
        tests = RC.TESTS[cid]
        d, a, r = rows_of(case, seed=500 + len(alpha))
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            vl, vinfo = obj.loglik_markov_batch(d, a, r)
            draws, rows, ll, info = obj.sample_markov_batch(d, a, r, tests[0], S, 700 + i, sigmatest=tests[2])
        assert (vinfo == 0).all() and same(info, vinfo) and same(ll, vl) and np.isfinite(draws).all(), cid
        assert draws.shape == (ROWS * S, sum(len(x) for x in tests[0])) and same(rows, np.repeat(np.arange(ROWS), S)), cid
        assert ref.second == "mirror"
        RC.add_pair(worst, cid, "draws", PH.err(draws[-S:], ref.draws), ref.bar, ref.e_second)
    RC.report([worst])
