"""The numpy mirror of the linear-time predictions, held-out scores, offsets' posterior and leave-one-out scores under a per-row noise
model (gpcc_amd.markov.predict_noise, heldout_noise, posterior_offsets_noise, loo_noise) against the extended-precision
references on the effective error bars, under bars measured on the reference side only (tests/_markov_noise_predict_cases.py); at
kappa = 1, nu = 0 the mirror is the plain mirror exactly; every injected slip misses a bar on most cases where it can act; the
predictors' kappa=, nu= and fit.noise_predictor.  The lines that start with "noise-predict" are kept in
profiles/markov/noise_predict_parity.log.

Which cases can catch which slip.  Every case has kappa != 1 and nu != 0 on some band, so heldout_raw_sigmatest (quantity: the held-out
value) and loo_var_raw (the leave-one-out variance and density) can act on all 72; kappa_linear (kappa sigma^2 for kappa^2 sigma^2: every
quantity) where some kappa is neither 0 nor 1, which leaves out the 12 one-band cases of the global-noise shape kappa = 0 (60);
noise_all_bands gives every band the first band's model and can act where there are two bands or more (48).  Where a slip cannot act
the test asserts that it changes no bit.

The tolerance of the comparisons of one mirror run with another on effective_std (CONTRACT_RTOL): the two differ in that the fresh data
set squares sqrt(kappa^2 sigma^2 + nu) again, 1.5 ulp of each variance at most; the filter carries a relative change of its variances
to its outputs multiplied by at most _markov_cases.factor (2 alpha^2 / sigma^2 <= 1250 on these cases) per step over N = 110 steps
(DESIGN.md 4.15): 1250 x 110 x 1.5 x 2^-53 = 2.3e-11.  1e-9 leaves room for the cancellation in a residual y - mu."""
import numpy as np
import pytest

import _loo_highprec as LH
import _markov_noise_cases as NC
import _markov_noise_predict_cases as C
import _predict_highprec as PH
from gpcc_amd import fit, markov

extended = pytest.mark.skipif(not PH.EXTENDED, reason=PH.SKIP_REASON)
PCASES = C.predict_cases()
LCASES = C.loo_cases()


def _mirror_predict(entry, slip=None, want=("mu", "held", "pmu")):
    """The mirror's quantities of one entry of predict_cases(), under _predict_highprec.Reference's names."""
    (cid, k, data, delays, alpha, rho, mb, tests), kappa, nu = entry
    got = {}
    if "mu" in want:
        got["mu"], got["var"], _, info = markov.predict_noise(k, *data, delays, alpha, rho, tests[0], kappa, nu, mb, _slip=slip)
        assert info == 0, cid
    if "held" in want:
        got["held"], _, info = markov.heldout_noise(k, *data, delays, alpha, rho, *tests, kappa, nu, mb, _slip=slip)
        assert info == 0, cid
    if "pmu" in want and mb:
        got["pmu"], got["pS"], _, info = markov.posterior_offsets_noise(k, *data, delays, alpha, rho, kappa, nu, _slip=slip)
        assert info == 0, cid
    return got


def _mirror_loo(entry, slip=None, rows=(0, 1)):
    (cid, k, data, delays, alpha, rho, mb, N), kappa, nu = entry
    out = [markov.loo_noise(k, *data, delays[m], alpha[m], rho[m], kappa[m], nu[m], mb, _slip=slip) for m in rows]
    assert all(o[5] == 0 for o in out), cid
    got = {"mu": np.stack([o[0] for o in out]), "var": np.stack([o[1] for o in out]), "lp": np.stack([o[2] for o in out]),
           "loo": np.array([o[3] for o in out])}
    if len(rows) == 2:
        got["mix_lp"], got["mix_loo"] = markov.loo_mix(got["lp"], LH.WEIGHTS)
    return got


def test_case_rules():
    assert len(PCASES) == 72 and len(LCASES) == 72
    for (case, kappa, nu) in PCASES:
        L = len(case[4])
        assert kappa.shape == (L,) and nu.shape == (L,) and np.all(kappa >= 0) and np.all(nu >= 0)
        assert np.any(kappa != 1.0) and np.any(nu != 0.0)
    assert sum(1 for (case, kappa, nu) in PCASES if kappa[0] == 0.0) == 36            # the global-noise shape: no reported bar enters
    for (case, kappa, nu) in LCASES:
        assert case[7] == 110 and kappa.shape == case[4].shape and np.all(kappa[1] == 1.3 * kappa[0]) and np.all(nu[1] > nu[0])


@extended
def test_every_reference_exists(oracle):
    """Before anything else: no case is left out, every reference is there and finite (its factorisations assert info = 0)."""
    for entry in PCASES:
        ref = C.predict_reference(oracle, entry)
        assert np.all(np.isfinite(ref.mu.astype(np.float64))) and np.all(ref.var > 0) and np.isfinite(float(ref.held)), entry[0][0]
        assert (ref.pmu is not None) == bool(entry[0][6]), entry[0][0]
    for entry in LCASES:
        ref = C.loo_reference(entry)
        assert np.all(ref.var > 0) and np.all(np.isfinite(ref.lp.astype(np.float64))) and np.isfinite(float(ref.mix_loo)), entry[0][0]


@extended
def test_mirror_meets_the_bars(oracle):
    worst = {q: PH.Worst("noise-predict mirror %s" % q) for q in ("mu", "var", "held", "pmu", "pS")}
    for entry in PCASES:
        ref, got = C.predict_reference(oracle, entry), _mirror_predict(entry)
        for q, v in got.items():
            worst[q].add(ref.ratio(q, v), entry[0][0])
    lworst = {q: LH.Worst("noise-predict mirror loo %s" % q) for q in LH.QUANTITIES}
    for entry in LCASES:
        ref, got = C.loo_reference(entry), _mirror_loo(entry)
        for q in LH.QUANTITIES:
            lworst[q].add(ref.ratio(q, got[q]), entry[0][0])
    PH.report(list(worst.values()) + list(lworst.values()))


def test_unit_noise_is_the_plain_mirror_exactly():
    for (case, _, _) in PCASES:
        cid, k, data, delays, alpha, rho, mb, tests = case
        L = len(alpha)
        for kappa, nu in ((None, None), (np.ones(L), np.zeros(L))):
            a, b = markov.predict_noise(k, *data, delays, alpha, rho, tests[0], kappa, nu, mb), markov.predict(k, *data, delays, alpha, rho, tests[0], mb)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:], cid
            assert markov.heldout_noise(k, *data, delays, alpha, rho, *tests, kappa, nu, mb) == markov.heldout(k, *data, delays, alpha, rho, *tests, mb), cid
            if mb:
                a, b = markov.posterior_offsets_noise(k, *data, delays, alpha, rho, kappa, nu), markov.posterior_offsets(k, *data, delays, alpha, rho)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:], cid
    for (case, _, _) in LCASES[::4]:
        cid, k, data, delays, alpha, rho, mb, N = case
        a, b = markov.loo_noise(k, *data, delays[0], alpha[0], rho[0], None, None, mb), markov.loo(k, *data, delays[0], alpha[0], rho[0], mb)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:], cid


@extended
@pytest.mark.parametrize("slip", C.SLIPS)
def test_slips_miss_a_bar(oracle, slip):
    """A slip is caught on a case when one of the quantities it can move misses its bar."""
    acted = caught = 0
    for pentry, lentry in zip(PCASES, LCASES):
        L, kappa = len(pentry[1]), pentry[1]
        if (slip == "noise_all_bands" and L == 1) or (slip == "kappa_linear" and np.all((kappa == 0.0) | (kappa == 1.0))):
            clean, got = _mirror_predict(pentry), _mirror_predict(pentry, slip)
            assert all(np.array_equal(clean[q], got[q]) for q in clean), pentry[0][0]
            continue
        acted += 1
        hit = False
        if slip != "loo_var_raw":
            ref = C.predict_reference(oracle, pentry)
            got = _mirror_predict(pentry, slip, want=("held",) if slip == "heldout_raw_sigmatest" else ("mu", "held", "pmu"))
            hit = any(ref.ratio(q, v) > 1.0 for q, v in got.items())
        if slip != "heldout_raw_sigmatest" and not hit:
            ref = C.loo_reference(lentry)
            got = _mirror_loo(lentry, slip, rows=(0,))
            hit = any(ref.ratio(q, got[q], rows=[0]) > 1.0 for q in ("var", "lp"))
        caught += hit
    print("noise-predict slip %s: caught on %d of the %d cases where it can act" % (slip, caught, acted))
    assert acted == {"noise_all_bands": 48, "kappa_linear": 60}.get(slip, 72) and caught > acted // 2, (slip, caught, acted)


def test_codes():
    (cid, k, data, delays, alpha, rho, mb, tests), kappa, nu = PCASES[5]
    bad_k, bad_v = kappa.copy(), nu.copy()
    bad_k[0], bad_v[-1] = -1.0, np.nan
    T, N = sum(len(a) for a in tests[0]), sum(len(a) for a in data[0])
    for kk, vv in ((bad_k, nu), (kappa, bad_v), (np.full(len(kappa), np.inf), nu)):
        mu, var, ll, info = markov.predict_noise(k, *data, delays, alpha, rho, tests[0], kk, vv, mb)
        assert info == -3 and np.isnan(mu).all() and mu.shape == (T,) and np.isnan(ll)
        assert markov.heldout_noise(k, *data, delays, alpha, rho, *tests, kk, vv, mb)[2] == -3
        lo = markov.loo_noise(k, *data, delays, alpha, rho, kk, vv, mb)
        assert lo[5] == -3 and np.isnan(lo[0]).all() and lo[0].shape == (N,)
    assert markov.predict_noise(k, *data, delays, -alpha, rho, tests[0], bad_k, nu, mb)[3] == -1          # -1 and -2 come first
    assert markov.loo_noise(k, *data, delays, alpha, -rho, bad_k, nu, mb)[5] == -2
    with pytest.raises(ValueError):
        markov.predict_noise(k, *data, delays, alpha, rho, tests[0], kappa, nu, mb, _slip="no_such_slip")


def test_predictor_arguments():
    (cid, k, (t, y, s), delays, alpha, rho, mb, tests), kappa, nu = PCASES[26]
    L = len(alpha)
    assert L == 2 and mb
    obj = markov.MarkovObjective(t, y, s, k)
    with pytest.raises(ValueError):
        fit.Predictor(obj, delays, alpha, rho, solver="dense", kappa=kappa)
    with pytest.raises(ValueError):
        fit.Predictor(obj, delays, alpha, rho, kappa=kappa, nu=nu)                     # the default solver is dense
    with pytest.raises(ValueError):
        fit.Predictor(obj, delays, alpha, rho, solver="markov", kappa=np.ones(L + 1))
    with pytest.raises(ValueError):
        fit.DelayAveragedPredictor(obj, [delays] * 3, [alpha] * 3, [rho] * 3, np.ones(3), solver="markov", nu=np.zeros((2, L)))
    pred = fit.Predictor(obj, delays, alpha, rho, solver="markov", kappa=kappa, nu=nu)
    with pytest.raises(NotImplementedError, match="effective_std"):
        pred([np.arange(3.0)] * L)
    with pytest.raises(NotImplementedError, match="effective_std"):
        pred.sample(np.arange(3.0), 2, 1)
    with pytest.raises(ValueError):
        pred.loo(solver="dense")
    assert fit.Predictor(obj, delays, alpha, rho, solver="markov").noise is None          # the defaults leave every call as it was
    plain = fit.Predictor(obj, delays, alpha, rho, solver="markov")
    unit = fit.Predictor(obj, delays, alpha, rho, solver="markov", kappa=np.ones(L))
    tt = np.linspace(-2.0, 32.0, 7)
    assert all(np.array_equal(a, b) for a, b in zip(plain(tt)[0] + plain(tt)[1], unit(tt)[0] + unit(tt)[1]))
    assert plain(*tests) == unit(*tests) and np.array_equal(plain.loo().z, unit.loo().z)
    # a row through MarkovObjective is a fresh MarkovObjective on effective_std: z standardised by the fitted variance
    fresh = fit.Predictor(markov.MarkovObjective(t, y, fit.effective_std(s, kappa, nu), k), delays, alpha, rho, solver="markov")
    a, b = pred.loo(), fresh.loo()
    assert np.allclose(a.z, b.z, rtol=1e-9, atol=1e-12) and np.allclose(a.sigma, b.sigma, rtol=1e-10) and abs(a.total - b.total) <= 1e-9 * abs(b.total)
    assert not np.allclose(a.z, plain.loo().z, rtol=1e-3)
    assert np.allclose(np.concatenate(pred(tt)[0]), np.concatenate(fresh(tt)[0]), rtol=1e-9, atol=1e-12)
    held = fresh(tests[0], tests[1], fit.effective_std(tests[2], kappa, nu))
    assert abs(pred(*tests) - held) <= 1e-9 * abs(held)
    with pytest.raises(NotImplementedError, match="effective_std"):
        fit.DelayAveragedPredictor(obj, [delays] * 2, [alpha] * 2, [rho] * 2, [1, 1], solver="markov", kappa=kappa).sample(tt, 2, 1)


def test_noise_predictor_mixes_the_rows_of_a_noise_fit(monkeypatch):
    (cid, k, (t, y, s), delays, alpha, rho, mb, tests), kappa, nu = PCASES[26]
    G, L = 3, len(alpha)
    cand = np.stack([delays, delays + [0.0, 0.25], delays + [0.0, 0.5]])
    nf = fit.NoiseGridFit(np.array([-10.0, -9.0, -11.5]), np.stack([alpha, 1.1 * alpha, 0.9 * alpha]), np.array([rho, 1.2 * rho, rho]),
                          np.stack([kappa, 1.3 * kappa, 0.8 * kappa]), np.stack([nu, nu + 0.01, 2 * nu]), 0, 0, None)
    obj = markov.MarkovObjective(t, y, s, k)
    # the default weights are getprobabilities(loglikel), which runs on the device: here its softmax in numpy stands in for it
    monkeypatch.setattr(fit, "getprobabilities", lambda ll: np.exp(ll - np.max(ll)) / np.sum(np.exp(ll - np.max(ll))))
    pred = fit.noise_predictor(obj, cand, nf)
    w = fit.getprobabilities(nf.loglikel)
    assert pred.solver == "markov" and np.array_equal(pred.weights, w) and pred.noise[0].shape == (G, L)
    assert np.array_equal(fit.noise_predictor(obj, cand, nf, weights=[1.0, 0.0, 1.0]).weights, [1.0, 0.0, 1.0])
    # against the loop it replaces: a fresh objective per row on effective_std, mixed on the host
    rows = [markov.MarkovObjective(t, y, fit.effective_std(s, nf.kappa[g], nf.nu[g]), k) for g in range(G)]
    held = [rows[g].heldout_loglik_markov_batch(cand[g], nf.alpha[g], [nf.rho[g]], tests[0], tests[1],
                                                fit.effective_std(tests[2], nf.kappa[g], nf.nu[g]))[0][0] for g in range(G)]
    mix = markov.mix_logsumexp(held, w)
    assert abs(pred.loglik(*tests) - mix) <= 1e-9 * abs(mix)
    tt = np.linspace(0.0, 30.0, 5)
    per = [rows[g].predict_markov_batch(cand[g], nf.alpha[g], [nf.rho[g]], [tt] * L) for g in range(G)]
    mu, var = markov.mix_moments(np.stack([p[0][0] for p in per]), np.stack([p[1][0] for p in per]), w)
    got = pred(tt)
    assert np.allclose(np.concatenate(got[0]), mu, rtol=1e-9, atol=1e-12)
    assert np.allclose(np.concatenate(got[1]), np.sqrt(np.maximum(var, 1e-6)), rtol=1e-9)
    lp = np.stack([rows[g].loo_markov_batch(cand[g], nf.alpha[g], [nf.rho[g]]).lp[0] for g in range(G)])
    scores = pred.loo()
    assert np.allclose(scores.lp, markov.loo_mix(lp, w)[0], rtol=1e-9, atol=1e-12) and np.isfinite(scores.z).all()
