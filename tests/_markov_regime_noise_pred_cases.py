"""The noise-model predictions, held-out scores, offsets' posterior, leave-one-out scores and draws, and the gradient of rows with their
own resampled data set, over tests/_markov_regime_cases.py (RC) and tests/_markov_regime_noise_cases.py (RN), whose cases, order, seeds,
noise models, batches and realisations stay as they are (tests/test_markov_regime_noise_pred_cpu.py,
tests/test_gpu_markov_regime_noise_pred.py): lambda x lag down to 5e-8, 4 and 8 bands (fixed offsets at 8) with three or more bands tied
on one shifted time, rho up to 3e5 for the gradient.

References and bars are the families' own, from the reference side and computed in a pool of CPU processes:
  predictions, held-out, postb   _predict_highprec.reference on the effective error bars sqrt(kappa^2 sigma^2 + nu) with the test error
                                 bars mapped by their band's (kappa, nu) (_markov_noise_predict_cases.predict_reference's rule) at the
                                 test points RC.TESTS[cid]; bar ref.bar[q].
  leave-one-out                  RC.loo_case(case), row one under the case's (kappa, nu), row two under 1.3 kappa and nu + 0.01
                                 (_markov_noise_predict_cases.loo_cases' rule); _markov_noise_predict_cases.loo_reference, whose bars are
                                 the linear-time ones already (no ref.scale).
  draws                          _markov_noise_sample_cases.reference of RC.SAMPLE_DRAWS draws under the row word ROWS - 1 (the case's
                                 row is the last of 65); sigmatest as given on the even-numbered cases of a tier's list and None (the
                                 latent curve) on the odd ones; bar ref.bar.
  resampled gradient             _grad_highprec.evaluate on RN.reduced_case(case, r), all 2L + 1 entries (OU's tau entries on tied cases
                                 included: the mean of the two tie orders); bar _grad_highprec.bar(ref).
RC's rule on top: outside the control tier max(existing bar, FACTOR x e_mirror), e_mirror = |numpy mirror - extended| of
markov.predict_noise, heldout_noise, posterior_offsets_noise, loo_noise with loo_mix, sample_noise, and loglik_grad_resampled with
resample_constants' means and variances -- measured on the CPU and never from the device.

Slips.  The mirror's own (_markov_noise_predict_cases.SLIPS, _markov_noise_sample_cases.SLIPS, loglik_grad_resampled's
"lag_from_merged" and "handle_sigma_b") and one made in the input, as RN.resample_slip_job does: "tie_swap" -- on every point whose
shifted time is shared by three or more bands, band l takes the noise model of band (l + 1) mod L, everything else stays, and the PLAIN
mirror runs on those error bars: what a kernel computes that takes a point's band from its merged position inside a tie."""
import numpy as np

import _grad_highprec as H
import _loo_highprec as LH
import _markov_noise_cases as NC
import _markov_noise_predict_cases as NP
import _markov_noise_sample_cases as NS
import _markov_regime_cases as RC
import _markov_regime_noise_cases as RN
import _predict_highprec as PH
from gpcc_amd import markov

ROWS = RN.ROWS
S = RC.SAMPLE_DRAWS
GROUP = {"mu": "predict", "var": "predict", "held": "held-out", "pmu": "postb", "pS": "postb"}
SAMPLE_SEED = 800
PREDICT_SLIPS = ("kappa_linear", "noise_all_bands", "heldout_raw_sigmatest", "tie_swap")
_cache = {}


def small(tier):
    """The nine N <= 120 noise cases of a k tier, in RC.cases()' order."""
    return RN.cases(tier, small=True)


# ---- predictions, held-out scores, postb ------------------------------------------------------------------------------------------------
def mirror_predict(case, slip=None, want=("mu", "held", "pmu")):
    """The noise mirror's quantities of a noise case at RC.TESTS, under _predict_highprec.Reference's names; info == 0 asserted."""
    cid, kernel, data, delays, alpha, rho, mb, N, kappa, nu = case
    tests = RC.TESTS[cid]
    got = {}
    if "mu" in want:
        got["mu"], got["var"], _, info = markov.predict_noise(kernel, *data, delays, alpha, rho, tests[0], kappa, nu, mb, _slip=slip)
        assert info == 0, (cid, slip)
    if "held" in want:
        got["held"], _, info = markov.heldout_noise(kernel, *data, delays, alpha, rho, *tests, kappa, nu, mb, _slip=slip)
        assert info == 0, (cid, slip)
    if "pmu" in want and mb:
        got["pmu"], got["pS"], _, info = markov.posterior_offsets_noise(kernel, *data, delays, alpha, rho, kappa, nu, _slip=slip)
        assert info == 0, (cid, slip)
    return got


def predict_reference(oracle, case):
    """The _predict_highprec.Reference of a noise case on its effective error bars (cached under a key of its own)."""
    cid, kernel, (t, y, s), delays, alpha, rho, mb, N, kappa, nu = case
    key = ("regime-noise-predict", cid)
    if key not in _cache:
        _cache[key] = PH.reference(oracle, kernel, (t, y, NC.effective(s, kappa, nu)), delays, alpha, rho, mb,
                                   NP.mapped_tests(RC.TESTS[cid], kappa, nu))
    return _cache[key]


def e_mirror(ref, got):
    """{quantity: max |mirror - reference|} of the quantities in got."""
    return {q: float(np.max(PH.err(v, getattr(ref, q)))) for q, v in got.items()}


def predict_job(case):
    """noise case -> (Reference, the noise mirror's {quantity: value}): a top-level function, for a process pool."""
    ref = predict_reference(RC._oracle(), case)
    got = mirror_predict(case)
    assert set(got) == set(ref.bar), case[0]
    return ref, got


def tie_points(case):
    """Per band the mask of the points whose shifted time is shared by three or more bands."""
    t, delays = case[2][0], case[3]
    three = {u for u, b in RC.shared_times(t, delays).items() if len(b) >= 3}
    return [np.array([float(u) in three for u in np.asarray(t[l]) - delays[l]]) for l in range(len(t))]


def tie_swap_errorbars(case):
    """The effective error bars with the tie-swap slip: on the points of tie_points() band l under band (l + 1) mod L's (kappa, nu)."""
    s, kappa, nu = case[2][2], case[8], case[9]
    L = len(s)
    good = NC.effective(s, kappa, nu)
    bad = NC.effective(s, np.roll(kappa, -1), np.roll(nu, -1))
    assert all(np.roll(kappa, -1)[l] == kappa[(l + 1) % L] for l in range(L))
    return [np.where(m, b, g) for m, g, b in zip(tie_points(case), good, bad)]


def predict_slip_job(job):
    """(noise case, slip of PREDICT_SLIPS) -> {quantity the slip touches: the mirror's value with the slip}."""
    case, slip = job
    cid, kernel, (t, y, s), delays, alpha, rho, mb, N, kappa, nu = case
    if slip == "tie_swap":
        eff = tie_swap_errorbars(case)
        tests = NP.mapped_tests(RC.TESTS[cid], kappa, nu)
        mu, var, _, info = markov.predict(kernel, t, y, eff, delays, alpha, rho, tests[0], mb)
        held, _, hinfo = markov.heldout(kernel, t, y, eff, delays, alpha, rho, *tests, mb)
        assert info == 0 and hinfo == 0, cid
        return {"mu": mu, "var": var, "held": held}
    return mirror_predict(case, slip, want=("held",) if slip == "heldout_raw_sigmatest" else ("mu", "held", "pmu"))


# ---- leave-one-out ------------------------------------------------------------------------------------------------------------------------
def loo_entry(case):
    """(RC.loo_case of a noise case, kappa[2, L], nu[2, L]): an entry of _markov_noise_predict_cases.loo_cases()' form."""
    kappa, nu = case[8], case[9]
    return RC.loo_case(case[:8]), np.stack([kappa, 1.3 * kappa]), np.stack([nu, nu + 0.01])


def mirror_loo(entry, slip=None):
    (cid, k, data, delays, alpha, rho, mb, N), kappa, nu = entry
    rows = [markov.loo_noise(k, *data, delays[m], alpha[m], rho[m], kappa[m], nu[m], mb, _slip=slip) for m in range(2)]
    assert all(r[5] == 0 for r in rows), (cid, slip)
    mir = {"mu": np.stack([r[0] for r in rows]), "var": np.stack([r[1] for r in rows]), "lp": np.stack([r[2] for r in rows]),
           "loo": np.array([r[3] for r in rows])}
    mir["mix_lp"], mir["mix_loo"] = markov.loo_mix(mir["lp"], LH.WEIGHTS)
    return mir


def loo_job(case):
    """noise case -> (_markov_noise_predict_cases.loo_reference of loo_entry(case), the noise mirror's {quantity: value})."""
    RC._oracle()
    entry = loo_entry(case)
    return NP.loo_reference(entry), mirror_loo(entry)


def loo_slip_job(job):
    case, slip = job
    return mirror_loo(loo_entry(case), slip)


# ---- draws --------------------------------------------------------------------------------------------------------------------------------
def sample_entry(case, idx):
    """The entry of _markov_noise_sample_cases' form of the idx-th case of a tier's list: sigmatest given on the even-numbered ones."""
    cid, kernel, data, delays, alpha, rho, mb, N, kappa, nu = case
    tt, yt, st = RC.TESTS[cid]
    return (cid, kernel, data, delays, alpha, rho, mb, (tt, yt, st if idx % 2 == 0 else None)), kappa, nu


def mirror_draws(entry, seed, slip=None):
    (cid, k, data, delays, alpha, rho, mb, tests), kappa, nu = entry
    out = [markov.sample_noise(k, *data, delays, alpha, rho, tests[0], kappa, nu, tests[2], mb, seed=seed, s=s, m=ROWS - 1, _slip=slip)
           for s in range(S)]
    assert all(o[2] == 0 for o in out), (cid, slip)
    return np.stack([o[0] for o in out])


def sample_job(job):
    """(noise case, its index in the tier's list) -> (_sample_highprec.Reference of S draws of row word ROWS - 1 without the map,
    the noise mirror's draws); the seed is SAMPLE_SEED + idx."""
    case, idx = job
    entry = sample_entry(case, idx)
    ref = NS.reference(RC._oracle(), entry, SAMPLE_SEED + idx, S, word=ROWS - 1)
    ref.G = ref.parts = None
    return ref, mirror_draws(entry, SAMPLE_SEED + idx)


def sample_slip_job(job):
    case, idx, slip = job
    return mirror_draws(sample_entry(case, idx), SAMPLE_SEED + idx, slip)


# ---- the gradient of rows with their own resampled data set ---------------------------------------------------------------------------
def mirror_regrad(case, r, slip=None):
    """(value, gradient[2L + 1]) of the mirror's loglik_grad_resampled on cell r with resample_constants' means and variances."""
    cid, kernel, (t, y, s), delays, alpha, rho, mb, N = case[:8]
    Y, counts = RN.realisations(case)
    mean, vb = markov.resample_constants(t, Y, counts, mb)
    ll, g, info = markov.loglik_grad_resampled(kernel, t, y, s, Y, counts, [r], delays, alpha, rho, mb, mean, vb, _slip=slip)
    assert info[0] == 0, (cid, r, slip)
    return float(ll[0]), g[0]


def regrad_job(job):
    """(case, r) -> (the extended Reference of the reduced fresh data set, the mirror's value, the mirror's gradient)."""
    case, r = job
    _, kernel, data, delays, alpha, rho, mb, _ = RN.reduced_case(case, r)
    ref = H.evaluate(kernel, *data, delays, alpha, rho, mb)
    assert ref.info == 0, (case[0], r)
    return (ref,) + mirror_regrad(case, r)


def regrad_references(pool, cases):
    """{(case id, r): regrad_job's} of the checked cells (RN.cells) of the cases."""
    jobs = [(c, r) for c in cases for r in RN.cells(c)]
    return {(c[0], r): v for (c, r), v in zip(jobs, pool.map(regrad_job, jobs))}


def regrad_slip_job(job):
    case, r, slip = job
    return mirror_regrad(case, r, slip)[1]


def grad_error(g, ref):
    e = np.abs(np.asarray(g, np.float64) - ref.grad)
    return float(np.max(np.where(np.isnan(e), np.inf, e)))
