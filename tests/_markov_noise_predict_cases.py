"""Cases, references and bars of the tests of the linear-time predictions, held-out scores, offsets' posterior and leave-one-out scores
under a per-row noise model v_i = kappa_l^2 sigma_i^2 + nu_l (tests/test_markov_noise_predict_cpu.py,
tests/test_gpu_markov_noise_predict.py).

Cases.  Predictions, held-out and postb: _markov_predict_cases.cpu_cases(), unchanged (72, N = 110), each with the noise model
_markov_noise_cases.noise_of() draws for the case of _markov_cases.cpu_cases() at the same place of the same product (N = 110 comes first
there, so the two lists run side by side: same kernel, bands, b-mode, rho and shape of delays).  Leave-one-out: _loo_highprec.cases() at
N = 110 (72, two rows each); the first row has noise_of(case), the second its kappa x 1.3 and nu + 0.01, so that the mixture mixes two
noise models.

References, in extended precision and from the reference side only.  The feature's contract is that a row's outputs are those of a
fresh data set with the error bars effective = sqrt(kappa^2 sigma^2 + nu), the test error bars of a held-out score mapped by the same
band's (kappa, nu).  So:
  predictions, held-out, postb   _predict_highprec.reference on (t, y, effective) with sigma* mapped: its values and its bars, those of
                                 tests/test_gpu_predict_highprec.py (its second fp64 evaluation is the PLAIN mirror on the effective
                                 error bars, not the code under test).
  leave-one-out                  per row from _predict_highprec.model on that row's effective error bars, _loo_highprec.row_values (the
                                 definition in longdouble, and in float64 on the 16-blocked Cholesky), brute_row (delete the point and
                                 condition on the rest) and mix_values; bar(q) = _loo_highprec's formula, 16 max(e_formula, e_brute,
                                 N 2^-53 terms(q)), times _markov_cases.factor(alpha, effective) / 16, the filter's conditioning -- of
                                 the row for mu, var, lp and loo, the larger of the two rows' for mix_lp and mix_loo.
Nothing in a bar comes from the noise mirror or from the device.  Every reference exists (info = 0: the factorisations assert it)."""
import numpy as np

import _loo_highprec as LH
import _markov_cases as MC
import _markov_noise_cases as NC
import _markov_predict_cases as PC
import _predict_highprec as PH

SLIPS = ("heldout_raw_sigmatest", "loo_var_raw", "kappa_linear", "noise_all_bands")
_cache = {}


def noise_id(cid):
    """The id of the case of _markov_cases.cpu_cases() (N = 110) that stands where a case of _markov_predict_cases.cpu_cases() stands."""
    return cid.replace("-L", "-N110-L", 1)


def predict_cases():
    """[(case of _markov_predict_cases.cpu_cases(), kappa[L], nu[L])], 72."""
    return [(c,) + NC.noise_of(noise_id(c[0])) for c in PC.cpu_cases()]


def mapped_tests(tests, kappa, nu):
    """(ttest, ytest, sigmatest) with the test error bars mapped by their band's (kappa, nu)."""
    return tests[0], tests[1], NC.effective(tests[2], kappa, nu)


def predict_reference(oracle, entry):
    """The _predict_highprec.Reference of one entry of predict_cases() on its effective error bars (cached)."""
    case, kappa, nu = entry
    cid, kernel, (t, y, s), delays, alpha, rho, mb, tests = case
    if cid not in _cache:
        _cache[cid] = PH.reference(oracle, kernel, (t, y, NC.effective(s, kappa, nu)), delays, alpha, rho, mb, mapped_tests(tests, kappa, nu))
    return _cache[cid]


def loo_cases():
    """[(case of _loo_highprec.cases() at N = 110, kappa[2, L], nu[2, L])], 72."""
    out = []
    for c in LH.cases():
        if c[7] != 110:
            continue
        kappa, nu = NC.noise_of(c[0])
        out.append((c, np.stack([kappa, 1.3 * kappa]), np.stack([nu, nu + 0.01])))
    return out


def loo_reference(entry):
    """The _loo_highprec.Reference of one entry of loo_cases(), each row on its own effective error bars (cached).  Its bars are the
    linear-time ones already (the factor is in them, per row), so ratio() is called without markov=True."""
    case, kappa, nu = entry
    cid, kernel, (t, y, s), delays, alpha, rho, mb, N = case
    if ("loo", cid) in _cache:
        return _cache[("loo", cid)]
    L, R = len(t), len(rho)
    eff = [NC.effective(s, kappa[m], nu[m]) for m in range(R)]
    models = [PH.model(kernel, t, y, eff[m], delays[m], alpha[m], rho[m], [np.zeros(0)] * L, mb) for m in range(R)]
    ext = [LH.row_values(m) for m in models]
    f64 = [LH.row_values(m, np.float64, LH.BLOCKED_NB) for m in models]
    tflat = np.concatenate([np.asarray(a, np.float64) for a in t])
    pts = LH._brute_points(tflat - delays[0][models[0].band])
    full = [LH.brute_row(m, np.arange(N)) for m in models]
    bru = [tuple(v[pts] for v in f) for f in full]

    def stack(rows, k):
        return np.stack([r_[k] for r_ in rows])

    ref = LH.Reference(bar={}, e_formula={}, e_brute={}, pts=pts, scale=1.0)
    ref.mu, ref.var, ref.lp = stack(ext, 0), stack(ext, 1), stack(ext, 2)
    ref.loo = ref.lp.sum(axis=1)
    ref.mix_lp = LH.mix_values(ref.lp, LH.WEIGHTS)
    ref.mix_loo = ref.mix_lp.sum()
    tmu, tlp = stack(ext, 3), stack(ext, 4)
    terms = {"mu": tmu, "var": ref.var.astype(np.float64), "lp": tlp, "loo": tlp.sum(axis=1), "mix_lp": tlp.max(axis=0),
             "mix_loo": float(tlp.max(axis=0).sum())}
    fm, fv, fl = stack(f64, 0), stack(f64, 1), stack(f64, 2)
    fmix = LH.mix_values(fl, LH.WEIGHTS)
    formula = {"mu": fm, "var": fv, "lp": fl, "loo": fl.sum(axis=1), "mix_lp": fmix, "mix_loo": fmix.sum()}
    bm, bv, bl = stack(bru, 0), stack(bru, 1), stack(bru, 2)
    bmix = LH.mix_values(bl, LH.WEIGHTS)
    bl_all = stack(full, 2)
    bmix_all = LH.mix_values(bl_all, LH.WEIGHTS)
    e_brute = {"mu": np.max(PH.err(bm, ref.mu[:, pts])), "var": np.max(PH.err(bv, ref.var[:, pts])),
               "lp": np.max(PH.err(bl, ref.lp[:, pts])), "loo": np.max(PH.err(bl_all.sum(axis=1), ref.loo)),
               "mix_lp": np.max(PH.err(bmix, ref.mix_lp[pts])), "mix_loo": float(PH.err(bmix_all.sum(), ref.mix_loo))}
    rowf = np.array([MC.factor(alpha[m], eff[m]) / LH.FACTOR for m in range(R)])      # the filter's conditioning, per row
    scale = {"mu": rowf[:, None], "var": rowf[:, None], "lp": rowf[:, None], "loo": rowf, "mix_lp": rowf.max(), "mix_loo": rowf.max()}
    for q in LH.QUANTITIES:
        ref.e_formula[q] = float(np.max(PH.err(formula[q], getattr(ref, q))))
        ref.e_brute[q] = float(e_brute[q])
        ref.bar[q] = scale[q] * LH.FACTOR * np.maximum(max(ref.e_formula[q], ref.e_brute[q]), N * LH.U53 * np.asarray(terms[q], np.float64))
    _cache[("loo", cid)] = ref
    return ref


def loo_ratios(ref, res):
    """{quantity: error / bar} of a LooResult (or the mirror's) holding both rows of a case and its mixture."""
    return {q: ref.ratio(q, getattr(res, q)) for q in LH.QUANTITIES}
