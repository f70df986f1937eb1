"""Cases, references and bars of the tests of the linear-time joint posterior draws under a per-row noise model v_i = kappa_l^2 sigma_i^2
+ nu_l (tests/test_markov_noise_sample_cpu.py, tests/test_gpu_markov_noise_sample.py).

Cases.  The 72 entries of _markov_noise_predict_cases.predict_cases() (N = 110), each with its noise model; sigmatest as given on the
even-numbered ones and None (the latent curve) on the odd ones, as _sample_highprec.cases() has it.

Reference, in extended precision and from the reference side only.  The feature's contract is that a row's draws are, with the same
seed, those of a fresh data set with the error bars effective = sqrt(kappa^2 sigma^2 + nu), the test error bars mapped by the same
band's (kappa, nu) and None left None (the latent curve takes no nu).  So the reference of an entry is
_sample_highprec.linear_reference on the case RESTATED on those error bars, under an id of its own (the helper and its witnesses cache
by id).  The bar is that helper's: 16 max(e_witness, e_second, e_blocked, floor) + the normals term, its second fp64 evaluation being the
PLAIN mirror markov.sample on the effective error bars.  Nothing in it comes from the noise mirror or from the device."""
import _markov_noise_cases as NC
import _markov_noise_predict_cases as NP
import _sample_highprec as SH
from gpcc_amd import rng

SLIPS = ("draw_obs_noise_raw", "draw_test_noise_raw", "kappa_linear", "noise_all_bands")
S = 3


def cases():
    """[(case, kappa[L], nu[L])], 72: the case of predict_cases() with tests = (ttest, ytest, sigmatest or None)."""
    out = []
    for idx, (case, kappa, nu) in enumerate(NP.predict_cases()):
        cid, k, data, delays, alpha, rho, mb, (tt, yt, st) = case
        out.append(((cid, k, data, delays, alpha, rho, mb, (tt, yt, st if idx % 2 == 0 else None)), kappa, nu))
    return out


def seed_of(idx):
    return 700 + idx


def word_of(idx):
    """Per-row counters (row word 0) on the even-numbered entries, mixture counters on the odd ones."""
    return rng.MIXROW if idx % 2 else 0


def restated(entry, cid=None):
    """The case of an entry on its effective error bars: what a fresh handle would be created with, and what it would be asked."""
    (c, k, (t, y, s), delays, alpha, rho, mb, (tt, yt, st)), kappa, nu = entry
    eff_tests = (tt, yt, None) if st is None else NP.mapped_tests((tt, yt, st), kappa, nu)
    return ((cid or c) + "-noise-sample" + ("" if st is not None else "-latent"), k, (t, y, NC.effective(s, kappa, nu)), delays, alpha, rho,
            mb, eff_tests)


def reference(oracle, entry, seed, n, word, cid=None):
    """The _sample_highprec.Reference of draws 0 .. n-1 of one entry (cached by the helper under the restated case's id)."""
    return SH.linear_reference(oracle, restated(entry, cid), seed, n, word)
