"""Cases, references and bars of the linear-time predictions, held-out log-likelihoods and offsets' posterior
(tests/test_markov_predict_cpu.py, tests/test_gpu_markov_predict.py).

Cases: OU / matern32 / matern52 x L in {1, 2, 3} x both b-modes x rho in {0.1, 3, 20, 300} on the light curves of
_markov_cases.lightcurves (N = 110; every time and delay a multiple of 2^-10, so a tie in shifted time is a tie; the shapes cycle through
"ties", "before" and "plain").  Test times per band: (a) beyond the data on both sides, (b) exactly on training points of the same band
and, in shifted time, of another band, (c) one time repeated, (d) handed over unsorted, (e) every other case one band has none.

References here are the fp64 dense witnesses, _predict_witness.predict_row for mu and var, _heldout_witness.heldout_row for the held-out
value, the reference's formulas (marginaliseb.jl:248-250) for postb, under the conditioning-scaled bars that the dense parity tests have
always used: max(1e-10, 64 eps cond_1(K)) x scale, and rtol 1e-7 / atol 1e-12 for postb.  Those bars are loose -- with b marginalised
the variance bar is above the 1e-8 jitter itself -- and measure no error of anything; the same cases are held against an
extended-precision reference under a bar measured on the reference side in tests/_predict_highprec.py
(tests/test_predict_highprec_cpu.py, tests/test_gpu_predict_highprec.py)."""
import itertools

import numpy as np

import _heldout_witness as HW
import _markov_cases as MC
import _predict_witness as PW

NL = {1: [110], 2: [60, 50], 3: [40, 40, 30]}
_cache = {}


def test_points(t, delays, seed, drop_band):
    """(ttest, ytest, sigmatest): lists of L arrays."""
    rg = np.random.default_rng(seed)
    L = len(t)
    tt, yt, st = [], [], []
    for l in range(L):
        o = (l + 1) % L                                            # another band (the same one when L = 1)
        own = np.sort(t[l])[[0, len(t[l]) // 2]]                   # (b) training points of this band ...
        other = np.sort(t[o])[[1, len(t[o]) - 1]] - delays[o] + delays[l]      # ... and, in shifted time, of another band
        a = np.concatenate([MC.snap(rg.uniform(-8.0, 0.0, 2)), MC.snap(rg.uniform(30.0, 38.0, 2)),    # (a) beyond the data
                            MC.snap(rg.uniform(0.0, 30.0, 5)), own, other])
        a = np.concatenate([a, a[5:6], own[:1]])                   # (c) repeated
        a = a[rg.permutation(len(a))]                              # (d) unsorted
        if l == drop_band:
            a = np.zeros(0)                                        # (e) Ntest = 0
        tt.append(a)
        yt.append(np.sin(0.4 * (a - delays[l]) + 0.1 * l) + 0.3 * l + 0.2 * rg.standard_normal(len(a)))
        st.append(0.2 + 0.05 * rg.random(len(a)))
    return tt, yt, st


def cpu_cases():
    """[(id, kernel, data, delays, alpha, rho, marginalise_b, (ttest, ytest, sigmatest))] in a fixed order."""
    out = []
    kinds = ("ties", "before", "plain")
    for idx, (L, kernel, mb, rho) in enumerate(itertools.product((1, 2, 3), MC.KERNELS, (True, False), MC.RHOS)):
        kind = kinds[idx % 3]
        t, y, s, delays = MC.lightcurves(NL[L], seed=2000 + idx, kind=kind)
        alpha = np.random.default_rng(idx).uniform(0.5, 2.0, L)
        drop = (idx // 3) % L if (L > 1 and idx % 2 == 0) else -1
        tests = test_points(t, delays, 3000 + idx, drop)
        out.append(("%s-L%d-b%d-rho%g-%s" % (kernel, L, mb, rho, kind), kernel, (t, y, s), delays, alpha, rho, mb, tests))
    return out


def predict_reference(oracle, case):
    """(mu, var, bar of mu, bar of var) of a case (cached)."""
    cid, kernel, data, delays, alpha, rho, mb, tests = case
    if ("p", cid) not in _cache:
        mu, var, cond, cmax = PW.predict_row(oracle, kernel, *data, delays, alpha, rho, tests[0], mb)
        _cache[("p", cid)] = (mu, var, PW.bar(cond, max(1.0, float(np.max(np.abs(mu))))), PW.bar(cond, cmax))
    return _cache[("p", cid)]


def heldout_reference(oracle, case):
    """(heldout, bar) of a case (cached)."""
    cid, kernel, data, delays, alpha, rho, mb, tests = case
    if ("h", cid) not in _cache:
        ref, cond = HW.heldout_row(oracle, kernel, *data, delays, alpha, rho, *tests, mb)
        _cache[("h", cid)] = (ref, HW.bar(cond, ref))
    return _cache[("h", cid)]


def postb_reference(oracle, kernel, t, y, s, delays, alpha, rho):
    """(mu_postb, Sigma_postb) by the reference's formulas, as tests/test_gpu_parity.py::test_posterior_offsets_vs_reference_formulas."""
    K0, _ = oracle.model_matrix(kernel, t, y, s, delays, alpha, rho, False)          # Sobs + K (no B)
    Nl = [len(a) for a in t]
    Q = np.zeros((sum(Nl), len(Nl)))
    o = 0
    for l, n in enumerate(Nl):
        Q[o:o + n, l] = 1
        o += n
    Y = np.concatenate(y)
    Sigb = np.diag(100 * np.array([np.var(a, ddof=1) for a in y]))
    mub = np.array([np.mean(a) for a in y])
    Sref = np.linalg.inv(np.linalg.inv(Sigb) + Q.T @ np.linalg.solve(K0, Q))       # marginaliseb.jl:248
    mref = Sref @ (Q.T @ np.linalg.solve(K0, Y) + np.linalg.solve(Sigb, mub))       # :250
    return mref, Sref


def assert_postb(mu, Sig, mref, Sref):
    np.testing.assert_allclose(Sig, Sref, rtol=1e-7, atol=1e-12)
    np.testing.assert_allclose(mu, mref, rtol=1e-7)
