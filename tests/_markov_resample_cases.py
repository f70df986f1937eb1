"""Cases, realisations and references of the resampled-data linear-time log-likelihood's tests (tests/test_markov_resample_cpu.py,
tests/test_gpu_markov_resample.py).

Cases: tests/_markov_realisations_cases.cases(): OU / matern32 / matern52 x L in {1, 2, 3} x both b-modes x rho in {0.1, 3, 300}, the
"ties", "before" and "plain" delay kinds as tests/_markov_cases.py deals them.  Per case R = 4 realisations from synthetic.resample:
the case's own y with counts of 1, flux randomisation only, random subset selection only, both.

The reference of a cell (case, realisation) is tests/_markov_cases.reference_and_bar on the REDUCED FRESH DATA SET: the distinct
selected points (t[sel], Y_r[sel], sigma[sel] / sqrt(count)) as a data set of their own -- its own band means and, with
marginalise_b, its own 100 var -- so the extended-precision dense value wherever numpy.longdouble is extended, with the family's bar
MC.bar(e_dense, N_kept, MC.factor(alpha, reduced sigma)), measured on the reference side.  No case is skipped or filtered:
synthetic.resample keeps at least 2 distinct points per band, which reduced() asserts."""
import numpy as np

import _markov_cases as MC
import _markov_realisations_cases as RC

R = 4
KINDS = ("own y", "flux", "subset", "flux + subset")
_real = {}


def cases(sizes=(110,)):
    return RC.cases(sizes)


def realisations(case):
    """(Y, counts) of a case: lists of L arrays (4, N_l) -- KINDS in this order (cached)."""
    from gpcc_amd import synthetic
    cid, _, (t, y, s), _, _, _, _, _ = case
    if cid not in _real:
        seed = sum(ord(ch) for ch in cid)
        Yf, _ = synthetic.resample(y, s, 1, seed, flux=True, subset=False)
        _, cs = synthetic.resample(y, s, 1, seed + 1, flux=False, subset=True)
        Yb, cb = synthetic.resample(y, s, 1, seed + 2, flux=True, subset=True)
        Y, counts = [], []
        for l in range(len(t)):
            yl = np.asarray(y[l], np.float64)[None, :]
            Y.append(np.concatenate([yl, Yf[l], yl, Yb[l]], axis=0))
            counts.append(np.concatenate([np.ones_like(cs[l]), np.ones_like(cs[l]), cs[l], cb[l]], axis=0))
        _real[cid] = (Y, counts)
    return _real[cid]


def reduced(data, Y, counts, r):
    """The reduced fresh data set of realisation r: (t[sel], Y_r[sel], sigma[sel] / sqrt(count)) per band, in the caller's order."""
    t, _, s = data
    out = ([], [], [])
    for l in range(len(t)):
        c = np.asarray(counts[l][r])
        keep = c > 0
        assert np.count_nonzero(keep) >= 2, (l, r)
        out[0].append(np.asarray(t[l], np.float64)[keep])
        out[1].append(np.asarray(Y[l][r], np.float64)[keep])
        out[2].append(np.asarray(s[l], np.float64)[keep] / np.sqrt(c[keep]))
    return out


def reduced_case(case, r):
    """Realisation r of a case as a case of tests/_markov_cases.py: its reduced data set, N = the kept points."""
    cid, kernel, data, delays, alpha, rho, mb, _ = case
    Y, counts = realisations(case)
    red = reduced(data, Y, counts, r)
    return ("%s/resampled%d" % (cid, r), kernel, red, delays, alpha, rho, mb, sum(len(a) for a in red[0]))


def reference(oracle, case, r):
    """(reference, bar, e_dense) of the cell (case, realisation r)."""
    return MC.reference_and_bar(oracle, reduced_case(case, r))


def rows(case):
    """The R rows of a case, one per realisation, all at the case's (tau, alpha, rho): (delays, alpha, rho, real)."""
    _, _, _, delays, alpha, rho, _, _ = case
    return np.tile(delays, (R, 1)), np.tile(alpha, (R, 1)), np.full(R, rho), np.arange(R)
