"""Cases, references and bars of the resampled-data linear-time gradient's tests (tests/test_markov_resample_grad_cpu.py,
tests/test_gpu_markov_resample_grad.py).

Cases and realisations: tests/_markov_resample_cases.py, unchanged -- OU / matern32 / matern52 x L in {1, 2, 3} x both b-modes x rho in
{0.1, 3, 300}, R = 4 realisations per case (own y, flux, subset, flux + subset).  The reference of a cell (case, realisation) is
_grad_highprec.evaluate on SC.reduced_case(case, r): the extended-precision dense gradient of the REDUCED FRESH DATA SET, with its own
band means and, with marginalise_b, its own 100 var.  The bar is _grad_highprec.bar(ref), the dense gradient's own bar, which depends
on the reference alone.  No cell is skipped or filtered."""
import numpy as np

import _grad_highprec as H
import _markov_resample_cases as SC
from _markov_grad_cases import WITNESS_BAR, Worst  # noqa: F401  (the tests take them from here)

R, KINDS = SC.R, SC.KINDS
BOTH = KINDS.index("flux + subset")
_cache = {}


def cases(sizes=(110,)):
    return SC.cases(sizes)


def reference(case, r):
    """The extended-precision Reference of the cell (case, realisation r), computed once and shared."""
    key = (case[0], r)
    if key not in _cache:
        _, kernel, data, delays, alpha, rho, mb, _ = SC.reduced_case(case, r)
        ref = H.evaluate(kernel, *data, delays, alpha, rho, mb)
        assert ref.info == 0, key
        _cache[key] = ref
    return _cache[key]


def tie_case(seed=5):
    """An OU case with an exact tie in shifted time between two KEPT points of different bands and a DROPPED point between them in the
    handle's merged order: (t, y, s, delays, Y, counts, (band, position) of the dropped point).  Band 0 has a point at the tied shifted
    time twice; its second copy is dropped, so that the merged order is kept (0), dropped (0), kept (1)."""
    import _markov_cases as MC
    from gpcc_amd import markov
    t, y, s, d0 = MC.lightcurves([30, 20], seed=seed, kind="ties")
    t = [np.array(a, np.float64) for a in t]
    ts = markov.prepare(t, y, s)[0]
    seq = markov.merge_order(ts, d0)
    sh = [ts[b][i] - d0[b] for b, i in seq]
    j = next(j for j in range(3, len(seq) - 1) if seq[j][0] == 1 and seq[j - 1][0] == 0 and sh[j] == sh[j - 1] and sh[j - 2] != sh[j]
             and sh[j + 1] != sh[j])
    # the band-0 point after the tied one is moved onto it: band 0 now holds the tied time twice, the merged order is 0, 0, 1
    b0, i0 = seq[j - 1]
    nxt = int(np.flatnonzero(t[0] == ts[0][i0 + 1])[0])
    t[0][nxt] = ts[0][i0]
    counts = [np.ones((1, len(a)), dtype=np.int64) for a in t]
    counts[0][0, nxt] = 0
    Y = [np.asarray(a, np.float64)[None, :].copy() for a in y]
    return t, y, s, np.asarray(d0, np.float64), Y, counts, (0, nxt)
