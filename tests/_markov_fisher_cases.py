"""Cases, references and bars of the tests of the linear-time Fisher information (tests/test_markov_fisher_cpu.py,
tests/test_gpu_markov_fisher.py).

Cases: _markov_hess_cases.cases(), 144 of them.  The reference is the extended-precision Fisher matrix ref.F of
_hess_highprec.evaluate(..., keep=True) with the per-block bars ref.bars["F"] of add_bars over all six blocks aa, ar, at, rr, rt, tt
(_markov_hess_full_cases.reference_job: the witness left out of the bars on rows with a cross-band tie), the ratio error / bar
multiplied by _markov_hess_cases.scale(case) as for the Hessian.  The Hessian's bars take no part.

OU's Fisher entries with a tau index are not defined by a filter order on a row with a cross-band tie in shifted time: those cases (12
of the 144, _markov_hess_full_cases.ou_tie) check the NaN contract and the (alpha, rho) block."""
import math

import numpy as np

import _hess_highprec as HH
import _markov_hess_cases as HC
import _markov_hess_full_cases as FC

SLIPS = ("no_innov", "prior_moment", "no_gain_tangent", "no_dh_moment", "tau_one_lag")
HYPER_BLOCKS = ("aa", "ar", "rr")
Worst = HC.Worst
cases = HC.cases
job = HC.job
reference_job = FC.reference_job
ou_tie = FC.ou_tie
tie_rows = FC.tie_rows
tau_mask = FC.tau_mask
device_limit = FC.device_limit


def ratios(fisher, ref, case, against=None, blocks=None):
    """{block: error / bar} of a (2L+1) x (2L+1) Fisher matrix against ref.F under ref.bars["F"] times scale(case) (against: another
    Fisher matrix to measure the distance to, with ref's bars; blocks: only these).  A block whose bar is 0 (the tau rows at L = 1) must
    be matched exactly; NaN counts as a miss."""
    want = ref.F if against is None else np.asarray(against, np.float64)
    err = np.abs(np.asarray(fisher, np.float64) - want)
    out = {}
    for b, m in HH.block_masks(ref.L).items():
        if blocks is not None and b not in blocks:
            continue
        e, bar = float(np.max(err[m])), ref.bars["F"][b]
        r = e / bar if bar > 0 else (0.0 if e == 0 else math.inf)
        out[b] = (r if r == r else math.inf) * HC.scale(case)
    return out


def bar_sum(ref, case):
    """The sum over all entries of the entry's bar (its block's, divided by scale(case)): what rounding may take from the smallest
    eigenvalue of a matrix that is positive semi-definite in exact arithmetic."""
    total = 0.0
    for b, m in HH.block_masks(ref.L).items():
        total += int(m.sum()) * ref.bars["F"][b]
    return total / HC.scale(case)


def pair_job(job):
    """(kernel, t, y, s, delays, alpha, rho, mb, a, b) -> loglik_fisher's entry (a, b) alone, without the value and the gradient: a
    top-level function for a process pool (the N = 16384 row of the device's test)."""
    from gpcc_amd import markov
    kernel, t, y, s, delays, alpha, rho, mb, a, b = job
    name, L, delays, alpha, rho, code, vb, means, p, n, train = markov._setup(kernel, t, y, s, delays, alpha, rho, mb)
    assert code == 0
    return markov._fisher_pass(name, train, alpha, rho, p, n, vb, min(a, b), max(a, b))
