"""Cases, references and the bar of the linear-time Hessian block's tests (tests/test_markov_hess_cpu.py, tests/test_gpu_markov_hess.py).

Cases: all of _markov_cases.cpu_cases() with N in {110, 150} -- OU / matern32 / matern52 x L in {1, 2, 3} x both b-modes x rho in
{0.1, 3, 20, 300}, the delays cycling through "ties", "before" and "plain": 144 cases.  (N = 767 is left out: the extended-precision
Hessian there is minutes per case.)

The reference is the extended-precision Hessian _hess_highprec.evaluate(..., keep=True) with the per-block bars of add_bars (the fp64
mirrors' and the torch witness's own errors against it, and the rounding floor of the sums: every ingredient from the reference side).
The blocks are aa, ar and rr of the leading (L + 1) x (L + 1) block.  The bars are those of a dense fp64 Hessian, whose factor is 16; the
filter's conditioning factor is _markov_cases.factor(alpha, std) = max(16, 2 max(alpha)^2 / min(sigma)^2) (the rounding
of the transition matrix in every predictive variance), so the ratio error / bar is multiplied by 16 / factor."""
import numpy as np

import _hess_highprec as HH
import _markov_cases as MC
import _markov_grad_cases as GC

SIZES = (110, 150)
SLIPS = ("no_d2a", "no_d2pinf", "no_cross", "no_hahb", "chain_rho")
Worst = GC.Worst


def cases(N=None):
    keep = SIZES if N is None else (N,)
    return [c for c in MC.cpu_cases() if c[7] in keep]


def job(case):
    """The argument of _hess_highprec.reference_job (a top-level function for a process pool) for a case."""
    _, kernel, data, delays, alpha, rho, mb, _ = case
    return (kernel, *data, delays, alpha, rho, mb)


def scale(case):
    """16 / factor: what the dense bars' ratio is multiplied by."""
    return MC.FACTOR / MC.factor(case[4], case[2][2])


def ratio(hess, ref, case, against=None):
    """The worst error / bar over the blocks aa, ar, rr of an (L + 1) x (L + 1) block (against: another block to measure the
    distance to, with ref's bars)."""
    n = len(case[4]) + 1
    other = None if against is None else (np.asarray(against, np.float64), None)
    if other is not None:     # ratio_blocks indexes `against` as the reference's full matrices
        full = np.full_like(ref.H, np.nan)
        full[:n, :n] = other[0]
        other = (full, ref.F)
    return HH.worst(HH.ratio_blocks(np.asarray(hess)[:n, :n], None, ref, against=other)) * scale(case)
