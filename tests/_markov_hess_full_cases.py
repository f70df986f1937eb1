"""Cases, references and bars of the tests of the linear-time full Hessian -- the rows of tau -- (tests/test_markov_hess_full_cpu.py,
tests/test_gpu_markov_hess_full.py).

Cases: _markov_hess_cases.cases(), 144 of them.  The reference is _hess_highprec.evaluate(..., keep=True) with the per-block bars of
add_bars over all six blocks aa, ar, at, rr, rt, tt, the ratio error / bar multiplied by _markov_hess_cases.scale(case) as for the
leading block.  On a row with a cross-band tie in shifted time (ref.ties) the bars are add_bars(ref, witness=False): the torch witness
cannot differentiate at a tie and its own error would make the tt bar vacuous (with it the tt ratio of
matern32-N110-L2-b1-rho3-ties is 1e-15, without it 0.011).  Hence reference_job here; _hess_highprec.reference_job is as it was.

OU has no second derivative by tau on a row with such a tie: those cases (12 of the 144, found by ou_tie() with numpy's intersect1d of
the bands' shifted times) check the NaN contract instead of the bars."""
import numpy as np

import _hess_highprec as HH
import _markov_hess_cases as HC

SLIPS = {"no_d2tau": ("tt",), "tau_one_lag": ("at", "rt", "tt"), "no_dF": ("rt",), "no_cross_tau": ("rt", "tt")}    # slip: the blocks it touches
TAU_BLOCKS = ("at", "rt", "tt")
# the README-size data (synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)) at delays (0, 2.03): (alpha, rho) at the mode
# of the Laplace polish over the numpy mirror, rounded to three digits -- a point where -H over (alpha, rho, tau_2) is positive definite
README_DELAYS = (0.0, 2.03)
README_MODE = {"OU": ((0.589, 1.002), 0.890), "matern32": ((0.574, 0.971), 0.427)}
Worst = HC.Worst
cases = HC.cases
job = HC.job


def reference_job(job):
    """_hess_highprec.reference_job with the witness left out of the bars on rows with a cross-band tie: a top-level function for a
    process pool."""
    try:
        import torch
        torch.set_num_threads(2)
    except Exception:
        pass
    ref = HH.evaluate(*job[:8], keep=True)
    if ref.info == 0:
        HH.add_bars(ref, witness=not ref.ties)
    ref.parts = {}
    return ref


def ou_tie(case):
    """Whether an OU case has two points of different bands at exactly the same shifted time."""
    _, kernel, data, delays, _, _, _, _ = case
    if kernel != "OU":
        return False
    return bool(tie_rows(data[0], delays)[0])


def tie_rows(tarray, delays):
    """Boolean [M]: the rows of delays[M, L] in which two points of different bands have exactly equal shifted times."""
    ts = [np.sort(np.asarray(t, np.float64)) for t in tarray]
    L = len(ts)
    delays = np.asarray(delays, np.float64).reshape(-1, L)
    return np.array([any(len(np.intersect1d(ts[l] - d[l], ts[m] - d[m])) > 0 for l in range(L) for m in range(l + 1, L)) for d in delays],
                    dtype=bool)


def tau_mask(L):
    """Boolean [2L+1, 2L+1]: the entries with a tau index."""
    m = np.zeros((2 * L + 1, 2 * L + 1), bool)
    m[L + 1:, :] = m[:, L + 1:] = True
    return m


def ratios(hess, ref, case, against=None):
    """{block: error / bar} over all six blocks of a (2L+1) x (2L+1) Hessian (against: another full Hessian to measure the distance
    to, with ref's bars)."""
    other = None if against is None else (np.asarray(against, np.float64), ref.F)
    return {b: r * HC.scale(case) for b, r in HH.ratio_blocks(np.asarray(hess), None, ref, against=other).items()}


def device_limit(case):
    """The device's allowance in bars: 2 on the rho = 300 cases (the mirror alone uses 0.72 there, and the device's ratio was seen at up to
    2.5 times the mirror's), 1 elsewhere."""
    return 2.0 if case[5] == 300.0 else 1.0
