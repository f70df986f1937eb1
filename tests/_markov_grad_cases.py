"""Cases, references and bars of the linear-time gradient's tests (tests/test_markov_grad_cpu.py, tests/test_gpu_markov_grad.py).

Cases: _markov_cases.cpu_cases(), unchanged -- OU / matern32 / matern52 x L in {1, 2, 3} x both b-modes x rho in {0.1, 3, 20, 300} x
N in {110, 150, 767}, the delays cycling through "ties", "before" and "plain".  The reference is the extended-precision gradient
_grad_highprec.evaluate of the dense trace formula and the bar is _grad_highprec.bar(ref), the dense gradient's own bar, which depends
on the reference alone.  The large shapes are those of tests/test_gpu_markov.py (LARGE, the same data, delays and hyperparameters),
checked against the fp64 torch witness within 1e-8 max|g|, the bar tests/test_gpu_gradient.py gives the dense device gradient."""
import numpy as np

import _grad_highprec as H
import _markov_cases as MC
from gpcc_amd import synthetic

SLIPS = ("one_sided", "no_dpinf", "tau_one_lag", "no_dh")
LARGE = {2048: ("OU", [1024, 1024]), 4095: ("matern32", [1500, 1300, 1295]), 4096: ("matern52", [2048, 2048])}   # test_gpu_markov.LARGE
WITNESS_BAR = 1e-8
_cache = {}


def cases(N=None):
    return [c for c in MC.cpu_cases() if N is None or c[7] in (N if isinstance(N, (tuple, list)) else (N,))]


def subset_767():
    """The fixed subset at N = 767: L = 3, rho in {0.1, 300}, all kernels, both b-modes."""
    return [c for c in MC.cpu_cases() if c[7] == 767 and len(c[4]) == 3 and c[5] in (0.1, 300.0)]


def reference(case):
    """The extended-precision Reference of a case (cached)."""
    cid, kernel, data, delays, alpha, rho, mb, _ = case
    if cid not in _cache:
        ref = H.evaluate(kernel, *data, delays, alpha, rho, mb)
        assert ref.info == 0, cid
        _cache[cid] = ref
    return _cache[cid]


def large(N, G):
    """(kernel, data, delays[G, L], alpha[G, L], rho[G]) of a large shape: test_gpu_markov.test_parity_large's grid cut to G delays."""
    kernel, Nl = LARGE[N]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=N)
    L = len(Nl)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    delays = np.zeros((G, L))
    delays[:, 1:] = np.linspace(0.0, 12.6, 64)[:G, None] * (1.0 + 0.5 * np.arange(L - 1))[None, :]
    return kernel, (t, y, s), delays, np.tile(alpha0, (G, 1)), np.full(G, rho0)


class Worst:
    """The worst error / bar of a group; add() asserts the bar."""

    def __init__(self, group):
        self.group, self.worst, self.where = group, 0.0, None

    def add(self, ratio, where, limit=1.0):
        if ratio >= self.worst:
            self.worst, self.where = ratio, where
        assert ratio <= limit, (self.group, where, ratio, limit)

    def report(self):
        line = "%s: worst error / bar %.3g (%s)" % (self.group, self.worst, self.where)
        print(line)
        return line
