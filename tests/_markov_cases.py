"""Cases, references and the bar of the linear-time log-likelihood's tests (tests/test_markov_cpu.py, tests/test_gpu_markov.py).

Cases: OU / matern32 / matern52 x L in {1, 2, 3} x both b-modes x rho in {0.1, 3, 20, 300} x N in {110, 150, 767}.  Every time and
delay is a multiple of 2^-10, so shifted times are exact and a tie is a tie; the last band's observations are handed over in
shuffled (unsorted) order.  The delays cycle through three shapes: "ties" (several points of the later bands coincide in shifted
time with points of band 1), "before" (tau larger than the span: one band lies wholly before the other) and "plain".

The bar is measured on the reference side, never from the filter: bar = F x max(e_dense, N 2^-53) relative, e_dense being the
relative error of the oracle's fp64 dense value against the extended-precision value (_grad_highprec.evaluate) of the same case --
or, where that reference is not available (longdouble not extended, or N too large for it), the relative disagreement of the two
independent dense references, oracle.loglik_batch and oracle/lapack_baseline.py.

F = max(16, 2 max(alpha)^2 / min(sigma)^2).  16 covers the filter's N sequential rank-one updates against the Cholesky's blocked
sums.  The second term is the filter's conditioning: the state's variance starts at Pinf_11 = 1 and is brought down
to the posterior variance by subtraction, so every predictive variance S = alpha^2 P_11 + sigma^2 carries the absolute rounding of
the fp64 transition matrix, eps alpha^2, i.e. up to eps alpha^2 / sigma^2 relative, accumulated over the N steps; the sum of
(log S + eps_i^2 / S) / 2, whose second part is about |loglik|, moves by up to 2 N eps alpha^2 / sigma^2 |loglik|.  (The same filter
run in extended precision on the fp64 transition matrices shows the same error: it is the rounding of A, not of the recursion.  Seen
at rho = 300, where neighbouring points are correlated to 1 - 1e-7.)

Not covered here -- lambda x lag below 1e-3, rho above 300, four and eight bands, three bands tied on one time: tests/_markov_regime_cases.py."""
import itertools

import numpy as np

import _grad_highprec as H

KERNELS = ("OU", "matern32", "matern52")
RHOS = (0.1, 3.0, 20.0, 300.0)
SHAPES = {110: {1: [110], 2: [60, 50], 3: [40, 40, 30]}, 150: {1: [150], 2: [80, 70], 3: [50, 50, 50]},
          767: {1: [767], 2: [400, 367], 3: [300, 200, 267]}}
GRID = 1024.0
FACTOR = 16.0
_cache = {}


def snap(x):
    return np.round(np.asarray(x, np.float64) * GRID) / GRID


def lightcurves(Nl, seed, kind):
    """(tarray, yarray, stdarray, delays): times in [0, 30] on the 2^-10 grid; see the module's docstring for `kind`."""
    rg = np.random.default_rng(seed)
    L = len(Nl)
    delays = np.zeros(L)
    if kind == "before":
        delays[1:] = snap(40.0 + 3.0 * np.arange(1, L))
    else:
        delays[1:] = snap(rg.uniform(-3.0, 5.0, L - 1))
    t, y, s = [], [], []
    for l, n in enumerate(Nl):
        tl = np.sort(snap(rg.uniform(0.0, 30.0, n)))
        if kind == "ties" and l > 0:     # shifted times of band 1 met exactly, one of them twice
            pick = rg.choice(len(t[0]), 4, replace=False)
            tl[:4] = t[0][pick] + delays[l]
            tl[4] = tl[3]
            tl = np.sort(tl)
        t.append(tl)
        y.append(np.sin(0.4 * (tl - delays[l]) + 0.1 * l) + 0.3 * l + 0.2 * rg.standard_normal(n))
        s.append(0.2 + 0.05 * rg.random(n))
    perm = rg.permutation(Nl[-1])        # unsorted input
    t[-1], y[-1], s[-1] = t[-1][perm], y[-1][perm], s[-1][perm]
    return t, y, s, delays


def cpu_cases():
    """[(id, kernel, data, delays, alpha, rho, marginalise_b, N)] in a fixed order."""
    out = []
    kinds = ("ties", "before", "plain")
    for idx, (N, L, kernel, mb, rho) in enumerate(itertools.product(sorted(SHAPES), (1, 2, 3), KERNELS, (True, False), RHOS)):
        kind = kinds[idx % 3]
        t, y, s, delays = lightcurves(SHAPES[N][L], seed=1000 + idx, kind=kind)
        alpha = np.random.default_rng(idx).uniform(0.5, 2.0, L)
        out.append(("%s-N%d-L%d-b%d-rho%g-%s" % (kernel, N, L, mb, rho, kind), kernel, (t, y, s), delays, alpha, rho, mb, N))
    return out


def extended(case):
    """The extended-precision value of a case (cached)."""
    cid, kernel, data, delays, alpha, rho, mb, _ = case
    if ("x", cid) not in _cache:
        ref = H.evaluate(kernel, *data, delays, alpha, rho, mb)
        assert ref.info == 0, cid
        _cache[("x", cid)] = ref.loglik
    return _cache[("x", cid)]


def dense(oracle, case):
    cid, kernel, data, delays, alpha, rho, mb, _ = case
    if ("d", cid) not in _cache:
        ll, info = oracle.loglik_batch(kernel, *data, delays[None, :], alpha[None, :], [rho], mb)
        assert info[0] == 0, cid
        _cache[("d", cid)] = float(ll[0])
    return _cache[("d", cid)]


def dense_pair_error(kernel, data, delays, alpha, rho, mb, dense_value):
    """Relative disagreement of the oracle's value with oracle/lapack_baseline.py's for one evaluation."""
    from oracle import lapack_baseline
    lp, info = lapack_baseline.loglik_lapack(kernel, *data, np.asarray(delays, np.float64), np.asarray(alpha, np.float64), float(rho), mb)
    assert info == 0
    return abs(lp - dense_value) / abs(dense_value)


def factor(alpha, stdarray):
    """F of the module's docstring."""
    return max(FACTOR, 2.0 * float(np.max(alpha)) ** 2 / float(min(np.min(s) for s in stdarray)) ** 2)


def bar(e_dense, N, F=FACTOR):
    """Relative bar of one case."""
    return F * max(e_dense, N * 2.0 ** -53)


def reference_and_bar(oracle, case):
    """(reference value, relative bar, e_dense) of a CPU case: the extended value where longdouble is extended, else the oracle's value
    with the two dense references' disagreement as e_dense."""
    cid, kernel, data, delays, alpha, rho, mb, N = case
    d = dense(oracle, case)
    if H.EXTENDED:
        ref = extended(case)
        e = abs(d - ref) / abs(ref)
    else:
        ref = d
        e = dense_pair_error(kernel, data, delays, alpha, rho, mb, d)
    return ref, bar(e, N, factor(alpha, data[2])), e


class Worst:
    def __init__(self, group):
        self.group, self.worst, self.where, self.err, self.bar = group, 0.0, None, 0.0, 0.0

    def add(self, err, b, where):
        if err / b >= self.worst:
            self.worst, self.where, self.err, self.bar = err / b, where, err, b
        assert err <= b, (where, err, b)

    def report(self):
        line = "%s: worst error / bar %.3g (error %.3g, bar %.3g, %s)" % (self.group, self.worst, self.err, self.bar, self.where)
        print(line)
        return line
