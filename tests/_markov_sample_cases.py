"""Cases, witnesses and the bar of the linear-time joint posterior draws (tests/test_markov_sample_cpu.py,
tests/test_gpu_markov_sample.py).

The bar is the dense draws' own, _sample_witness.bar(cond_1(K_aug), ref) = max(1e-10, 64 eps cond_1) max(1, max |ref|), measured on the
oracle's matrices and never from the code under test.  The witnesses are dense algebra on the same matrices
(_heldout_witness.blocks): the predictive mean mu_b + kB*' K^-1 (Y - bbar), the covariance C - kB*' K^-1 kB* (C includes JITTER and
diag sigma*^2), and the Matheron draw mu_pred + g~ - kB*' K^-1 r~ + noise of a given prior draw (r~, g~, noise).

small_cases(): N = 6 .. 15, T = 3 .. 7, three kernels x both b-modes x L = 1, 2, 3 -- small enough to push every unit normal through the
draw.  Every time and delay is a multiple of 2^-10.  Each case has a time repeated inside a band, a test point on a training point of
its own band, and (L > 1) a training point and a test point of a later band that meet points of band 1 in shifted time."""
import itertools

import numpy as np

import _heldout_witness as HW
import _markov_cases as MC
import _markov_predict_cases as PC
import _sample_witness as SW

_cache = {}


def small_cases():
    """[(id, kernel, data, delays, alpha, rho, marginalise_b, (ttest, None, sigmatest))] in a fixed order; sigmatest is None (the
    latent curve) on every third case."""
    out = []
    shapes = {1: [9], 2: [7, 6], 3: [6, 4, 5]}
    rhos = (0.4, 9.0, 300.0)
    for idx, (L, kernel, mb) in enumerate(itertools.product((1, 2, 3), MC.KERNELS, (True, False))):
        rg = np.random.default_rng(7000 + idx)
        delays = np.zeros(L)
        delays[1:] = MC.snap(rg.uniform(-1.5, 2.0, L - 1))
        t, y, s, tt, st = [], [], [], [], []
        for l, n in enumerate(shapes[L]):
            tl = np.sort(MC.snap(rg.uniform(0.0, 8.0, n)))
            tl[1] = tl[0]                                            # a tie inside the band
            if l == 0:
                first = tl.copy()
            else:
                tl[2] = first[3] + delays[l]                         # a tie across bands in shifted time
            a = MC.snap(rg.uniform(-1.0, 9.0, {1: 2 + idx % 2, 2: 1, 3: int(l == 0)}[L]))
            a = np.concatenate([a, tl[-1:]])                         # a test point on a training point of its band
            if l > 0:
                a = np.concatenate([a, first[4:5] + delays[l]])       # ... and on one of band 1 in shifted time
            t.append(tl[rg.permutation(n)])
            y.append(np.sin(0.7 * (t[-1] - delays[l])) + 0.4 * l + 0.2 * rg.standard_normal(n))
            s.append(0.2 + 0.05 * rg.random(n))
            tt.append(a[rg.permutation(len(a))])
            st.append(0.1 + 0.1 * rg.random(len(a)))
        alpha = rg.uniform(0.5, 2.0, L)
        rho = rhos[(idx + L) % 3]
        out.append(("small-%s-L%d-b%d-rho%g" % (kernel, L, mb, rho), kernel, (t, y, s), delays, alpha, rho, mb,
                    (tt, None, None if idx % 3 == 2 else st)))
    return out


def cpu_cases():
    """The 72 cases of the linear-time predictions (N = 110) with their test noise."""
    return PC.cpu_cases()


def witness(oracle, case):
    """(mean[T], cov[T, T], kB*' K^-1 [T, N], cond_1(K_aug), mu_b[bands of the test points]) of a case (cached)."""
    cid, kernel, data, delays, alpha, rho, mb, tests = case
    if cid not in _cache:
        tt, st = tests[0], tests[2]
        if st is None:
            st = [np.zeros(len(a)) for a in tt]
        K, resid, kB, C, bs, mub = HW.blocks(oracle, kernel, *data, delays, alpha, rho, tt, st, mb)
        W = np.linalg.solve(K, kB).T
        S = C - W @ kB
        Ka = np.block([[K, kB], [kB.T, C]])
        cond = np.linalg.norm(Ka, 1) * np.linalg.norm(np.linalg.inv(Ka), 1)
        _cache[cid] = (W @ resid + mub[bs], 0.5 * (S + S.T), W, cond, mub[bs])
    return _cache[cid]


def matheron(oracle, case, rt, gt, noise):
    """The dense-algebra draw of a prior draw: mu_pred + g~ - kB*' K^-1 r~ + noise, and its bar."""
    mean, _, W, cond, _ = witness(oracle, case)
    ref = mean + gt - W @ rt + noise
    return ref, SW.bar(cond, ref)


def dims(case):
    data, tests = case[2], case[7]
    return sum(len(a) for a in data[0]), sum(len(a) for a in tests[0])
