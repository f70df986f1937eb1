"""Rows with their own resampled data set on the CPU (gpcc_amd.markov.loglik_resampled, the numpy restatement of
csrc/gpcc_markov_resample.hip.h): every cell of tests/_markov_resample_cases.py against the extended-precision dense value of its
reduced fresh data set under the family's bar; what a count means; synthetic.resample; fit.realisation_refits against gpcc_grid on
each realisation's own data set (exactly) and from a warm start; the ValueError paths."""
import numpy as np
import pytest

import _markov_cases as MC
import _markov_resample_cases as SC
from gpcc_amd import fit, markov, synthetic

CASES = SC.cases((110,))


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_mirror_against_the_reduced_data_sets_reference(oracle, kernel):
    picked = [c for c in CASES if c[1] == kernel]
    assert len(picked) == 3 * 2 * 3
    worst = {k: MC.Worst("mirror %s, %s" % (kernel, k)) for k in SC.KINDS}
    for case in picked:
        cid, k, data, delays, alpha, rho, mb, N = case
        Y, counts = SC.realisations(case)
        d, a, rh, real = SC.rows(case)
        ll, info = markov.MarkovObjective(*data, k, marginalise_b=mb).loglik_markov_resampled(Y, d, a, rh, real, counts=counts)
        assert ll.shape == (SC.R,) and (info == 0).all(), cid
        for r in range(SC.R):
            ref, b, _ = SC.reference(oracle, case, r)
            worst[SC.KINDS[r]].add(abs(ll[r] - ref) / abs(ref), b, (cid, r))
    for w in worst.values():
        assert w.where is not None
        w.report()


def test_what_a_count_means(oracle):
    """A count of 3 is the point once with sigma / sqrt 3 (under the bar of the reduced data set); a count of 0 is the point's absence
    (exactly: the reduced data set through markov.loglik); nothing kept is (0.0, 0)."""
    case = next(c for c in CASES if c[1] == "matern32" and len(c[3]) == 2 and c[6] and c[5] == 3.0)
    cid, k, (t, y, s), delays, alpha, rho, mb, N = case
    counts = [np.ones((3, len(a)), dtype=np.int64) for a in t]
    counts[0][0, 7] = 3
    counts[1][0, 11] = 3
    counts[0][1, [3, 4, 20]] = 0
    counts[1][1, 0] = 0
    counts[0][2, :] = 0
    counts[1][2, :] = 0
    Y = [np.tile(np.asarray(a, np.float64), (3, 1)) for a in y]
    d, a, rh = np.tile(delays, (3, 1)), np.tile(alpha, (3, 1)), np.full(3, rho)
    # the constants of the unreduced data for every realisation, so that only the counts differ
    ll, info = markov.loglik_resampled(k, t, y, s, Y, counts, [0, 1, 2], d, a, rh, mb)
    assert (info == 0).all() and ll[2] == 0.0
    s3 = [np.array(x, np.float64) for x in s]
    s3[0][7] /= np.sqrt(3.0)
    s3[1][11] /= np.sqrt(3.0)
    once, oinfo = markov.loglik_resampled(k, t, y, s3, [x[:1] for x in Y], None, [0], delays, alpha, rho, mb, mean=markov.band_means(t, y)[:1],
                                          sigma_b=markov.prepare(t, y, s, mb)[3][None, :])
    ref, b, _ = MC.reference_and_bar(oracle, case)
    assert oinfo[0] == 0 and abs(ll[0] - once[0]) <= b * abs(ref)
    assert ll[0] != ll[1]
    # the reduced data set with its own constants: markov.loglik's value exactly (the same _pass on the same numbers)
    own, winfo = markov.MarkovObjective(t, y, s, k, marginalise_b=mb).loglik_markov_resampled(Y, d, a, rh, [0, 1, 2], counts=counts,
                                                                                              sigma_b="handle", center="handle")
    assert np.array_equal(own, ll) and np.array_equal(winfo, info)
    keep = [c[1] > 0 for c in counts]
    red = [[np.asarray(x, np.float64)[kp] for x, kp in zip(arr, keep)] for arr in (t, y, s)]
    Y1, c1 = [x[1:2] for x in Y], [c[1:2] for c in counts]
    mean, vb = markov.resample_constants(t, Y1, c1, mb)
    fresh = markov.loglik(k, *red, delays, alpha, rho, mb)
    got, ginfo = markov.loglik_resampled(k, t, y, s, Y1, c1, [0], delays, alpha, rho, mb, mean=mean, sigma_b=vb)
    assert fresh[1] == 0 and ginfo[0] == 0 and got[0] == fresh[0]
    # info counts the kept points: sigma = 0 at two kept points that coincide in shifted time, dropped points before them
    tz, yz, sz, dz = MC.lightcurves([30, 20], seed=5, kind="ties")
    ts = markov.prepare(tz, yz, sz)[0]
    seq = markov.merge_order(ts, dz)
    sh = [ts[bb][i] - dz[bb] for bb, i in seq]
    single = lambda q: np.count_nonzero(tz[seq[q][0]] == ts[seq[q][0]][seq[q][1]]) == 1
    j = next(j for j in range(3, len(seq)) if seq[j][0] != seq[j - 1][0] and sh[j] == sh[j - 1] and single(j) and single(j - 1)
             and (j + 1 == len(seq) or sh[j + 1] != sh[j]) and sh[j - 2] != sh[j])
    cz = [np.ones((1, len(x)), dtype=np.int64) for x in tz]
    for bb, i in (seq[j - 1], seq[j]):
        sz[bb][np.where(tz[bb] == ts[bb][i])[0]] = 0.0
    for bb, i in seq[:2]:                                    # two dropped points ahead of the pair
        cz[bb][0, np.where(tz[bb] == ts[bb][i])[0][0]] = 0
    lz, iz = markov.loglik_resampled("OU", tz, yz, sz, [np.asarray(x)[None, :] for x in yz], cz, [0], dz, [1.0, 1.0], 2.0, False)
    dropped = sum(int((x == 0).sum()) for x in cz)
    assert dropped >= 1 and iz[0] == j + 1 - dropped and np.isnan(lz[0])


def test_resample():
    t, y, s, _ = synthetic.simulate_lightcurves((40, 35, 3), seed=2)
    Y, c = synthetic.resample(y, s, 6, seed=11)
    Y2, c2 = synthetic.resample(y, s, 6, seed=11)
    Y3, c3 = synthetic.resample(y, s, 2, seed=11)
    Y4, _ = synthetic.resample(y, s, 2, seed=12)
    for l in range(3):
        n = len(y[l])
        assert Y[l].shape == c[l].shape == (6, n) and c[l].dtype.kind == "i"
        assert np.array_equal(Y[l], Y2[l]) and np.array_equal(c[l], c2[l])               # reproducible from the seed
        assert np.array_equal(Y[l][:2], Y3[l]) and np.array_equal(c[l][:2], c3[l])       # realisation r is the same in any R
        assert not np.array_equal(Y3[l], Y4[l])
        assert (c[l].sum(axis=1) == n).all() and (c[l] >= 0).all()
        assert (np.count_nonzero(c[l], axis=1) >= 2).all()                               # (band 3 has 3 points: redraws happen)
        assert not np.array_equal(Y[l][0], y[l])
    _, ones = synthetic.resample(y, s, 3, seed=1, subset=False)
    assert all((a == 1).all() for a in ones)
    same, cs = synthetic.resample(y, s, 3, seed=1, flux=False)
    assert all(np.array_equal(a, np.tile(np.asarray(b), (3, 1))) for a, b in zip(same, y))
    assert any((a != 1).any() for a in cs)
    with pytest.raises(ValueError):
        synthetic.resample(y, s, 0, seed=1)
    with pytest.raises(ValueError):
        synthetic.resample([y[0][:1]], [s[0][:1]], 1, seed=1)


def _softmax(ll, logprior=None):
    z = np.asarray(ll, np.float64) + (0.0 if logprior is None else np.asarray(logprior, np.float64))
    e = np.exp(z - z.max())
    return e / e.sum()


def _readme():
    t, y, s, _ = synthetic.simulate_lightcurves((55, 55))
    return t, y, s


def test_refits_are_gpcc_grids_of_each_data_set():
    """start=None, counts of 1: realisation r's refit is gpcc_grid(engine="python", solver="markov") on (t, Y_r, sigma), exactly --
    both run the same _pass on the same numbers, from the same candidates."""
    t, y, s = _readme()
    cand = np.stack([np.zeros(4), np.array([0.5, 2.0, 3.5, 9.0])], 1)
    rnd, _ = synthetic.resample(y, s, 1, seed=5, subset=False)
    Y = [np.concatenate([np.asarray(a, np.float64)[None, :], b]) for a, b in zip(y, rnd)]
    obj = markov.MarkovObjective(t, y, s, "OU")
    out = fit.realisation_refits(obj, cand, Y, iterations=25, seed=3, probabilities=_softmax)
    assert out.loglikel.shape == (2, 4) and out.alpha.shape == (2, 4, 2) and out.rho.shape == (2, 4) and out.start_loglikel is None
    calls = 0
    for r in range(2):
        yr = [a[r] for a in Y]
        res = fit.gpcc_grid(t, yr, s, kernel="OU", candidatedelays=cand, iterations=25, seed=3, engine="python", solver="markov",
                            objective=markov.MarkovObjective(t, yr, s, "OU"))
        assert np.array_equal(out.loglikel[r], res.loglikel) and np.array_equal(out.alpha[r], res.alpha)
        assert np.array_equal(out.rho[r], res.rho)
        calls += res.f_calls
    assert out.f_calls == calls
    assert np.array_equal(out.delays.prob[1], _softmax(out.loglikel[1]))
    assert out.delays.mean_delay.shape == (2, 2) and out.delays.map_index.shape == (2,)


def test_refits_from_a_warm_start():
    t, y, s = _readme()
    cand = np.stack([np.zeros(3), np.array([1.0, 2.0, 6.0])], 1)
    Y, counts = synthetic.resample(y, s, 3, seed=9)
    obj = markov.MarkovObjective(t, y, s, "matern32")
    a0, r0 = np.tile([np.var(y[0], ddof=1), np.var(y[1], ddof=1)], (3, 1)), np.array([3.5, 3.5, 25.0])     # (25: clipped into the range)
    out = fit.realisation_refits(obj, cand, Y, counts, iterations=12, start=(a0, r0), probabilities=_softmax)
    assert out.loglikel.shape == (3, 3) and np.isfinite(out.loglikel).all()
    assert (out.loglikel >= out.start_loglikel).all() and (out.loglikel > out.start_loglikel).any()
    assert (out.rho > 0.1).all() and (out.rho < 20.0).all() and (out.alpha > 0).all()
    # the start as given, and the returned optimum, evaluated afresh
    real = np.repeat(np.arange(3), 3)
    at, info = obj.loglik_markov_resampled(Y, np.tile(cand, (3, 1)), np.tile(a0, (3, 1)), np.tile(np.minimum(r0, 20.0 - 1e-6), 3), real,
                                           counts=counts)
    assert (info == 0).all()
    ok = np.tile(r0 < 20.0, 3)
    assert np.all(np.abs(at - out.start_loglikel.reshape(-1))[ok] <= 1e-9 * np.abs(at[ok]))
    again, info = obj.loglik_markov_resampled(Y, np.tile(cand, (3, 1)), out.alpha.reshape(-1, 2), out.rho.reshape(-1), real, counts=counts)
    assert (info == 0).all() and np.array_equal(again.reshape(3, 3), out.loglikel)


def test_value_errors():
    t, y, s = _readme()
    Y, counts = synthetic.resample(y, s, 2, seed=1)
    obj = markov.MarkovObjective(t, y, s, "OU")
    d, a, rh = [[0.0, 1.0]] * 2, [[1.0, 1.0]] * 2, [2.0, 2.0]
    ll, info = obj.loglik_markov_resampled(Y, d, a, rh, [0, 1], counts=counts)
    assert (info == 0).all() and np.isfinite(ll).all()
    for real in ([0, 2], [-1, 0], [0]):
        with pytest.raises(ValueError):
            obj.loglik_markov_resampled(Y, d, a, rh, real, counts=counts)
    bad = [c.copy() for c in counts]
    bad[1][0, 3] = -1
    with pytest.raises(ValueError):
        obj.loglik_markov_resampled(Y, d, a, rh, [0, 1], counts=bad)
    one = [c.copy() for c in counts]
    one[0][1, :] = 0
    one[0][1, 5] = 55
    with pytest.raises(ValueError):
        obj.loglik_markov_resampled(Y, d, a, rh, [0, 1], counts=one)              # a band with one distinct point, marginalise_b
    ll2, info2 = obj.loglik_markov_resampled(Y, d, a, rh, [0, 1], counts=one, sigma_b="handle")
    assert (info2 == 0).all() and ll2[0] != ll[0] and np.isfinite(ll2).all()
    free = markov.MarkovObjective(t, y, s, "OU", marginalise_b=False)
    assert np.isfinite(free.loglik_markov_resampled(Y, d, a, rh, [0, 1], counts=one)[0]).all()
    with pytest.raises(ValueError):
        obj.loglik_markov_resampled(Y, d, a, rh, [0, 1], counts=counts, center="median")
    with pytest.raises(ValueError):
        obj.loglik_markov_resampled(Y, d, a, rh, [0, 1], counts=counts, sigma_b=np.ones((3, 2)))
