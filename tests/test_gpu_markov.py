"""gpcc_loglik_markov_batch on the device: parity with the extended-precision reference over the CPU cases of tests/_markov_cases.py
and with the dense references at N = 2048, 4095 and 4096 (bar: tests/_markov_cases.py, measured on the reference side; the worst
error / bar of each group is printed); bitwise invariance over batch sizes, row order and handle flavours; refusals and failures;
the fit with solver="markov"; the memory of a handle that only ever calls this entry."""
import numpy as np
import pytest

import _grad_highprec as H
import _markov_cases as MC
import gpcc_amd
from gpcc_amd import _capi, fit, markov, synthetic

pytestmark = pytest.mark.gpu

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
UNSUPPORTED = -3


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_parity_cpu_cases(oracle, kernel):
    worst = {N: MC.Worst("device parity %s N = %d" % (kernel, N)) for N in MC.SHAPES}
    n = 0
    for case in MC.cpu_cases():
        cid, k, data, delays, alpha, rho, mb, N = case
        if k != kernel:
            continue
        n += 1
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll, info = obj.loglik_markov_batch(delays[None, :], alpha[None, :], [rho])
        assert info[0] == 0, cid
        ref, b, _ = MC.reference_and_bar(oracle, case)
        worst[N].add(abs(ll[0] - ref) / abs(ref), b, cid)
        host, _ = markov.loglik(k, *data, delays, alpha, rho, mb)        # the numpy mirror: the same algorithm, another rounding order
        assert abs(ll[0] - host) <= 2 * b * abs(ref), cid
    assert n == 3 * 3 * 2 * len(MC.RHOS)
    for w in worst.values():
        w.report()


LARGE = {2048: ("OU", [1024, 1024]), 4095: ("matern32", [1500, 1300, 1295]), 4096: ("matern52", [2048, 2048])}


@pytest.mark.parametrize("N", sorted(LARGE))
def test_parity_large(oracle, N):
    """A 64-delay grid against oracle.loglik_batch; per delay, e_dense = the disagreement of the oracle with oracle/lapack_baseline.py."""
    kernel, Nl = LARGE[N]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=N)
    L = len(Nl)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    G = 64
    delays = np.zeros((G, L))
    delays[:, 1:] = np.linspace(0.0, 12.6, G)[:, None] * (1.0 + 0.5 * np.arange(L - 1))[None, :]
    alpha = np.tile(alpha0, (G, 1))
    rho = np.full(G, rho0)
    with gpcc_amd.Objective(t, y, s, KERN[kernel]) as obj:
        ll, info = obj.loglik_markov_batch(delays, alpha, rho)
    ref, rinfo = oracle.loglik_batch(kernel, t, y, s, delays, alpha, rho, True, nthreads=16)
    assert (info == 0).all() and (rinfo == 0).all()
    worst = MC.Worst("device parity %s N = %d, 64 delays" % (kernel, N))
    F = MC.factor(alpha0, s)
    for g in range(G):
        e = MC.dense_pair_error(kernel, (t, y, s), delays[g], alpha[g], rho[g], True, ref[g])
        worst.add(abs(ll[g] - ref[g]) / abs(ref[g]), MC.bar(e, N, F) + e, g)
    worst.report()


def _batch(L, M, seed):
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), rg.uniform(-3.0, 45.0, (M, L - 1))], 1)
    return delays, rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))


@pytest.mark.parametrize("kernel,Nl,mb", [("matern52", [300, 200, 267], True), ("OU", [60, 50], False), ("matern32", [2048, 2048], True)])
def test_bitwise_invariance(kernel, Nl, mb):
    t, y, s, _ = MC.lightcurves(Nl, seed=7, kind="ties")
    L = len(Nl)
    delays, alpha, rho = _batch(L, 1024, seed=len(Nl))
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        full, info = obj.loglik_markov_batch(delays, alpha, rho)
        assert (info == 0).all() and np.isfinite(full).all()
        for M in (1, 63, 64, 65):
            ll, inf = obj.loglik_markov_batch(delays[:M], alpha[:M], rho[:M])
            assert np.array_equal(ll, full[:M]) and (inf == 0).all(), M
        perm = np.random.default_rng(1).permutation(1024)
        ll, _ = obj.loglik_markov_batch(delays[perm], alpha[perm], rho[perm])
        assert np.array_equal(ll, full[perm])
        for key, val in (("streams", 1), ("slots_per_stream", 8), ("small_n", 0), ("chain_max", 0)):
            obj.set_option(key, val)
        ll, _ = obj.loglik_markov_batch(delays[:65], alpha[:65], rho[:65])
        assert np.array_equal(ll, full[:65])
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, precision="fp32") as o32:
        ll, inf = o32.loglik_markov_batch(delays[:65], alpha[:65], rho[:65])
        assert np.array_equal(ll, full[:65]) and (inf == 0).all()
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, devices=[0, 0]) as om:
        ll, inf = om.loglik_markov_batch(delays[:65], alpha[:65], rho[:65])
        assert np.array_equal(ll, full[:65]) and (inf == 0).all()


def test_refusals_and_failures(oracle):
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loglik_markov_batch([d0], [[1.0, 1.0]], [2.0])
        assert ei.value.code == UNSUPPORTED and "rbf" in ei.value.message
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.set_option("fit_markov", 1)
        assert ei.value.code == UNSUPPORTED
    delays, alpha, rho = _batch(2, 8, seed=5)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        good, ginfo = obj.loglik_markov_batch(delays, alpha, rho)
        assert (ginfo == 0).all()
        a2, r2, d2 = alpha.copy(), rho.copy(), delays.copy()
        a2[1, 0] = 0.0
        a2[2, 1] = -1.0
        r2[3] = 0.0
        r2[4] = -2.0
        a2[5, 1] = np.nan
        r2[6] = np.nan
        ll, info = obj.loglik_markov_batch(d2, a2, r2)
        dl, dinfo = obj.loglik_batch(d2, a2, r2)
        bad = [1, 2, 3, 4, 5, 6]
        assert list(info[[1, 2, 3, 4, 5]]) == [-1, -1, -2, -2, -1] and np.array_equal(info[:6], dinfo[:6])
        assert info[6] != 0 and dinfo[6] != 0                      # a NaN rho passes the argument checks and fails at the first pivot
        assert np.isnan(ll[bad]).all() and np.isnan(dl[bad]).all()
        assert np.array_equal(ll[[0, 7]], good[[0, 7]]) and (info[[0, 7]] == 0).all()      # the neighbours are untouched
    # five bands: with marginalised offsets unsupported, without them fine
    t5, y5, s5, d5 = MC.lightcurves([30, 25, 20, 25, 30], seed=12, kind="ties")
    a5 = np.linspace(0.6, 1.4, 5)
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=True) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loglik_markov_batch([d5], [a5], [2.0])
        assert ei.value.code == UNSUPPORTED
        assert obj.loglik_batch([d5], [a5], [2.0])[1][0] == 0      # the handle still serves the dense path
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=False) as obj:
        ll, info = obj.loglik_markov_batch([d5], [a5], [2.0])
        ref, _ = oracle.loglik_batch("OU", t5, y5, s5, [d5], [a5], [2.0], False)
        e = MC.dense_pair_error("OU", (t5, y5, s5), d5, a5, 2.0, False, ref[0])
        assert info[0] == 0 and abs(ll[0] - ref[0]) / abs(ref[0]) <= MC.bar(e, 130, MC.factor(a5, s5)) + e
    # sigma = 0 at two observations that coincide in shifted time: the second one's predictive variance is 0
    t, y, s, d0 = MC.lightcurves([30, 20], seed=5, kind="ties")
    ts = markov.prepare(t, y, s)[0]
    seq = markov.merge_order(ts, d0)
    sh = [ts[b][i] - d0[b] for b, i in seq]
    single = lambda q: np.count_nonzero(t[seq[q][0]] == ts[seq[q][0]][seq[q][1]]) == 1     # (a time that is not repeated inside its band)
    j = next(j for j in range(1, len(seq)) if seq[j][0] != seq[j - 1][0] and sh[j] == sh[j - 1] and single(j) and single(j - 1)
             and (j + 1 == len(seq) or sh[j + 1] != sh[j]) and (j < 2 or sh[j - 2] != sh[j]))
    for b, i in (seq[j - 1], seq[j]):
        s[b][np.where(t[b] == ts[b][i])[0]] = 0.0
    host = markov.loglik("OU", t, y, s, d0, [1.0, 1.0], 2.0, False)
    assert host[1] == j + 1
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU, marginalise_b=False) as obj:
        ll, info = obj.loglik_markov_batch([d0, d0 + [0.0, 0.37]], [[1.0, 1.0]] * 2, [2.0, 2.0])
        assert info[0] == j + 1 and np.isnan(ll[0])
        assert info[1] == 0 and np.isfinite(ll[1])                 # no tie at the other delay: its neighbour is fine


def test_fit_with_markov_solver(oracle):
    t, y, s, _ = synthetic.simulate_lightcurves((55, 55))
    grid = np.arange(0.0, 20.01, 0.2)
    cand = np.stack([np.zeros_like(grid), grid], 1)
    assert len(grid) == 101
    kw = dict(kernel=gpcc_amd.OU, candidatedelays=cand, iterations=100, seed=1, rhomin=0.1, rhomax=20.0)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        plain = obj.grid_loglik(cand, 100, init_params=None, seed=1)
        dense = fit.gpcc_grid(t, y, s, objective=obj, **kw)
        before = obj.get_option("markov_count")
        mk = fit.gpcc_grid(t, y, s, objective=obj, solver="markov", **kw)
        assert obj.get_option("markov_count") > before and obj.get_option("fit_markov") == 0
        again = fit.gpcc_grid(t, y, s, objective=obj, solver="dense", **kw)
        obj.set_option("fit_markov", 0)
        plain2 = obj.grid_loglik(cand, 100, init_params=None, seed=1)
        at_fit, info = obj.loglik_batch(cand, mk.alpha, mk.rho)
    # fit_markov = 0, set or never touched, before or after a markov fit: the same bits
    for a, b in zip(plain[:5], plain2[:5]):
        assert np.array_equal(a, b)
    assert np.array_equal(dense.loglikel, again.loglikel) and np.array_equal(dense.alpha, again.alpha) and np.array_equal(dense.rho, again.rho)
    assert (info == 0).all()
    worst = MC.Worst("markov fit: dense value at the fitted (alpha, rho)")
    for g in range(len(grid)):
        if H.EXTENDED:
            ref = H.evaluate("OU", t, y, s, cand[g], mk.alpha[g], mk.rho[g], True).loglik
            e = abs(at_fit[g] - ref) / abs(ref)
        else:
            e = MC.dense_pair_error("OU", (t, y, s), cand[g], mk.alpha[g], mk.rho[g], True, at_fit[g])
        worst.add(abs(mk.loglikel[g] - at_fit[g]) / abs(at_fit[g]), MC.bar(e, 110, MC.factor(mk.alpha[g], s)) + e, g)
    worst.report()
    assert int(np.argmax(gpcc_amd.getprobabilities(mk.loglikel))) == int(np.argmax(gpcc_amd.getprobabilities(dense.loglikel)))


def test_memory_of_a_markov_only_handle():
    """N = 16384: the handle allocates the sorted light curves and the staging, none of the N^2 workspace; the light curves do not fit
    the LDS here, so this is also the global-memory path against the numpy mirror."""
    import torch
    Nl = [8192, 8192]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=3)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    delays = np.stack([np.zeros(64), np.linspace(0.0, 12.6, 64)], 1)
    alpha, rho = np.tile(alpha0, (64, 1)), np.full(64, rho0)
    torch.cuda.synchronize()
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        free0, _ = torch.cuda.mem_get_info(0)
        ll, info = obj.loglik_markov_batch(delays, alpha, rho)
        ll2, _ = obj.loglik_markov_batch(delays[:3], alpha[:3], rho[:3])
        free1, _ = torch.cuda.mem_get_info(0)
        assert obj.get_option("workspace_slots") == obj.get_option("slots_per_stream")     # (never built)
    print("N = 16384 markov-only handle: %.2f MiB of growth" % ((free0 - free1) / 2.0 ** 20))
    assert free0 - free1 < 4 * 2 ** 20
    assert (info == 0).all() and np.array_equal(ll2, ll[:3])
    for g in (0, 63):
        host, hinfo = markov.loglik("matern52", t, y, s, delays[g], alpha[g], rho[g], True)
        assert hinfo == 0 and abs(ll[g] - host) <= MC.bar(0.0, 16384, MC.factor(alpha0, s)) * abs(host)
