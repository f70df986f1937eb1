"""gpcc_loglik_markov_multi_batch on the device: parity with the dense reference of tests/_markov_realisations_cases.py over its
N = 110 and N = 150 cases and one N = 767 case per kernel (bar: tests/_markov_cases.py's, measured on the reference side, per
realisation; the worst error / bar of each group is printed) and agreement with gpcc_loglik_markov_batch; bitwise invariance of a
cell (m, r) over R, M, orders, chunks, handle flavours and launch shapes; the unstaged path; refusals and failures; memory; the
flux-randomisation error bar of a delay end to end."""
import ctypes

import numpy as np
import pytest

import _markov_cases as MC
import _markov_realisations_cases as RC
import gpcc_amd
from gpcc_amd import _capi, fit, markov, synthetic

pytestmark = pytest.mark.gpu

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
ARGUMENT, UNSUPPORTED = -1, -3
RB = 8                                   # realisations per lane (csrc/gpcc_markov_multi.hip.h; read back in test_block_size)
CASES = RC.cases((110, 150))


def test_block_size():
    t, y, s, _ = MC.lightcurves([30, 20], seed=3, kind="plain")
    for kernel in MC.KERNELS:
        for mb in (True, False):
            with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
                assert obj.get_option("markov_multi_block") == RB


def _parity(oracle, case, worst):
    """One case with R = RB + 1 realisations and both centrings against the dense reference; every other case without marginalise_b
    takes the fresh data set's reference for its own means.  The column of the handle's own y under the handle's means against
    loglik_markov_batch: twice the bar (not bitwise: another statement order)."""
    cid, k, data, delays, alpha, rho, mb, N = case
    R = RB + 1
    Y = RC.realisations(case, R)
    own = RC.own_means(Y)
    with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
        ll_h, info_h = obj.loglik_markov_realisations(Y, delays[None, :], alpha[None, :], [rho], center="handle")
        ll_o, info_o = obj.loglik_markov_realisations(Y, delays[None, :], alpha[None, :], [rho], center="own")
        ll_e, info_e = obj.loglik_markov_realisations(np.concatenate(Y, axis=1), delays[None, :], alpha[None, :], [rho], center=own)
        single, info_s = obj.loglik_markov_batch(delays[None, :], alpha[None, :], [rho])
        handle = obj.constants()[0]
    assert ll_h.shape == ll_o.shape == (1, R) and info_h[0] == 0 and info_o[0] == 0 and info_s[0] == 0, cid
    assert np.array_equal(ll_e, ll_o) and info_e[0] == 0, cid
    refs = RC.general_reference(oracle, case, Y, np.tile(handle, (R, 1)))
    for r, (ref, b, _) in enumerate(refs):
        worst["handle means"].add(abs(ll_h[0, r] - ref) / abs(ref), b, (cid, r))
    assert abs(ll_h[0, 0] - single[0]) <= 2 * refs[0][1] * abs(refs[0][0]), cid
    if not mb and sum(map(ord, cid)) % 2 == 0:
        for r in range(R):
            ref, b, _ = RC.fresh_reference(oracle, case, Y, r, tag="fresh%d-" % R)
            worst["own means, fresh data set"].add(abs(ll_o[0, r] - ref) / abs(ref), b, (cid, r))
    else:
        for r, (ref, b, _) in enumerate(RC.general_reference(oracle, case, Y, own)):
            worst["own means"].add(abs(ll_o[0, r] - ref) / abs(ref), b, (cid, r))


@pytest.mark.parametrize("N", [110, 150])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_parity_cpu_cases(oracle, kernel, N):
    worst = {w: MC.Worst("device %s N = %d, %s" % (kernel, N, w)) for w in ("handle means", "own means", "own means, fresh data set")}
    picked = [c for c in CASES if c[1] == kernel and c[7] == N]
    assert len(picked) == 3 * 2 * len(RC.RHOS)
    for case in picked:
        _parity(oracle, case, worst)
    for w in worst.values():
        assert w.where is not None
        w.report()


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_parity_767(oracle, kernel):
    case = next(c for c in RC.cases((767,)) if c[1] == kernel and len(c[3]) == 3 and c[6] and c[5] == 3.0)
    worst = {w: MC.Worst("device %s N = 767, %s" % (kernel, w)) for w in ("handle means", "own means", "own means, fresh data set")}
    _parity(oracle, case, worst)
    worst["handle means"].report()
    worst["own means"].report()


def test_rescaled_realisations_reach_the_fresh_reference(oracle):
    """marginalise_b: a realisation rescaled to the handle's band means and variances has the handle's Sigma_b."""
    worst = MC.Worst("device, rescaled realisations against the fresh data set (marginalise_b)")
    picked = [c for c in CASES if c[6] and c[5] == 3.0 and c[7] == 110 and len(c[3]) == 2]
    assert len(picked) == 3
    for case in picked:
        cid, k, data, delays, alpha, rho, mb, N = case
        Y = RC.rescale_to(data[1], RC.realisations(case))
        with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
            ll, info = obj.loglik_markov_realisations(Y, delays[None, :], alpha[None, :], [rho], center="own")
        assert info[0] == 0
        for r in range(RC.R):
            ref, b, _ = RC.fresh_reference(oracle, case, Y, r, tag="rescaled")
            worst.add(abs(ll[0, r] - ref) / abs(ref), b, (cid, r))
    worst.report()


def _batch(L, M, seed):
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), rg.uniform(-3.0, 45.0, (M, L - 1))], 1)
    return delays, rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))


@pytest.mark.parametrize("kernel,Nl,mb", [("matern52", [300, 200, 267], True), ("OU", [60, 50], False), ("matern32", [40, 41], True)])
def test_bitwise_invariance_of_a_cell(kernel, Nl, mb):
    """Cell (m, r) does not depend on R, on M, on the order of rows or realisations, on the chunk or on the handle's flavour."""
    t, y, s, _ = MC.lightcurves(Nl, seed=7, kind="ties")
    L, N = len(Nl), sum(Nl)
    M, R = 257, 3 * RB + 2
    delays, alpha, rho = _batch(L, M, seed=L)
    Y = np.concatenate(synthetic.flux_randomise(y, s, R, seed=5), axis=1)
    mean = np.random.default_rng(3).normal(0.0, 0.1, (R, L)) + RC.own_means(np.split(Y, np.cumsum(Nl)[:-1], axis=1))   # an explicit (R, L) array
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        count = obj.get_option("markov_count")
        full, info = obj.loglik_markov_realisations(Y, delays, alpha, rho, center=mean)
        assert obj.get_option("markov_count") == count + M * R
        assert full.shape == (M, R) and (info == 0).all() and np.isfinite(full).all()
        for Rs in (1, RB - 1, RB, RB + 1, 3 * RB + 2):
            ll, inf = obj.loglik_markov_realisations(Y[:Rs], delays, alpha, rho, center=mean[:Rs])
            assert np.array_equal(ll, full[:, :Rs]) and (inf == 0).all(), Rs
        perm = np.random.default_rng(1).permutation(R)
        ll, _ = obj.loglik_markov_realisations(Y[perm], delays, alpha, rho, center=mean[perm])
        assert np.array_equal(ll, full[:, perm])
        sub = perm[:RB + 3]                                                   # a subset in another order: other blocks, other positions
        ll, _ = obj.loglik_markov_realisations(Y[sub], delays, alpha, rho, center=mean[sub])
        assert np.array_equal(ll, full[:, sub])
        for Ms in (1, 63, 64, 65, 257):
            ll, inf = obj.loglik_markov_realisations(Y, delays[:Ms], alpha[:Ms], rho[:Ms], center=mean)
            assert np.array_equal(ll, full[:Ms]) and (inf == 0).all(), Ms
        rows = np.random.default_rng(2).permutation(M)
        ll, _ = obj.loglik_markov_realisations(Y, delays[rows], alpha[rows], rho[rows], center=mean)
        assert np.array_equal(ll, full[rows])
        for chunk in (1, RB, 2 * RB, 2 * RB + 3):                            # 1 block per chunk (1 rounds up to a block), 2 blocks
            obj.set_option("markov_multi_chunk", chunk)
            assert obj.get_option("markov_multi_chunk") == chunk
            ll, _ = obj.loglik_markov_realisations(Y, delays[:65], alpha[:65], rho[:65], center=mean)
            assert np.array_equal(ll, full[:65]), chunk
        obj.set_option("markov_multi_chunk", 0)
        with pytest.raises(gpcc_amd.GpccError):
            obj.set_option("markov_multi_chunk", -1)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, precision="fp32") as o32:
        ll, inf = o32.loglik_markov_realisations(Y, delays[:65], alpha[:65], rho[:65], center=mean)
        assert np.array_equal(ll, full[:65]) and (inf == 0).all()
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, devices=[0, 0]) as om:
        ll, inf = om.loglik_markov_realisations(Y, delays[:65], alpha[:65], rho[:65], center=mean)
        assert np.array_equal(ll, full[:65]) and (inf == 0).all()


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("wpw", [4, 2])
@pytest.mark.parametrize("kernel,Nl,mb", [("matern32", [22, 19], True), ("OU", [15, 13, 12], False)])
def test_cells_do_not_depend_on_the_launch_shape(kernel, Nl, mb, wpw):
    """N = 41 / 40, R = RB + 1 (two lanes per row): a batch that runs four (two) waves per workgroup with a ragged last workgroup,
    bitwise against the same rows in one-wave calls (tests/test_gpu_markov_launch_shapes.py's shapes)."""
    t, y, s, _ = MC.lightcurves(Nl, seed=31 + len(Nl), kind="plain")
    L, C, ny, R = len(Nl), _cus(), 2, RB + 1
    if wpw == 4:
        M = 128 * C + 1
    else:
        blocks = (3 * C // 2) // ny
        blocks -= 1 - blocks % 2
        M = 64 * (blocks - 1) + 1
    waves = (M + 63) // 64 * ny
    assert waves > 2 * C if wpw == 4 else C < waves <= 2 * C, (M, C)
    rg = np.random.default_rng(M)
    delays = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 8.0, (M, L - 1)))], 1)
    alpha, rho = rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))
    alpha[M - 1, L - 1] = -0.5                                               # the last row fails, alone in the last workgroup
    Y = synthetic.flux_randomise(y, s, R, seed=8)
    rpw = 64 * wpw
    nb = (M + rpw - 1) // rpw
    windows = [(0, 64), (M - 65, 64), (M - 1, 1)] + [(k * rpw - 32, 64) for k in sorted({1, nb // 2, nb - 2})]
    assert all(0 <= r0 and r0 + n <= M for r0, n in windows) and nb >= 4 and M % rpw == 1
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        big, info = obj.loglik_markov_realisations(Y, delays, alpha, rho)
        assert info[M - 1] == -1 and (info[:M - 1] == 0).all()
        assert np.isnan(big[M - 1]).all() and np.isfinite(big[:M - 1]).all()
        for r0, n in windows:
            sl = slice(r0, r0 + n)
            small, sinfo = obj.loglik_markov_realisations(Y, delays[sl], alpha[sl], rho[sl])
            assert np.array_equal(big[sl], small, equal_nan=True) and np.array_equal(info[sl], sinfo), (M, r0)


def test_unstaged_path():
    """N = 7000 does not fit the LDS: t and sigma^2 come through the caches too.  Own means, no marginalise_b: each column against
    loglik_markov_batch on a fresh handle of that realisation, both within the smallest bar F N 2^-53 of the value (device against
    device: the dense reference is too slow here)."""
    Nl = [3500, 3500]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=4)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    M, R, N = 64, RB + 1, sum(Nl)
    delays = np.stack([np.zeros(M), np.linspace(0.0, 12.6, M)], 1)
    alpha, rho = np.tile(alpha0, (M, 1)), np.full(M, rho0)
    Y = [np.concatenate([np.asarray(a)[None, :], b]) for a, b in zip(y, synthetic.flux_randomise(y, s, R - 1, seed=6))]
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32, marginalise_b=False) as obj:
        ll, info = obj.loglik_markov_realisations(Y, delays, alpha, rho, center="own")
    assert (info == 0).all() and np.isfinite(ll).all()
    tol = 2 * MC.factor(alpha0, s) * N * 2.0 ** -53
    worst = 0.0
    for r in range(R):
        with gpcc_amd.Objective(t, [a[r] for a in Y], s, gpcc_amd.matern32, marginalise_b=False) as fresh:
            one, finfo = fresh.loglik_markov_batch(delays, alpha, rho)
        assert (finfo == 0).all()
        rel = np.max(np.abs(ll[:, r] - one) / np.abs(one))
        worst = max(worst, rel / tol)
        assert rel <= tol, (r, rel, tol)
    print("unstaged N = 7000: worst disagreement / (2 F N 2^-53) %.3g" % worst)


def _raw(obj, M, delays, alpha, rho, R, Y, mean):
    """The C entry itself (for the arguments the Python wrapper refuses first)."""
    dp = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ll = np.full((max(M, 1), max(R, 1)), -7.0)
    info = np.zeros(max(M, 1), np.int32)
    keep = [np.ascontiguousarray(a, np.float64) for a in (delays, alpha, rho)]
    rc = _capi.load().gpcc_loglik_markov_multi_batch(obj._h, M, dp(keep[0]), dp(keep[1]), dp(keep[2]), R, dp(Y), dp(mean), dp(ll),
                                                     info.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return rc, ll


def test_refusals_and_failures():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="plain")
    Y = np.concatenate(synthetic.flux_randomise(y, s, RB + 2, seed=2), axis=1)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loglik_markov_realisations(Y, [d0], [[1.0, 1.0]], [2.0])
        assert ei.value.code == UNSUPPORTED and "rbf" in ei.value.message
        assert obj.loglik_batch([d0], [[1.0, 1.0]], [2.0])[1][0] == 0            # the handle still serves its other entries
    delays, alpha, rho = _batch(2, 8, seed=5)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        good, ginfo = obj.loglik_markov_realisations(Y, delays, alpha, rho)
        assert (ginfo == 0).all() and np.isfinite(good).all()
        # R = 0 and a NULL Y: argument errors of the C entry; M = 0 returns 0 and touches nothing
        rc, _ = _raw(obj, 8, delays, alpha, rho, 0, Y, None)
        assert rc == ARGUMENT
        rc, _ = _raw(obj, 8, delays, alpha, rho, RB + 2, None, None)
        assert rc == ARGUMENT
        rc, out = _raw(obj, 0, delays, alpha, rho, RB + 2, Y, None)
        assert rc == 0 and (out == -7.0).all()
        rc, out = _raw(obj, 8, delays, alpha, rho, RB + 2, Y, None)          # NULL mean: the handle's band means
        handle, _ = obj.loglik_markov_realisations(Y, delays, alpha, rho, center="handle")
        assert rc == 0 and np.array_equal(out, handle) and not np.array_equal(handle, good)
        with pytest.raises(ValueError):
            obj.loglik_markov_realisations(Y[:, :-1], delays, alpha, rho)
        with pytest.raises(ValueError):
            obj.loglik_markov_realisations(Y, delays, alpha, rho, center="median")
        # failing rows: loglik_markov_batch's codes, NaN in all their R entries, the neighbours bitwise untouched
        a2, r2 = alpha.copy(), rho.copy()
        a2[1, 0] = 0.0
        a2[2, 1] = -1.0
        r2[3] = 0.0
        r2[4] = -2.0
        a2[5, 1] = np.nan
        r2[6] = np.nan
        ll, info = obj.loglik_markov_realisations(Y, delays, a2, r2)
        _, sinfo = obj.loglik_markov_batch(delays, a2, r2)
        assert np.array_equal(info, sinfo) and list(info[[1, 2, 3, 4, 5]]) == [-1, -1, -2, -2, -1] and info[6] != 0
        assert np.isnan(ll[1:7]).all() and np.array_equal(ll[[0, 7]], good[[0, 7]])
        # a flux that is not finite poisons its own column alone
        Yb = Y.copy()
        Yb[2, 17] = np.nan
        Yb[RB, 70] = np.inf
        Yb[RB + 1, 3] = -np.inf
        ll, info = obj.loglik_markov_realisations(Yb, delays, alpha, rho)
        bad = [2, RB, RB + 1]
        ok = [r for r in range(RB + 2) if r not in bad]
        assert (info == 0).all() and np.isnan(ll[:, bad]).all() and np.array_equal(ll[:, ok], good[:, ok])
    # five bands: with marginalised offsets unsupported, without them fine
    t5, y5, s5, d5 = MC.lightcurves([30, 25, 20, 25, 30], seed=12, kind="ties")
    a5 = np.linspace(0.6, 1.4, 5)
    Y5 = synthetic.flux_randomise(y5, s5, 3, seed=1)
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=True) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loglik_markov_realisations(Y5, [d5], [a5], [2.0])
        assert ei.value.code == UNSUPPORTED
        assert obj.loglik_batch([d5], [a5], [2.0])[1][0] == 0
    with gpcc_amd.Objective(t5, y5, s5, gpcc_amd.OU, marginalise_b=False) as obj:
        ll, info = obj.loglik_markov_realisations(Y5, [d5], [a5], [2.0])
        host, hinfo = markov.loglik_realisations("OU", t5, y5, s5, Y5, d5, a5, 2.0, False, mean=RC.own_means(Y5))
        assert info[0] == 0 and hinfo[0] == 0
        assert np.all(np.abs(ll - host) <= 2 * MC.bar(0.0, 130, MC.factor(a5, s5)) * np.abs(host))
    # sigma = 0 at two observations that coincide in shifted time: info = j for the row, whatever the fluxes
    t, y, s, d0 = MC.lightcurves([30, 20], seed=5, kind="ties")
    ts = markov.prepare(t, y, s)[0]
    seq = markov.merge_order(ts, d0)
    sh = [ts[b][i] - d0[b] for b, i in seq]
    single = lambda q: np.count_nonzero(t[seq[q][0]] == ts[seq[q][0]][seq[q][1]]) == 1
    j = next(j for j in range(1, len(seq)) if seq[j][0] != seq[j - 1][0] and sh[j] == sh[j - 1] and single(j) and single(j - 1)
             and (j + 1 == len(seq) or sh[j + 1] != sh[j]) and (j < 2 or sh[j - 2] != sh[j]))
    for b, i in (seq[j - 1], seq[j]):
        s[b][np.where(t[b] == ts[b][i])[0]] = 0.0
    Yz = synthetic.flux_randomise(y, [np.full_like(a, 0.2) for a in s], 3, seed=4)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU, marginalise_b=False) as obj:
        ll, info = obj.loglik_markov_realisations(Yz, [d0, d0 + [0.0, 0.37]], [[1.0, 1.0]] * 2, [2.0, 2.0])
        assert info[0] == j + 1 and np.isnan(ll[0]).all()
        assert info[1] == 0 and np.isfinite(ll[1]).all()


def test_memory_of_a_realisations_only_handle():
    """N = 16384: the handle allocates the sorted light curves, the staging and the chunk's scratch, none of the N^2 workspace;
    markov_multi_bytes reports the scratch."""
    import torch
    Nl = [8192, 8192]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=3)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    M, R, N = 64, RB + 1, sum(Nl)
    delays = np.stack([np.zeros(M), np.linspace(0.0, 12.6, M)], 1)
    alpha, rho = np.tile(alpha0, (M, 1)), np.full(M, rho0)
    Y = synthetic.flux_randomise(y, s, R, seed=2)
    torch.cuda.synchronize()
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        assert obj.get_option("markov_multi_bytes") == 0
        free0, _ = torch.cuda.mem_get_info(0)
        ll, info = obj.loglik_markov_realisations(Y, delays, alpha, rho)
        ll2, _ = obj.loglik_markov_realisations(Y, delays[:3], alpha[:3], rho[:3])
        free1, _ = torch.cuda.mem_get_info(0)
        assert obj.get_option("workspace_slots") == obj.get_option("slots_per_stream")     # (never built)
        scratch = obj.get_option("markov_multi_bytes")
    chunk = 2 * RB                                                           # R = RB + 1 in whole blocks
    assert scratch == 8 * (2 * chunk * N + chunk * 2 + chunk * M) + 4 * N
    print("N = 16384 realisations-only handle: %.2f MiB of growth, %.2f MiB of it scratch" % ((free0 - free1) / 2.0 ** 20, scratch / 2.0 ** 20))
    assert free0 - free1 < scratch + 8 * 2 ** 20                             # (the N^2 workspace would be gigabytes)
    assert (info == 0).all() and np.isfinite(ll).all() and np.array_equal(ll2, ll[:3])
    host, hinfo = markov.loglik_realisations("matern52", t, y, s, [a[:2] for a in Y], delays[63], alpha[63], rho[63], True,
                                             mean=RC.own_means([a[:2] for a in Y]))
    assert hinfo[0] == 0 and np.all(np.abs(ll[63, :2] - host[0]) <= MC.bar(0.0, N, MC.factor(alpha0, s)) * np.abs(host[0]))


def test_flux_randomisation_end_to_end():
    """README-size data with a known delay: the grid fit, R = 200 flux randomisations, the delay posterior of each in one call --
    against the loop it replaces, 200 fresh handles and 200 loglik_markov_batch calls (both within the smallest bar of the value)."""
    t, y, s, true = synthetic.simulate_lightcurves((55, 55))
    grid = np.arange(0.0, 20.01, 0.2)
    cand = np.stack([np.zeros_like(grid), grid], 1)
    assert len(grid) == 101
    R = 200
    rnd = synthetic.flux_randomise(y, s, R, seed=3)
    Y = [np.concatenate([np.asarray(a)[None, :], b]) for a, b in zip(y, rnd)]                 # realisation 0: the unrandomised y
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU, marginalise_b=False) as obj:
        res = fit.gpcc_grid(t, y, s, kernel=gpcc_amd.OU, candidatedelays=cand, iterations=100, seed=1, rhomin=0.1, rhomax=20.0,
                            objective=obj, marginalise_b=False)
        out = fit.realisation_delays(obj, cand, res.alpha, res.rho, Y)
        ll, info = obj.loglik_markov_realisations(Y, cand, res.alpha, res.rho)
    assert out.prob.shape == (R + 1, 101) and out.map_index.shape == (R + 1,) and out.mean_delay.shape == (R + 1, 2)
    assert np.all(np.abs(out.prob.sum(axis=1) - 1.0) <= 1e-12) and (out.prob >= 0).all()
    best = int(np.argmax(gpcc_amd.getprobabilities(res.loglikel)))
    assert out.map_index[0] == best
    assert (info == 0).all()
    worst = 0.0
    for r in range(R + 1):
        with gpcc_amd.Objective(t, [a[r] for a in Y], s, gpcc_amd.OU, marginalise_b=False) as fresh:
            one, finfo = fresh.loglik_markov_batch(cand, res.alpha, res.rho)
        assert (finfo == 0).all()
        tol = 2 * np.array([MC.bar(0.0, 110, MC.factor(res.alpha[g], s)) for g in range(101)])
        rel = np.abs(ll[:, r] - one) / np.abs(one)
        worst = max(worst, float(np.max(rel / tol)))
        assert (rel <= tol).all(), (r, float(np.max(rel / tol)))
        assert np.array_equal(out.prob[r], gpcc_amd.getprobabilities(ll[:, r]))
    scatter = out.mean_delay[1:, 1].std(ddof=1)
    print("flux randomisation, R = 200: delay %.2f (true %.1f), scatter of the posterior-mean delay %.3f; worst disagreement with the "
          "loop / (2 F N 2^-53) %.3g" % (out.mean_delay[0, 1], true[1], scatter, worst))
    assert scatter > 0.0 and np.isfinite(out.mean_delay).all()
    assert (out.mean_delay[:, 1] >= grid[0]).all() and (out.mean_delay[:, 1] <= grid[-1]).all() and (out.mean_delay[:, 0] == 0.0).all()
