"""gpcc_sample_noise_markov_batch on the device: the draws against the extended-precision reference on each row's
effective error bars (tests/_markov_noise_sample_cases.py: the plain reference and its own bar, nothing of it from the noise mirror or
the device) on all 72 cases and on the edge shapes; bitwise gpcc_sample_markov_batch at kappa = 1, nu = 0 in every shipped <P, NOFF>,
both modes; loglik and info bitwise the noise predictions'; info = -3; draws that do not depend on M, the row order, the chunking or
the launch shape; the finish tiles; the unstaged path; mutations of the device's own output; memory.  Each group prints its worst
error / bar in a line that starts with "noise-sample" (profiles/markov/noise_sample_parity.log keeps them)."""
import numpy as np
import pytest

import _markov_cases as MC
import _markov_noise_sample_cases as C
import _markov_predict_cases as PC
import _sample_highprec as SH
import gpcc_amd
import test_gpu_markov_sample as TM
import test_gpu_sample_highprec as GS
from gpcc_amd import fit, rng

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not SH.EXTENDED, reason=SH.SKIP_REASON)

KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
NOT_DRAWN = -14
CASES = C.cases()
NOISE_LANE_BYTES = 16                      # csrc: GPCC_MARKOV_NOISE_LANE_BYTES, beside GPCC_MKP_LANE_BYTES


def _device(entry, n, seed, mixture):
    """n draws of the one row of an entry, per-row counters (row word 0) or mixture counters."""
    (cid, k, data, delays, alpha, rho, mb, tests), kappa, nu = entry
    kw = dict(weights=[1.0]) if mixture else {}
    with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
        dr, rows, ll, info = obj.sample_markov_noise_batch([delays], [alpha], [rho], kappa, nu, tests[0], n, seed, sigmatest=tests[2], **kw)
    assert info[0] == 0 and dr.shape == (n, sum(len(a) for a in tests[0])) and (rows == 0).all(), cid
    return dr


def _compare(oracle, rows, group):
    """rows: [(entry, seed, mixture)]."""
    worst = SH.Worst("noise-sample device draws " + group)
    for entry, seed, mixture in rows:
        ref = C.reference(oracle, entry, seed, C.S, rng.MIXROW if mixture else 0)
        r = ref.ratio(_device(entry, C.S, seed, mixture))
        print("noise draws %s: error / bar %.3g (bar %.3g of which the normals term %.3g)" % (entry[0][0], r, float(np.max(ref.bar)),
                                                                                           float(np.max(ref.bar)) - ref.base))
        worst.add(r, entry[0][0])
    SH.report([worst])


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------
@extended
@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_parity_cases(oracle, kernel, L):
    print("build: %s" % gpcc_amd.build_info())
    mine = [i for i, e in enumerate(CASES) if e[0][1] == kernel and len(e[1]) == L]
    assert len(mine) == 8
    _compare(oracle, [(CASES[i], C.seed_of(i), bool(i % 2)) for i in mine], "%s L = %d" % (kernel, L))


def _with_noise(case, seed):
    rg = np.random.default_rng(seed)
    L = len(case[4])
    return (case, rg.uniform(0.5, 2.0, L), rg.uniform(0.0, 0.05, L))


@extended
def test_parity_edge_shapes(oracle):
    """N = 2; L = 8 without offsets; Matern-5/2 with 4 marginalised offsets (<3, 4>); a band with a tie inside it and a test point on a
    training point (_sample_highprec.branch_band, which also has lags on either side of the process-noise branch)."""
    shapes = [("matern32", [1, 1], [1, 0], False), ("matern52", [3, 4, 2, 3, 4, 2, 3, 2], [1, 0, 1, 1, 0, 1, 1, 1], False),
              ("matern52", [5, 4, 6, 3], [2, 1, 2, 1], True)]
    rows = [(_with_noise(TM._tiny(k, Nl, Nt, mb, seed=sum(Nl) + len(Nl)), i), 41, bool(i % 2)) for i, (k, Nl, Nt, mb) in enumerate(shapes)]
    band, _ = SH.branch_band("matern32", 3.0, True)
    t, tt = band[2][0][0], band[7][0][0]
    assert len(np.unique(t)) < len(t) and np.isin(tt, t).any()            # the tie, the test point on a training point
    rows.append((_with_noise(band, 9), 77, False))
    latent = (band[0] + "-asked-latent",) + band[1:7] + ((band[7][0], None, None),)
    rows.append((_with_noise(latent, 10), 78, True))
    _compare(oracle, rows, "edge shapes")


# ---- 2. bitwise at kappa = 1, nu = 0 -------------------------------------------------------------------------------------------------
def _eq(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("noff", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_unit_noise_is_bitwise_the_plain_entry(kernel, noff):
    """<P, NOFF> = <order of the kernel, noff>: 21 rows, failing ones (alpha <= 0, rho <= 0, rho NaN) among them, with and without
    sigmatest; per-row and mixture modes; kappa / nu as explicit arrays, None and (L,) broadcast.  draws, draw_row, loglik and info."""
    Nl = [13, 11, 9, 8][:noff] if noff else [13, 11]
    L, M, mb = len(Nl), 21, noff > 0
    t, y, s, d0 = MC.lightcurves(Nl, seed=40 + noff, kind="ties" if L > 1 else "plain")
    tt, _, st = PC.test_points(t, d0, 50 + noff, -1)
    delays, alpha, rho = TM._batch(L, M, seed=noff)
    delays[0] = d0
    alpha[5, L - 1] = 0.0
    rho[9] = -1.0
    rho[14] = np.nan
    w = np.random.default_rng(3).uniform(0.1, 1.0, M)
    w[3] = 0.0
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        for sig in (st, None):
            per = obj.sample_markov_batch(delays, alpha, rho, tt, 2, 31, sigmatest=sig)
            mix = obj.sample_markov_batch(delays, alpha, rho, tt, 70, 31, weights=w, sigmatest=sig)
            assert list(per[3][[5, 9]]) == [-1, -2] and per[3][14] != 0 and np.count_nonzero(per[3]) == 3 and mix[3][3] == NOT_DRAWN
            assert np.isfinite(per[0][:10]).all() and np.isnan(per[0][10:12]).all()
            for kappa, nu in ((np.ones((M, L)), np.zeros((M, L))), (None, None), (np.ones(L), None), (None, np.zeros(L))):
                assert _eq(obj.sample_markov_noise_batch(delays, alpha, rho, kappa, nu, tt, 2, 31, sigmatest=sig), per), (kernel, noff)
                assert _eq(obj.sample_markov_noise_batch(delays, alpha, rho, kappa, nu, tt, 70, 31, sigmatest=sig, weights=w), mix), (kernel, noff)


# ---- 3. loglik, info -----------------------------------------------------------------------------------------------------------------
def _noisy_batch(M, L, seed):
    rg = np.random.default_rng(seed)
    delays, alpha, rho = TM._batch(L, M, seed)
    rho = np.exp(rg.uniform(np.log(0.5), np.log(30.0), M))
    return delays, alpha, rho, rg.uniform(0.0, 2.0, (M, L)), rg.uniform(0.001, 0.05, (M, L))


def test_loglik_info_and_minus_three():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=11, kind="ties")
    tt, _, st = PC.test_points(t, d0, 12, -1)
    M, L, S = 9, 2, 3
    d, a, r, kappa, nu = _noisy_batch(M, L, 5)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        good = obj.sample_markov_noise_batch(d, a, r, kappa, nu, tt, S, 8, sigmatest=st)
        pred = obj.predict_markov_noise_batch(d, a, r, tt, kappa, nu)
        assert (good[3] == 0).all() and np.isfinite(good[0]).all()
        assert np.array_equal(good[2], pred[2]) and np.array_equal(good[3], pred[3])            # the same tap launch
        assert np.array_equal(good[1], np.repeat(np.arange(M), S))
        plain = obj.sample_markov_batch(d, a, r, tt, S, 8, sigmatest=st)
        assert np.array_equal(good[1], plain[1]) and not np.array_equal(good[0], plain[0])      # another model, the same rows
        a2, r2, k2, v2 = a.copy(), r.copy(), kappa.copy(), nu.copy()
        a2[1, 0], k2[1, 1] = 0.0, -1.0      # -1 before -3
        r2[2], v2[2, 0] = 0.0, -0.5         # -2 before -3
        k2[3, 0] = -1e-300
        v2[4, 1] = np.nan
        k2[5, 1] = np.inf
        v2[6, 0] = -1e-300
        want = np.array([0, -1, -2, -3, -3, -3, -3, 0, 0])
        bad = want != 0
        dr, rows, ll, info = obj.sample_markov_noise_batch(d, a2, r2, k2, v2, tt, S, 8, sigmatest=st)
        p2 = obj.predict_markov_noise_batch(d, a2, r2, tt, k2, v2)
        assert list(info) == list(want) and np.array_equal(info, p2[3]) and np.array_equal(ll, p2[2], equal_nan=True)
        lanes = np.repeat(bad, S)
        assert np.isnan(dr[lanes]).all() and np.isnan(ll[bad]).all()
        assert np.array_equal(dr[~lanes], good[0][~lanes]) and np.array_equal(ll[~bad], good[2][~bad])     # the neighbours keep their bits
        # the mixture: a -3 row with weight makes its own draws NaN, with weight 0 it is never evaluated
        w = np.ones(M)
        mixed = obj.sample_markov_noise_batch(d, a2, r2, k2, v2, tt, 60, 8, sigmatest=st, weights=w)
        clean = obj.sample_markov_noise_batch(d, a, r, kappa, nu, tt, 60, 8, sigmatest=st, weights=w)
        assert np.array_equal(mixed[1], clean[1]) and np.array_equal(mixed[1], rng.pick_rows(8, 60, w))
        hit = bad[mixed[1]]
        assert hit.any() and np.isnan(mixed[0][hit]).all() and np.array_equal(mixed[0][~hit], clean[0][~hit])
        w0 = np.where(bad, 0.0, 1.0)
        skipped = obj.sample_markov_noise_batch(d, a2, r2, k2, v2, tt, 60, 8, sigmatest=st, weights=w0)
        assert (skipped[3][bad] == NOT_DRAWN).all() and np.isnan(skipped[2][bad]).all() and np.isfinite(skipped[0]).all()
        assert _eq(skipped, obj.sample_markov_noise_batch(d, a, r, kappa, nu, tt, 60, 8, sigmatest=st, weights=w0))
        with pytest.raises(ValueError):
            obj.sample_markov_noise_batch(d, a, r, np.ones((M, L + 1)), None, tt, S, 8)
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.sample_markov_noise_batch(d, a, r, kappa, nu, tt, 0, 8)
        assert ei.value.code == -1
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.sample_markov_noise_batch(d, a, r, kappa, nu, tt, S, 8)
        assert ei.value.code == -3 and "gpcc_sample_noise_markov_batch" in ei.value.message


# ---- 4. independence -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,Nl,mb", [("matern52", [30, 20, 27], True), ("OU", [60, 50], False)])
def test_draws_do_not_depend_on_the_batch(kernel, Nl, mb):
    t, y, s, d0 = MC.lightcurves(Nl, seed=7, kind="ties")
    L, M, S, seed = len(Nl), 5, 30, 99
    tt, _, st = PC.test_points(t, d0, 8, -1)
    d, a, r, kappa, nu = _noisy_batch(M, L, L)
    rev = slice(None, None, -1)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb) as obj:
        full = obj.sample_markov_noise_batch(d, a, r, kappa, nu, tt, S, seed, sigmatest=st)
        assert (full[3] == 0).all() and np.isfinite(full[0]).all()
        one = obj.sample_markov_noise_batch(d[:1], a[:1], r[:1], kappa[:1], nu[:1], tt, S, seed, sigmatest=st)           # M = 1 vs M = 5
        assert np.array_equal(one[0], full[0][:S]) and one[2][0] == full[2][0]
        # the row order: mixture counters carry no row word, so draw s is the draw s of a one-row mixture call on the parameters of the
        # row it fell on -- rows with different noise models among them -- whatever the order of the rows
        w = np.array([0.3, 0.0, 0.2, 0.4, 0.1])
        mix = obj.sample_markov_noise_batch(d, a, r, kappa, nu, tt, 150, seed, sigmatest=st, weights=w)
        back = obj.sample_markov_noise_batch(d[rev], a[rev], r[rev], kappa[rev], nu[rev], tt, 150, seed, sigmatest=st, weights=w[rev])
        assert np.array_equal(mix[1], rng.pick_rows(seed, 150, w)) and np.array_equal(back[1], rng.pick_rows(seed, 150, w[rev]))
        assert set(mix[1]) == {0, 2, 3, 4} and mix[3][1] == NOT_DRAWN and back[3][3] == NOT_DRAWN
        for m in (0, 2, 3, 4):
            alone = obj.sample_markov_noise_batch(d[m:m + 1], a[m:m + 1], r[m:m + 1], kappa[m:m + 1], nu[m:m + 1], tt, 150, seed,
                                                  sigmatest=st, weights=[1.0])
            for got, sel in ((mix, mix[1] == m), (back, back[1] == M - 1 - m)):
                assert sel.sum() > 5 and np.array_equal(alone[0][sel], got[0][sel]), m
            assert alone[2][0] == mix[2][m] == back[2][M - 1 - m]
        try:
            for rows_opt, draws_opt in ((1, 0), (0, 64), (1, 64)):
                obj.set_option("markov_chunk_rows", rows_opt)
                obj.set_option("markov_sample_chunk_draws", draws_opt)
                assert _eq(obj.sample_markov_noise_batch(d, a, r, kappa, nu, tt, S, seed, sigmatest=st), full), (rows_opt, draws_opt)
                assert _eq(obj.sample_markov_noise_batch(d, a, r, kappa, nu, tt, 150, seed, sigmatest=st, weights=w), mix), (rows_opt, draws_opt)
        finally:
            obj.set_option("markov_chunk_rows", 0)
            obj.set_option("markov_sample_chunk_draws", 0)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, precision="fp32") as o32:      # an fp32 handle, on its fp64 twin
        assert _eq(o32.sample_markov_noise_batch(d, a, r, kappa, nu, tt, S, seed, sigmatest=st), full)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb, devices=[0, 0]) as om:
        assert _eq(om.sample_markov_noise_batch(d, a, r, kappa, nu, tt, S, seed, sigmatest=st), full)


# ---- 5. the finish tiles ---------------------------------------------------------------------------------------------------------------
@extended
@pytest.mark.parametrize("T", [1, 63, 64, 65])
def test_finish_tiles(oracle, T):
    t, y, s, delays = MC.lightcurves([12, 9], seed=64, kind="ties")
    rg = np.random.default_rng(T)
    Nt = [T - T // 3, T // 3]
    tt = [MC.snap(rg.uniform(-2.0, 32.0, n)) for n in Nt]
    st = [0.2 + 0.05 * rg.random(n) for n in Nt]
    entry = (("finish-T%d" % T, "matern32", (t, y, s), delays, np.array([1.2, 0.8]), 3.0, True, (tt, None, st)), np.array([1.6, 0.7]),
             np.array([0.02, 0.0]))
    ref = C.reference(oracle, entry, 65, 65, 0)
    worst = SH.Worst("noise-sample device draws finish tiles T = %d, lanes 1 / 63 / 64 / 65" % T)
    for n in (1, 63, 64, 65):
        dr = _device(entry, n, 65, False)
        worst.add(float(np.max(SH.err(dr, ref.draws[:n]) / ref.bar[:n])), n)
    SH.report([worst])


# ---- 6. the unstaged path --------------------------------------------------------------------------------------------------------------
def test_unstaged_draws_are_the_staged_ones():
    """test_gpu_sample_highprec's geometry (L = 8 without offsets, N + T = 6496) under this kernel's LDS: 20 (N + T) + 8 + (40 + 16) L
    threads is 158 600 <= 156 KiB for one wave and 187 272 for two.  64 draws are one wave per workgroup: staged.  64 CUs' worth of waves
    plus one, in one chunk, are two waves per workgroup: unstaged.  The first 64 draws of both calls are the same bits."""
    import torch
    (t, y, s), tt, st, delays, alpha, rho = GS._unstaged_problem()
    N, T, L = sum(map(len, t)), sum(map(len, tt)), len(t)
    fits = lambda threads: GS.POINT_BYTES * (N + T) + 8 + (GS.LANE_BYTES + NOISE_LANE_BYTES) * L * threads <= GS.LDS_MAX     # noqa: E731
    assert fits(64) and not fits(128)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lanes = 64 * cus + 64
    assert 8 * (N + T) * ((lanes + 255) // 256 * 256) < 2 ** 30
    rg = np.random.default_rng(8)
    kappa, nu = rg.uniform(0.5, 2.0, L), rg.uniform(0.0, 0.02, L)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32, marginalise_b=False) as obj:
        few = obj.sample_markov_noise_batch([delays], [alpha], [rho], kappa, nu, tt, 64, 19, sigmatest=st)
        obj.set_option("markov_sample_chunk_draws", lanes)
        many = obj.sample_markov_noise_batch([delays], [alpha], [rho], kappa, nu, tt, lanes, 19, sigmatest=st)
        obj.set_option("markov_sample_chunk_draws", 0)
    assert few[3][0] == 0 and many[3][0] == 0 and few[2][0] == many[2][0]
    assert few[0].shape == (64, T) and many[0].shape == (lanes, T) and np.isfinite(many[0]).all()
    differ = int(np.sum(few[0] != many[0][:64]))
    print("noise-sample unstaged (%d lanes, two waves per workgroup) against staged (64 lanes): %d of %d values differ" % (lanes, differ, 64 * T))
    assert differ == 0


# ---- 7. mutations ------------------------------------------------------------------------------------------------------------------------
@extended
def test_mutations_miss_the_bar(oracle):
    """On the device's own output at the Matern-3/2 cases with two bands and test noise (both b-modes, rho = 0.1 and 20): draw s against
    the reference of draw s + 1; and the draw as it would be with the test noise left unmapped -- the difference of the two references
    (sigmatest raw against mapped, the training error bars effective in both) added to the device's draw."""
    picked = [i for i, e in enumerate(CASES) if e[0][1] == "matern32" and len(e[1]) == 2 and i % 2 == 0]
    assert len(picked) == 4
    low = {"next draw": np.inf, "test noise unmapped": np.inf}
    for idx in picked:
        entry = CASES[idx]
        ref = C.reference(oracle, entry, C.seed_of(idx), C.S + 1, C.word_of(idx))
        dr = _device(entry, C.S, C.seed_of(idx), bool(idx % 2))
        assert float(np.max(SH.err(dr, ref.draws[:C.S]) / ref.bar[:C.S])) <= 1.0
        low["next draw"] = min(low["next draw"], float(np.max(SH.err(dr, ref.draws[1:]) / ref.bar[1:])))
        (cid, k, data, delays, alpha, rho, mb, tests), kappa, nu = entry
        eff = C.restated(entry)
        raw = (eff[0] + "-raw-sigmatest",) + eff[1:7] + (tests,)
        other = SH.linear_reference(oracle, raw, C.seed_of(idx), C.S + 1, C.word_of(idx))
        shifted = dr + (other.draws[:C.S] - ref.draws[:C.S]).astype(np.float64)
        low["test noise unmapped"] = min(low["test noise unmapped"], float(np.max(SH.err(shifted, ref.draws[:C.S]) / ref.bar[:C.S])))
    for name, v in low.items():
        print("noise-sample mutation %s: smallest error / bar %.3g" % (name, v))
    assert all(v > 1.0 for v in low.values()), low


# ---- 8. the predictors -------------------------------------------------------------------------------------------------------------------
def test_predictors_sample_under_a_noise_model():
    t, y, s, d0 = MC.lightcurves([60, 50], seed=13, kind="plain")
    cand = np.stack([np.zeros(3), d0[1] + np.array([-0.5, 0.0, 0.5])], 1)
    alpha, rho, w = np.tile([1.0, 0.8], (3, 1)), np.array([2.0, 3.0, 4.0]), np.array([0.2, 0.5, 0.3])
    kappa, nu = np.array([[1.2, 0.8], [1.5, 1.0], [0.9, 1.1]]), np.array([[0.01, 0.0], [0.02, 0.01], [0.0, 0.03]])
    grid = np.linspace(-1.0, 31.0, 9)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        pred = fit.Predictor(obj, cand[1], alpha[1], rho[1], solver="markov", kappa=kappa[1], nu=nu[1])
        bands = pred.sample(grid, 4, 11, solver="markov")
        raw = obj.sample_markov_noise_batch(cand[1:2], alpha[1:2], rho[1:2], kappa[1:2], nu[1:2], [grid, grid], 4, 11)[0]
        assert [b.shape for b in bands] == [(4, 9), (4, 9)] and np.array_equal(np.concatenate(bands, 1), raw)
        with pytest.raises(NotImplementedError, match="effective_std"):
            pred.sample(grid, 4, 11)
        nf = fit.NoiseGridFit(np.log(w), alpha, rho, kappa, nu, 0, 0, None)
        avg = fit.noise_predictor(obj, cand, nf, weights=w)
        mb, rows = avg.sample(grid, 50, 12, solver="markov")
        plain_rows = fit.DelayAveragedPredictor(obj, cand, alpha, rho, w, solver="markov").sample(grid, 50, 12, solver="markov")[1]
        assert np.array_equal(rows, plain_rows) and all(np.isfinite(b).all() and b.shape == (50, 9) for b in mb)
        direct = obj.sample_markov_noise_batch(cand, alpha, rho, kappa, nu, [grid, grid], 50, 12, weights=w)
        assert np.array_equal(np.concatenate(mb, 1), direct[0]) and np.array_equal(rows, direct[1])


# ---- 9. memory -------------------------------------------------------------------------------------------------------------------------
def test_memory_at_16384():
    """test_gpu_markov_sample.test_memory_at_16384 under a noise model, the first call of a handle: the plain entry's documented buffers
    plus 16 L bytes for kappa | nu of the one drawn row, and none of the N^2 workspace."""
    import torch
    rg = np.random.default_rng(16384)
    Nl = [8192, 8192]
    t = [np.sort(MC.snap(rg.uniform(0.0, 2000.0, n))) for n in Nl]
    y = [np.sin(0.05 * a) + 0.1 * rg.standard_normal(len(a)) for a in t]
    s = [0.1 + 0.05 * rg.random(len(a)) for a in t]
    tt = [MC.snap(rg.uniform(0.0, 2000.0, 64)) for _ in range(2)]
    N, T, S, n, L = 16384, 128, 64, 5, 2
    kappa, nu = [[1.4, 0.8]], [[0.002, 0.0]]
    torch.cuda.synchronize()
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        free0, _ = torch.cuda.mem_get_info(0)
        dr, _, ll, info = obj.sample_markov_noise_batch([[0.0, 3.0]], [[1.0, 0.9]], [20.0], kappa, nu, tt, S, 7)
        free1, _ = torch.cuda.mem_get_info(0)
        assert obj.get_option("workspace_slots") == obj.get_option("slots_per_stream")     # (never built)
        ints = 4 * (N + 3 * S + 1)
        assert obj.get_option("markov_sample_bytes") == 16 * T * n + 8 * (N + T) * 256 + ints
        pll = obj.predict_markov_noise_batch([[0.0, 3.0]], [[1.0, 0.9]], [20.0], tt, kappa, nu)[2]
    documented = 16 * T * (n + n * (n + 1) // 2) + 16 * T * n + 16 * T + 8 * (N + T) * 256 + 8 * S * T + ints + 24 * N + 16 * L
    print("noise-sample N = 16384: %.2f MiB of growth (documented buffers %.2f MiB)" % ((free0 - free1) / 2.0 ** 20, documented / 2.0 ** 20))
    assert info[0] == 0 and np.isfinite(dr).all() and dr.shape == (S, T) and ll[0] == pll[0]
    assert free0 - free1 < documented + 4 * 2 ** 20       # (test_gpu_markov_predict.py's allowance for the allocator and the staging)
