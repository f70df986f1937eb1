"""The joint posterior draws on the device -- gpcc_sample_batch and gpcc_sample_markov_batch -- against the extended-precision reference
(tests/_sample_highprec.py), under its bar 16 max(e_witness, e_second, e_blocked, floor) (+ the normals term, linear-time draws):
measured on the CPU, nothing of it from the device, no cond term and no 1e-10 floor (tests/test_sample_highprec_cpu.py shows what it
rejects and what it lets pass).

  normals       sample_batch(return_noise=True) at N = 2, T = 1024, S = 64, per-row and mixture counters: every zeta against the
                longdouble Box-Muller of the same Philox words within the derived nu = 16 2^-53 max(r, 2^-53).  The one place the
                device's log / sqrt / sin / cos are held to a derived bound; gpccrng::normal4_stream, the linear-time draws' source,
                has the same body, which is what their normals term rests on.
  dense draws   the 72 cases of _markov_predict_cases.cpu_cases() (N = 110), 3 draws each, sigmatest given on the even-numbered
                cases and None on the odd ones, per-row and mixture counters alternating; rbf on the L = 2 cases; the device's own
                zeta (held to nu first) is the reference's input.  Tile edges: test_gpu_heldout.GEOMETRY at N in {2, 127, 128, 129,
                385}, OU and matern52, both b-modes, S in {1, 129} (gpcc_sample_tiles takes <= 128 draws per workgroup and
                generates zeta 64 rows at a time).
  linear-time   the same 72 cases, 3 draws each, the same alternations; the four edge shapes of test_gpu_markov_sample.py; one band
                per kernel and rho in {0.1, 3, 300} built for the process-noise branch (_sample_highprec.branch_band: the two fp64
                lags on either side of lambda d = 1, a lag of 2^-10, a tie, a lag of 40); lanes and T in {1, 63, 64, 65}
                (gpcc_markov_draw_finish transposes 64 x 64 tiles).
  unstaged      gpcc_markov_draw with the points in global memory (two waves per workgroup at L = 8, N + T = 6496), without a
                reference: the same draws as the staged launch, bitwise; and one draw against the numpy mirror under a borrowed bar.
  mutations     on the device's own output, per family: draw s against the reference of draw s + 1, and the draw with JITTER taken
                out of the test noise (the reference's difference added), must miss the bar.

References are built once per case and cached.  Every group prints its worst error / bar in a line that starts with "highprec"
before the first assertion; profiles/sample/highprec_parity.log keeps them."""
import numpy as np
import pytest

import _markov_cases as MC
import _sample_highprec as SH
import gpcc_amd
import test_gpu_heldout as TH
import test_gpu_markov_sample as TM
import test_gpu_predict_highprec as GP
from gpcc_amd import markov, rng

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not SH.EXTENDED, reason=SH.SKIP_REASON)]

KERN = {"OU": gpcc_amd.OU, "rbf": gpcc_amd.rbf, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
CASES = SH.cases()
EDGES = (2, 127, 128, 129, 385)
S = 3
_dense = {}


def _word(idx):
    return rng.MIXROW if idx % 2 else 0


def _normals_ratio(z, seed, word):
    """max |zeta - longdouble Box-Muller| / nu of the device's zeta (S, T) of one row."""
    ref, nu = SH.dense_normals(seed, z.shape[1], range(z.shape[0]), word)
    return float(np.max(SH.err(z, ref) / nu))


def test_normals():
    rg = np.random.default_rng(1024)
    data = ([np.array([1.0, 4.5])], [np.array([0.3, -0.2])], [np.array([0.2, 0.25])])
    tt = [np.sort(rg.uniform(0.0, 6.0, 1024))]
    worst = SH.Worst("highprec normals of sample_batch, N = 2, T = 1024, S = 64 (error / nu)")
    with gpcc_amd.Objective(*data, gpcc_amd.OU) as obj:
        for kw, word in ((dict(), 0), (dict(weights=[1.0]), rng.MIXROW)):
            dr, _, _, info, z = obj.sample_batch([[0.0]], [[1.0]], [2.0], tt, 64, 31, return_noise=True, fallback=False, **kw)
            assert info[0] == 0 and z.shape == (64, 1024) and np.isfinite(dr).all()
            worst.add(_normals_ratio(z, 31, word), "per-row" if not word else "mixture")
    SH.report([worst])


# -- dense draws --------------------------------------------------------------------------------------------------------------------
def _dense_case(oracle, idx, kernel=None):
    """(device draws (S, T), Reference, error / nu of the device's zeta, zeta) of case idx (cached)."""
    if (idx, kernel) not in _dense:
        cid, k, data, delays, alpha, rho, mb, tests = CASES[idx]
        kw = dict(weights=[1.0]) if idx % 2 else {}
        with gpcc_amd.Objective(*data, KERN[kernel or k], marginalise_b=mb) as obj:
            dr, _, _, info, z = obj.sample_batch(delays[None, :], alpha[None, :], [rho], tests[0], S, 900 + idx, sigmatest=tests[2],
                                                 return_noise=True, fallback=False, **kw)
        assert info[0] == 0 and dr.shape == z.shape == (S, sum(len(a) for a in tests[0])), cid
        ref = SH.dense_reference(oracle, kernel or k, data, delays, alpha, rho, mb, tests[0], tests[2], z)
        _dense[(idx, kernel)] = (dr, ref, _normals_ratio(z, 900 + idx, _word(idx)), z)
    return _dense[(idx, kernel)]


def _compare_dense(oracle, indices, group, kernel=None):
    worst, wz = SH.Worst("highprec dense draws " + group), SH.Worst("highprec dense draws' zeta (error / nu) " + group)
    for idx in indices:
        dr, ref, rz, _ = _dense_case(oracle, idx, kernel)
        r = ref.ratio(dr)
        print("dense draws %s%s: error / bar %.3g (bar %.3g, old bar %.3g)" % (CASES[idx][0], "" if kernel is None else " as " + kernel, r,
                                                                             ref.bar, ref.old_bar))
        worst.add(r, CASES[idx][0])
        wz.add(rz, CASES[idx][0])
    SH.report([wz, worst])


def _select(kernel, L):
    out = [i for i, c in enumerate(CASES) if c[1] == kernel and len(c[2][0]) == L]
    assert len(out) == 2 * len(MC.RHOS)
    return out


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_cases_dense(oracle, kernel, L):
    _compare_dense(oracle, _select(kernel, L), "%s L = %d" % (kernel, L))


@pytest.mark.parametrize("data_of", MC.KERNELS)
def test_cases_dense_rbf(oracle, data_of):
    _compare_dense(oracle, _select(data_of, 2), "rbf on the L = 2 cases of %s" % data_of, kernel="rbf")


@pytest.mark.parametrize("N", EDGES)
def test_tile_edges_dense(oracle, N):
    """S = 129 and S = 1 of each row: the first draw of both is the same draw (its normals are those of (seed, row, s = 0))."""
    T = sum(TH.GEOMETRY[N][1])
    worst = {n: SH.Worst("highprec dense draws edges N = %d, T = %d, S = %d" % (N, T, n)) for n in (1, 129)}
    wz = SH.Worst("highprec dense draws' zeta (error / nu) edges N = %d, T = %d" % (N, T))
    for name, mb, data, delays, alpha, rho, Nt, seed in GP._edge_rows(TH, N):
        tt, _, st = TH._testset(data[0], data[1], delays, Nt, seed=seed)
        with gpcc_amd.Objective(*data, KERN[name], marginalise_b=mb) as obj:
            many = obj.sample_batch(delays[None, :], alpha[None, :], [rho], tt, 129, seed, sigmatest=st, return_noise=True, fallback=False)
            one = obj.sample_batch(delays[None, :], alpha[None, :], [rho], tt, 1, seed, sigmatest=st, return_noise=True, fallback=False)
        assert many[3][0] == 0 and one[3][0] == 0 and np.array_equal(one[4][0], many[4][0])
        wz.add(_normals_ratio(many[4], seed, 0), (name, mb))
        ref = SH.dense_reference(oracle, name, data, delays, alpha, rho, mb, tt, st, many[4])
        r129, r1 = ref.ratio(many[0]), float(np.max(SH.err(one[0][0], ref.draws[0]) / ref.bar))
        print("dense draws edges N = %d %s b%d: error / bar S = 129 %.3g, S = 1 %.3g (bar %.3g, old bar %.3g)" % (N, name, mb, r129, r1, ref.bar,
                                                                                                            ref.old_bar))
        worst[129].add(r129, (name, mb))
        worst[1].add(r1, (name, mb))
    SH.report([wz] + list(worst.values()))


# -- linear-time draws --------------------------------------------------------------------------------------------------------------
def _linear_device(case, n, seed, mixture):
    cid, k, data, delays, alpha, rho, mb, tests = case
    kw = dict(weights=[1.0]) if mixture else {}
    with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
        dr, _, _, info = obj.sample_markov_batch(delays[None, :], alpha[None, :], [rho], tests[0], n, seed, sigmatest=tests[2], **kw)
    assert info[0] == 0 and dr.shape == (n, sum(len(a) for a in tests[0])), cid
    return dr


def _compare_linear(oracle, rows, group):
    """rows: [(case, seed, mixture)]."""
    worst = SH.Worst("highprec linear-time draws " + group)
    for case, seed, mixture in rows:
        ref = SH.linear_reference(oracle, case, seed, S, rng.MIXROW if mixture else 0)
        r = ref.ratio(_linear_device(case, S, seed, mixture))
        print("linear-time draws %s: error / bar %.3g (bar %.3g of which the normals term %.3g, old bar %.3g)"
              % (case[0], r, float(np.max(ref.bar)), float(np.max(ref.bar)) - ref.base, ref.old_bar))
        worst.add(r, case[0])
    SH.report([worst])


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_cases_linear(oracle, kernel, L):
    _compare_linear(oracle, [(CASES[i], 500 + i, bool(i % 2)) for i in _select(kernel, L)], "%s L = %d" % (kernel, L))


def test_edge_shapes_linear(oracle):
    shapes = [("matern32", [1, 1], [1, 0], False), ("OU", [7, 5], [0, 4], True), ("matern52", [5, 4, 6, 3], [2, 1, 2, 1], True),
              ("matern52", [3, 4, 2, 3, 4, 2, 3, 2], [1, 0, 1, 1, 0, 1, 1, 1], False)]         # test_gpu_markov_sample.test_parity_edge_shapes'
    _compare_linear(oracle, [(TM._tiny(k, Nl, Nt, mb, seed=sum(Nl) + len(Nl)), 41, False) for k, Nl, Nt, mb in shapes], "edge shapes")


@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_process_noise_branch_linear(oracle, kernel):
    rows = []
    for i, rho in enumerate((0.1, 3.0, 300.0)):
        case, (d_lo, d_hi) = SH.branch_band(kernel, rho, bool(i % 2))
        lam, lags = markov.rate(kernel, rho), np.diff(np.sort(np.concatenate([case[2][0][0], case[7][0][0]])))
        assert lam * d_lo <= 1.0 < lam * d_hi and d_lo in lags and d_hi in lags and 2.0 ** -10 in lags and 0.0 in lags and 40.0 in lags
        rows.append((case, 77 + i, bool(i % 2)))
    _compare_linear(oracle, rows, "process-noise branch %s" % kernel)


@pytest.mark.parametrize("T", [1, 63, 64, 65])
def test_finish_edges_linear(oracle, T):
    t, y, s, delays = MC.lightcurves([12, 9], seed=64, kind="ties")
    rg = np.random.default_rng(T)
    Nt = [T - T // 3, T // 3]
    tt = [MC.snap(rg.uniform(-2.0, 32.0, n)) for n in Nt]
    st = [0.2 + 0.05 * rg.random(n) for n in Nt]
    case = ("finish-T%d" % T, "matern32", (t, y, s), delays, np.array([1.2, 0.8]), 3.0, True, (tt, None, st))
    ref = SH.linear_reference(oracle, case, 65, 65, 0)
    worst = SH.Worst("highprec linear-time draws finish edges T = %d, lanes 1 / 63 / 64 / 65" % T)
    for n in (1, 63, 64, 65):
        dr = _linear_device(case, n, 65, False)
        worst.add(float(np.max(SH.err(dr, ref.draws[:n]) / ref.bar[:n])), n)
    SH.report([worst])


# -- the unstaged path --------------------------------------------------------------------------------------------------------------
LDS_MAX, POINT_BYTES, LANE_BYTES = 156 * 1024, 20, 40            # csrc: GPCC_MARKOV_LDS_MAX, GPCC_MKS_POINT_BYTES, GPCC_MKP_LANE_BYTES


def _unstaged_problem():
    rg = np.random.default_rng(6496)
    Nl, Nt = [800] * 8, [12] * 8
    t = [np.sort(MC.snap(rg.uniform(0.0, 800.0, n))) for n in Nl]
    y = [np.sin(0.05 * a + l) + 0.2 * l + 0.1 * rg.standard_normal(len(a)) for l, a in enumerate(t)]
    s = [0.1 + 0.05 * rg.random(len(a)) for a in t]
    tt = [MC.snap(rg.uniform(-5.0, 805.0, n)) for n in Nt]
    st = [0.2 + 0.05 * rg.random(n) for n in Nt]
    delays = np.concatenate([[0.0], MC.snap(rg.uniform(-3.0, 5.0, 7))])
    return (t, y, s), tt, st, delays, rg.uniform(0.5, 2.0, 8), 20.0


def test_unstaged_draws_are_the_staged_ones(oracle):
    """L = 8 without offsets, N + T = 6496: the points fit LDS beside the cursors of one wave (20 (N + T) + 8 + 40 L 64 = 150 408 <=
    156 KiB) and not beside those of two (170 888).  64 draws are one wave per workgroup: staged.  64 CUs' worth of waves plus one --
    one chunk by markov_sample_chunk_draws -- are two waves per workgroup (markov_launch): unstaged, every lane reading global
    memory.  A draw's bits depend on seed, row, s and m alone, so the first 64 draws of both calls are equal bitwise.
    Scratch: 8 (N + T) bytes per lane of the 256-rounded chunk, 0.81 GiB at 256 CUs."""
    import torch
    (t, y, s), tt, st, delays, alpha, rho = _unstaged_problem()
    N, T, L = sum(map(len, t)), sum(map(len, tt)), len(t)
    fits = lambda threads: POINT_BYTES * (N + T) + 8 + LANE_BYTES * L * threads <= LDS_MAX                # noqa: E731
    assert fits(64) and not fits(128)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lanes = 64 * cus + 64
    assert 8 * (N + T) * ((lanes + 255) // 256 * 256) < 2 ** 30
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32, marginalise_b=False) as obj:
        few = obj.sample_markov_batch(delays[None, :], alpha[None, :], [rho], tt, 64, 19, sigmatest=st)
        obj.set_option("markov_sample_chunk_draws", lanes)
        many = obj.sample_markov_batch(delays[None, :], alpha[None, :], [rho], tt, lanes, 19, sigmatest=st)
        obj.set_option("markov_sample_chunk_draws", 0)
    assert few[3][0] == 0 and many[3][0] == 0 and few[2][0] == many[2][0]
    assert few[0].shape == (64, T) and many[0].shape == (lanes, T) and np.isfinite(many[0]).all()
    differ = int(np.sum(few[0] != many[0][:64]))
    print("highprec linear-time draws unstaged (%d lanes, two waves per workgroup) against staged (64 lanes): %d of %d values differ"
          % (lanes, differ, 64 * T))
    assert differ == 0
    # one draw against the numpy mirror.  The bar is BORROWED, not measured at this N: twice the largest bar of the N = 110 cases of
    # the same kernel (a longdouble factorisation of N = 6400 does not fit a test of seconds).
    borrowed = 2.0 * max(float(np.max(SH.linear_reference(oracle, CASES[i], 500 + i, S, _word(i)).bar))
                         for i, c in enumerate(CASES) if c[1] == "matern32")
    mir, _, info = markov.sample("matern32", t, y, s, delays, alpha, rho, tt, st, False, seed=19, s=lanes - 1, m=0)
    e = float(np.max(np.abs(many[0][lanes - 1] - mir)))
    print("highprec linear-time draws unstaged, draw %d against the numpy mirror: error %.3g, borrowed bar %.3g" % (lanes - 1, e, borrowed))
    assert info == 0 and e <= borrowed


# -- mutations ----------------------------------------------------------------------------------------------------------------------
def test_mutations_miss_the_bar(oracle):
    """On the device's own output at the Matern-3/2 cases with two bands and test noise (both b-modes, rho = 0.1 and 20)."""
    low = {("dense", "next draw"): np.inf, ("dense", "no JITTER"): np.inf, ("linear-time", "next draw"): np.inf,
           ("linear-time", "no JITTER"): np.inf}
    picked = [i for i in _select("matern32", 2) if i % 2 == 0]
    assert len(picked) == 4
    for idx in picked:
        cid, k, data, delays, alpha, rho, mb, tests = CASES[idx]
        N, T = sum(map(len, data[0])), sum(map(len, tests[0]))
        st = SH._flat(tests[2])
        # dense
        dr, ref, _, z = _dense_case(oracle, idx)
        assert ref.ratio(dr) <= 1.0, cid
        r = {("dense", "next draw"): float(np.max(SH.err(dr[:-1], ref.draws[1:]) / ref.bar))}
        m = SH.model(k, *data, delays, alpha, rho, tests[0], mb)
        without = SH.dense_draws(m, np.sqrt(st * st - SH.LD(SH.JITTER)), z)[0]
        r[("dense", "no JITTER")] = ref.ratio(dr + (without - ref.draws).astype(np.float64))
        # linear-time
        lref = SH.linear_reference(oracle, CASES[idx], 500 + idx, S, _word(idx))
        ld = _linear_device(CASES[idx], S, 500 + idx, bool(idx % 2))
        assert lref.ratio(ld) <= 1.0, cid
        r[("linear-time", "next draw")] = float(np.max(SH.err(ld[:-1], lref.draws[1:]) / lref.bar[1:]))
        z3 = rng.point_normals(500 + idx, N + T + 1, range(S), _word(idx))[:, N:N + T, 3].astype(SH.LD)
        diff = (st - np.sqrt(SH.LD(SH.JITTER) + st * st))[None, :] * z3
        r[("linear-time", "no JITTER")] = lref.ratio(ld + diff.astype(np.float64))
        for what in r:
            low[what] = min(low[what], r[what])
    for (family, what), v in low.items():
        print("highprec %s draws mutation, %s: smallest error / bar %.3g" % (family, what, v))
    assert all(v > 1.0 for v in low.values()), low
