"""gpcc_sample_batch on the device: every drawn row against the numpy witness (tests/_sample_witness.py) and against Objective.predict +
a numpy Cholesky for the device's own normals, over kernels, b-modes, band counts and tile edges of the training and test points; the
normals and the row choice against the host mirror (gpcc_amd.rng); bitwise invariance over batch sizes, slot and stream options, fp32
handles and prefixes in S; loglik and info against the held-out path; the statistics of the draws; training and test-block failures
and the Python fallback; and DelayAveragedPredictor.sample at the README size.

The bar is max(1e-10, 64 eps cond_1(K_aug)) * max(1, max |f*|) (tests/test_sample_cpu.py shows that it rejects the injected slips)."""

import numpy as np
import pytest

import _grad_witness as W
import _sample_witness as SW
import gpcc_amd
from gpcc_amd import fit, rng, synthetic
from test_gpu_heldout import GEOMETRY, KERNELS, Worst, _testset

pytestmark = pytest.mark.gpu

NOT_DRAWN = -14


def _host_draws(obj, d, a, r, tt, st, z):
    mu, Sig = obj.predict(d, a, r, tt)
    if st is not None:
        Sig = Sig + np.diag(np.concatenate(st) ** 2)
    return mu[None, :] + z @ np.linalg.cholesky(Sig).T


@pytest.mark.parametrize("N", sorted(GEOMETRY))
def test_parity(oracle, N):
    Nl, Nt = GEOMETRY[N]
    L, T, S = len(Nl), sum(Nt), 3
    data = W.ragged_data(Nl, seed=N)
    worst = Worst("sample parity N = %d, L = %d, T = %d" % (N, L, T))
    for ki, (name, kern) in enumerate(KERNELS.items()):
        for mb in (True, False):
            delays, alpha, rho = W.random_params(L, 2, seed=N + 10 * ki + mb)
            tt, yt, st = _testset(data[0], data[1], delays[0], Nt, seed=N + ki)
            sig = st if (ki + mb) % 2 else None
            with gpcc_amd.Objective(*data, kern, marginalise_b=mb) as obj:
                dr, rows, ll, info, z = obj.sample_batch(delays, alpha, rho, tt, S, seed=N + ki, sigmatest=sig, return_noise=True)
                held, hl, hi, _, _ = obj.heldout_loglik_batch(delays, alpha, rho, tt, yt, st if sig is not None else [0 * a for a in st])
                assert (info == 0).all() and np.array_equal(info, hi) and np.array_equal(ll, hl), (name, mb)
                assert dr.shape == (2 * S, T) and np.array_equal(rows, np.repeat([0, 1], S))
                for m in range(2):
                    zm = z[m * S:(m + 1) * S]
                    zr = rng.normals(N + ki, T, np.arange(S), m)
                    assert np.max(np.abs(zm - zr)) <= 1e-13, (name, mb, m)
                    ref, cond = SW.draws(oracle, name, *data, delays[m], alpha[m], rho[m], tt, sig, zm, marginalise_b=mb)
                    hd = _host_draws(obj, delays[m], alpha[m], rho[m], tt, sig, zm)
                    got = dr[m * S:(m + 1) * S]
                    worst.add(np.max(np.abs(got - ref)) / SW.bar(cond, ref), ((name, mb), m, "witness"))
                    worst.add(np.max(np.abs(got - hd)) / SW.bar(cond, hd), ((name, mb), m, "predict"))
    worst.report()


@pytest.mark.parametrize("N", [4095, 4096])
def test_large(oracle, N):
    Nl = [N // 2, N - N // 2]
    data = W.ragged_data(Nl, seed=N)
    delays, alpha, rho = W.random_params(2, 2, seed=N)
    tt, _, st = _testset(data[0], data[1], delays[0], [512, 512], seed=N)
    worst = Worst("sample N = %d, T = 1024" % N)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
        dr, _, _, info, z = obj.sample_batch(delays, alpha, rho, tt, 2, seed=1, sigmatest=st, return_noise=True)
        assert (info == 0).all()
        for m in range(2):
            ref, cond = SW.draws(oracle, "matern32", *data, delays[m], alpha[m], rho[m], tt, st, z[2 * m:2 * m + 2])
            worst.add(np.max(np.abs(dr[2 * m:2 * m + 2] - ref)) / SW.bar(cond, ref), m)
    worst.report()


def _repeat_data():
    data = W.ragged_data([170, 130], seed=300)
    delays, alpha, rho = W.random_params(2, 40, seed=31)
    tt, _, st = _testset(data[0], data[1], delays[0], [150, 140], seed=3)
    return data, delays, alpha, rho, tt, st


def test_invariance():
    data, delays, alpha, rho, tt, st = _repeat_data()
    S, seed = 5, 77
    w = np.random.default_rng(4).random(40) ** 2
    w[[1, 8]] = 0.0
    with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
        full = obj.sample_batch(delays, alpha, rho, tt, S, seed, sigmatest=st)
        again = obj.sample_batch(delays, alpha, rho, tt, S, seed, sigmatest=st)
        seven = obj.sample_batch(delays[:7], alpha[:7], rho[:7], tt, S, seed, sigmatest=st)
        short = obj.sample_batch(delays, alpha, rho, tt, 3, seed, sigmatest=st)
        held = obj.heldout_loglik_batch(delays, alpha, rho, tt, [0 * a for a in tt], st)
        mix = obj.sample_batch(delays, alpha, rho, tt, 300, seed, weights=w)
        mix_short = obj.sample_batch(delays, alpha, rho, tt, 200, seed, weights=w)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32, slots_per_stream=8) as obj8:
        eight = obj8.sample_batch(delays, alpha, rho, tt, S, seed, sigmatest=st)
        mix8 = obj8.sample_batch(delays, alpha, rho, tt, 300, seed, weights=w)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32, slots_per_stream=3, streams=2) as obj3:
        three = obj3.sample_batch(delays, alpha, rho, tt, S, seed, sigmatest=st)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32, precision="fp32") as o32:
        f32 = o32.sample_batch(delays, alpha, rho, tt, S, seed, sigmatest=st)
    with gpcc_amd.Objective(*data, gpcc_amd.matern32, devices=[0, 0]) as om:
        multi = om.sample_batch(delays, alpha, rho, tt, S, seed, sigmatest=st)
    assert (full[3] == 0).all() and np.isfinite(full[0]).all()
    assert np.array_equal(full[2], held[1]) and np.array_equal(full[3], held[2])
    for k in range(4):
        for other in (again, eight, three, f32, multi):
            assert np.array_equal(full[k], other[k]), k
        assert np.array_equal(full[k][:7 * S], seven[k]) if k < 2 else np.array_equal(full[k][:7], seven[k]), k
    for i in (0, 6, 39):
        one = None
        with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
            one = obj.sample_batch(delays[i:i + 1], alpha[i:i + 1], rho[i:i + 1], tt, S, seed, sigmatest=st)
        # a row's draws carry the row index in their counter: row i of the batch is not row 0 of a one-row call, but its factor is
        assert one[2][0] == full[2][i] and one[3][0] == full[3][i]
    d = full[0].reshape(40, S, -1)
    assert np.array_equal(d[:, :3].reshape(40 * 3, -1), short[0])                     # prefixes in S
    assert np.array_equal(mix[0][:200], mix_short[0]) and np.array_equal(mix[1][:200], mix_short[1])
    for k in range(4):
        assert np.array_equal(mix[k], mix8[k], equal_nan=True), k
    assert np.array_equal(mix[1], rng.pick_rows(seed, 300, w))
    drawn = np.zeros(40, bool)
    drawn[mix[1]] = True
    assert np.all(mix[3][~drawn] == NOT_DRAWN) and np.isnan(mix[2][~drawn]).all()
    assert np.array_equal(mix[2][drawn], held[1][drawn]) and np.array_equal(mix[3][drawn], held[2][drawn])
    assert not drawn[[1, 8]].any()


def test_one_row_matches_a_single_row_call():
    """Row m of a batch uses counter row word m: a one-row call of the same (tau, alpha, rho) at row 0 draws with row word 0, which is
    row 0 of the batch bitwise."""
    data, delays, alpha, rho, tt, st = _repeat_data()
    with gpcc_amd.Objective(*data, gpcc_amd.OU) as obj:
        full = obj.sample_batch(delays[:4], alpha[:4], rho[:4], tt, 4, 9)
        one = obj.sample_batch(delays[:1], alpha[:1], rho[:1], tt, 4, 9)
    for k in range(4):
        assert np.array_equal(full[k][:4] if k < 2 else full[k][:1], one[k]), k


def test_statistics_one_row():
    data = W.ragged_data([60, 50], seed=5)
    delays, alpha, rho = np.array([[0.0, 2.0]]), np.array([[1.2, 0.9]]), np.array([3.0])
    tt = [np.linspace(0, 20, 5), np.linspace(3, 18, 3)]
    S = 20000
    with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
        dr, _, _, info, _ = obj.sample_batch(delays, alpha, rho, tt, S, seed=2024, return_noise=True)
        mu, Sig = obj.predict(delays[0], alpha[0], rho[0], tt)
    assert info[0] == 0
    m = dr.mean(0)
    C = np.cov(dr.T, bias=False)
    se_m = np.sqrt(np.diag(Sig) / S)
    d = np.sqrt(np.diag(Sig))
    se_c = np.sqrt((np.outer(d ** 2, d ** 2) + Sig ** 2) / S)
    print("one row: mean %.2f SE, covariance %.2f SE" % (np.max(np.abs(m - mu) / se_m), np.max(np.abs(C - Sig) / se_c)))
    assert np.all(np.abs(m - mu) <= 5 * se_m)
    assert np.all(np.abs(C - Sig) <= 5 * se_c)


def test_mixture_statistics():
    data = W.ragged_data([70, 60], seed=8)
    G = 12
    grid = np.linspace(0.0, 6.0, G)
    delays = np.stack([np.zeros(G), grid], 1)
    alpha, rho = np.tile([1.1, 0.9], (G, 1)), np.full(G, 2.5)
    w = np.exp(-0.5 * (grid - 3.0) ** 2)
    w[[0, 5]] = 0.0
    tt = [np.linspace(0, 25, 10), np.linspace(2, 22, 10)]
    S = 20000
    with gpcc_amd.Objective(*data, gpcc_amd.OU) as obj:
        dr, rows, ll, info = obj.sample_batch(delays, alpha, rho, tt, S, seed=11, weights=w)
        _, _, _, _, mix_mu, mix_var = obj.predict_batch(delays, alpha, rho, tt, weights=w)
    assert np.array_equal(rows, rng.pick_rows(11, S, w))
    assert np.all(info[[0, 5]] == NOT_DRAWN)
    m, v = dr.mean(0), dr.var(0, ddof=1)
    m4 = np.mean((dr - m) ** 4, 0)
    se_m, se_v = np.sqrt(mix_var / S), np.sqrt(np.maximum(m4 - v ** 2, 0) / S)
    print("mixture: mean %.2f SE, variance %.2f SE" % (np.max(np.abs(m - mix_mu) / se_m), np.max(np.abs(v - mix_var) / se_v)))
    assert np.all(np.abs(m - mix_mu) <= 5 * se_m)
    assert np.all(np.abs(v - mix_var) <= 5 * se_v)


def test_training_failure_rows():
    from test_gpu_gradient_edges import _failure_data
    data = _failure_data()
    N = sum(len(a) for a in data[0])
    delays = np.array([[0, 10, 20], [0, 1, 20], [0, 10, 12], [0, -5, 7.5], [0, 10, 3], [0, 6, 17]], float)
    M = len(delays)
    alpha = np.ones((M, 3))
    alpha[[0, 3, 5]] = [[0.9, 1.2, 1.1], [1.3, 0.7, 1.0], [1.0, 1.0, 0.8]]
    rho = np.full(M, 3.0)
    tt = [np.linspace(0, 30, 50), np.linspace(1, 29, 7), np.linspace(2, 20, 140)]
    S = 4
    with gpcc_amd.Objective(*data, gpcc_amd.OU, marginalise_b=False, slots_per_stream=8) as obj:
        dr, rows, ll, info = obj.sample_batch(delays, alpha, rho, tt, S, seed=3)
        held = obj.heldout_loglik_batch(delays, alpha, rho, tt, [0 * a for a in tt], [0 * a for a in tt])
        bad = info != 0
        assert bad.sum() >= 2 and np.all((info[bad] >= 1) & (info[bad] <= N)), info
        assert np.array_equal(info, held[2]) and np.array_equal(ll, held[1], equal_nan=True)
        d = dr.reshape(M, S, -1)
        assert np.isnan(d[bad]).all() and np.isfinite(d[~bad]).all()
        good = np.flatnonzero(~bad)
        sub = obj.sample_batch(delays[:good[-1] + 1], alpha[:good[-1] + 1], rho[:good[-1] + 1], tt, S, seed=3)
        assert np.array_equal(sub[0].reshape(-1, S, d.shape[2])[good], d[good])       # failures change no other row


def test_test_block_failure_and_fallback():
    """Two identical test times in one band and a large alpha: the latent test block Sigma_pred + 1e-8 I is singular in fp64 (as in
    tests/test_gpu_heldout.py); the device reports N + j with NaN draws, and the fallback redraws the row from nearestposdef with the
    same normals."""
    data = W.ragged_data([90, 70], seed=7)
    N = 160
    tt = [np.array([5.0, 12.5, 12.5, 20.0]), np.array([3.0, 17.0])]
    delays, rho = np.array([[0.0, 2.0], [0.0, 2.5]]), np.array([2.0, 2.0])
    seen = None
    with gpcc_amd.Objective(*data, gpcc_amd.matern52, marginalise_b=False) as obj:
        for a in (1e1, 1e2, 1e3, 1e4, 1e5, 1e6):
            alpha = np.array([[a, 1.0], [1.0, 1.0]])
            dr, rows, ll, info, z = obj.sample_batch(delays, alpha, rho, tt, 3, seed=5, return_noise=True, fallback=False)
            if info[0] > N:
                seen = (a, alpha, dr, ll, info, z)
                break
        assert seen is not None, "no test-block failure reported up to alpha = 1e6"
        a, alpha, dr, ll, info, z = seen
        assert N < info[0] <= N + 6 and np.isnan(dr[:3]).all() and (info[1] != 0 or np.isfinite(dr[3:]).all())
        held = obj.heldout_loglik_batch(delays, alpha, rho, tt, [0 * x for x in tt], [0 * x for x in tt], fallback=False)
        assert np.array_equal(info, held[2]) and np.array_equal(ll, held[1])
        d2, _, l2, i2, z2 = obj.sample_batch(delays, alpha, rho, tt, 3, seed=5, return_noise=True)
        assert np.array_equal(z2, z) and np.array_equal(i2, info) and np.array_equal(d2[3:], dr[3:], equal_nan=info[1] > N)
        mu, Sig = obj.predict(delays[0], alpha[0], rho[0], tt)
        ref = mu[None, :] + z[:3] @ np.linalg.cholesky(fit.nearestposdef(Sig, minimumeigenvalue=1e-6)).T
        assert np.array_equal(d2[:3], ref)
        d3 = obj.sample_batch(delays, alpha, rho, tt, 3, seed=5)[0]                     # the fallback's normals from the mirror
        assert np.max(np.abs(d3[:3] - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
    print("test-block failure at alpha = %g: info = N + %d" % (a, info[0] - N))


def test_argument_errors():
    data, delays, alpha, rho, tt, st = _repeat_data()
    with gpcc_amd.Objective(*data, gpcc_amd.OU) as obj:
        with pytest.raises(AssertionError):
            obj.sample_batch(delays, alpha, rho, tt[:1], 2, 1)
        with pytest.raises(gpcc_amd.GpccError):
            obj.sample_batch(delays, alpha, rho, [np.zeros(0)] * 2, 2, 1)
        with pytest.raises(gpcc_amd.GpccError):
            obj.sample_batch(delays, alpha, rho, tt, 0, 1)
        with pytest.raises(ValueError):
            obj.sample_batch(delays, alpha, rho, tt, 2, 1, sigmatest=[st[0], st[1][:3]])
        for bad in ([-1.0] + [1.0] * 39, [np.nan] + [1.0] * 39, [0.0] * 40):
            with pytest.raises(gpcc_amd.GpccError) as ei:
                obj.sample_batch(delays, alpha, rho, tt, 2, 1, weights=np.array(bad))
            assert ei.value.code == -1


def test_readme_delay_averaged_draws():
    """DelayAveragedPredictor.sample at the README size: a gpcc_grid fit over 101 delays, 10 000 draws on 2 x 201 test times; the rows
    follow the weights, and each draw is a draw of its own row's Gaussian (checked against Predictor.sample's row for a few draws)."""
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    grid = np.arange(0.0, 20.01, 0.2)
    cand = np.stack([np.zeros_like(grid), grid], 1)
    res = fit.gpcc_grid(t, y, s, kernel=gpcc_amd.OU, candidatedelays=cand, iterations=40, rhomin=0.1, rhomax=20.0)
    p = gpcc_amd.getprobabilities(res.loglikel)
    tgrid = np.linspace(-2.0, 22.0, 201)
    S = 10000
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        dap = fit.DelayAveragedPredictor(obj, cand, res.alpha, res.rho, p)
        bands, rows = dap.sample(tgrid, S, seed=1)
        assert len(bands) == 2 and bands[0].shape == (S, 201) and np.isfinite(bands[0]).all() and np.isfinite(bands[1]).all()
        assert np.array_equal(rows, rng.pick_rows(1, S, p))
        freq = np.bincount(rows, minlength=len(p)) / S
        assert np.all(np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / S) + 1e-12)
        tau = dap.delays[rows, 1]
        assert abs(np.mean(tau) - np.sum(p * grid)) <= 5 * np.sqrt(np.sum(p * (grid - np.sum(p * grid)) ** 2) / S) + 1e-12
        mu, sig = dap(tgrid)
        for l in range(2):
            assert np.all(np.abs(bands[l].mean(0) - mu[l]) <= 5 * sig[l] / np.sqrt(S) + 1e-9)
        one = fit.Predictor(obj, cand[50], res.alpha[50], res.rho[50]).sample(tgrid, 3, seed=1)
        assert one[0].shape == (3, 201) and np.isfinite(one[0]).all()
