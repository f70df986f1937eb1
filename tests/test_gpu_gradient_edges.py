"""gpcc_loglik_grad_batch at the edges of its tile and band bookkeeping, against the extended-precision reference
(tests/_grad_highprec.py): tile counts 1 to 6 with band boundaries on and next to tile edges, eight bands, degenerate geometry,
the corners of the hyper-parameter envelope, failures in a chosen tile, several groups per stream, and N = 16384.

Every comparison uses _grad_highprec.ratio (error / bar, bar = max(1e-11, 64 eps64 cond_1(K)) max(1, max|g_ref|)); the worst ratio
of each group of cases is printed.  The references are computed in a pool of CPU processes that never touch the GPU."""
import multiprocessing
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _grad_highprec as H
import _grad_witness as W
import gpcc_amd
from gpcc_amd import _capi

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)]

KERNELS = {"OU": gpcc_amd.OU, "rbf": gpcc_amd.rbf, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}

# N -> band lengths: band boundaries at, before and after tile edges (128, 256, 384, 512)
GEOMETRY = {1: [1], 2: [2], 127: [60, 67], 128: [100, 28], 129: [127, 2], 255: [128, 127], 256: [129, 127], 257: [128, 129],
            383: [127, 128, 128], 384: [128, 128, 128], 385: [129, 127, 129], 640: [256, 384], 641: [128, 384, 129]}


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


class Cases:
    """Device rows waiting for their references: add() per row, then check() compares them all and prints the worst ratio."""

    def __init__(self, group):
        self.group, self.jobs, self.rows = group, [], []

    def add(self, name, data, mb, delays, alpha, rho, ll, grad, label, vl=None):
        """vl: loglik_batch's value of the same row, where the case has it."""
        self.jobs.append((name, *data, delays, alpha, rho, mb))
        self.rows.append((float(ll), np.array(grad), len(alpha), label, None if vl is None else float(vl)))

    def check(self, pool):
        worst, where = 0.0, None
        for ref, (ll, g, L, label, vl) in zip(pool.map(H.evaluate_job, self.jobs), self.rows):
            assert ref.info == 0, (label, ref.info)
            # the value: the same conditioning-scaled bar, relative to max(1, |loglik|) -- the gradient call's and loglik_batch's
            value_bar = max(1e-11, 64 * H.EPS64 * ref.cond) * max(1.0, abs(ref.loglik))
            assert abs(ll - ref.loglik) <= value_bar, (label, ll, ref.loglik)
            if vl is not None:
                assert abs(vl - ref.loglik) <= value_bar, (label, vl, ref.loglik)
            r = H.ratio(g, ref)
            assert r <= 1.0, (label, r, g, ref.grad, ref.cond)
            if L > 1:   # a common shift of all delays leaves the likelihood unchanged
                assert abs(np.sum(g[L + 1:])) <= H.bar(ref), (label, g)
            else:
                assert g[L + 1] == 0.0, (label, g)
            if r >= worst:
                worst, where = r, label
        print("%s: %d rows, worst error / bar %.3g (%s)" % (self.group, len(self.rows), worst, where))
        return worst


def _run(obj, delays, alpha, rho):
    """The gradient call, and loglik_batch on the same rows: the same info, NaN rows where it is not 0.  (The values of the two
    paths differ by up to ~eps64 cond(K) relative: each is compared with the reference in Cases.check.)
    -> (ll, grad, info, vl)."""
    ll, grad, info = obj.loglik_grad_batch(delays, alpha, rho)
    vl, vinfo = obj.loglik_batch(delays, alpha, rho)
    assert np.array_equal(info, vinfo), (info, vinfo)
    ok = info == 0
    assert np.isnan(grad[~ok]).all() and np.isnan(ll[~ok]).all() and np.isnan(vl[~ok]).all()
    return ll, grad, info, vl


def _no_one_point_band_with_b(data, name):
    """A one-point band has no sample variance: with b marginalised the handle refuses it (GPCC_ERR_ARGUMENT), as loglik does."""
    with pytest.raises(_capi.GpccError) as e:
        gpcc_amd.Objective(*data, KERNELS[name], marginalise_b=True)
    assert e.value.code == -1 and "observations" in str(e.value)


def test_tile_geometry(pool):
    cases = Cases("tile geometry")
    for N, Nl in GEOMETRY.items():
        data = W.ragged_data(Nl, seed=N)
        L = len(Nl)
        delays, alpha, rho = W.random_params(L, 3, seed=N + 1)
        for ki, name in enumerate(KERNELS):
            for mb in (True, False):
                if mb and min(Nl) < 2:
                    _no_one_point_band_with_b(data, name)
                    continue
                with gpcc_amd.Objective(*data, KERNELS[name], marginalise_b=mb, slots_per_stream=8) as obj:
                    ll, grad, info, vl = _run(obj, delays, alpha, rho)
                assert (info == 0).all(), (N, name, mb, info)
                rows = range(3) if N < 600 else [ki % 3]   # (the reference's time)
                for i in rows:
                    cases.add(name, data, mb, delays[i], alpha[i], rho[i], ll[i], grad[i], (N, name, mb, i), vl=vl[i])
    cases.check(pool)


def test_many_bands(pool):
    cases = Cases("eight bands")
    layouts = [([1, 2, 3, 40, 127, 128, 129, 90], (False,)), ([2, 2, 3, 40, 127, 128, 129, 89], (True,)),
               ([16] * 8, (True, False))]
    for Nl, modes in layouts:
        data = W.ragged_data(Nl, seed=len(Nl) + Nl[0])
        delays, alpha, rho = W.random_params(8, 3, seed=Nl[0])
        for name in KERNELS:
            for mb in modes:
                with gpcc_amd.Objective(*data, KERNELS[name], marginalise_b=mb, slots_per_stream=8) as obj:
                    ll, grad, info, vl = _run(obj, delays, alpha, rho)
                assert (info == 0).all() and grad.shape == (3, 17)
                for i in range(3):
                    cases.add(name, data, mb, delays[i], alpha[i], rho[i], ll[i], grad[i], (sum(Nl), Nl[0], name, mb, i), vl=vl[i])
        if Nl[0] == 1:
            _no_one_point_band_with_b(data, "OU")
    # N = 1030 on one row
    Nl = [1, 2, 3, 40, 127, 128, 129, 600]
    data = W.ragged_data(Nl, seed=5)
    delays, alpha, rho = W.random_params(8, 1, seed=6)
    with gpcc_amd.Objective(*data, gpcc_amd.matern52, marginalise_b=False, slots_per_stream=8) as obj:
        ll, grad, info, vl = _run(obj, delays, alpha, rho)
    assert info[0] == 0
    cases.add("matern52", data, False, delays[0], alpha[0], rho[0], ll[0], grad[0], (1030, "matern52"), vl=vl[0])
    cases.check(pool)


def _dyadic(x):
    return np.round(np.asarray(x) * 1024) / 1024


def test_degenerate_geometry(pool):
    cases = Cases("degenerate geometry")
    rg = np.random.default_rng(17)
    base = W.ragged_data([70, 60], seed=17)
    for d in base[0]:
        d[:] = _dyadic(d)
    geoms = []
    # points of both bands at exactly the same shifted time (s = 0 across bands; OU's dk/ds(0) = 0)
    t = [base[0][0].copy(), base[0][1].copy()]
    t[1][::3] = t[0][:20][:len(t[1][::3])] + 1.5
    t[1] = np.sort(t[1])
    geoms.append(("coincident", (t, base[1], base[2]), [0.0, 1.5]))
    # a band of one point
    geoms.append(("one-point band", ([base[0][0], base[0][1][:1]], [base[1][0], base[1][1][:1]], [base[2][0], base[2][1][:1]]),
                  [0.0, 2.0]))
    # delays that put band 2 before band 1
    geoms.append(("reversed", ([base[0][0], base[0][1] + 40.0], base[1], base[2]), [0.0, 80.0]))
    # a delay so large that the bands do not overlap (k = 0 between them)
    geoms.append(("disjoint", base, [0.0, 1.0e4]))
    for label, data, dl in geoms:
        M = 2
        delays = np.tile(dl, (M, 1))
        alpha = rg.uniform(0.5, 1.5, (M, 2))
        rho = rg.uniform(0.8, 4.0, M)
        for name in KERNELS:
            for mb in (True, False):
                if mb and label == "one-point band":
                    _no_one_point_band_with_b(data, name)
                    continue
                with gpcc_amd.Objective(*data, KERNELS[name], marginalise_b=mb, slots_per_stream=8) as obj:
                    ll, grad, info, vl = _run(obj, delays, alpha, rho)
                assert (info == 0).all(), (label, name, mb, info)
                for i in range(M):
                    cases.add(name, data, mb, delays[i], alpha[i], rho[i], ll[i], grad[i], (label, name, mb, i), vl=vl[i])
    cases.check(pool)


def test_hyperparameter_envelope(pool):
    """alpha in {1e-2, 1e2}, rho in {0.05, 300}, sigma in {0.05, 1}: where the device factorises, the gradient meets the
    conditioning-scaled bar; where it does not, the row is NaN with loglik_batch's info (_run)."""
    cases = Cases("hyper-parameter envelope")
    combos = [(a, r) for a in (1e-2, 1e2) for r in (0.05, 300.0)]
    failed = 0
    for Nl in ([22, 18], [70, 58]):
        t, y, _ = W.ragged_data(Nl, seed=sum(Nl))
        delays = np.tile([0.0, 1.25], (len(combos), 1))
        alpha = np.array([[a, a] for a, _ in combos])
        rho = np.array([r for _, r in combos])
        for sig in (0.05, 1.0):
            data = (t, y, [np.full(n, sig) for n in Nl])
            for name in KERNELS:
                for mb in (True, False):
                    with gpcc_amd.Objective(*data, KERNELS[name], marginalise_b=mb, slots_per_stream=8) as obj:
                        ll, grad, info, vl = _run(obj, delays, alpha, rho)
                    for i in range(len(combos)):
                        if info[i] != 0:
                            failed += 1
                            continue
                        cases.add(name, data, mb, delays[i], alpha[i], rho[i], ll[i], grad[i],
                                  (sum(Nl), sig, name, mb) + combos[i], vl=vl[i])
    print("hyper-parameter envelope: %d rows failed on the device (NaN, loglik_batch's info)" % failed)
    cases.check(pool)


def _failure_data():
    """N = 513 in bands of 100, 200, 213 (mb = False, OU), with four isolated pairs of zero-noise points 1e6 apart from everything
    else, each pair split over two bands.  A pair's 2 x 2 block is alpha alpha' [[1, k], [k, 1]], k = k(its shifted lag): with
    unit alpha it is exactly singular when the delays align the pair (lag 0), and the first non-positive pivot is the pair's later
    point.  The pairs: (band, index) -> (band, index) and the delay difference that aligns them."""
    data = W.ragged_data([100, 200, 213], seed=513)
    t, y, s = (list(map(np.copy, a)) for a in data)
    pairs = [((0, 50), (1, 10), 1.0e6, 1.0),     # later point 110 (tile 0)
             ((1, 150), (2, 20), 2.0e6, 2.0),    # later point 320 (tile 2)
             ((0, 60), (2, 150), 3.0e6, 3.0),    # later point 450 (tile 3)
             ((1, 20), (2, 212), 4.0e6, 4.0)]    # later point 512 (tile 4: the last real point)
    for (b0, i0), (b1, i1), T, c in pairs:
        t[b0][i0], t[b1][i1] = T, T + c
        s[b0][i0] = s[b1][i1] = 0.0
    return (t, y, s)


def test_failure_in_a_chosen_tile(pool):
    data = _failure_data()
    off = [0, 100, 300]
    # rows: valid, pair 1 aligned (tau_1 - tau_0 = 1), pair 2 (tau_2 - tau_1 = 2), valid, pair 3 (tau_2 - tau_0 = 3),
    # pair 4 (tau_2 - tau_1 = 4), valid
    delays = np.array([[0, 10, 20], [0, 1, 20], [0, 10, 12], [0, -5, 7.5], [0, 10, 3], [0, 10, 14], [0, 6, 17]], float)
    want = [0, off[1] + 10 + 1, off[2] + 20 + 1, 0, off[2] + 150 + 1, off[2] + 212 + 1, 0]
    M = len(delays)
    alpha = np.ones((M, 3))
    alpha[[0, 3, 6]] = [[0.9, 1.2, 1.1], [1.3, 0.7, 1.0], [1.0, 1.0, 0.8]]
    rho = np.full(M, 3.0)
    cases = Cases("failure in a chosen tile")
    with gpcc_amd.Objective(*data, gpcc_amd.OU, marginalise_b=False, slots_per_stream=8) as obj:
        ll, grad, info, vl = _run(obj, delays, alpha, rho)
        print("failure rows: info %s (expected %s)" % (info, want))
        assert list(info) == want
        bad = np.array(want) > 0
        assert np.isnan(grad[bad]).all() and np.isnan(ll[bad]).all()
        for i in np.flatnonzero(~bad):
            l1, g1, i1 = obj.loglik_grad_batch(delays[i:i + 1], alpha[i:i + 1], rho[i:i + 1])
            assert i1[0] == 0 and l1[0] == ll[i] and np.array_equal(g1[0], grad[i]), i
            cases.add("OU", data, False, delays[i], alpha[i], rho[i], ll[i], grad[i], ("valid row", i), vl=vl[i])
    cases.check(pool)


@pytest.mark.parametrize("N", [257, 1030])
def test_several_groups_per_stream(pool, N):
    """slots_per_stream = 4 on 2 streams: M = 19 at N = 257 (five groups), M = 11 at N = 1030 (three groups); bitwise equal to
    one-row calls and to a default handle, also after the slot count changes (ensure_grad reallocates)."""
    name, Nl, M = ("matern32", [128, 129], 19) if N == 257 else ("OU", [400, 330, 300], 11)
    data = W.ragged_data(Nl, seed=N)
    delays, alpha, rho = W.random_params(len(Nl), M, seed=N)
    with gpcc_amd.Objective(*data, KERNELS[name]) as ref_obj:
        ref = ref_obj.loglik_grad_batch(delays, alpha, rho)
    assert (ref[2] == 0).all()
    with gpcc_amd.Objective(*data, KERNELS[name], slots_per_stream=4, streams=2) as obj:
        for slots in (4, 3):
            obj.set_option("slots_per_stream", slots)
            got = obj.loglik_grad_batch(delays, alpha, rho)
            assert obj.get_option("workspace_slots") == slots and obj.get_option("workspace_streams") == 2
            for x, y in zip(got, ref):
                assert np.array_equal(x, y), slots
        for i in range(M):
            one = obj.loglik_grad_batch(delays[i:i + 1], alpha[i:i + 1], rho[i:i + 1])
            assert one[0][0] == ref[0][i] and np.array_equal(one[1][0], ref[1][i]), i
    cases = Cases("several groups per stream, N = %d" % N)
    cases.add(name, data, True, delays[0], alpha[0], rho[0], ref[0][0], ref[1][0], (N, 0))
    cases.check(pool)


def test_largest_size_against_finite_differences():
    """N = 16384 (2 x 8192, Matern-5/2) on one row, on a handle of one slot on one stream: against central differences of its own
    fp64 values (the gradient path's), with the bar of the N = 4096 test."""
    data = W.ragged_data([8192, 8192], seed=16384)
    L = 2
    delays, alpha, rho = W.random_params(L, 1, seed=16)
    with gpcc_amd.Objective(*data, gpcc_amd.matern52, slots_per_stream=1, streams=1) as obj:
        t0 = time.perf_counter()
        ll, grad, info = obj.loglik_grad_batch(delays, alpha, rho)
        dt = time.perf_counter() - t0
        assert info[0] == 0
        x0 = np.concatenate([alpha[0], rho, delays[0]])
        H_ = 1e-5 * np.maximum(np.abs(x0), 1.0)
        X = np.repeat(x0[None, :], 2 * len(x0), 0)
        for i in range(len(x0)):
            X[2 * i, i] += H_[i]
            X[2 * i + 1, i] -= H_[i]
        t1 = time.perf_counter()
        lf, _, finfo = obj.loglik_grad_batch(X[:, L + 1:], X[:, :L], X[:, L])
        dt_fd = time.perf_counter() - t1
        assert (finfo == 0).all()
        vl, vinfo = obj.loglik_batch(delays, alpha, rho)
    assert vinfo[0] == 0 and abs(ll[0] - vl[0]) <= 1e-10 * abs(vl[0])
    fd = (lf[0::2] - lf[1::2]) / (2 * H_)
    g = grad[0]
    err = np.max(np.abs(g - fd))
    print("N = 16384: one value + gradient %.3f s (first call, allocation included); %d more in one call %.3f s; "
          "|g - fd| / (1e-5 |g|) = %.3g" % (dt, len(X), dt_fd, err / (1e-5 * np.linalg.norm(g))))
    assert err <= 1e-5 * np.linalg.norm(g), (g, fd)
    assert abs(g[L + 1:].sum()) <= 1e-9 * np.linalg.norm(g[L + 1:])
