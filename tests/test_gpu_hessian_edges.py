"""gpcc_loglik_hess_batch and its block mode at the edges of their tile and band bookkeeping, block by block against the
extended-precision reference (tests/_hess_highprec.py): tile counts 1 to 6 with band boundaries on and next to tile edges, eight bands,
degenerate geometry, the corners of the hyper-parameter envelope, failures in a chosen tile, several groups per stream with a slot
reallocation, and a mutation check on three bands.

Every comparison uses _hess_highprec.ratio_blocks: per block (aa, ar, at, rr, rt, tt) error / bar, bar = 16 max(fp64 mirror's error,
torch witness's error, N 2^-53 max(|T1| + |T2| + |T3|)), every ingredient computed on the CPU.  The worst ratio per block of each group
is printed.  The references are computed in a pool of CPU processes that never touch the GPU."""
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _grad_highprec as GH
import _grad_witness as W
import _hess_highprec as HH
import gpcc_amd
from test_gpu_gradient_edges import GEOMETRY, KERNELS, _dyadic, _failure_data, _no_one_point_band_with_b
from test_gpu_hessian import _exact

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not HH.EXTENDED, reason=HH.SKIP_REASON)]


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


class Cases:
    """Device rows waiting for their references: add() per row, then check() compares them all and prints the worst ratios."""

    def __init__(self, group):
        self.group, self.jobs, self.rows = group, [], []

    def add(self, name, data, mb, delays, alpha, rho, out, i, label, faults=()):
        """out: loglik_hess_batch's result; i: its row"""
        self.jobs.append((name, *data, delays[i], alpha[i], rho[i], mb, tuple(faults)))
        self.rows.append((float(out[0][i]), np.array(out[1][i]), np.array(out[2][i]), np.array(out[3][i]), label))

    def check(self, pool, refs=None):
        worst, where, missed = {}, {}, []
        refs = list(pool.map(HH.reference_job, self.jobs)) if refs is None else refs
        for ref, (ll, g, H, F, label) in zip(refs, self.rows):
            assert ref.info == 0, (label, ref.info)
            assert abs(ll - ref.loglik) <= HH.value_bar(ref), (label, ll, ref.loglik)
            rg = GH.ratio(g, ref)
            assert rg <= 1.0, (label, rg, g, ref.grad, ref.cond)
            r = HH.ratio_blocks(H, F, ref)
            for b, v in r.items():
                if v >= worst.get(b, 0.0):
                    worst[b], where[b] = v, label
            if HH.worst(r) > 1.0:     # (every row that misses is reported before the group fails)
                missed.append(label)
                with np.printoptions(precision=17, linewidth=200):
                    print("MISSED %s: error / bar %s, cond_1(K) %.3g\n bars %s\n device H\n%s\n reference H\n%s\n device F\n%s\n"
                          " reference F\n%s" % (label, {b: "%.3g" % v for b, v in r.items()}, ref.cond, ref.bars, H, ref.H, F, ref.F))
            if ref.L == 1:
                assert not H[:, 2].any() and not F[:, 2].any(), (label, H)
        print("%s: %d rows, worst error / bar per block: %s" % (self.group, len(self.rows),
              ", ".join("%s %.3g %s" % (b, worst[b], (where[b],)) for b in HH.BLOCKS if b in worst)))
        assert not missed, (len(missed), missed)
        return refs


def _run(obj, delays, alpha, rho, exact=True):
    """The Hessian call with the gradient call, the block-mode call and loglik_batch on the same rows: one info, NaN rows where it is
    not 0, the gradient path's bits, bitwise symmetry, the hyper block bitwise the leading block; on the rows that factorised,
    test_gpu_hessian._exact (translation invariance and F >= 0 to 1e-9 of max |H|; exact=False leaves those two to the caller)."""
    out = obj.loglik_hess_batch(delays, alpha, rho)
    ll, grad, hess, fisher, info = out
    gl, gg, ginfo = obj.loglik_grad_batch(delays, alpha, rho)
    hl, hg, hh, hf, hinfo = obj.loglik_hess_hyper_batch(delays, alpha, rho)
    vl, vinfo = obj.loglik_batch(delays, alpha, rho)
    n = obj.L + 1
    assert np.array_equal(info, ginfo) and np.array_equal(info, vinfo) and np.array_equal(info, hinfo), (info, ginfo, vinfo, hinfo)
    ok = info == 0
    for a in (ll, grad, hess, fisher, vl, hl, hg, hh, hf):
        assert np.isnan(a[~ok]).all() and np.isfinite(a[ok]).all()
    assert np.array_equal(ll[ok], gl[ok]) and np.array_equal(grad[ok], gg[ok])
    assert np.array_equal(ll[ok], hl[ok]) and np.array_equal(grad[ok], hg[ok])
    assert np.array_equal(hh[ok], hess[ok][:, :n, :n]) and np.array_equal(hf[ok], fisher[ok][:, :n, :n])
    assert np.array_equal(hess[ok], np.swapaxes(hess[ok], 1, 2)) and np.array_equal(fisher[ok], np.swapaxes(fisher[ok], 1, 2))
    if exact:
        _exact(obj.L, ll[ok], grad[ok], hess[ok], fisher[ok], info[ok], gl[ok], gg[ok], ginfo[ok])
    return out


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
                    out = _run(obj, delays, alpha, rho)
                assert (out[4] == 0).all(), (N, name, mb, out[4])
                rows = range(3) if N < 200 else [(ki + mb) % 3]   # (the reference's time: one row per kernel and b-mode from N = 255)
                for i in rows:
                    cases.add(name, data, mb, delays, alpha, rho, out, i, (N, name, mb, i))
    cases.check(pool)


def test_many_bands(pool):
    cases = Cases("eight bands")
    layouts = [([1, 2, 3, 40, 127, 128, 129, 90], (False,)), ([2, 2, 3, 40, 127, 128, 129, 89], (True,)),
               ([16] * 8, (True, False))]
    for Nl, modes in layouts:
        data = W.ragged_data(Nl, seed=len(Nl) + Nl[0])
        delays, alpha, rho = W.random_params(8, 3, seed=Nl[0])
        for ki, name in enumerate(KERNELS):
            for mb in modes:
                with gpcc_amd.Objective(*data, KERNELS[name], marginalise_b=mb, slots_per_stream=8) as obj:
                    out = _run(obj, delays, alpha, rho)
                assert (out[4] == 0).all() and out[2].shape == (3, 17, 17)
                for i in (range(3) if sum(Nl) < 200 else [ki % 3]):   # (P = 17 at N = 520: one row per kernel)
                    cases.add(name, data, mb, delays, alpha, rho, out, i, (sum(Nl), Nl[0], name, mb, i))
        if Nl[0] == 1:
            _no_one_point_band_with_b(data, "OU")
    # N = 1030 on one row
    Nl = [1, 2, 3, 40, 127, 128, 129, 600]
    data = W.ragged_data(Nl, seed=5)
    delays, alpha, rho = W.random_params(8, 1, seed=6)
    with gpcc_amd.Objective(*data, gpcc_amd.matern52, marginalise_b=False, slots_per_stream=8) as obj:
        out = _run(obj, delays, alpha, rho)
    assert out[4][0] == 0
    cases.add("matern52", data, False, delays, alpha, rho, out, 0, (1030, "matern52"))
    cases.check(pool)


def test_degenerate_geometry(pool):
    cases = Cases("degenerate geometry")
    rg = np.random.default_rng(17)
    base = W.ragged_data([70, 60], seed=17)
    for d in base[0]:
        d[:] = _dyadic(d)
    geoms = []
    # points of both bands at exactly the same shifted time (s = 0 across bands: OU's convention at 0, twenty pairs)
    t = [base[0][0].copy(), base[0][1].copy()]
    t[1][::3] = t[0][:20][:len(t[1][::3])] + 1.5
    t[1] = np.sort(t[1])
    geoms.append(("coincident", (t, base[1], base[2]), [0.0, 1.5]))
    # a band of one point
    geoms.append(("one-point band", ([base[0][0], base[0][1][:1]], [base[1][0], base[1][1][:1]], [base[2][0], base[2][1][:1]]),
                  [0.0, 2.0]))
    # delays that put band 2 before band 1
    geoms.append(("reversed", ([base[0][0], base[0][1] + 40.0], base[1], base[2]), [0.0, 80.0]))
    # a delay so large that the bands do not overlap: k and its derivatives are 0 between them
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
                    out = _run(obj, delays, alpha, rho)
                assert (out[4] == 0).all(), (label, name, mb, out[4])
                if label == "disjoint":
                    # every cross-band table is exactly zero: H and F are block diagonal over the bands, every delay entry is zero
                    for A in (out[2], out[3]):
                        assert not A[:, 0, 1].any() and not A[:, 3:, :].any(), (name, mb, A)
                for i in range(M):
                    cases.add(name, data, mb, delays, alpha, rho, out, i, (label, name, mb, i))
    refs = cases.check(pool)
    assert sum(r.ties for r in refs) == 2 * 4 * 2     # (the coincident rows, and only they)


def test_hyperparameter_envelope(pool):
    """alpha in {1e-2, 1e2}, rho in {0.05, 300}, sigma in {0.05, 1}: where the device factorises, every block meets its bar, which
    scales with the conditioning through the fp64 mirror's error; where it does not, the row is NaN with loglik_batch's info (_run).
    At most a quarter of the rows may fail on the device, and the extended reference factorises every row the device does.
    (test_gpu_hessian._exact's fixed 1e-9 max |H| does not scale with cond_1(K), 1.6e9 here: translation invariance is held to the
    blocks' bars instead, L bars per row sum.)

    Measured on an MI355X: no row fails to factorise and every row is within its bars, worst error / bar aa 0.92, ar 0.63, at 0.16,
    rr 0.52, rt 0.62, tt 0.31 or less.  Three rows at N = 40, sigma = 0.05, alpha = 100, rho = 300 stood out at rr 2.7 and tt 3.3
    before the mirror ran the device's blocks of 16 (_hess_highprec.py); they are at rr <= 0.23, rt <= 0.62, tt <= 0.14."""
    cases = Cases("hyper-parameter envelope")
    combos = [(a, r) for a in (1e-2, 1e2) for r in (0.05, 300.0)]
    failed = total = 0
    rows = []
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
                        out = _run(obj, delays, alpha, rho, exact=False)
                    for i in range(len(combos)):
                        total += 1
                        if out[4][i] != 0:
                            failed += 1
                            continue
                        cases.add(name, data, mb, delays, alpha, rho, out, i, (sum(Nl), sig, name, mb) + combos[i])
                        rows.append((out[2][i], out[3][i]))
    print("hyper-parameter envelope: %d of %d rows failed on the device (NaN, loglik_batch's info)" % (failed, total))
    assert 4 * failed <= total
    refs = cases.check(pool)
    L = 2
    for ref, (H, F) in zip(refs, rows):
        for which, A in (("H", H), ("F", F)):
            s = np.abs(A[:, L + 1:].sum(1))
            bars = ref.bars[which]
            assert (s[:L] <= L * bars["at"]).all() and s[L] <= L * bars["rt"] and (s[L + 1:] <= L * bars["tt"]).all(), (which, A, bars)


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
        out = _run(obj, delays, alpha, rho)
        ll, grad, hess, fisher, info = out
        print("failure rows: info %s (expected %s)" % (info, want))
        assert list(info) == want
        bad = np.array(want) > 0
        assert np.isnan(ll[bad]).all() and np.isnan(grad[bad]).all() and np.isnan(hess[bad]).all() and np.isnan(fisher[bad]).all()
        for i in np.flatnonzero(~bad):
            one = obj.loglik_hess_batch(delays[i:i + 1], alpha[i:i + 1], rho[i:i + 1])
            for x, y in zip(one, out):
                assert np.array_equal(x[0], y[i]), i
            cases.add("OU", data, False, delays, alpha, rho, out, i, ("valid row", i))
    cases.check(pool)


@pytest.mark.parametrize("N", [257, 1030])
def test_several_groups_per_stream_and_reallocation(pool, N):
    """slots_per_stream = 4, then 3, on 2 streams: M = 19 at N = 257, M = 11 at N = 1030 (several groups per stream).  Bitwise equal
    to a default handle and to one-row calls, before and after the slot count changes (ensure_hess reallocates: hess_slots follows),
    with full and block-mode calls interleaved on the one handle."""
    name, Nl, M = ("matern32", [128, 129], 19) if N == 257 else ("OU", [400, 330, 300], 11)
    data = W.ragged_data(Nl, seed=N)
    L = len(Nl)
    delays, alpha, rho = W.random_params(L, M, seed=N)
    with gpcc_amd.Objective(*data, KERNELS[name]) as ref_obj:
        ref = ref_obj.loglik_hess_batch(delays, alpha, rho)
    assert (ref[4] == 0).all()
    with gpcc_amd.Objective(*data, KERNELS[name], slots_per_stream=4, streams=2) as obj:
        assert obj.get_option("hess_slots") == 0
        for slots in (4, 3):
            obj.set_option("slots_per_stream", slots)
            blk = obj.loglik_hess_hyper_batch(delays, alpha, rho)
            got = obj.loglik_hess_batch(delays, alpha, rho)
            blk2 = obj.loglik_hess_hyper_batch(delays, alpha, rho)
            assert obj.get_option("workspace_slots") == slots and obj.get_option("workspace_streams") == 2
            assert obj.get_option("hess_slots") == 2 * slots
            for x, y in zip(got, ref):
                assert np.array_equal(x, y), slots
            for b in (blk, blk2):
                assert np.array_equal(b[0], ref[0]) and np.array_equal(b[1], ref[1]) and np.array_equal(b[4], ref[4])
                assert np.array_equal(b[2], ref[2][:, :L + 1, :L + 1]) and np.array_equal(b[3], ref[3][:, :L + 1, :L + 1]), slots
        for i in range(M):
            one = obj.loglik_hess_batch(delays[i:i + 1], alpha[i:i + 1], rho[i:i + 1])
            for x, y in zip(one, ref):
                assert np.array_equal(x[0], y[i]), i
        _run(obj, delays[:3], alpha[:3], rho[:3])
    cases = Cases("several groups per stream, N = %d" % N)
    cases.add(name, data, True, delays, alpha, rho, ref, 0, (N, 0))
    cases.check(pool)


MUTATIONS = [("k2_scale", 3, 1 + 1e-6), ("even_sign", 4, 1, 0), ("even_sign_tab", 4), ("no_delta_tt", 1), ("t3_once", 2, 1),
             ("no_delta_at", 2), ("drop_transpose", 2, 2, 0)]


@pytest.mark.parametrize("name", ["matern32", "OU"])
def test_device_against_mutated_references_on_three_bands(pool, name):
    """N = 300 in three bands (three tiles), delays in play: the device's H and F are within the bars of the clean reference and
    outside them for each faulted recomputation (k_rr off by 1e-6, the sign of RS in one tile and in the finish, the delta_lm terms,
    one T3 tile pair counted once, one transposed table pair dropped)."""
    data, delays, alpha, rho = HH.mutation_data(ties=(name == "OU"))
    delays, alpha, rho = delays[None, :], alpha[None, :], np.array([rho])
    faults = MUTATIONS + ([("ou_kss0", -1), ("ou_kss0", 0)] if name == "OU" else [])
    cases = Cases("three-band mutation check, %s" % name)
    with gpcc_amd.Objective(*data, KERNELS[name]) as obj:
        out = _run(obj, delays, alpha, rho)
    assert out[4][0] == 0
    cases.add(name, data, True, delays, alpha, rho, out, 0, (name, 300), faults=faults)
    ref = cases.check(pool)[0]
    assert ref.ties == (name == "OU")
    closest = np.inf
    for f in faults:
        r = HH.worst(HH.ratio_blocks(out[2][0], out[3][0], ref, against=ref.faulted[f]))
        assert r > 1.0, (f, r)
        closest = min(closest, r)
    print("%s: the device is outside the bars of %d faulted references; closest at %.3g x the bar" % (name, len(faults), closest))
