"""The value reference of tests/_loglik_highprec.py checked on the CPU: the value-only route against the full evaluate (the same
bits) and against mpmath, every case of the device tests (info, cond, the oracle against both bars), the fp64 tiled restatement
against the inner bar, and the inner bar against every slip tile_value can make, in every place it can make it.

The cases run once, in a pool of processes (one job per (N, kernel, b-mode): three references, three clean restatements and, for
OU and rbf, the faults)."""
import collections
import multiprocessing
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _grad_highprec as H
import _grad_witness as W
import _loglik_highprec as V

pytestmark = pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)

FAULT_KERNELS = ("OU", "rbf")


@pytest.fixture(scope="module")
def scan():
    """{(N, kernel, mb): ([Value per row], [clean error / inner bar per row], {fault: record})} (_loglik_highprec.case_job)."""
    jobs = [((N, k, mb), k in FAULT_KERNELS) for N in sorted(V.CASES, reverse=True) for k in V.KERNELS for mb in V.modes(N)]
    t0 = time.perf_counter()
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        out = {case: rest for case, *rest in ex.map(V.case_job, jobs)}
    print("%d cases (%d references) in %.1f s" % (len(out), 3 * len(out), time.perf_counter() - t0))
    return out


@pytest.mark.parametrize("Nl,kernel,mb", [([65, 64], "OU", True), ([65, 64], "matern52", False), ([129, 127, 129], "rbf", False),
                                          ([128, 384, 129], "matern32", True)])
def test_value_only_route_gives_the_full_reference_bits(Nl, kernel, mb):
    N = sum(Nl)
    data = W.ragged_data(Nl, seed=N)
    delays, alpha, rho = W.random_params(len(Nl), 1, seed=N + 1)
    t0 = time.perf_counter()
    full = H.evaluate(kernel, *data, delays[0], alpha[0], rho[0], mb)
    t1 = time.perf_counter()
    only = H.evaluate(kernel, *data, delays[0], alpha[0], rho[0], mb, value_only=True)
    t2 = time.perf_counter()
    print("N = %d %s: full reference %.2f s, value only %.2f s" % (N, kernel, t1 - t0, t2 - t1))
    assert full.info == 0 and only.info == 0
    assert only.loglik == full.loglik
    assert abs(only.cond - full.cond) <= 1e-6 * full.cond        # (fp64 LAPACK against the extended inverse: it scales a bar)


@pytest.mark.parametrize("kernel", V.KERNELS)
@pytest.mark.parametrize("mb", [True, False])
def test_value_only_reference_against_mpmath(kernel, mb):
    """The 40-digit log-likelihood of test_grad_highprec_cpu.py's case, from the reference formulas."""
    mp = pytest.importorskip("mpmath").mp
    from test_grad_highprec_cpu import _mp_loglik
    mp.dps = 40
    data = W.ragged_data([13, 11], seed=3 + V.KERNELS.index(kernel))
    delays, alpha, rho = np.array([0.0, 1.25]), np.array([0.9, 1.4]), 2.5
    ref = H.evaluate(kernel, *data, delays, alpha, rho, mb, value_only=True)
    x = [mp.mpf(float(v)) for v in np.concatenate([alpha, [rho], delays])]
    ll = _mp_loglik(mp, kernel, *data, x[3:], x[:2], x[2], mb)
    assert ref.info == 0 and abs(float(ll) - ref.loglik) <= 1e-15 * abs(ref.loglik)


def test_groups_carry_the_reference_rows():
    for N in (2, 385):
        d3, a3, r3 = V.rows(N)
        assert r3[1] == 0.1 and r3[2] == 300.0 and (a3[2] == 2.0).all()
        for M in (1, 2, 3, 5, 40):
            d, a, r, which = V.group(N, M)
            assert d.shape == (M, len(V.CASES[N])) and which == {1: {0: 0}, 2: {0: 0, 1: 1}, 3: {0: 0, 1: 1, 2: 2}}.get(M, {0: 0, 2: 2, M - 1: 1})
            for at, src in which.items():
                assert np.array_equal(d[at], d3[src]) and np.array_equal(a[at], a3[src]) and r[at] == r3[src]
            if M >= 2:
                assert r[1] == 0.1          # (row 1 is at rho = 0.1 whether it is compared or not)


def test_every_case_factorises_and_the_oracle_is_inside_both_bars(scan):
    worst_in = worst_out = worst_cond = slowest = 0.0
    for case, (vals, _, _) in scan.items():
        for row, v in enumerate(vals):
            assert v.info == 0, (case, row, v.info)
            assert v.cond <= V.COND_MAX, (case, row, v.cond)
            rin, rout = V.ratios(v.oracle, v)
            assert rin <= 1.0 and rout <= 1.0, (case, row, rin, rout)
            worst_in, worst_out, worst_cond, slowest = max(worst_in, rin), max(worst_out, rout), max(worst_cond, v.cond), max(slowest, v.seconds)
    print("oracle: worst error / inner bar %.3g, / outer bar %.3g; largest cond_1(K) %.3g; slowest value-only reference %.2f s (in the pool)"
          % (worst_in, worst_out, worst_cond, slowest))


def test_tiled_restatement_is_inside_the_inner_bar(scan):
    worst, where = 0.0, None
    for case, (_, clean, _) in scan.items():
        for row, r in enumerate(clean):
            if case[0] >= 129:
                assert r <= 1.0, (case, row, r)
            if r >= worst:
                worst, where = r, case + (row,)
    print("fp64 tile_value: worst error / inner bar %.3g %s" % (worst, where))


@pytest.mark.parametrize("kernel", V.KERNELS)
def test_fp64_elements_are_within_the_ulps_the_inner_bar_allows(oracle, kernel):
    """The elements of the two fp64 assemblies on the CPU against the extended ones, as the value feels them (element_ulps): within
    U ulps where b is marginalised (there U's term is the bar), and their first-order displacement inside the bar on every row."""
    for N, mb, row in ((160, True, 0), (385, True, 2), (385, True, 1), (385, False, 1)):
        key = (N, kernel, mb, row)
        args = V.args_of(*key)
        v = V.reference(args)
        K, _ = oracle.model_matrix(*args)
        (u_oracle, d_oracle), (u_tile, d_tile) = V.element_ulps(key, K), V.element_ulps(key, V.prepare(args)["Kp"][:N, :N])
        print("%s: elements off by %.3f ulps (oracle), %.3f (tile_value); first-order displacement / inner bar %.3g, %.3g"
              % (key, u_oracle, u_tile, d_oracle / V.inner_bar(v), d_tile / V.inner_bar(v)))
        assert max(d_oracle, d_tile) <= V.inner_bar(v)
        if mb:
            assert max(u_oracle, u_tile) <= V.U


def test_inner_bar_rejects_every_injected_fault(scan):
    """Every fault of tile_value in every place it exists, on the OU and rbf cases of every size and b-mode: the comparison the device
    test makes -- its three rows against the inner bar -- must reject it on at least one row.  Not asserted, but counted: the
    dropped k-slices and skipped z blocks of OU without b that no row rejects.  There K is the covariance of a Markov process
    plus noise, the factor's tiles away from the diagonal are themselves below 1e-8 of it, and the value moves by less than an
    honest fp64 run's own rounding (|faulted - clean| <= 2 bars on all three rows): nothing a test of the value could see.
    For the record: the instances whose displacement on row 0 is below 1e-8 relative, invisible to the oracle tests' tolerance."""
    total, below, by_row, unseen = (collections.Counter() for _ in range(4))
    smallest = {}
    for case, (vals, _, table) in scan.items():
        if case[1] not in FAULT_KERNELS:
            continue
        assert table, case
        for f, (hit, rel, moved) in table.items():
            total[f[0]] += 1
            below[f[0]] += rel < 1e-8
            by_row[hit] += 1
            if hit is None:
                assert case[1] == "OU" and not case[2] and f[0] in ("drop_kslice", "z_skip"), (case, f, rel, moved)
                assert moved <= 2.0, (case, f, moved)
                unseen[(case[0], f[0])] += 1
    for kind in total:
        print("%-12s %5d instances, %4d below 1e-8 relative on row 0" % (kind, total[kind], below[kind]))
    print("rejected on row 0: %d, only on row 2: %d, only on row 1: %d; unseen (OU without b): %s"
          % (by_row[0], by_row[2], by_row[1], dict(unseen)))
    assert set(total) == {"fp32_tile", "drop_kslice", "z_skip", "pad_logdet", "pad_rhs", "b_straddle", "sep_single"}
