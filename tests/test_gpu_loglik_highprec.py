"""gpcc_loglik_batch on every factorisation path (the table) against the extended-precision value
(tests/_loglik_highprec.py), at the smallest sizes at which each path's bookkeeping can go wrong: N = 2 ... 1025, four kernels, both
b-modes, three rows of every group (the first, the last, row 2: a random row, rho = 0.1, and rho = 300 with alpha = 2).

Every row is held to both bars of _loglik_highprec (the inner one sees a tile that passed through fp32; the outer one is the
project's value bar).  A path is forced by options that exist, and shown to have run by the library's counters where it has one:
small_n_count, chain_count, fp32_chain_count, and profile_get()'s launches per kind (profiling keeps a group in one piece, so the
configurations that run a group as two halves are checked by value alone).

The references do not depend on the path: all 288 are queued once per module in a pool of CPU processes that never touch the
GPU, smallest first, and a test waits for the ones it needs.  Every (path, N) prints its worst error / bar in a line that starts
with "highprec-loglik"; profiles/loglik/highprec_parity.log keeps them."""
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import pytest

import _loglik_highprec as V

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not V.EXTENDED, reason=V.SKIP_REASON)]

SMALL = [N for N in V.CASES if N <= 383]
ONE_WAVE = [N for N in V.CASES if N <= 191]
TILED = [N for N in V.CASES if N >= 384]


@pytest.fixture(scope="module")
def gp():
    import torch
    torch.cuda.init()
    import gpcc_amd
    return gpcc_amd


@pytest.fixture(scope="module")
def refs():
    """{(N, kernel, mb, row): future of (key, Value)}."""
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield {key: ex.submit(V.job, key) for key in V.all_keys(sorted(V.CASES))}


class Path:
    """The rows of one path: run() evaluates a group on a handle and queues its three rows, report() compares them all and
    prints one line per size."""

    def __init__(self, name, refs):
        self.name, self.refs, self.rows = name, refs, []

    def run(self, obj, N, kernel, mb, M, what=""):
        delays, alpha, rho, which = V.group(N, M)
        ll, info = obj.loglik_batch(delays, alpha, rho)
        assert (info == 0).all(), (self.name, N, kernel, mb, M, what, info)
        for at, src in which.items():
            self.rows.append(((N, kernel, mb, src), float(ll[at]), (M, at, what)))
        return ll

    def report(self):
        worst = {}
        for key, x, where in self.rows:
            v = self.refs[key].result()[1]
            assert v.info == 0 and v.cond <= V.COND_MAX, (key, v)
            rin, rout = V.ratios(x, v)
            w = worst.setdefault(key[0], [0.0, 0.0, 0, 0.0])
            w[0], w[1], w[2] = max(w[0], rin), max(w[1], rout), w[2] + 1
            w[3] = max(w[3], abs(x - v.loglik) / V.inner_bar(v, u=0.0))      # (a record: the inner bar without its element term)
        for N, (rin, rout, n, rsum) in sorted(worst.items()):
            print("highprec-loglik %-34s N = %4d: %4d rows, worst error / inner bar %.3g, / outer bar %.3g  (/ the summation term alone %.3g)"
                  % (self.name, N, n, rin, rout, rsum))
        for key, x, where in self.rows:
            v = self.refs[key].result()[1]
            rin, rout = V.ratios(x, v)
            assert rin <= 1.0 and rout <= 1.0, (self.name, key, where, rin, rout, x, v.loglik)


def handles(gp, sizes, slots=40, kernels=V.KERNELS, **kw):
    for N in sizes:
        for kernel in kernels:
            for mb in V.modes(N):
                with gp.Objective(*V.data(N), kernel, marginalise_b=mb, slots_per_stream=slots, **kw) as obj:
                    yield N, kernel, mb, obj


def launches(obj, fn):
    """{kind: launches} of fn() with the profile on (one group in one piece on one stream)."""
    obj.profile(True)
    obj.profile_reset()
    fn()
    out = {k: n for k, (n, _) in obj.profile_get().items()}
    obj.profile(False)
    return out


def counted(obj, key, fn):
    before = obj.get_option(key)
    fn()
    return obj.get_option(key) - before


def test_oracle_for_comparison(refs):
    worst = {}
    for key, f in refs.items():
        v = f.result()[1]
        assert v.info == 0 and v.cond <= V.COND_MAX, (key, v)
        rin, rout = V.ratios(v.oracle, v)
        w = worst.setdefault(key[0], [0.0, 0.0])
        w[0], w[1] = max(w[0], rin), max(w[1], rout)
    for N, (rin, rout) in sorted(worst.items()):
        print("highprec-loglik %-34s N = %4d: worst error / inner bar %.3g, / outer bar %.3g" % ("(the CPU oracle)", N, rin, rout))


def test_small_n_one_wave_per_evaluation(gp, refs):
    path = Path("small-N, one wave", refs)
    for N, kernel, mb, obj in handles(gp, ONE_WAVE):
        obj.set_option("small_wide_max", 0)
        assert counted(obj, "small_n_count", lambda: path.run(obj, N, kernel, mb, 40)) == 40
        n = launches(obj, lambda: path.run(obj, N, kernel, mb, 2))
        assert n["small_eval"] == 1 and sum(n.values()) == 1 and obj.get_option("chain_count") == 0
    path.report()


def test_small_n_four_waves_per_evaluation(gp, refs):
    path = Path("small-N, four waves", refs)
    for N, kernel, mb, obj in handles(gp, SMALL):
        assert obj.get_option("small_n_active") == 1
        assert counted(obj, "small_n_count", lambda: path.run(obj, N, kernel, mb, 40)) == 40
        if N <= 191:
            obj.set_option("small_wide_max", 256)
            assert counted(obj, "small_n_count", lambda: path.run(obj, N, kernel, mb, 40, "small_wide_max = 256")) == 40
        n = launches(obj, lambda: path.run(obj, N, kernel, mb, 1))
        assert n["small_eval"] == 1 and sum(n.values()) == 1
    path.report()


def test_tile_kernels_at_small_n(gp, refs):
    """small_n = 0: one tile (N = 2, 111: the diagonal step alone) and three tiles (N = 383: the persistent launch for 5
    evaluations, the left-looking trio for 40)."""
    path = Path("tile kernels, small_n = 0", refs)
    for N, kernel, mb, obj in handles(gp, [2, 111, 383]):
        obj.set_option("small_n", 0)
        assert obj.get_option("small_n_active") == 0
        took = counted(obj, "chain_count", lambda: path.run(obj, N, kernel, mb, 5))
        assert took == (5 if N > 128 else 0)
        n = launches(obj, lambda: path.run(obj, N, kernel, mb, 40))
        assert n["small_eval"] == 0 and n["diag_factor"] == (N + 127) // 128 and obj.get_option("small_n_count") == 0
    path.report()


@pytest.mark.parametrize("N", TILED)
def test_persistent_launch(gp, refs, N):
    """1 and 2 evaluations (quarter-tile updates), 5 (helpers), 12, 13 (the wide policy: 13 nt^2 <= 1024), and at N = 1025 column
    blocks of 8 / 4 / 2 / 1 (chain_batch_min = 1)."""
    path = Path("persistent launch", refs)
    nt = (N + 127) // 128
    for N, kernel, mb, obj in handles(gp, [N], slots=16):
        for M in (1, 2, 5, 12, 13):
            took = counted(obj, "chain_count", lambda: path.run(obj, N, kernel, mb, M))
            assert took == (M if M <= 12 or M * nt * nt <= 1024 else 0), (N, M, took)
        if N == 1025:
            obj.set_option("chain_batch_min", 1)
            for M in (1, 5):
                assert counted(obj, "chain_count", lambda: path.run(obj, N, kernel, mb, M, "chain_batch_min = 1")) == M
    path.report()


@pytest.mark.parametrize("N", TILED)
def test_right_looking_few_evaluations(gp, refs, N):
    path = Path("right-looking, few evaluations", refs)
    nt = (N + 127) // 128
    for N, kernel, mb, obj in handles(gp, [N], slots=16):
        obj.set_option("chain_max", 0)
        for M in (1, 5, 12):
            n = launches(obj, lambda: path.run(obj, N, kernel, mb, M))
            assert n["small_step"] == nt - 1 and n["panel_trsm"] == nt - 1 and n["diag_factor"] == 1 and n["panel_update"] == 0, (M, n)
            path.run(obj, N, kernel, mb, M, "unprofiled")
        assert obj.get_option("chain_count") == 0
    path.report()


@pytest.mark.parametrize("N", TILED)
def test_three_kernel_left_looking(gp, refs, N):
    """chain_max = 0, fold = 2: 13 and 40 evaluations in one piece (split_min = 0), with and without the right-looking tail
    (it needs 6 tiles), 13 by default (two right-looking halves), 40 as two halves (split_nt_min = 2)."""
    path = Path("three-kernel left-looking", refs)
    nt = (N + 127) // 128
    for N, kernel, mb, obj in handles(gp, [N]):
        obj.set_option("chain_max", 0)
        path.run(obj, N, kernel, mb, 13, "default: two halves")
        path.run(obj, N, kernel, mb, 40, "default")
        obj.set_option("split_nt_min", 2)
        path.run(obj, N, kernel, mb, 40, "split_nt_min = 2: two halves")
        obj.set_option("split_min", 0)
        for tail in ((1, 0) if nt >= 6 else (1,)):
            obj.set_option("hybrid_tail", tail)
            for M in (13, 40):
                n = launches(obj, lambda: path.run(obj, N, kernel, mb, M, "split_min = 0, hybrid_tail = %d" % tail))
                assert n["diag_factor"] == nt and n["panel_trsm"] == nt - 1 and n["small_step"] == 0 and n["panel_update"] >= nt - 1, (M, n)
                path.run(obj, N, kernel, mb, M, "split_min = 0, hybrid_tail = %d, unprofiled" % tail)
        assert obj.get_option("chain_count") == 0
    path.report()


@pytest.mark.parametrize("N", TILED)
def test_fused_update_solve(gp, refs, N):
    """fold = 1: 13 evaluations with fused_solve_min = 13 (chain_max = 0, in one piece), with and without the fold; at N = 641
    also the benchmarked group size, 112 at default options."""
    path = Path("fused update-solve", refs)
    nt = (N + 127) // 128
    for N, kernel, mb, obj in handles(gp, [N], slots=112 if N == 641 else 16):
        if N == 641:
            n = launches(obj, lambda: path.run(obj, N, kernel, mb, 112, "default"))
            assert n["diag_factor"] == nt and n["panel_update"] == nt - 1 and n["panel_trsm"] == 0 and n["small_step"] == 0, n
            path.run(obj, N, kernel, mb, 112, "default, unprofiled")
        for key, value in (("chain_max", 0), ("split_min", 0), ("fused_solve_min", 13)):
            obj.set_option(key, value)
        for fold in (1, 0):
            obj.set_option("fold_assembly", fold)
            n = launches(obj, lambda: path.run(obj, N, kernel, mb, 13, "fold_assembly = %d" % fold))
            assert n["diag_factor"] == nt and n["panel_update"] == nt - 1 and n["panel_trsm"] == 0 and n["small_step"] == 0, n
            path.run(obj, N, kernel, mb, 13, "fold_assembly = %d, unprofiled" % fold)
        assert obj.get_option("chain_count") == 0
    path.report()


def test_fp32_handle_on_its_fp64_twin(gp, refs):
    """One evaluation on an fp32 handle goes to its fp64 twin's persistent launch: fp64 bits, the same bars."""
    path = Path("fp32 handle, fp64 twin", refs)
    for N, kernel, mb, obj in handles(gp, [641], slots=16, precision="fp32"):
        assert counted(obj, "fp32_chain_count", lambda: path.run(obj, N, kernel, mb, 1)) == 1
        assert obj.get_option("fp32_guard_count") == 0
    path.report()


def test_device_elements_within_the_ulps_the_inner_bar_allows(gp):
    """The device's elements (gpcc_model_matrix: the table exp, the separable products) against the extended-precision ones, as the
    value feels them (_loglik_highprec.element_ulps): within U ulps where b is marginalised -- there U's term is the inner bar --
    and their first-order displacement inside the inner bar on every row."""
    jobs = []
    for N, kernel, mb, obj in handles(gp, [385], slots=2):
        delays, alpha, rho = V.rows(N)
        for row in V.ROWS:
            jobs.append(((N, kernel, mb, row), obj.model_matrix(delays[row], alpha[row], rho[row])))
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        out = list(ex.map(V.element_job, jobs))
        vals = dict(ex.map(V.job, [key for key, _ in jobs]))
    worst_u = worst_d = 0.0
    for (key, _), (u, d) in zip(jobs, out):
        r = d / V.inner_bar(vals[key])
        print("highprec-loglik device elements %s: %.3f ulps as the value feels them, first-order displacement / inner bar %.3g" % (key, u, r))
        worst_d = max(worst_d, r)
        if key[2]:
            worst_u = max(worst_u, u)
    print("highprec-loglik device elements: worst u with b %.3f (U = %g), worst first-order displacement / inner bar %.3g" % (worst_u, V.U, worst_d))
    assert worst_u <= V.U and worst_d <= 1.0
