"""A row's bits do not depend on the launch shape (gpcc_markov.hip.h; markov_launch of gpcc_hip.hip): the nine linear-time entries on
batches whose kernels run four and two waves per workgroup, with a ragged last workgroup, bitwise against the same rows in calls of
at most 64 rows -- one wave, one workgroup along x.  The launcher counts ceil(rows / 64) * ny waves, ny being the kernel's lanes per
row (its grid's y), and takes one wave per workgroup up to C waves (C: the device's CUs), two up to 2 C and four beyond.

Two tiny problems, so that a call takes milliseconds: Matern-3/2 with bands of 7 and 5 points and marginalised offsets (<2, 2>), and
OU with bands of 6, 5 and 4 points and fixed offsets (<1, 0>).  Per entry a batch of 128 C + 1 rows (above 2 C waves in every
kernel) and one whose widest kernel -- the one the entry adds to those it shares -- has between C and 2 C waves; for the draws one
row with that many draws, the lanes of one gpcc_markov_draw launch.  The last row fails (alpha <= 0): it is alone in the last
workgroup, whose other lanes compute it again and store nothing.  No tolerance: the reference is the library's own one-wave launch."""
import numpy as np
import pytest

import _markov_cases as MC
import gpcc_amd

pytestmark = pytest.mark.gpu

PROBLEMS = {"matern32-b": ("matern32", [7, 5], True, [3, 2]), "OU-fixed": ("OU", [6, 5, 4], False, [2, 3, 2])}
KERN = {"OU": gpcc_amd.OU, "matern32": gpcc_amd.matern32}
_open = {}


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _problem(name):
    """The handle of a problem (kept for the module), its test points and their observations."""
    if name not in _open:
        kernel, Nl, mb, Nt = PROBLEMS[name]
        t, y, s, _ = MC.lightcurves(Nl, seed=31 + len(Nl), kind="plain")
        rg = np.random.default_rng(5 + len(Nl))
        tt = [MC.snap(rg.uniform(-2.0, 32.0, n)) for n in Nt]
        yt = [np.sin(0.4 * a) + 0.3 * l + 0.2 * rg.standard_normal(len(a)) for l, a in enumerate(tt)]
        st = [0.1 + 0.1 * rg.random(n) for n in Nt]
        _open[name] = (gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=mb), tt, yt, st)
    return _open[name]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for obj, _, _, _ in _open.values():
        obj.close()
    _open.clear()


def _rows(L, M, seed):
    """M rows (tau, alpha, rho); the last one fails."""
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 8.0, (M, L - 1)))], 1)
    alpha, rho = rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))
    alpha[M - 1, L - 1] = -0.5
    return delays, alpha, rho


# entry -> (the call: every output array of the rows handed over, ny of the kernel the entry adds (L bands, OU or not))
def _loo(obj, d, a, r, tt, yt, st):
    o = obj.loo_markov_batch(d, a, r)
    return o.mu, o.var, o.lp, o.loo, o.loglik, o.info


ENTRIES = {
    "loglik": (lambda obj, d, a, r, tt, yt, st: obj.loglik_markov_batch(d, a, r), lambda L, ou: 1),
    "grad": (lambda obj, d, a, r, tt, yt, st: obj.loglik_grad_markov_batch(d, a, r), lambda L, ou: L + 1 + (2 * L if ou else L)),
    "hess_hyper": (lambda obj, d, a, r, tt, yt, st: obj.loglik_hess_hyper_markov_batch(d, a, r), lambda L, ou: (L + 1) * (L + 2) // 2),
    "hess": (lambda obj, d, a, r, tt, yt, st: obj.loglik_hess_markov_batch(d, a, r), lambda L, ou: L * L + 2 * L + L * (L - 1) // 2),
    "predict": (lambda obj, d, a, r, tt, yt, st: obj.predict_markov_batch(d, a, r, tt)[:4], lambda L, ou: 2),
    "heldout": (lambda obj, d, a, r, tt, yt, st: obj.heldout_loglik_markov_batch(d, a, r, tt, yt, st)[:3], lambda L, ou: 2),
    "postb": (lambda obj, d, a, r, tt, yt, st: obj.posterior_offsets_markov_batch(d, a, r), lambda L, ou: 1),
    "loo": (_loo, lambda L, ou: 2),
}
CASES = [(p, e) for p in PROBLEMS for e in ENTRIES if not (e == "postb" and not PROBLEMS[p][2])]


def _batch_rows(C, ny, waves_per_workgroup):
    """M with a ragged last workgroup of one row: four waves per workgroup: 128 C + 1; two: ceil(M / 64) ny between C and 2 C."""
    if waves_per_workgroup == 4:
        return 128 * C + 1
    blocks = (3 * C // 2) // ny
    blocks -= 1 - blocks % 2               # odd: M - 1 is a multiple of the workgroup's 128 rows
    return 64 * (blocks - 1) + 1


def _windows(M, rows_per_workgroup):
    """(first row, rows <= 64): the first 64 rows, the last 65 (the last workgroup holds row M - 1 alone), three windows across a
    boundary between two full workgroups."""
    nb = (M + rows_per_workgroup - 1) // rows_per_workgroup
    w = [(0, 64), (M - 65, 64), (M - 1, 1)]
    for k in sorted({1, nb // 2, nb - 2}):
        w.append((k * rows_per_workgroup - 32, 64))
    assert all(0 <= r0 and r0 + n <= M for r0, n in w) and nb >= 4 and M % rows_per_workgroup == 1
    return w


@pytest.mark.parametrize("wpw", [4, 2])
@pytest.mark.parametrize("problem,entry", CASES)
def test_rows_do_not_depend_on_the_launch_shape(problem, entry, wpw):
    obj, tt, yt, st = _problem(problem)
    kernel, Nl, mb, _ = PROBLEMS[problem]
    call, ny_of = ENTRIES[entry]
    L, C = len(Nl), _cus()
    ny = ny_of(L, kernel == "OU")
    M = _batch_rows(C, ny, wpw)
    waves = (M + 63) // 64 * ny
    assert waves > 2 * C if wpw == 4 else C < waves <= 2 * C, (M, ny, C)
    delays, alpha, rho = _rows(L, M, seed=M + ny)
    big = call(obj, delays, alpha, rho, tt, yt, st)
    info = big[-1]
    assert info[M - 1] != 0 and (info[:M - 1] == 0).all()                     # the failing row alone
    assert all(np.isnan(x[M - 1]).all() for x in big[:-1]) and np.isfinite(big[0][:M - 1]).all()
    for r0, n in _windows(M, 64 * wpw):
        sl = slice(r0, r0 + n)
        small = call(obj, delays[sl], alpha[sl], rho[sl], tt, yt, st)
        assert len(small) == len(big)
        for k, (x, y) in enumerate(zip(big, small)):
            assert np.array_equal(x[sl], y, equal_nan=True), (problem, entry, M, r0, k)


# ---- staged against unstaged light curves for the same row ---------------------------------------------------------------------------
STAGING_NL = [600] * 8
LDS_MAX = 156 * 1024                              # GPCC_MARKOV_LDS_MAX (gpcc_markov.hip.h)
# entry -> (the call, bytes per lane and band beside the staged light curves (GPCC_MARKOV_LANE_BYTES, + GPCC_MARKOV_NOISE_LANE_BYTES),
#           ny of the entry's widest kernel)
STAGING_ENTRIES = {
    "loglik": (lambda obj, d, a, r, kap, nu: obj.loglik_markov_batch(d, a, r), 28, lambda L, ou: 1),
    "noise": (lambda obj, d, a, r, kap, nu: obj.loglik_markov_noise_batch(d, a, r, kap, nu), 44, lambda L, ou: 1),
    "grad": (lambda obj, d, a, r, kap, nu: obj.loglik_grad_markov_batch(d, a, r), 28, ENTRIES["grad"][1]),
}


def _lds_bytes(N, L, threads, lane_bytes):
    """gpcc_markov_lds_bytes / gpcc_markov_noise_lds_bytes with the light curves staged."""
    return 24 * N + lane_bytes * L * threads


@pytest.mark.parametrize("entry", list(STAGING_ENTRIES))
@pytest.mark.parametrize("kernel", ["OU", "matern32"])
def test_rows_do_not_depend_on_staging(kernel, entry):
    """Eight bands of 600 points (N = 4800), fixed offsets: beside the lanes' part of a workgroup of 64 lanes the light curves fit the LDS
    and are staged; beside that of 256 lanes they do not and come through the caches (markov_launch decides it from the workgroup's
    size, which it takes from the batch's).  A batch that runs four waves per workgroup, bitwise against the same rows in calls of at
    most 64 rows: "a row's bits depend on the row alone" also across the two sources of the light curves.  The two preconditions are
    asserted from the headers' formulas, so that the test fails if the constants move instead of comparing staged with staged."""
    call, lane_bytes, ny_of = STAGING_ENTRIES[entry]
    L, N, C = len(STAGING_NL), sum(STAGING_NL), _cus()
    assert _lds_bytes(N, L, 64, lane_bytes) <= LDS_MAX < _lds_bytes(N, L, 256, lane_bytes)          # 64 lanes stage, 256 do not ...
    assert lane_bytes * L * 256 <= LDS_MAX                                                       # ... and still launch
    ny = ny_of(L, kernel == "OU")
    M = next(m for m in range(1, 1 << 30, 256) if (m + 63) // 64 * ny > 2 * C)                   # M % 256 == 1: the last row alone
    assert M % 256 == 1 and (M + 63) // 64 * ny > 2 * C and (M - 256 + 63) // 64 * ny <= 2 * C, (M, ny, C)
    t, y, s, _ = MC.lightcurves(STAGING_NL, seed=31 + L, kind="plain")
    delays, alpha, rho = _rows(L, M, seed=M + ny)
    rg = np.random.default_rng(M)
    kappa, nu = rg.uniform(0.5, 2.0, (M, L)), rg.uniform(0.0, 0.05, (M, L))
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=False) as obj:
        big = call(obj, delays, alpha, rho, kappa, nu)
        info = big[-1]
        assert info[M - 1] != 0 and (info[:M - 1] == 0).all()                                    # the failing row alone
        assert all(np.isnan(x[M - 1]).all() for x in big[:-1]) and all(np.isfinite(x[:M - 1]).all() for x in big[:-1])
        nb = (M + 255) // 256
        for r0, n in [(0, 64), (M - 1, 1), (max(nb // 2, 1) * 256 - 32, 64)]:                    # the last: across a workgroup border
            assert 0 <= r0 and r0 + n <= M
            sl = slice(r0, r0 + n)
            small = call(obj, delays[sl], alpha[sl], rho[sl], kappa[sl], nu[sl])
            assert len(small) == len(big)
            for k, (x, z) in enumerate(zip(big, small)):
                assert np.array_equal(x[sl], z, equal_nan=True), (kernel, entry, M, r0, k)


@pytest.mark.parametrize("wpw", [4, 2])
@pytest.mark.parametrize("problem", list(PROBLEMS))
def test_draws_do_not_depend_on_the_launch_shape(problem, wpw):
    """One row, S draws in one gpcc_markov_draw launch of S lanes, against the same (seed, s) in launches of 64 lanes
    (markov_sample_chunk_draws = 64, as tests/test_gpu_sample_highprec.py::test_unstaged_draws_are_the_staged_ones)."""
    obj, tt, yt, st = _problem(problem)
    L, C = len(PROBLEMS[problem][1]), _cus()
    S = _batch_rows(C, 1, wpw)
    assert (S + 63) // 64 > 2 * C if wpw == 4 else C < (S + 63) // 64 <= 2 * C
    delays, alpha, rho = _rows(L, 2, seed=S)
    args = (delays[:1], alpha[:1], rho[:1], tt, S, 77)
    big = obj.sample_markov_batch(*args, sigmatest=st)
    obj.set_option("markov_sample_chunk_draws", 64)
    try:
        small = obj.sample_markov_batch(*args, sigmatest=st)
    finally:
        obj.set_option("markov_sample_chunk_draws", 0)
    assert big[3][0] == 0 and big[0].shape == (S, sum(map(len, tt))) and np.isfinite(big[0]).all()
    for k, (x, y) in enumerate(zip(big, small)):
        assert np.array_equal(x, y), (problem, S, k)
