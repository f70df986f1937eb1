"""A row's bits do not depend on the launch shape (gpcc_markov.hip.h; markov_launch of gpcc_hip.hip): sixteen linear-time entries -- the
eight plain ones and the draws, the four noise-model predictions and the noise-model draws, the resampled value and its gradient -- on
batches whose kernels run four and two waves per workgroup, with a ragged last workgroup, bitwise against the same rows in calls of
at most 64 rows -- one wave, one workgroup along x.  The launcher counts ceil(rows / 64) * ny waves, ny being the kernel's lanes per
row (its grid's y), and takes one wave per workgroup up to C waves (C: the device's CUs), two up to 2 C and four beyond.

Two tiny problems, so that a call takes milliseconds: Matern-3/2 with bands of 7 and 5 points and marginalised offsets (<2, 2>), and
OU with bands of 6, 5 and 4 points and fixed offsets (<1, 0>).  Per entry a batch of 128 C + 1 rows (above 2 C waves in every
kernel) and one whose widest kernel -- the one the entry adds to those it shares -- has between C and 2 C waves; for the draws one
row with that many draws, the lanes of one gpcc_markov_draw launch.  The last row fails (alpha <= 0): it is alone in the last
workgroup, whose other lanes compute it again and store nothing.  Every row has its own (kappa, nu) for the noise-model entries and,
for the resampled ones, one of R = 4 realisations of the problem in turn, one of which drops a point and counts another twice.  No
tolerance: the reference is the library's own one-wave launch."""
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


REALISATIONS = 4


def _rows(L, M, seed):
    """M rows (tau, alpha, rho, kappa, nu, real); the last one fails."""
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 8.0, (M, L - 1)))], 1)
    alpha, rho = rg.uniform(0.4, 2.0, (M, L)), np.exp(rg.uniform(np.log(0.1), np.log(300.0), M))
    alpha[M - 1, L - 1] = -0.5
    kappa, nu = rg.uniform(0.5, 2.0, (M, L)), rg.uniform(0.0, 0.05, (M, L))
    return delays, alpha, rho, kappa, nu, np.arange(M) % REALISATIONS


def _realisations(name):
    """(Y, counts) of a problem, lists of L arrays (4, N_l): the problem's own fluxes, two flux randomisations, and a third that drops
    the second point of band 0 and counts its fourth twice."""
    _, Nl, _, _ = PROBLEMS[name]
    _, y, s, _ = MC.lightcurves(Nl, seed=31 + len(Nl), kind="plain")
    rg = np.random.default_rng(9 + len(Nl))
    Y = [np.stack([np.asarray(y[l], np.float64) + (r > 0) * np.asarray(s[l]) * rg.standard_normal(n) for r in range(REALISATIONS)])
         for l, n in enumerate(Nl)]
    counts = [np.ones((REALISATIONS, n), dtype=np.int64) for n in Nl]
    counts[0][3, 1], counts[0][3, 3] = 0, 2
    return Y, counts


# entry -> (the call: every output array of the rows w = (tau, alpha, rho, kappa, nu, real) handed over, ny of the kernel the entry adds
# (L bands, OU or not): the y of its grid, markov_launch's ny in gpcc_hip.hip)
def _loo(obj, name, w, tt, yt, st):
    o = obj.loo_markov_batch(*w[:3])
    return o.mu, o.var, o.lp, o.loo, o.loglik, o.info


def _noise_loo(obj, name, w, tt, yt, st):
    o = obj.loo_markov_noise_batch(*w[:5])
    return o.mu, o.var, o.lp, o.loo, o.loglik, o.info


def _resampled(method):
    def call(obj, name, w, tt, yt, st):
        Y, counts = _realisations(name)
        return getattr(obj, method)(Y, w[0], w[1], w[2], w[5], counts=counts)
    return call


def _grad_slots(L, ou):
    return L + 1 + (2 * L if ou else L)        # gpcc_markov_grad_slots


ENTRIES = {
    "loglik": (lambda obj, name, w, tt, yt, st: obj.loglik_markov_batch(*w[:3]), lambda L, ou: 1),
    "grad": (lambda obj, name, w, tt, yt, st: obj.loglik_grad_markov_batch(*w[:3]), _grad_slots),
    "hess_hyper": (lambda obj, name, w, tt, yt, st: obj.loglik_hess_hyper_markov_batch(*w[:3]), lambda L, ou: (L + 1) * (L + 2) // 2),
    "hess": (lambda obj, name, w, tt, yt, st: obj.loglik_hess_markov_batch(*w[:3]), lambda L, ou: L * L + 2 * L + L * (L - 1) // 2),
    "predict": (lambda obj, name, w, tt, yt, st: obj.predict_markov_batch(*w[:3], tt)[:4], lambda L, ou: 2),
    "heldout": (lambda obj, name, w, tt, yt, st: obj.heldout_loglik_markov_batch(*w[:3], tt, yt, st)[:3], lambda L, ou: 2),
    "postb": (lambda obj, name, w, tt, yt, st: obj.posterior_offsets_markov_batch(*w[:3]), lambda L, ou: 1),
    "loo": (_loo, lambda L, ou: 2),
    # gpcc_markov_noise_taps: the forward and the backward filter (tap mode, update mode), the forward filter alone (postb);
    # gpcc_markov_noise_loo_taps: both filters
    "noise_predict": (lambda obj, name, w, tt, yt, st: obj.predict_markov_noise_batch(*w[:3], tt, w[3], w[4])[:4], lambda L, ou: 2),
    "noise_heldout": (lambda obj, name, w, tt, yt, st: obj.heldout_loglik_markov_noise_batch(*w[:3], tt, yt, st, w[3], w[4])[:3],
                      lambda L, ou: 2),
    "noise_postb": (lambda obj, name, w, tt, yt, st: obj.posterior_offsets_markov_noise_batch(*w[:5]), lambda L, ou: 1),
    "noise_loo": (_noise_loo, lambda L, ou: 2),
    # gpcc_markov_resample: one lane per row; gpcc_markov_resample_grad: one per (row, slot), the plain gradient's slots
    "resampled": (_resampled("loglik_markov_resampled"), lambda L, ou: 1),
    "resampled_grad": (_resampled("loglik_grad_markov_resampled"), _grad_slots),
}
CASES = [(p, e) for p in PROBLEMS for e in ENTRIES if not (e.endswith("postb") and not PROBLEMS[p][2])]


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
    rows = _rows(L, M, seed=M + ny)
    big = call(obj, problem, rows, tt, yt, st)
    info = big[-1]
    assert info[M - 1] != 0 and (info[:M - 1] == 0).all()                     # the failing row alone
    assert all(np.isnan(x[M - 1]).all() for x in big[:-1]) and np.isfinite(big[0][:M - 1]).all()
    for r0, n in _windows(M, 64 * wpw):
        sl = slice(r0, r0 + n)
        small = call(obj, problem, tuple(x[sl] for x in rows), tt, yt, st)
        assert len(small) == len(big)
        for k, (x, y) in enumerate(zip(big, small)):
            assert np.array_equal(x[sl], y, equal_nan=True), (problem, entry, M, r0, k)


# ---- staged against unstaged light curves for the same row ---------------------------------------------------------------------------
STAGING_NL = [600] * 8
STAGING_NT = [1, 2, 1, 1, 2, 1, 1, 1]             # a handful of test points
LDS_MAX = 156 * 1024                              # GPCC_MARKOV_LDS_MAX (gpcc_markov.hip.h)
# copies of the headers' constants, to be kept in step with them by hand: a constant that moves there has to move here too, and then the
# preconditions below say whether the shapes still stage at 64 lanes and not at 256
LANE_BYTES, PRED_LANE_BYTES, NOISE_LANE_BYTES = 28, 40, 16     # GPCC_MARKOV_LANE_BYTES, GPCC_MKP_LANE_BYTES, GPCC_MARKOV_NOISE_LANE_BYTES
DRAW_POINT_BYTES = 20                                           # GPCC_MKS_POINT_BYTES


def _filter_staged(N, T):
    return 24 * N                                 # gpcc_markov_lds_bytes: the light curves


def _taps_staged(tw):
    return lambda N, T: 24 * N + 8 * tw * T       # gpcc_mkp_lds_bytes: and tw doubles per test point (1: tap mode, 3: update mode)


def _draw_staged(N, T):
    return DRAW_POINT_BYTES * (N + T) + 8         # gpcc_mks_lds_bytes


def _staging_resampled(obj, w, aux):
    return obj.loglik_grad_markov_resampled(aux["Y"], w[0], w[1], w[2], w[5] % 2, counts=aux["counts"])


# entry -> (the call on the rows w = (tau, alpha, rho, kappa, nu, real), bytes per lane and band beside the staged part, the staged
#           part's bytes (N, T), ny of the entry's widest kernel)
STAGING_ENTRIES = {
    "loglik": (lambda obj, w, aux: obj.loglik_markov_batch(*w[:3]), LANE_BYTES, _filter_staged, lambda L, ou: 1),
    "noise": (lambda obj, w, aux: obj.loglik_markov_noise_batch(*w[:5]), LANE_BYTES + NOISE_LANE_BYTES, _filter_staged, lambda L, ou: 1),
    "grad": (lambda obj, w, aux: obj.loglik_grad_markov_batch(*w[:3]), LANE_BYTES, _filter_staged, ENTRIES["grad"][1]),
    "noise_predict": (lambda obj, w, aux: obj.predict_markov_noise_batch(*w[:3], aux["tt"], w[3], w[4])[:4], PRED_LANE_BYTES + NOISE_LANE_BYTES,
                      _taps_staged(1), lambda L, ou: 2),
    "noise_heldout": (lambda obj, w, aux: obj.heldout_loglik_markov_noise_batch(*w[:3], aux["tt"], aux["yt"], aux["st"], w[3], w[4])[:3],
                      PRED_LANE_BYTES + NOISE_LANE_BYTES, _taps_staged(3), lambda L, ou: 2),
    "resampled_grad": (_staging_resampled, LANE_BYTES, _filter_staged, _grad_slots),
}


def _lds_bytes(N, T, L, threads, lane_bytes, staged):
    """gpcc_markov_lds_bytes, gpcc_markov_noise_lds_bytes, gpcc_mknp_lds_bytes or gpcc_mksn_lds_bytes with the light curves staged."""
    return staged(N, T) + lane_bytes * L * threads


def _staging_problem(L):
    """Eight bands of 600 points, test points with their observations, and two realisations: the own fluxes, and a flux randomisation
    that drops the third point of band 1 and counts its fifth twice."""
    t, y, s, _ = MC.lightcurves(STAGING_NL, seed=31 + L, kind="plain")
    rg = np.random.default_rng(77)
    tt = [MC.snap(rg.uniform(-2.0, float(np.max(t[l])) + 2.0, n)) for l, n in enumerate(STAGING_NT)]
    aux = {"tt": tt, "yt": [np.sin(0.4 * a) + 0.2 * rg.standard_normal(len(a)) for a in tt], "st": [0.1 + 0.1 * rg.random(len(a)) for a in tt]}
    aux["Y"] = [np.stack([np.asarray(y[l], np.float64), np.asarray(y[l], np.float64) + np.asarray(s[l]) * rg.standard_normal(len(y[l]))])
                for l in range(L)]
    aux["counts"] = [np.ones((2, len(a)), dtype=np.int64) for a in y]
    aux["counts"][1][1, 2], aux["counts"][1][1, 4] = 0, 2
    return (t, y, s), aux


@pytest.mark.parametrize("entry", list(STAGING_ENTRIES))
@pytest.mark.parametrize("kernel", ["OU", "matern32"])
def test_rows_do_not_depend_on_staging(kernel, entry):
    """Eight bands of 600 points (N = 4800), fixed offsets: beside the lanes' part of a workgroup of 64 lanes the light curves fit the LDS
    and are staged; beside that of 256 lanes they do not and come through the caches (markov_launch decides it from the workgroup's
    size, which it takes from the batch's).  A batch that runs four waves per workgroup, bitwise against the same rows in calls of at
    most 64 rows: "a row's bits depend on the row alone" also across the two sources of the light curves.  The two preconditions are
    asserted from the headers' formulas, so that the test fails if the constants move instead of comparing staged with staged.  The
    noise-model taps (56 bytes per lane and band, 112 KiB at 256 lanes) in tap mode (predictions) and update mode (held-out score), and
    the resampled gradient, whose OU rows run 25 slots each.

    The leave-one-out entries are left out: they split the rows into chunks by their tap scratch (markov_tap_chunk: 128 MiB over
    2 N nrec doubles a row, 832 rows for OU and 320 for Matern-3/2 at N = 4800) and the launch shape is decided per chunk, two lanes a
    row: at most 26 waves, never more than the device's CUs, so every chunk runs one wave per workgroup and stages."""
    call, lane_bytes, staged, ny_of = STAGING_ENTRIES[entry]
    L, N, T, C = len(STAGING_NL), sum(STAGING_NL), sum(STAGING_NT), _cus()
    assert _lds_bytes(N, T, L, 64, lane_bytes, staged) <= LDS_MAX < _lds_bytes(N, T, L, 256, lane_bytes, staged)   # 64 lanes stage, 256 do not ...
    assert lane_bytes * L * 256 <= LDS_MAX                                                       # ... and still launch
    ny = ny_of(L, kernel == "OU")
    M = next(m for m in range(1, 1 << 30, 256) if (m + 63) // 64 * ny > 2 * C)                   # M % 256 == 1: the last row alone
    assert M % 256 == 1 and (M + 63) // 64 * ny > 2 * C and (M - 256 + 63) // 64 * ny <= 2 * C, (M, ny, C)
    (t, y, s), aux = _staging_problem(L)
    rows = _rows(L, M, seed=M + ny)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=False) as obj:
        big = call(obj, rows, aux)
        info = big[-1]
        assert info[M - 1] != 0 and (info[:M - 1] == 0).all()                                    # the failing row alone
        assert all(np.isnan(x[M - 1]).all() for x in big[:-1]) and all(np.isfinite(x[:M - 1]).all() for x in big[:-1])
        nb = (M + 255) // 256
        for r0, n in [(0, 64), (M - 1, 1), (max(nb // 2, 1) * 256 - 32, 64)]:                    # the last: across a workgroup border
            assert 0 <= r0 and r0 + n <= M
            sl = slice(r0, r0 + n)
            small = call(obj, tuple(x[sl] for x in rows), aux)
            assert len(small) == len(big)
            for k, (x, z) in enumerate(zip(big, small)):
                assert np.array_equal(x[sl], z, equal_nan=True), (kernel, entry, M, r0, k)


@pytest.mark.parametrize("kernel", ["OU", "matern32"])
def test_noise_draws_do_not_depend_on_staging(kernel):
    """The same eight bands under gpcc_markov_noise_draw (56 bytes per lane and band beside 20 bytes a staged point): one row, S draws in
    one launch of S lanes, four waves per workgroup and unstaged, against the same (seed, s) in launches of 64 C lanes, one wave per
    workgroup and staged.  A draw's normals depend on (seed, s) and the row's word, not on the lane, so the draws are the same bits."""
    L, N, T, C = len(STAGING_NL), sum(STAGING_NL), sum(STAGING_NT), _cus()
    lane_bytes = PRED_LANE_BYTES + NOISE_LANE_BYTES
    assert _lds_bytes(N, T, L, 64, lane_bytes, _draw_staged) <= LDS_MAX < _lds_bytes(N, T, L, 256, lane_bytes, _draw_staged)
    assert lane_bytes * L * 256 <= LDS_MAX
    S = next(m for m in range(1, 1 << 30, 256) if (m + 63) // 64 > 2 * C)
    assert 8 * (N + T) * ((S + 255) // 256 * 256) < 2 ** 31                                      # the draw kernel's scratch
    (t, y, s), aux = _staging_problem(L)
    d, a, r, kappa, nu, _ = (x[:1] for x in _rows(L, 2, seed=S))
    args = (d, a, r, kappa, nu, aux["tt"], S, 77)
    with gpcc_amd.Objective(t, y, s, KERN[kernel], marginalise_b=False) as obj:
        try:
            obj.set_option("markov_sample_chunk_draws", S)                                       # one launch: more than 2 C waves
            big = obj.sample_markov_noise_batch(*args, sigmatest=aux["st"])
            obj.set_option("markov_sample_chunk_draws", 64 * C)                                  # C waves a launch at most: 64 lanes
            small = obj.sample_markov_noise_batch(*args, sigmatest=aux["st"])
        finally:
            obj.set_option("markov_sample_chunk_draws", 0)
    assert big[3][0] == 0 and big[0].shape == (S, T) and np.isfinite(big[0]).all()
    for k, (x, z) in enumerate(zip(big, small)):
        assert np.array_equal(x, z), (kernel, S, k)


DRAWS = {"sample_markov_batch": lambda obj, w, tt, S, st: obj.sample_markov_batch(*w[:3], tt, S, 77, sigmatest=st),
         "sample_markov_noise_batch": lambda obj, w, tt, S, st: obj.sample_markov_noise_batch(*w[:5], tt, S, 77, sigmatest=st)}


@pytest.mark.parametrize("wpw", [4, 2])
@pytest.mark.parametrize("problem", list(PROBLEMS))
def test_draws_do_not_depend_on_the_launch_shape(problem, wpw):
    """One row, S draws in one gpcc_markov_draw launch of S lanes, against the same (seed, s) in launches of 64 lanes
    (markov_sample_chunk_draws = 64, as tests/test_gpu_sample_highprec.py::test_unstaged_draws_are_the_staged_ones); the same under the
    row's own noise model in gpcc_markov_noise_draw."""
    obj, tt, yt, st = _problem(problem)
    L, C = len(PROBLEMS[problem][1]), _cus()
    S = _batch_rows(C, 1, wpw)
    assert (S + 63) // 64 > 2 * C if wpw == 4 else C < (S + 63) // 64 <= 2 * C
    w = tuple(x[:1] for x in _rows(L, 2, seed=S))
    for entry, draw in DRAWS.items():
        big = draw(obj, w, tt, S, st)
        obj.set_option("markov_sample_chunk_draws", 64)
        try:
            small = draw(obj, w, tt, S, st)
        finally:
            obj.set_option("markov_sample_chunk_draws", 0)
        assert big[3][0] == 0 and big[0].shape == (S, sum(map(len, tt))) and np.isfinite(big[0]).all()
        for k, (x, y) in enumerate(zip(big, small)):
            assert np.array_equal(x, y), (problem, entry, S, k)
