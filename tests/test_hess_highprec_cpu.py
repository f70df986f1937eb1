"""The extended-precision Hessian reference (tests/_hess_highprec.py) checked on the CPU: against the fp64 torch witness, the numpy
formula and the extended gradient; against second differences of a 40-digit mpmath log-likelihood; its tiled recomputation against its
trace formula; and the per-block comparator of the device tests against every slip a tiled implementation can make, in every position."""
import time

import numpy as np
import pytest

import _grad_highprec as GH
import _grad_witness as W
import _hess_highprec as HH
import _hess_witness as HW

pytestmark = pytest.mark.skipif(not HH.EXTENDED, reason=HH.SKIP_REASON)

KERNELS = ["OU", "rbf", "matern32", "matern52"]
SIZES = {1: [23], 2: [19, 31], 3: [17, 9, 26]}   # test_hessian_cpu.py's shapes
EPS_LD = float(np.finfo(HH.LD).eps)


def _size(ref):
    """max over the entries of |T1| + |T2| + |T3|"""
    return float(np.max(np.sum(np.abs(ref.terms), 0)))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("mb", [True, False])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_reference_against_witness_formula_and_gradient(kernel, mb, L):
    data = W.ragged_data(SIZES[L], seed=20 * L + KERNELS.index(kernel))
    delays, alpha, rho = W.random_params(L, 2, seed=L + 7)
    for i in range(2):
        args = (kernel, *data, delays[i], alpha[i], rho[i], mb)
        ref = HH.add_bars(HH.evaluate(*args, keep=True))
        assert ref.info == 0 and not ref.ties
        lw, gw, Hw, Fw = HW.hessian_and_fisher(*args)
        Hf, Ff = HW.formula(*args)
        assert abs(ref.loglik - lw) <= 1e-12 * abs(lw)
        rel = max(1e-10, 64 * HH.EPS64 * ref.cond)     # (the fp64 restatements are good to ~eps64 cond_1(K); rbf reaches 1e8)
        for got in (Hw, Hf):
            assert np.max(np.abs(got - ref.H)) <= rel * np.max(np.abs(ref.H)), (got, ref.H, ref.cond)
        for got in (Fw, Ff):
            assert np.max(np.abs(got - ref.F)) <= rel * np.max(np.abs(ref.F)), (got, ref.F, ref.cond)
        assert HH.worst(HH.ratio_blocks(Hw, Fw, ref)) <= 1.0
        # the gradient: the same trace formula as _grad_highprec's, on a K summed in another order (~eps cond apart)
        g = GH.evaluate(*args)
        assert g.info == 0 and abs(ref.loglik - g.loglik) <= 1e-15 * abs(g.loglik)
        assert float(np.max(np.abs(ref.grad_ld - g.grad_ld))) <= 8 * EPS_LD * ref.cond * float(np.max(g.scale)), (ref.grad_ld, g.grad_ld)
        assert GH.ratio(ref.grad, g) <= 1e-4
        # a common shift of all delays leaves the likelihood unchanged: the rows sum to zero over the tau columns
        if L > 1:
            for A in (ref.H_ld, ref.F_ld):
                assert float(np.max(np.abs(A[:, L + 1:].sum(1)))) <= 8 * EPS_LD * ref.cond * _size(ref), A
        else:
            assert not ref.H_ld[:, 2].any() and not ref.F_ld[:, 2].any() and not ref.terms[:, :, 2].any()


def _mp_loglik(mp, kernel, data, x, L, mb, smooth=()):
    """objective(alpha, rho) at x = [alpha, rho, tau] in mpmath at the working precision.  smooth: pairs (i, j) of points whose OU
    kernel value is cosh(s / rho), the mean of exp(-s / rho) and exp(+s / rho), instead of exp(-|s| / rho)."""
    tarray, yarray, stdarray = data
    alpha, rho, delays = x[:L], x[L], x[L + 1:]
    band = [l for l, t in enumerate(tarray) for _ in t]
    t = [mp.mpf(float(v)) for a in tarray for v in a]
    y = [mp.mpf(float(v)) for a in yarray for v in a]
    sd = [mp.mpf(float(v)) for a in stdarray for v in a]
    N = len(t)
    mean = [mp.fsum(mp.mpf(float(v)) for v in a) / len(a) for a in yarray]
    var = [mp.fsum((mp.mpf(float(v)) - m) ** 2 for v in a) / (len(a) - 1) for a, m in zip(yarray, mean)]
    u = [t[i] - delays[band[i]] for i in range(N)]

    def k(i, j):
        s = u[i] - u[j]
        r = abs(s)
        if kernel == "OU":
            return mp.cosh(s / rho) if (i, j) in smooth or (j, i) in smooth else mp.exp(-r / rho)
        if kernel == "rbf":
            return mp.exp(-s * s / (4 * rho))
        if kernel == "matern32":
            a = mp.sqrt(3) * r / rho
            return (1 + a) * mp.exp(-a)
        a = mp.sqrt(5) * r / rho
        return (1 + a + a * a / 3) * mp.exp(-a)

    K = mp.matrix(N, N)
    for i in range(N):
        for j in range(i + 1):
            v = alpha[band[i]] * alpha[band[j]] * k(i, j)
            if mb and band[i] == band[j]:
                v += 100 * var[band[i]]
            if i == j:
                v += sd[i] ** 2
            K[i, j] = K[j, i] = v
    C = mp.cholesky(K)
    z = []
    for i in range(N):
        z.append((y[i] - mean[band[i]] - mp.fsum(C[i, j] * z[j] for j in range(i))) / C[i, i])
    return -mp.fsum(v * v for v in z) / 2 - mp.fsum(mp.log(C[i, i]) for i in range(N)) - N * mp.log(2 * mp.pi) / 2


def _second_differences(f, x0, h):
    """Central second differences of f at x0 -> float64 [P, P]: truncation ~h^2, rounding ~4 |f| 10^-dps / h^2."""
    P = len(x0)
    f0 = f(x0)

    def at(*moves):
        x = list(x0)
        for i, sgn in moves:
            x[i] += sgn * h
        return f(x)

    H = np.zeros((P, P))
    for a in range(P):
        H[a, a] = float((at((a, 1)) - 2 * f0 + at((a, -1))) / h ** 2)
        for b in range(a + 1, P):
            H[a, b] = H[b, a] = float((at((a, 1), (b, 1)) - at((a, 1), (b, -1)) - at((a, -1), (b, 1)) + at((a, -1), (b, -1))) / (4 * h * h))
    return H, f0


@pytest.mark.parametrize("kernel", KERNELS + ["OU-tie"])
@pytest.mark.parametrize("mb", [True, False])
def test_reference_against_mpmath_second_differences(kernel, mb):
    """Central second differences of the 40-digit log-likelihood, h = 1e-10 (truncation ~1e-20 f'''', rounding ~1e-18), verify every
    entry of the reference's H to 1e-15 of the size of its terms, for two bands of 13 + 11 points.

    "OU-tie" puts one pair of points of the two bands at the same shifted time.  The library's convention there (k_s = 0, k_rs = 0,
    k_ss = 1 / rho^2) is k_ss's one-sided limit from either side, and the three values together are the derivatives at 0 of
    cosh(s / rho), the mean of the kernel's smooth branches exp(-s / rho) and exp(+s / rho): the reference's H equals, to the same
    1e-15, the second differences of the likelihood with that pair's kernel value read as cosh(s / rho).  Differencing the
    likelihood itself across the kink gives something else: exp(-|s| / rho) falls by h / rho on both sides of 0, so the second
    difference in a delay of the pair carries -2 G_ij alpha_p alpha_q / (rho h), the kink's delta, which grows without bound as
    h -> 0 (1e10 times the entry's size at h = 1e-10); the last assertion checks that figure."""
    mp = pytest.importorskip("mpmath").mp
    mp.dps = 40
    tie = kernel == "OU-tie"
    kernel = "OU" if tie else kernel
    data = W.ragged_data([13, 11], seed=3 + KERNELS.index(kernel))
    delays, alpha, rho, L = np.array([0.0, 1.25]), np.array([0.9, 1.4]), 2.5, 2
    smooth = ()
    if tie:
        data[0][0][6] = np.round(data[0][0][6] * 1024) / 1024    # (so that t + tau is exact)
        data[0][1][4] = data[0][0][6] + delays[1]                # t - tau equal across the bands: s = 0 off the diagonal
        smooth = ((6, 13 + 4),)
    ref = HH.evaluate(kernel, *data, delays, alpha, rho, mb, keep=True)
    assert ref.info == 0 and ref.ties == tie
    x0 = [mp.mpf(float(v)) for v in np.concatenate([alpha, [rho], delays])]
    h = mp.mpf(10) ** -10
    fd, ll = _second_differences(lambda x: _mp_loglik(mp, kernel, data, x, L, mb, smooth), x0, h)
    assert abs(float(ll) - ref.loglik) <= 1e-15 * abs(ref.loglik)
    err = float(np.max(np.abs(fd - ref.H)))
    print("%s mb=%s: max |H - mpmath second differences| = %.3g (size of the terms %.3g)" % (kernel, mb, err, _size(ref)))
    assert err <= 1e-15 * max(1.0, _size(ref)), (fd, ref.H)
    if tie:
        st = ref.parts["st"]
        i, j = smooth[0]
        assert st["S"][i, j] == 0
        G = st["w"][i] * st["w"][j] - st["C"][i, j]
        a = L + 1 + 1     # tau_2
        f = lambda x: _mp_loglik(mp, kernel, data, x, L, mb)   # noqa: E731
        xp, xm = list(x0), list(x0)
        xp[a] += h
        xm[a] -= h
        across = float((f(xp) - 2 * f(x0) + f(xm)) / h ** 2)
        delta = -2 * float(G) * alpha[0] * alpha[1] / (rho * float(h))
        print("across the kink: second difference %.6g, the reference %.6g, the kink's delta -2 G aa / (rho h) = %.6g"
              % (across, ref.H[a, a], delta))
        assert abs(across - ref.H[a, a] - delta) <= 1e-6 * abs(delta) and abs(delta) > 1e6 * abs(ref.H[a, a])


def _mutation_case(kernel, mb, ties=False):
    data, delays, alpha, rho = HH.mutation_data(ties)
    return HH.add_bars(HH.evaluate(kernel, *data, delays, alpha, rho, mb, keep=True))


def test_tiled_recomputation_matches_trace_formula():
    """tile_hessian in extended precision against the trace formula, full and block mode: the difference is the order of the sums."""
    for kernel in KERNELS:
        ref = _mutation_case(kernel, True)
        for Pa in (None, ref.L + 1):
            H, F = HH.tile_hessian(ref, Pa=Pa)
            n = H.shape[0]
            assert float(np.max(np.abs(H - ref.H_ld[:n, :n]))) <= 1e-16 * _size(ref), kernel
            assert float(np.max(np.abs(F - ref.F_ld[:n, :n]))) <= 1e-16 * _size(ref), kernel
            assert HH.worst(HH.ratio_blocks(H, F, ref)) <= 1e-3


@pytest.mark.parametrize("mb", [True, False])
def test_comparator_rejects_each_injected_fault(mb):
    """Every fault of tile_hessian's list, in every position it can occur at N = 300 (3 tiles, 3 bands): ratio_blocks must put each
    one above 1 in at least one block.  The smallest rejection ratio is printed."""
    smallest, where, count = np.inf, None, 0

    def reject(ref, fault, Pa=None, label=None):
        nonlocal smallest, where, count
        r = HH.worst(HH.ratio_blocks(*HH.tile_hessian(ref, fault, Pa=Pa), ref))
        assert r > 1.0, (label or fault, r)
        count += 1
        if r < smallest:
            smallest, where = r, label or fault

    ref = _mutation_case("matern32", mb)
    assert HH.worst(HH.ratio_blocks(*HH.tile_hessian(ref), ref)) <= 1e-3
    for f in HH.all_faults(L=3, nt=3):
        reject(ref, f)
    for a in range(ref.L + 1):     # block mode
        reject(ref, ("pa_confusion", a), Pa=ref.L + 1)
    for kernel in KERNELS:         # k_rr, k_rs, k_ss of each kernel off by 1e-6 relative
        rk = ref if kernel == "matern32" else _mutation_case(kernel, mb)
        for x in (3, 4, 5):
            reject(rk, ("k2_scale", x, 1 + 1e-6), label=(kernel, HH.TABLES[x], "1e-6"))
    rt = _mutation_case("OU", mb, ties=True)     # OU's k_ss(0): needs cross-band pairs at the same shifted time
    assert rt.ties and rt.e_witness is None
    assert HH.worst(HH.ratio_blocks(*HH.tile_hessian(rt), rt)) <= 1e-3
    Hf, Ff = HW.formula("OU", *rt.parts["args"][1:])          # (the numpy formula has the library's convention)
    assert np.max(np.abs(Hf - rt.H)) <= 1e-9 * np.max(np.abs(rt.H))
    for v in (-1, 0):
        reject(rt, ("ou_kss0", v))
    print("mb=%s: %d injected faults rejected; smallest error / bar %.3g (%s)" % (mb, count, smallest, where))


def test_the_old_bar_accepts_a_wrong_k_rr_on_three_bands():
    """Why the bar changed: test_gpu_hessian.ratio (one bar for the matrix, relative to max |H|) applied to "k_rr off by 1e-6" on
    three bands accepts it; the per-block comparator rejects it."""
    from test_gpu_hessian import ratio as old_ratio
    for kernel in ("matern32", "OU"):
        ref = _mutation_case(kernel, True)
        H, F = HH.tile_hessian(ref, ("k2_scale", 3, 1 + 1e-6))
        H = H.astype(np.float64)
        L = ref.L
        moved = float(abs(H[L, L] - ref.H[L, L]))
        old = old_ratio(H, ref.H, ref.cond)
        new = HH.ratio_blocks(H, F, ref)
        print("%s, three bands, k_rr off by 1e-6: H_rr moves by %.3g (|H_rr| = %.3g, max |H| = %.3g); old error / bar %.3g (accepted), "
              "per block %.3g (rejected)" % (kernel, moved, abs(ref.H[L, L]), np.max(np.abs(ref.H)), old, new["rr"]))
        assert old <= 1.0 and new["rr"] > 1.0


def test_one_mirror_run_is_no_bar_on_an_ill_conditioned_K():
    """Why e_mirror is the largest error of several fp64 runs: at the envelope's corner alpha = 100, rho = 300 (cond_1(K) up to 1.6e9)
    an fp64 run's error in a block is one draw of a rounding error amplified by cond_1(K).  Bars made from the LAPACK run alone (with
    the witness and the floor) are missed by the 64-blocked and the reversed run, which are the same algorithm in the same precision
    with the factorisation summed in another order, in some of these 32 rows; the count and the worst ratio are printed."""
    missed, worst_r, rows = 0, 0.0, 0
    for Nl in ([22, 18], [70, 58]):
        t, y, _ = W.ragged_data(Nl, seed=sum(Nl))
        for sig in (0.05, 1.0):
            data = (t, y, [np.full(n, sig) for n in Nl])
            for kernel in KERNELS:
                for mb in (True, False):
                    ref = HH.add_bars(HH.evaluate(kernel, *data, [0.0, 1.25], [100.0, 100.0], 300.0, mb, keep=True))
                    assert ref.info == 0
                    e = HH.mirror_errors(ref)
                    assert set(e) == set(HH.MIRRORS)
                    rows += 1
                    r = 0.0
                    for which in ("H", "F"):
                        for b in ref.floor[which]:
                            one = HH.FACTOR * max([e["lapack"][which][b], ref.floor[which][b]]
                                                  + ([ref.e_witness[which][b]] if ref.e_witness else []))
                            r = max(r, max(e["blocked"][which][b], e["reversed"][which][b]) / one)
                            assert max(v[which][b] for v in e.values()) <= ref.bars[which][b]
                    missed += r > 1.0
                    worst_r = max(worst_r, r)
    print("bars from one fp64 run: missed by another run of the same algorithm in %d of %d rows, by up to %.3g x" % (missed, rows, worst_r))
    assert missed >= 1


def test_blocks_of_16_carry_rounding_the_other_runs_do_not():
    """Why one mirror run factorises and inverts in blocks of 16, the device's pivot block: at N = 40 a 64-blocked run is one block,
    i.e. plain forward substitution.  At the corner alpha = 100, rho = 300, sigma = 0.05, N = 40, bars made from the other three runs
    are exceeded by the 16-blocked run (its X = L^-1 has off-diagonal blocks formed with inverted diagonal blocks) in some of the
    eight rows; each is printed."""
    t, y, _ = W.ragged_data([22, 18], seed=40)
    data = (t, y, [np.full(n, 0.05) for n in (22, 18)])
    missed = 0
    for kernel in KERNELS:
        for mb in (True, False):
            ref = HH.add_bars(HH.evaluate(kernel, *data, [0.0, 1.25], [100.0, 100.0], 300.0, mb, keep=True))
            e = HH.mirror_errors(ref)
            over = {}
            for which in ("H", "F"):
                for b in ref.floor[which]:
                    rest = HH.FACTOR * max([e[m][which][b] for m in HH.MIRRORS if m != "blocked16"] + [ref.floor[which][b]]
                                           + ([ref.e_witness[which][b]] if ref.e_witness else []))
                    if e["blocked16"][which][b] > rest:
                        over[which + " " + b] = "%.3g" % (e["blocked16"][which][b] / rest)
            if over:
                missed += 1
                print("%s mb=%s cond_1(K) %.3g: the 16-blocked run over the other runs' bars: %s" % (kernel, mb, ref.cond, over))
    assert missed >= 1


def test_reference_time_at_n_1030():
    """The reference's cost at the largest size the device tests give it (one evaluation, L = 8, P = 17), bars included."""
    Nl = [1, 2, 3, 40, 127, 128, 129, 600]
    data = W.ragged_data(Nl, seed=5)
    delays, alpha, rho = W.random_params(8, 1, seed=6)
    t0 = time.perf_counter()
    ref = HH.reference_job(("matern52", *data, delays[0], alpha[0], rho[0], False))
    dt = time.perf_counter() - t0
    print("extended-precision Hessian reference with its bars at N = %d, P = 17: %.1f s" % (sum(Nl), dt))
    assert ref.info == 0 and np.all(np.isfinite(ref.H))
    for which in ("H", "F"):
        print("  %s: e_mirror %s\n     e_witness %s\n     floor %s" % (which, *({b: "%.2e" % v for b, v in src[which].items()}
                                                                     for src in (ref.e_mirror, ref.e_witness, ref.floor))))
