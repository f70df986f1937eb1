"""gpcc_loo_batch and gpcc_loo_markov_batch on the device: both against the extended-precision definition with the bars of
tests/_loo_highprec.py (measured on the reference side only), the linear-time entry against its numpy mirror and against the dense
entry; tile boundaries and L = 1 .. 8; one larger run; loglik and info against the sibling entries; bitwise independence of the batch,
the chunking, the options, fp32 and two-device handles; NULL outputs, weights with zeros and the memory of a linear-time-only handle.
The lines that start with "loo-parity" are kept in profiles/loo/loo_parity.log."""
import itertools

import numpy as np
import pytest

import _loo_highprec as LH
import _markov_cases as MC
import _predict_highprec as PH
import gpcc_amd
from gpcc_amd import markov

pytestmark = pytest.mark.gpu

KERNELS = {"OU": gpcc_amd.OU, "rbf": gpcc_amd.rbf, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
UNSUPPORTED, ARGUMENT = -3, -1
ROWS = ("mu", "var", "lp", "loo")


def _got(res):
    return {"mu": res.mu, "var": res.var, "lp": res.lp, "loo": res.loo, "mix_lp": res.mix_lp, "mix_loo": res.mix_loo}


def _check_case(case, worst, with_markov):
    """One case on the device: the dense entry within its bar; the linear-time entry within its bar, within two bars of the mirror
    and within the sum of the two bars of the dense entry; loglik and info bitwise the siblings'."""
    cid, k, data, delays, alpha, rho, mb, N = case
    ref = LH.reference(case)
    with gpcc_amd.Objective(*data, KERNELS[k], marginalise_b=mb) as obj:
        dense = obj.loo_batch(delays, alpha, rho, weights=LH.WEIGHTS)
        gl, _, gi = obj.loglik_grad_batch(delays, alpha, rho)
        assert (dense.info == 0).all() and np.array_equal(dense.info, gi) and np.array_equal(dense.loglik, gl), cid
        d = _got(dense)
        for q in LH.QUANTITIES:
            worst["dense " + q].add(ref.ratio(q, d[q]), cid)
        if not with_markov:
            return
        lin = obj.loo_markov_batch(delays, alpha, rho, weights=LH.WEIGHTS)
        ml, mi = obj.loglik_markov_batch(delays, alpha, rho)
        assert (lin.info == 0).all() and np.array_equal(lin.info, mi) and np.array_equal(lin.loglik, ml), cid
        g = _got(lin)
        rows = [markov.loo(k, *data, delays[m], alpha[m], rho[m], mb) for m in range(len(rho))]
        mir = {"mu": np.stack([r[0] for r in rows]), "var": np.stack([r[1] for r in rows]), "lp": np.stack([r[2] for r in rows]),
               "loo": np.array([r[3] for r in rows])}
        mir["mix_lp"], mir["mix_loo"] = markov.loo_mix(mir["lp"], LH.WEIGHTS)
        for q in LH.QUANTITIES:
            b = ref.bar[q]
            worst["linear " + q].add(ref.ratio(q, g[q], markov=True), cid)
            worst["linear vs mirror " + q].add(float(np.max(np.abs(g[q] - mir[q]) / (2.0 * ref.scale * b))), cid)
            worst["linear vs dense " + q].add(float(np.max(np.abs(g[q] - d[q]) / ((1.0 + ref.scale) * b))), cid)


def _report(worst):
    for w in worst.values():
        print(w.line())
    missed = [w.line() for w in worst.values() if not w.worst <= 1.0]
    assert not missed, missed


def _groups(tag, with_markov=True):
    names = ["dense "] + (["linear ", "linear vs mirror ", "linear vs dense "] if with_markov else [])
    return {n + q: LH.Worst("loo-parity %s %s%s" % (tag, n, q)) for n in names for q in LH.QUANTITIES}


@pytest.mark.skipif(not LH.EXTENDED, reason=LH.SKIP_REASON)
@pytest.mark.parametrize("kernel,N,mb", list(itertools.product(MC.KERNELS, (110, 150), (True, False))))
def test_parity_on_the_cpu_cases(kernel, N, mb):
    worst = _groups("%s N=%d b%d" % (kernel, N, mb))
    n = 0
    for case in LH.cases():
        if (case[1], case[7], case[6]) == (kernel, N, mb):
            _check_case(case, worst, True)
            n += 1
    assert n == 3 * len(MC.RHOS)
    _report(worst)


@pytest.mark.skipif(not LH.EXTENDED, reason=LH.SKIP_REASON)
def test_parity_rbf_dense():
    worst = _groups("rbf", False)
    for case in LH.rbf_cases():
        _check_case(case, worst, False)
    _report(worst)


# N -> band lengths: the tile (128) boundaries 127, 128, 129, 256, 257, 383, 384 and L = 1 .. 8
GEOMETRY = {127: [40, 40, 47], 128: [16] * 8, 129: [33, 32, 32, 32], 130: [26] * 5, 256: [128, 128], 257: [37] * 6 + [35], 383: [383],
            384: [64] * 6}


@pytest.mark.skipif(not LH.EXTENDED, reason=LH.SKIP_REASON)
@pytest.mark.parametrize("N", sorted(GEOMETRY))
def test_tile_boundaries(N):
    """b marginalised up to L = 4; beyond, the linear-time entry refuses it (asserted) and both entries run with fixed b."""
    Nl = GEOMETRY[N]
    L = len(Nl)
    kernel = MC.KERNELS[N % 3]
    t, y, s, d0 = MC.lightcurves(Nl, seed=N, kind="ties")
    d1 = d0.copy()
    d1[1:] += 2.0 ** -4
    a0 = np.random.default_rng(N).uniform(0.5, 2.0, L)
    mb = L <= markov.MAX_OFFSET_BANDS
    case = ("%s-N%d-L%d-b%d" % (kernel, N, L, mb), kernel, (t, y, s), np.stack([d0, d1]), np.stack([a0, 1.25 * a0]), np.array([3.0, 2.4]),
            mb, N)
    if not mb:
        with gpcc_amd.Objective(t, y, s, KERNELS[kernel], marginalise_b=True) as obj:
            with pytest.raises(gpcc_amd.GpccError) as ei:
                obj.loo_markov_batch(case[3], case[4], case[5])
            assert ei.value.code == UNSUPPORTED
    worst = _groups("tile N=%d L=%d" % (N, L))
    _check_case(case, worst, True)
    _report(worst)


def _k64(kernel, d, rho):
    """The Markov kernels in float64 (src/util.jl:15-52)."""
    a = {"OU": 1.0, "matern32": np.sqrt(3.0), "matern52": np.sqrt(5.0)}[kernel] * np.abs(d) / rho
    return np.exp(-a) * {"OU": 1.0, "matern32": 1.0 + a, "matern52": 1.0 + a + a * a / 3.0}[kernel]


def _fp64_rows(kernel, data, delays, alpha, rho, mb):
    """(values a, values b, terms) per row of the definition in float64 by two independent routes: G_ii = sum_k X_ki^2 and w = X'X r
    with X the inverse of the Cholesky factor, and LAPACK's inverse of K itself."""
    t, y, s = (np.concatenate([np.asarray(a, np.float64) for a in arrs]) for arrs in data)
    band = PH._bands(data[0])
    mean = np.array([np.mean(a) for a in data[1]])
    sigb = np.array([100.0 * np.var(a, ddof=1) if mb else 0.0 for a in data[1]])
    r = y - mean[band]
    out = []
    for m_ in range(len(rho)):
        u = t - delays[m_][band]
        K = alpha[m_][band][:, None] * alpha[m_][band][None, :] * _k64(kernel, u[:, None] - u[None, :], rho[m_])
        K += sigb[band][:, None] * (band[:, None] == band[None, :])
        K[np.diag_indices(len(t))] += s * s
        both = []
        X = np.linalg.inv(np.linalg.cholesky(K))
        G = np.linalg.inv(K)
        for g, w in ((np.sum(X * X, axis=0), X.T @ (X @ r)), (np.diagonal(G), G @ r)):
            var, dd = 1.0 / g, w / g
            both.append((y - dd, var, -0.5 * (np.log(2.0 * np.pi) + np.log(var) + dd * dd / var)))
        tmu = np.abs(y) + np.abs(G * r[None, :]).sum(axis=1) / g
        tlp = 0.5 * (np.log(2.0 * np.pi) + np.abs(np.log(var)) + dd * dd / var)
        out.append((both[0], both[1], (tmu, var, tlp)))
    return out


def test_larger_run():
    """N = 2048, 4 rows: the dense entry against the linear-time one within the sum of their bars.  The extended reference does not
    reach this size in test time, so the bar's error term is the disagreement of two independent float64 evaluations of the definition
    (through the inverse of the Cholesky factor, and LAPACK's inverse of K), as _markov_cases does where the extended value is not available:
    bar = 16 max(|a - b|, N 2^-53 terms), the linear-time one times factor / 16."""
    N, Nl = 2048, [1024, 1024]
    t, y, s, d0 = MC.lightcurves(Nl, seed=2048, kind="ties")
    delays = np.stack([d0 + [0.0, k * 2.0 ** -3] for k in range(4)])
    alpha = np.array([[1.0, 0.8], [1.2, 0.9], [0.7, 1.4], [1.5, 1.1]])
    rho = np.array([2.0, 3.0, 5.0, 8.0])
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        dense = obj.loo_batch(delays, alpha, rho)
        lin = obj.loo_markov_batch(delays, alpha, rho)
        gl, _, gi = obj.loglik_grad_batch(delays, alpha, rho)
        ml, mi = obj.loglik_markov_batch(delays, alpha, rho)
    assert (dense.info == 0).all() and (lin.info == 0).all()
    assert np.array_equal(dense.loglik, gl) and np.array_equal(dense.info, gi) and np.array_equal(lin.loglik, ml) and np.array_equal(lin.info, mi)
    scale = MC.factor(alpha, s) / LH.FACTOR
    worst = {q: LH.Worst("loo-parity N=2048 dense vs linear %s" % q) for q in ROWS}
    for m_, (a, b, terms) in enumerate(_fp64_rows("matern32", (t, y, s), delays, alpha, rho, True)):
        for j, q in enumerate(("mu", "var", "lp")):
            e = float(np.max(np.abs(a[j] - b[j])))
            bar = LH.FACTOR * np.maximum(e, N * LH.U53 * terms[j])
            worst[q].add(float(np.max(np.abs(getattr(dense, q)[m_] - getattr(lin, q)[m_]) / ((1.0 + scale) * bar))), m_)
        e = abs(float(a[2].sum() - b[2].sum()))
        bar = LH.FACTOR * max(e, N * LH.U53 * float(terms[2].sum()))
        worst["loo"].add(abs(dense.loo[m_] - lin.loo[m_]) / ((1.0 + scale) * bar), m_)
    _report(worst)


def _pool(M, L, seed):
    rg = np.random.default_rng(seed)
    delays = np.concatenate([np.zeros((M, 1)), MC.snap(rg.uniform(-3.0, 5.0, (M, L - 1)))], 1)
    return delays, rg.uniform(0.5, 2.0, (M, L)), rg.uniform(0.3, 30.0, M)


def _same(a, b, sel=slice(None), mix=True):
    ok = all(np.array_equal(getattr(a, q), getattr(b, q)[sel], equal_nan=True) for q in ROWS + ("loglik", "info"))
    if mix:
        ok = ok and np.array_equal(a.mix_lp, b.mix_lp, equal_nan=True) and (a.mix_loo == b.mix_loo or (a.mix_loo != a.mix_loo and b.mix_loo != b.mix_loo))
    return ok


@pytest.mark.parametrize("entry", ["loo_batch", "loo_markov_batch"])
def test_bitwise_independence(entry):
    """A row's bits do not depend on M (1 / 63 / 64 / 65), the row order, the chunking, the slot and stream options, the handle's
    precision or the number of devices; the mixture does not depend on the grouping either."""
    t, y, s, _ = MC.lightcurves([80, 70], seed=77, kind="ties")
    delays, alpha, rho = _pool(65, 2, seed=7)
    w = np.random.default_rng(3).random(65) ** 2
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52) as obj:
        full = getattr(obj, entry)(delays, alpha, rho, weights=w)
        assert (full.info == 0).all() and _same(getattr(obj, entry)(delays, alpha, rho, weights=w), full)
        for M in (1, 63, 64):
            part = getattr(obj, entry)(delays[:M], alpha[:M], rho[:M])
            assert _same(part, full, slice(0, M), mix=False), M
        one = getattr(obj, entry)(delays[64:], alpha[64:], rho[64:], weights=[2.0])
        assert _same(one, full, slice(64, 65), mix=False)
        assert np.array_equal(one.mix_lp, full.lp[64])                     # one row of weight 1 returns the row's bits
        perm = np.random.default_rng(1).permutation(65)
        assert _same(getattr(obj, entry)(delays[perm], alpha[perm], rho[perm]), full, perm, mix=False)
        for chunk in (1, 7, 64):
            obj.set_option("markov_chunk_rows", chunk)
            assert _same(getattr(obj, entry)(delays, alpha, rho, weights=w), full), chunk
        obj.set_option("markov_chunk_rows", 0)
    for kw in (dict(slots_per_stream=8), dict(slots_per_stream=3, streams=2), dict(precision="fp32"), dict(devices=[0, 0])):
        with gpcc_amd.Objective(t, y, s, gpcc_amd.matern52, **kw) as o2:
            assert _same(getattr(o2, entry)(delays, alpha, rho, weights=w), full), kw


def test_info_codes_and_neighbours():
    """alpha <= 0, rho <= 0 and NaN rows: info and loglik bitwise the siblings', the row's outputs NaN, the neighbours untouched; a
    failed row with weight makes the mixture NaN, with weight 0 it is skipped."""
    t, y, s, _ = MC.lightcurves([70, 60], seed=5, kind="plain")
    delays, alpha, rho = _pool(9, 2, seed=9)
    alpha[1, 0] = -1.0
    alpha[3, 1] = 0.0
    rho[5] = -2.0
    rho[7] = np.nan
    bad = np.array([1, 3, 5, 7])
    good = np.array([0, 2, 4, 6, 8])
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        for entry, sibling in (("loo_batch", lambda: obj.loglik_grad_batch(delays, alpha, rho)[::2]),
                               ("loo_markov_batch", lambda: obj.loglik_markov_batch(delays, alpha, rho))):
            res = getattr(obj, entry)(delays, alpha, rho)
            sl, si = sibling()
            assert np.array_equal(res.info, si) and np.array_equal(res.loglik, sl, equal_nan=True), entry
            assert res.info[1] == -1 and res.info[3] == -1 and res.info[5] == -2 and res.info[7] != 0 and (res.info[good] == 0).all()
            for q in ROWS:
                assert np.isnan(getattr(res, q)[bad]).all() and np.isfinite(getattr(res, q)[good]).all(), (entry, q)
            clean = getattr(obj, entry)(delays[good], alpha[good], rho[good])
            assert _same(clean, res, good, mix=False), entry
            w = np.where(np.isin(np.arange(9), bad), 0.0, 1.0 + np.arange(9))
            m0 = getattr(obj, entry)(delays, alpha, rho, weights=w)
            m1 = getattr(obj, entry)(delays[good], alpha[good], rho[good], weights=w[good])
            assert np.array_equal(m0.mix_lp, m1.mix_lp) and m0.mix_loo == m1.mix_loo and np.isfinite(m0.mix_loo), entry
            w[1] = 0.5
            m2 = getattr(obj, entry)(delays, alpha, rho, weights=w)
            assert np.isnan(m2.mix_lp).all() and np.isnan(m2.mix_loo), entry


def test_null_outputs_and_arguments():
    """Every combination of NULL outputs returns the bits of the full call for the others; mix_lp or mix_loo without weights, bad
    weights and an rbf handle on the linear-time entry are refused before any device work."""
    t, y, s, _ = MC.lightcurves([60, 50], seed=21, kind="ties")
    delays, alpha, rho = _pool(3, 2, seed=2)
    w = np.array([0.2, 0.0, 0.8])
    names = ("mu", "var", "lp", "loo", "mix_lp", "mix_loo", "loglik", "info")
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        for entry in ("loo_batch", "loo_markov_batch"):
            full = getattr(obj, entry)(delays, alpha, rho, weights=w)
            for mask in range(1 << len(names)):
                want = [n for j, n in enumerate(names) if mask >> j & 1]
                res = getattr(obj, entry)(delays, alpha, rho, weights=w, outputs=want)
                for n in names:
                    a, b = getattr(res, n), getattr(full, n)
                    assert (a is None) if n not in want else np.array_equal(a, b), (entry, want, n)
            with pytest.raises(gpcc_amd.GpccError) as ei:
                getattr(obj, entry)(delays, alpha, rho, outputs=["mix_lp"])
            assert ei.value.code == ARGUMENT
            for badw in ([1.0, -1.0, 1.0], [0.0] * 3, [1.0, np.nan, 1.0], [np.inf, 1.0, 1.0]):
                with pytest.raises(gpcc_amd.GpccError) as ei:
                    getattr(obj, entry)(delays, alpha, rho, weights=np.array(badw))
                assert ei.value.code == ARGUMENT
            with pytest.raises(ValueError):
                getattr(obj, entry)(delays, alpha, rho, weights=np.ones(2))
    with gpcc_amd.Objective(t, y, s, gpcc_amd.rbf) as obj:
        with pytest.raises(gpcc_amd.GpccError) as ei:
            obj.loo_markov_batch(delays, alpha, rho)
        assert ei.value.code == UNSUPPORTED and "rbf" in ei.value.message
        assert (obj.loo_batch(delays, alpha, rho).info == 0).all()


def test_linear_time_only_handle_builds_no_workspace():
    """N = 1024, 70 rows: a handle that only calls the linear-time entry never builds the N^2 workspace and grows by the documented
    buffers (the tap scratch of the 70 rows, which the budget holds in one chunk, 24 N bytes per row, the mixture and the indices),
    each of the twelve allocations rounded up to the allocator's 2 MiB granule; the N^2 workspace would be 1 GiB."""
    import torch
    Nl = [512, 512]
    t, y, s, d0 = MC.lightcurves(Nl, seed=1024, kind="plain")
    M, N, nrec = 70, 1024, 4 + 10
    delays, alpha, rho = _pool(M, 2, seed=4)
    torch.cuda.synchronize()
    with gpcc_amd.Objective(t, y, s, gpcc_amd.matern32) as obj:
        free0, _ = torch.cuda.mem_get_info(0)
        res = obj.loo_markov_batch(delays, alpha, rho, weights=np.ones(M))
        free1, _ = torch.cuda.mem_get_info(0)
        assert obj.get_option("workspace_slots") == obj.get_option("slots_per_stream")     # (never built)
        assert obj.get_option("markov_tap_bytes") == 16 * N * nrec * M
        ll, info = obj.loglik_markov_batch(delays, alpha, rho)
    documented = 16 * N * nrec * M + 24 * N * M + 32 * N + 16 * M + 8 * N
    assert free0 - free1 < documented + 12 * 2 * 2 ** 20, (free0 - free1, documented)
    assert (res.info == 0).all() and np.array_equal(res.loglik, ll) and np.array_equal(res.info, info)
    row = markov.loo("matern32", t, y, s, delays[69], alpha[69], rho[69], True)
    assert np.max(np.abs(res.lp[69] - row[2])) <= 1e-9 * np.max(np.abs(row[2])) and abs(res.loo[69] - row[3]) <= 1e-9 * abs(row[3])


def test_predictors():
    """Predictor.loo and DelayAveragedPredictor.loo: mu, sigma, lp, z and the total, dense and linear-time."""
    from gpcc_amd import fit
    t, y, s, _ = MC.lightcurves([60, 50], seed=33, kind="plain")
    delays, alpha, rho = _pool(4, 2, seed=6)
    yflat = np.concatenate(y)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        for solver, entry in (("dense", obj.loo_batch), ("markov", obj.loo_markov_batch)):
            one = fit.Predictor(obj, delays[0], alpha[0], rho[0]).loo(solver=solver)
            res = entry(delays[:1], alpha[:1], rho[:1])
            assert np.array_equal(one.mu, res.mu[0]) and np.array_equal(one.sigma, np.sqrt(res.var[0])) and np.array_equal(one.lp, res.lp[0])
            assert np.array_equal(one.z, (yflat - res.mu[0]) / np.sqrt(res.var[0])) and one.total == res.loo[0]
            w = np.array([0.1, 0.2, 0.3, 0.4])
            dap = fit.DelayAveragedPredictor(obj, delays, alpha, rho, w).loo(solver=solver)
            res = entry(delays, alpha, rho, weights=w)
            assert np.array_equal(dap.lp, res.mix_lp) and dap.total == res.mix_loo
            # the mixture given y_-i, point by point from the rows: weights q_g proportional to p_g / p_g(y_i | y_-i)
            p = w / w.sum()
            for i in (0, 17, 59, 60, 109):
                q = p / np.exp(res.lp[:, i] - res.lp[:, i].max())
                q = q / q.sum()
                m1 = float(np.sum(q * res.mu[:, i]))
                v1 = float(np.sum(q * (res.var[:, i] + res.mu[:, i] ** 2)) - m1 * m1)
                assert abs(dap.mu[i] - m1) <= 1e-12 * max(1.0, abs(m1)) and abs(dap.sigma[i] ** 2 - v1) <= 1e-10 * v1, (solver, i)
                assert abs(dap.z[i] - (yflat[i] - m1) / np.sqrt(v1)) <= 1e-9 * max(1.0, abs(dap.z[i]))
            assert abs(np.log(np.sum(p * np.exp(-(res.lp[:, 5] - res.lp[:, 5].min())))) - res.lp[:, 5].min() + dap.lp[5]) <= 1e-12
