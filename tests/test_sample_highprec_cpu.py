"""The extended-precision reference of the joint posterior draws and its bar (tests/_sample_highprec.py) check themselves, without a
GPU:

  the reference   against mpmath: the longdouble Box-Muller normals, the process-noise factor C C' against the 80-digit Q = Pinf -
                  A Pinf A' (lags 2^-10 .. 50 rho, rho = 0.1 .. 300, the two fp64 lags on either side of lambda d = 1 and of the
                  reference's own change of form), and the dense and linear-time draws of one tiny case per kernel and b-mode (N = 12,
                  T = 5, a test point on a training point).  Condition: 64 x finer than what each is judged by at 2^-53 -- the draws by the
                  bar's floor, (N + T) 2^-53 (|mu| + sum |L zeta|) (dense) and (N + T) 2^-53 (|mu| + |g~| + |c| + |noise|)
                  (linear-time), the largest over the case's draws and entries as in the bar (the reference's own rounding is
                  relative to sums like sum |kB* w| and the alpha^2-sized terms that cancel in S, in any precision: an entry
                  whose mean and normals happen to be small, or rho = 300, costs it tens of eps of the bare terms);
                  Q by 2^-53 sqrt(Q_ii Q_jj); the normals by 2^-53 r.  The agreement is printed in units of the longdouble eps.
  the normals     gpcc_amd.rng's fp64 normals within the derived nu of the longdouble ones
  slips           every slip of _sample_witness.draws and of markov.sample misses the bar on every case of the 72 where, by the
                  case's construction (CAN_ACT), it can act; the smallest miss is printed
  rounding        fp64 evaluations in other orders pass it: the mirror with every process-noise integral off by one eps, the
                  64-blocked dense run, LAPACK on the training points in reversed order
  the old bar     a draw wrong by 1e-10 passes max(1e-10, 64 eps cond_1) max(1, max |f*|) and misses the new bar."""
import numpy as np
import pytest

import _heldout_witness as HW
import _markov_cases as MC
import _markov_sample_cases as SC
import _sample_highprec as SH
import _sample_witness as SW
from gpcc_amd import markov, rng

pytestmark = pytest.mark.skipif(not SH.EXTENDED, reason=SH.SKIP_REASON)

CASES = SH.cases()
LDEPS = float(np.finfo(SH.LD).eps)
FINE = 2.0 ** -59                    # 64 x finer than 2^-53
S = 3
_dense = {}


def _word(idx):
    return rng.MIXROW if idx % 2 else 0


def _dense_ref(oracle, idx):
    """(Reference, zeta) of the dense draws of case idx for rng.normals' zeta (cached)."""
    if idx not in _dense:
        cid, k, data, delays, alpha, rho, mb, tests = CASES[idx]
        zeta = rng.normals(900 + idx, sum(len(a) for a in tests[0]), range(S), _word(idx))
        _dense[idx] = (SH.dense_reference(oracle, k, data, delays, alpha, rho, mb, tests[0], tests[2], zeta), zeta)
    return _dense[idx]


def _linear_ref(oracle, idx):
    return SH.linear_reference(oracle, CASES[idx], 500 + idx, S, _word(idx))


# -- against mpmath -----------------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath as mp
    mp.mp.dps = 80
    return mp


def test_normals_against_mpmath_and_fp64_within_nu():
    mp = _mp()
    x = SH.words(11, 16, range(4), 0, rng.STREAM_NORMALS)
    z, nu = SH.box_muller(x)
    worst = 0.0
    for b, zb in zip(x.reshape(-1, 4)[:32], z.reshape(-1, 4)[:32]):
        for p in range(2):
            u1, u2 = mp.mpf(int(b[2 * p] >> np.uint64(11)) + 1) / 2 ** 53, mp.mpf(int(b[2 * p + 1] >> np.uint64(11))) / 2 ** 53
            r = mp.sqrt(-2 * mp.log(u1))
            for got, want in ((zb[2 * p], r * mp.cos(2 * mp.pi * u2)), (zb[2 * p + 1], r * mp.sin(2 * mp.pi * u2))):
                worst = max(worst, float(abs(_mp_of(got) - want) / r))
    print("longdouble Box-Muller against mpmath: at most %.3g longdouble eps of r" % (worst / LDEPS))
    assert worst <= FINE
    zd, nud = SH.dense_normals(7, 1024, range(1024), [0] * 512 + [rng.MIXROW] * 512)
    zp, nup = SH.point_normals(7, 1024, range(64), [0] * 32 + [rng.MIXROW] * 32)
    rd = float(np.max(SH.err(rng.normals(7, 1024, range(1024), [0] * 512 + [rng.MIXROW] * 512), zd) / nud))
    rp = float(np.max(SH.err(rng.point_normals(7, 1024, range(64), [0] * 32 + [rng.MIXROW] * 32), zp) / nup))
    print("fp64 normals on the CPU against the longdouble ones: rng.normals %.3g nu (2^20 normals), rng.point_normals %.3g nu (2^18)"
          % (rd, rp))
    assert rd <= 1.0 and rp <= 1.0
    assert np.all(nud >= 16 * SH.U53 * SH.U53) and np.all(nud <= 16 * SH.U53 * 9.0)


def _mp_of(v):
    """An mpf of a longdouble or float64, exactly."""
    import mpmath as mp
    v = SH.LD(v)
    hi = np.float64(v)
    return mp.mpf(float(hi)) + mp.mpf(float(np.float64(v - SH.LD(hi))))


def _mp_process(kernel, d, rho):
    """(A, Pinf, Q = Pinf - A Pinf A') of the kernel's state at lag d (an mpf) in mpmath."""
    mp = _mp()
    lam = mp.sqrt({"OU": 1, "matern32": 3, "matern52": 5}[kernel]) / mp.mpf(float(rho))
    x, e = lam * d, mp.exp(-lam * d)
    if kernel == "OU":
        A, P = mp.matrix([[e]]), mp.matrix([[1]])
    elif kernel == "matern32":
        A, P = e * mp.matrix([[1 + x, d], [-lam * lam * d, 1 - x]]), mp.matrix([[1, 0], [0, lam ** 2]])
    else:
        l2 = lam * lam
        A = e * mp.matrix([[1 + x + x * x / 2, d * (1 + x), d * d / 2], [-l2 * lam * d * d / 2, 1 + x - x * x, d * (1 - x / 2)],
                           [l2 * x * (x / 2 - 1), lam * x * (x - 3), 1 - 2 * x + x * x / 2]])
        P = mp.matrix([[1, 0, -l2 / 3], [0, l2 / 3, 0], [-l2 / 3, 0, lam ** 4]])
    return A, P, P - A * P * A.T


def _mp_upper_factor(Q):
    """C upper triangular with C C' = Q, eliminated from the last component."""
    mp = _mp()
    p = Q.rows
    C = mp.zeros(p, p)
    for j in range(p - 1, -1, -1):
        C[j, j] = mp.sqrt(Q[j, j] - sum(C[j, k] ** 2 for k in range(j + 1, p)))
        for i in range(j):
            C[i, j] = (Q[i, j] - sum(C[i, k] * C[j, k] for k in range(j + 1, p))) / C[j, j]
    return C


@pytest.mark.parametrize("kernel", markov.KERNELS)
def test_process_noise_factor_against_80_digits(kernel):
    mp = _mp()
    worst = (0.0, None)
    for rho in (0.1, 3.0, 20.0, 300.0):
        lam64 = markov.rate(kernel, rho)
        lam = SH.rate(kernel, rho)
        d_lo, d_hi = SH.branch_band(kernel, rho, False)[1]
        assert lam64 * d_lo <= 1.0 < lam64 * d_hi and d_hi == np.nextafter(d_lo, np.inf)
        edge = float(SH.SERIES_MAX / lam)
        lags = [2.0 ** -10 * k for k in (1, 3, 17, 100, 256, 277, 301, 1000, 5000)] + [0.3 / lam64, d_lo, d_hi, np.nextafter(edge, 0.0),
                                                                                        np.nextafter(edge, np.inf), 40.0, 50.0 * rho]
        sc = 1 / np.sqrt(np.diagonal(SH.stationary(kernel, lam)))
        for d in lags:
            C = SH.sim_factor(kernel, d, lam)
            got = sc[:, None] * (C @ C.T) * sc[None, :]
            _, P, Q = _mp_process(kernel, mp.mpf(float(d)), rho)
            for i in range(len(sc)):
                for j in range(len(sc)):
                    want = Q[i, j] / mp.sqrt(P[i, i] * P[j, j])
                    scale = mp.sqrt(Q[i, i] * Q[j, j] / (P[i, i] * P[j, j]))
                    e = float(abs(_mp_of(got[i, j]) - want) / scale)
                    worst = max(worst, (e, (rho, float(d), i, j)))
    print("%s: longdouble C C' against the 80-digit Q: at most %.3g longdouble eps of sqrt(Q_ii Q_jj) at (rho, d, i, j) = %s (condition %.3g)"
          % (kernel, worst[0] / LDEPS, worst[1], FINE / LDEPS))
    assert worst[0] <= FINE


def _tiny(kernel, mb):
    """N = 7 + 5, T = 3 + 2 on the 2^-10 grid; the last test point of band 2 sits on a training point of band 1 in shifted time."""
    rg = np.random.default_rng(40 + len(kernel) + mb)
    delays = np.array([0.0, MC.snap(rg.uniform(-1.0, 2.0))])
    t = [np.sort(MC.snap(rg.uniform(0.0, 8.0, n))) for n in (7, 5)]
    y = [np.sin(0.7 * (t[l] - delays[l])) + 0.4 * l + 0.2 * rg.standard_normal(len(t[l])) for l in range(2)]
    s = [0.2 + 0.05 * rg.random(len(a)) for a in t]
    tt = [MC.snap(rg.uniform(-1.0, 9.0, 3)), np.array([MC.snap(rg.uniform(-1.0, 9.0)), t[0][3] + delays[1]])]
    st = [0.2 + 0.05 * rg.random(len(a)) for a in tt]
    rho = {"OU": 0.4, "rbf": 2.0, "matern32": 9.0, "matern52": 300.0}[kernel]
    return ("tiny-%s-b%d" % (kernel, mb), kernel, (t, y, s), delays, rg.uniform(0.5, 2.0, 2), rho, mb, (tt, None, st))


def _mp_kernel(kernel, s, rho):
    mp = _mp()
    r = abs(s)
    if kernel == "OU":
        return mp.exp(-r / rho)
    if kernel == "rbf":
        return mp.exp(-s * s / (4 * rho))
    if kernel == "matern32":
        a = mp.sqrt(3) * r / rho
        return (1 + a) * mp.exp(-a)
    a = mp.sqrt(5) * r / rho
    return (1 + a + a * a / 3) * mp.exp(-a)


def _mp_model(case):
    """(K, kB, cB + diag(sigma*^2 + JITTER), y - mean, mean of the test points' bands, Sigma_b, sd) of a case in mpmath."""
    mp = _mp()
    cid, kernel, (t, y, s), delays, alpha, rho, mb, (tt, _, st) = case
    f = lambda v: mp.mpf(float(v))                                                                     # noqa: E731
    band = [l for l, a in enumerate(t) for _ in a]
    bs = [l for l, a in enumerate(tt) for _ in a]
    u = [f(v) - f(delays[l]) for l, a in enumerate(t) for v in a]
    us = [f(v) - f(delays[l]) for l, a in enumerate(tt) for v in a]
    sd = [f(v) for a in s for v in a]
    sst = [f(v) for a in st for v in a]
    mean = [sum(f(v) for v in a) / len(a) for a in y]
    Sigb = [100 * sum((f(v) - m) ** 2 for v in a) / (len(a) - 1) if mb else mp.mpf(0) for a, m in zip(y, mean)]
    al, rh = [f(v) for v in alpha], f(rho)
    cov = lambda p, a, q, b: al[p] * al[q] * _mp_kernel(kernel, a - b, rh) + (Sigb[p] if p == q else 0)   # noqa: E731
    N, T = len(u), len(us)
    K = mp.matrix(N, N)
    kB = mp.matrix(N, T)
    cB = mp.matrix(T, T)
    for i in range(N):
        for j in range(N):
            K[i, j] = cov(band[i], u[i], band[j], u[j]) + (sd[i] ** 2 if i == j else 0)
        for j in range(T):
            kB[i, j] = cov(band[i], u[i], bs[j], us[j])
    for i in range(T):
        for j in range(T):
            cB[i, j] = cov(bs[i], us[i], bs[j], us[j]) + (sst[i] ** 2 + f(SH.JITTER) if i == j else 0)
    resid = mp.matrix([f(v) - mean[l] for l, a in enumerate(y) for v in a])
    return K, kB, cB, resid, mp.matrix([mean[q] for q in bs]), Sigb, sd, sst


@pytest.mark.parametrize("mb", [True, False])
@pytest.mark.parametrize("kernel", ["OU", "rbf", "matern32", "matern52"])
def test_draws_against_40_digits(kernel, mb):
    mp = _mp()
    case = _tiny(kernel, mb)
    cid, _, data, delays, alpha, rho, _, (tt, _, st) = case
    N, T = SC.dims(case)
    assert (N, T) == (12, 5) and np.isin(tt[1][-1] - delays[1], data[0][0]).any()
    K, kB, C, resid, meanq, Sigb, sd, sst = _mp_model(case)
    Kinv_kB = mp.inverse(K) * kB
    mu = Kinv_kB.T * resid + meanq
    Sm = C - kB.T * Kinv_kB
    Lc = mp.cholesky((Sm + Sm.T) / 2)
    zeta = rng.normals(5, T, range(S), 0)
    m = SH.model(kernel, *data, delays, alpha, rho, tt, mb)
    draws, terms, _ = SH.dense_draws(m, st, zeta)
    worst = 0.0
    for s in range(S):
        want = mu + Lc * mp.matrix([mp.mpf(float(v)) for v in zeta[s]])
        worst = max(worst, max(float(abs(_mp_of(draws[s, j]) - want[j])) for j in range(T)) / ((N + T) * float(np.max(terms))))
    print("%s dense draw: longdouble against mpmath at most %.3g longdouble eps of (N + T) (|mu| + sum |L zeta|) (condition %.3g)"
          % (cid, worst / LDEPS, FINE / LDEPS))
    dense_worst = worst
    if kernel == "rbf":
        assert dense_worst <= FINE
        return
    # the linear-time draw: the walk of _sample_highprec.merged_points with the 80-digit A and Q = Pinf - A Pinf A'
    p, Kc = markov.order(kernel), 4 * (N + T + 1)
    Rt, Gg, Gn = mp.zeros(N, Kc), mp.zeros(T, Kc), mp.zeros(T, Kc)
    X, sprev = None, None
    for (sv, kind, b, _, e) in SH.merged_points(data[0], tt, delays):
        sv = _mp_of(sv)
        if X is None:
            X, Cf = mp.zeros(p, Kc), _mp_upper_factor(_mp_process(kernel, mp.mpf(1), rho)[1])
        elif sv != sprev:
            A, _, Q = _mp_process(kernel, sv - sprev, rho)
            X, Cf = A * X, _mp_upper_factor(Q)
        else:
            Cf = mp.zeros(p, p)
        for i in range(p):
            for c in range(p):
                X[i, 4 * e + c] += Cf[i, c]
        sprev = sv
        f = [mp.mpf(float(alpha[b])) * X[0, c] for c in range(Kc)]
        f[4 * (N + T) + b] += mp.sqrt(Sigb[b])
        if kind == 0:
            f[4 * e + 3] += sd[e]
        for c in range(Kc):
            (Rt if kind == 0 else Gg)[e if kind == 0 else e - N, c] = f[c]
        if kind == 1:
            Gn[e - N, 4 * e + 3] = mp.sqrt(mp.mpf(float(SH.JITTER)) + sst[e - N] ** 2)
    G = Gg - Kinv_kB.T * Rt + Gn
    lmu, lGg, lC, lGn, _ = SH.linear_map(kernel, data, delays, alpha, rho, mb, tt, st)
    xi = rng.point_normals(5, N + T + 1, range(S), 0).reshape(S, -1)
    worst, x = 0.0, xi.astype(SH.LD).T
    scale = (N + T) * float(np.max(np.abs(lmu)[:, None] + np.abs(lGg @ x) + np.abs(lC @ x) + np.abs(lGn @ x)))
    for s in range(S):
        got = lmu + (lGg - lC + lGn) @ x[:, s]
        want = mu + G * mp.matrix([mp.mpf(float(v)) for v in xi[s]])
        worst = max(worst, max(float(abs(_mp_of(got[j]) - want[j])) for j in range(T)) / scale)
    print("%s linear-time draw: longdouble against mpmath at most %.3g longdouble eps of (N + T) (|mu| + |g~| + |c| + |noise|) (condition %.3g)"
          % (cid, worst / LDEPS, FINE / LDEPS))
    assert dense_worst <= FINE and worst <= FINE


# -- the bar ------------------------------------------------------------------------------------------------------------------------
def _has_tie(case):
    _, _, (t, _, _), delays, _, _, _, tests = case
    train = np.concatenate([np.asarray(a) - delays[l] for l, a in enumerate(t)])
    star = np.concatenate([np.asarray(a) - delays[l] for l, a in enumerate(tests[0])])
    return bool(np.isin(star, train).any())


def _matern_rho300(case):
    """A Matern kernel at rho = 300: the points lie on the 2^-10 grid inside [0, 30], so every lag has lambda d < 1 (the series in the
    healthy code) and the smallest ones lambda d ~ 1e-5, where Q's leading entry, ~x^3 or ~x^5 of a unit diagonal, is far below the
    2^-53 rounding of the difference Pinf - A Pinf A' that "q_by_difference" forms: its first pivot is rounding."""
    return case[1] != "OU" and case[5] == 300.0


CAN_ACT = {("witness", "no_jitter"): lambda c: True, ("witness", "transpose"): lambda c: True, ("witness", "no_bbar"): lambda c: True,
           ("witness", "shift"): lambda c: True, ("witness", "no_b_cross"): lambda c: bool(c[6]),
           ("mirror", "no_flip"): lambda c: c[1] != "OU", ("mirror", "tie_both"): _has_tie, ("mirror", "no_prior"): lambda c: True,
           ("mirror", "no_obs_noise"): lambda c: True, ("mirror", "no_offset_draw"): lambda c: bool(c[6]), ("mirror", "plus"): lambda c: True,
           ("mirror", "merged_index"): lambda c: True, ("mirror", "q_by_difference"): _matern_rho300}


@pytest.mark.parametrize("source,slip", sorted(CAN_ACT))
def test_bar_rejects_slips(oracle, source, slip):
    acts = [i for i, c in enumerate(CASES) if CAN_ACT[(source, slip)](c)]
    assert len(acts) >= (12 if slip == "q_by_difference" else 36), len(acts)
    ratios = []
    for idx in acts:
        cid, k, data, delays, alpha, rho, mb, tests = CASES[idx]
        if source == "witness":
            ref, zeta = _dense_ref(oracle, idx)
            try:
                got = SW.draws(oracle, k, *data, delays, alpha, rho, tests[0], tests[2], zeta, marginalise_b=mb, slip=slip)[0]
            except np.linalg.LinAlgError:                  # no_jitter on the latent curve: repeated test times leave S singular
                got = np.full(ref.draws.shape, np.nan)
            ratios.append((ref.ratio(got), cid))
        else:
            ref = _linear_ref(oracle, idx)
            got = markov.sample(k, *data, delays, alpha, rho, tests[0], tests[2], mb, seed=500 + idx, s=0, m=_word(idx), _slip=slip)[0]
            ratios.append((float(np.max(SH.err(got, ref.draws[0]) / ref.bar[0])), cid))
    low = min(ratios)
    print("%s %s: smallest error / bar %.3g (%s) over the %d cases it can act on" % (source, slip, low[0], low[1], len(acts)))
    missed = [(r, cid) for r, cid in ratios if not r > 1.0]
    assert not missed, missed


def _reversed_lapack(oracle, case, zeta=None, prior=None):
    """The witness's algebra by LAPACK with the training points in reversed order: the dense draws of zeta, or the Matheron draw of
    the prior draw (r~, g~, noise)."""
    cid, k, data, delays, alpha, rho, mb, tests = case
    st = tests[2] if tests[2] is not None else [np.zeros(len(a)) for a in tests[0]]
    K, resid, kB, C, bs, mub = HW.blocks(oracle, k, *data, delays, alpha, rho, tests[0], st, mb)
    W = np.linalg.solve(K[::-1, ::-1], kB[::-1]).T
    mu = W @ resid[::-1] + mub[bs]
    if prior is not None:
        return mu + prior[1] - W @ prior[0][::-1] + prior[2]
    Sm = C - W @ kB[::-1]
    return mu[None, :] + zeta @ np.linalg.cholesky(0.5 * (Sm + Sm.T)).T


def test_legitimate_rounding_passes(oracle, monkeypatch):
    """fp64 evaluations that no term of the bar was measured on."""
    eps = np.finfo(np.float64).eps
    plain = markov._lower_gammas
    worst = {n: SH.Worst("rounding: " + n) for n in ("mirror, every process-noise integral off by one eps", "dense draws, 64-blocked",
                                                     "dense draws, LAPACK on reversed points", "linear-time draws, LAPACK on reversed points")}
    for idx, case in enumerate(CASES):
        cid, k, data, delays, alpha, rho, mb, tests = case
        ref, zeta = _dense_ref(oracle, idx)
        m = SH.model(k, *data, delays, alpha, rho, tests[0], mb)
        worst["dense draws, 64-blocked"].add(ref.ratio(SH.dense_draws(m, tests[2], zeta, np.float64, SH.NB, direct=True)[0]), cid)
        worst["dense draws, LAPACK on reversed points"].add(ref.ratio(_reversed_lapack(oracle, case, zeta=zeta)), cid)
        lref = _linear_ref(oracle, idx)
        kw = dict(seed=500 + idx, s=0, m=_word(idx))
        prior = markov.prior_draw(k, *data, delays, alpha, rho, tests[0], tests[2], mb, **kw)
        got = _reversed_lapack(oracle, case, prior=prior)
        worst["linear-time draws, LAPACK on reversed points"].add(float(np.max(SH.err(got, lref.draws[0]) / lref.bar[0])), cid)
        monkeypatch.setattr(markov, "_lower_gammas", lambda K, y: [g * (1.0 + (eps if j % 2 else -eps)) for j, g in enumerate(plain(K, y))])
        got = markov.sample(k, *data, delays, alpha, rho, tests[0], tests[2], mb, **kw)[0]
        monkeypatch.setattr(markov, "_lower_gammas", plain)
        worst["mirror, every process-noise integral off by one eps"].add(float(np.max(SH.err(got, lref.draws[0]) / lref.bar[0])), cid)
    SH.report(worst.values())


def test_bars_against_the_old_bar(oracle):
    """The new bar over the old one, max(1e-10, 64 eps cond_1(K_aug)) max(1, max |f*|), on the 72 cases; and the old bar's slack: a
    draw wrong by 1e-10 in one entry passes the old bar (on every case, by its floor) and misses the new one wherever that is below
    1e-10 -- on most cases, the first of each family among them."""
    for name, refs in (("dense", [_dense_ref(oracle, i)[0] for i in range(len(CASES))]),
                       ("linear-time", [_linear_ref(oracle, i) for i in range(len(CASES))])):
        bars = np.array([float(np.max(r.bar)) for r in refs])
        old = np.array([r.old_bar for r in refs])
        given = np.arange(len(CASES)) % 2 == 0
        print("%s draws: new bar %.2g .. %.2g with test noise (old %.2g .. %.2g), %.2g .. %.2g on the latent curve (old %.2g .. %.2g); "
              "new / old %.2g .. %.2g" % (name, bars[given].min(), bars[given].max(), old[given].min(), old[given].max(), bars[~given].min(),
                                         bars[~given].max(), old[~given].min(), old[~given].max(), (bars / old).min(), (bars / old).max()))
        assert np.all(bars < old)
        wrong = np.array(refs[0].draws, dtype=np.float64)
        wrong[0, 0] += 1e-10
        assert abs(wrong[0, 0] - float(refs[0].draws[0, 0])) <= refs[0].old_bar and refs[0].ratio(wrong) > 1.0
        caught = sum(1e-10 > float(np.max(r.bar)) for r in refs)
        print("%s draws: an entry off by 1e-10 passes the old bar on all 72 cases and misses the new one on %d (%s: %.3g of the new bar)"
              % (name, caught, CASES[0][0], refs[0].ratio(wrong)))
        assert caught >= 36
