"""The numpy mirror of the linear-time joint posterior draws under a per-row noise model (gpcc_amd.markov.sample_noise)
against the extended-precision reference of tests/_markov_noise_sample_cases.py -- the plain reference on each row's effective error
bars, under its own bar -- on all 72 cases; exact equality with markov.sample at kappa = 1, nu = 0; the four test slips, each missing
the bar wherever it can act and changing no bit elsewhere; the codes; and the wiring of Predictor.sample /
DelayAveragedPredictor.sample under kappa=, nu=.  Lines that start with "noise-sample" are kept in
profiles/markov/noise_sample_parity.log."""
import numpy as np
import pytest

import _markov_noise_sample_cases as C
import _sample_highprec as SH
from gpcc_amd import fit, markov

extended = pytest.mark.skipif(not SH.EXTENDED, reason=SH.SKIP_REASON)
CASES = C.cases()


def _mirror(entry, idx, s, slip=None):
    (cid, k, data, delays, alpha, rho, mb, tests), kappa, nu = entry
    draw, ll, info = markov.sample_noise(k, *data, delays, alpha, rho, tests[0], kappa, nu, tests[2], mb, seed=C.seed_of(idx), s=s,
                                         m=C.word_of(idx), _slip=slip)
    assert info == 0, cid
    return draw


def test_case_rules():
    assert len(CASES) == 72
    for idx, ((cid, k, data, delays, alpha, rho, mb, tests), kappa, nu) in enumerate(CASES):
        assert (tests[2] is None) == bool(idx % 2) and sum(len(a) for a in data[0]) == 110, cid
        assert kappa.shape == nu.shape == alpha.shape and np.any(kappa != 1.0) and np.any(nu != 0.0), cid
    ids = [C.restated(e)[0] for e in CASES]
    assert len(set(ids)) == 72 and not set(ids) & {c[0] for c in SH.cases()}          # ids of their own: the helper caches by id


@extended
def test_mirror_meets_the_bar(oracle):
    """No case is left out: every reference exists (its factorisations assert it) and the mirror is within its bar."""
    worst = SH.Worst("noise-sample mirror draws, 72 cases x %d draws (error / bar)" % C.S)
    for idx, entry in enumerate(CASES):
        ref = C.reference(oracle, entry, C.seed_of(idx), C.S, C.word_of(idx))
        assert np.all(np.isfinite(ref.draws.astype(np.float64))), entry[0][0]
        worst.add(ref.ratio(np.stack([_mirror(entry, idx, s) for s in range(C.S)])), entry[0][0])
    SH.report([worst])


def test_unit_noise_is_the_plain_mirror_exactly():
    for idx, ((cid, k, data, delays, alpha, rho, mb, tests), _, _) in enumerate(CASES):
        L = len(alpha)
        kw = dict(seed=C.seed_of(idx), s=1, m=C.word_of(idx))
        plain = markov.sample(k, *data, delays, alpha, rho, tests[0], tests[2], mb, **kw)
        for kappa, nu in ((None, None), (np.ones(L), np.zeros(L))):
            got = markov.sample_noise(k, *data, delays, alpha, rho, tests[0], kappa, nu, tests[2], mb, **kw)
            assert np.array_equal(got[0], plain[0]) and got[1:] == plain[1:], cid


CAN_ACT = {"draw_obs_noise_raw": lambda e: True,
           "draw_test_noise_raw": lambda e: e[0][7][2] is not None,
           "kappa_linear": lambda e: not np.all((e[1] == 0.0) | (e[1] == 1.0)),
           "noise_all_bands": lambda e: len(e[1]) >= 2}


@extended
@pytest.mark.parametrize("slip", C.SLIPS)
def test_slips_miss_the_bar(oracle, slip):
    assert set(C.SLIPS) == set(CAN_ACT) == set(markov.NOISE_SAMPLE_SLIPS)
    ratios = []
    for idx, entry in enumerate(CASES):
        got = _mirror(entry, idx, 0, slip)
        if not CAN_ACT[slip](entry):
            assert np.array_equal(got, _mirror(entry, idx, 0)), entry[0][0]
            continue
        ref = C.reference(oracle, entry, C.seed_of(idx), C.S, C.word_of(idx))
        ratios.append((float(np.max(SH.err(got, ref.draws[0]) / ref.bar[0])), entry[0][0]))
    low = min(ratios)
    print("noise-sample slip %s: smallest error / bar %.3g (%s) over the %d cases it can act on" % (slip, low[0], low[1], len(ratios)))
    assert len(ratios) == {"draw_test_noise_raw": 36, "kappa_linear": 60, "noise_all_bands": 48}.get(slip, 72)
    missed = [(r, cid) for r, cid in ratios if not r > 1.0]
    assert not missed, missed


def test_codes():
    (cid, k, data, delays, alpha, rho, mb, tests), kappa, nu = CASES[4]
    T = sum(len(a) for a in tests[0])
    bad_k, bad_v = kappa.copy(), nu.copy()
    bad_k[0], bad_v[-1] = -1.0, np.nan
    for kk, vv in ((bad_k, nu), (kappa, bad_v), (np.full(len(kappa), np.inf), nu)):
        draw, ll, info = markov.sample_noise(k, *data, delays, alpha, rho, tests[0], kk, vv, tests[2], mb)
        assert info == -3 and draw.shape == (T,) and np.isnan(draw).all() and np.isnan(ll)
    assert markov.sample_noise(k, *data, delays, -alpha, rho, tests[0], bad_k, nu, tests[2], mb)[2] == -1       # -1 and -2 come first
    assert markov.sample_noise(k, *data, delays, alpha, -rho, tests[0], bad_k, nu, tests[2], mb)[2] == -2
    with pytest.raises(ValueError):
        markov.sample_noise(k, *data, delays, alpha, rho, tests[0], kappa, nu, tests[2], mb, _slip="heldout_raw_sigmatest")
    assert markov.NOISE_PREDICT_SLIPS == ("heldout_raw_sigmatest", "loo_var_raw", "kappa_linear", "noise_all_bands")


def test_the_mirror_objective_draws_rows_under_their_own_models():
    (cid, k, (t, y, s), delays, alpha, rho, mb, tests), kappa, nu = CASES[26]
    obj = markov.MarkovObjective(t, y, s, k, marginalise_b=mb)
    kk, vv = np.stack([kappa, 1.3 * kappa]), np.stack([nu, nu + 0.01])
    dr, rows, ll, info = obj.sample_markov_noise_batch([delays] * 2, [alpha] * 2, [rho] * 2, kk, vv, tests[0], 2, 9, sigmatest=tests[2])
    assert dr.shape[0] == 4 and list(rows) == [0, 0, 1, 1] and list(info) == [0, 0]
    for m in range(2):
        one = markov.sample_noise(k, t, y, s, delays, alpha, rho, tests[0], kk[m], vv[m], tests[2], mb, seed=9, s=1, m=m)
        assert np.array_equal(dr[2 * m + 1], one[0]) and ll[m] == one[1]
    # a row is the plain mirror on a fresh data set with the effective error bars, the same seed: to rounding
    fresh = markov.sample(k, t, y, fit.effective_std(s, kk[1], vv[1]), delays, alpha, rho, tests[0],
                          fit.effective_std(tests[2], kk[1], vv[1]), mb, seed=9, s=0, m=1)
    assert np.allclose(dr[2], fresh[0], rtol=1e-9, atol=1e-11)


class _Recorder:
    def __init__(self, out):
        self.calls, self.out = [], out

    def __call__(self, *args, **kw):
        self.calls.append((args, kw))
        return self.out


def test_predictors_route_sample_through_the_noise_entry(monkeypatch):
    (cid, k, (t, y, s), delays, alpha, rho, mb, tests), kappa, nu = CASES[26]
    L, G, S = len(alpha), 3, 5
    assert L == 2
    obj = markov.MarkovObjective(t, y, s, k)
    tt = np.linspace(0.0, 30.0, 4)
    pred = fit.Predictor(obj, delays, alpha, rho, solver="markov", kappa=kappa, nu=nu)
    for solver in (None, "dense"):                                    # the dense path has no noise model
        with pytest.raises(NotImplementedError, match="effective_std"):
            pred.sample(tt, S, 1, solver=solver)
    canned = (np.arange(S * 2 * 4, dtype=np.float64).reshape(S, 8), np.zeros(S, np.int32), np.zeros(1), np.zeros(1, np.int32))
    rec = _Recorder(canned)
    monkeypatch.setattr(obj, "sample_markov_noise_batch", rec)
    monkeypatch.setattr(obj, "sample_markov_batch", _Recorder(None))
    bands = pred.sample(tt, S, 17, sigmatest=0.1 * np.ones(4), solver="markov")
    assert len(rec.calls) == 1 and not obj.sample_markov_batch.calls
    args, kw = rec.calls[0]
    assert np.array_equal(args[0], delays[None, :]) and np.array_equal(args[1], alpha[None, :]) and list(args[2]) == [rho]
    assert np.array_equal(args[3], kappa[None, :]) and np.array_equal(args[4], nu[None, :]) and args[3].shape == (1, L)
    assert len(args[5]) == L and all(np.array_equal(b, tt) for b in args[5]) and args[6:] == (S, 17)
    assert all(np.array_equal(b, 0.1 * np.ones(4)) for b in kw["sigmatest"]) and "weights" not in kw
    assert [b.shape for b in bands] == [(S, 4), (S, 4)] and np.array_equal(np.concatenate(bands, 1), canned[0])
    # the delay average: one call for the whole mixture, every row under its own model, `row` passed through
    cand = np.stack([delays, delays + [0.0, 0.25], delays + [0.0, 0.5]])
    kk, vv, w = np.stack([kappa, 1.3 * kappa, 0.8 * kappa]), np.stack([nu, nu + 0.01, 2 * nu]), np.array([0.2, 0.5, 0.3])
    avg = fit.DelayAveragedPredictor(obj, cand, [alpha] * G, [rho] * G, w, solver="markov", kappa=kk, nu=vv)
    with pytest.raises(NotImplementedError, match="effective_std"):
        avg.sample(tt, S, 1)
    picked = np.array([1, 1, 0, 2, 1], np.int32)
    rec = _Recorder((canned[0], picked, np.zeros(G), np.zeros(G, np.int32)))
    monkeypatch.setattr(obj, "sample_markov_noise_batch", rec)
    bands, row = avg.sample(tt, S, 23, solver="markov")
    assert len(rec.calls) == 1 and row is picked
    args, kw = rec.calls[0]
    assert np.array_equal(args[0], cand) and np.array_equal(args[3], kk) and np.array_equal(args[4], vv) and args[6:] == (S, 23)
    assert np.array_equal(kw["weights"], w) and kw["sigmatest"] is None and np.array_equal(np.concatenate(bands, 1), canned[0])
    # (L,) broadcasts over the rows
    avg = fit.DelayAveragedPredictor(obj, cand, [alpha] * G, [rho] * G, w, solver="markov", kappa=kappa)
    avg.sample(tt, S, 23, solver="markov")
    assert np.array_equal(rec.calls[1][0][3], np.tile(kappa, (G, 1))) and np.array_equal(rec.calls[1][0][4], np.zeros((G, L)))
    # without a noise model nothing changed: the plain entry
    monkeypatch.setattr(obj, "sample_markov_batch", _Recorder(canned))
    fit.Predictor(obj, delays, alpha, rho, solver="markov").sample(tt, S, 17, solver="markov")
    assert len(obj.sample_markov_batch.calls) == 1 and len(rec.calls) == 2
    assert "solver=\"markov\"" in fit.noise_predictor.__doc__
