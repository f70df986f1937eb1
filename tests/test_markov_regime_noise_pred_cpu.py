"""The numpy mirror (gpcc_amd.markov) of the noise-model predictions, held-out scores, offsets' posterior, leave-one-out scores and draws,
and of the gradient of rows with their own resampled data set, against the extended-precision references over
tests/_markov_regime_noise_pred_cases.py: 4 and 8 bands with three or more bands tied on one shifted time, lambda x lag down to 5e-8, rho
up to 3e5 for the gradient.  It shows that the references alone stay within the bars and that every condition on the cases holds,
counted from the data: info == 0 on all sides (asserted where the jobs run), test points and the promised tie structure on every
case with three or more bands, a tie of three bands left in the subset cells; no case or cell is filtered.  In the control tier
(k = 0) the mirror is held to each family's existing bar as it stands; in the other tiers the bar is max(existing, 16 e_mirror),
trivial for the mirror itself, and what is printed per pair (-s) is how far the existing bar is exceeded.  Per family one injected slip
has to miss the bar of a quantity it touches by a factor of two at L = 8, k = 0 and k = 14; so has the tie-swap slip (a point's noise
taken by another band inside a tie of three bands) for the predictions and held-out scores."""
import math
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _grad_highprec as H
import _loo_highprec as LH
import _markov_noise_sample_cases as NS
import _markov_regime_cases as RC
import _markov_regime_noise_cases as RN
import _markov_regime_noise_pred_cases as RP
import _markov_resample_cases as SC
import _predict_highprec as PH

pytestmark = pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)

K_TIERS = RC.TIERS[:4]


@pytest.fixture(scope="module")
def pool(oracle):
    """The workers reach the CPU oracle through RC._oracle(), which loads it: the session's oracle fixture has built it before they start."""
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


def test_conditions_are_counted_from_the_data():
    seen = ties = 0
    for tier in K_TIERS:
        cases = RP.small(tier)
        assert len(cases) == 9 and [c[0] for c in cases] == [c[0] for c in RC.small_cases(tier)]
        assert sum(1 for c in cases if not RC.ships_hessian(c)) == 1                    # <3, 4> is among them: these entries ship it
        for idx, case in enumerate(cases):
            cid, k, (t, y, s), delays, alpha, rho, mb, N, kappa, nu = case
            L = len(alpha)
            tt, yt, st = RC.TESTS[cid]
            assert len(tt) == len(yt) == len(st) == L and sum(len(a) for a in tt) > 0, cid
            assert mb == (L < 8), cid                                                   # 8 bands: <P, 0>
            assert (RP.sample_entry(case, idx)[0][7][2] is None) == bool(idx % 2), cid
            lc, k2, v2 = RP.loo_entry(case)
            assert np.array_equal(k2[1], 1.3 * kappa) and np.array_equal(v2[1], nu + 0.01) and np.array_equal(k2[0], kappa), cid
            masks = RP.tie_points(case)
            if L >= 3:
                RC.check_ties(t, delays)
                # the tie-swap slip acts: at least three bands hold a tied point, one band two of them at one time
                assert sum(1 for m in masks if m.any()) >= 3 and sum(int(m.sum()) for m in masks) >= 7, cid
                bad = RP.tie_swap_errorbars(case)
                assert any((b[m] != g[m]).any() for b, g, m in zip(bad, RP.NC.effective(s, kappa, nu), masks)), cid
                assert all(np.array_equal(b[~m], g[~m]) for b, g, m in zip(bad, RP.NC.effective(s, kappa, nu), masks)), cid
                ties += 1
            else:
                assert not any(m.any() for m in masks), cid
    assert ties == 4 * 6
    for tier in RC.TIERS:
        cases = RN.resample_cases(tier)
        assert len(cases) == (9 if tier in K_TIERS else 6)
        for c in cases:
            Y, counts = RN.realisations(c)
            assert RN.cells(c) == (tuple(range(RN.R)) if c[7] <= RC.SMALL else (3,)), c[0]
            for r in RN.cells(c):
                if len(c[4]) >= 3 and r in RN.SUBSET_CELLS:
                    assert all(RN.subset_condition(c[2][0], c[3], counts, r)), (c[0], r)
                    seen += 1
    assert seen == 2 * 6 * 4 + 18


@pytest.mark.parametrize("tier", K_TIERS)
def test_noise_predict_heldout_postb_loo_and_draws(pool, tier):
    cases = RP.small(tier)
    pred = list(pool.map(RP.predict_job, cases))
    loo = list(pool.map(RP.loo_job, cases))
    draw = list(pool.map(RP.sample_job, [(c, i) for i, c in enumerate(cases)]))
    worst = {w: RC.Worst("mirror noise %s, tier %s" % (w, tier)) for w in ("predict", "held-out", "postb", "loo", "draws")}
    for case, (p, pm), (lref, lm), (d, dm) in zip(cases, pred, loo, draw):
        cid, mb = case[0], case[6]
        assert set(p.bar) == {"mu", "var", "held"} | ({"pmu", "pS"} if mb else set()) and p.second == "mirror", cid
        for q, em in RP.e_mirror(p, pm).items():
            RC.add_pair(worst[RP.GROUP[q]], cid, q, PH.err(pm[q], getattr(p, q)), p.bar[q], em)
        assert set(lm) == set(LH.QUANTITIES), cid
        for q, em in RP.e_mirror(lref, lm).items():
            RC.add_pair(worst["loo"], cid, "loo " + q, PH.err(lm[q], getattr(lref, q)), lref.bar[q], em)
        assert d.second == "mirror" and np.all(np.isfinite(d.draws.astype(np.float64))) and dm.shape == d.draws.shape, cid
        RC.add_pair(worst["draws"], cid, "draws", PH.err(dm, d.draws), d.bar, float(np.max(PH.err(dm, d.draws))))
    assert worst["postb"].pairs == 2 * 6 and worst["predict"].pairs == 18
    RC.report(worst.values())                              # (in the control tier: under the existing bars as they stand)


@pytest.mark.parametrize("tier", RC.TIERS)
def test_resampled_gradient(pool, tier):
    cases = RN.resample_cases(tier)
    refs = RP.regrad_references(pool, cases)
    assert len(refs) == sum(len(RN.cells(c)) for c in cases) == (36 if tier in K_TIERS else 6)
    worst = RC.Worst("mirror resampled gradient, tier %s" % tier)
    for case in cases:
        L = len(case[4])
        for r in RN.cells(case):
            ref, ll, g = refs[(case[0], r)]
            assert g.shape == (2 * L + 1,) and np.isfinite(g).all() and ref.grad.shape == (2 * L + 1,), (case[0], r)
            e = RP.grad_error(g, ref)
            RC.add_pair(worst, case[0], "cell %d (%s)" % (r, SC.KINDS[r]), e, H.bar(ref), e)
    RC.report([worst])


# ---- one slip per family is caught at L = 8, k = 0 and k = 14; the tie-swap slip too -----------------------------------------------------
def _ratio(err, existing, e_mirror, cid):
    b, active = RC.regime_bar(existing, e_mirror, cid)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.asarray(err, np.float64) / b)), active


def test_slips_are_caught_at_eight_bands_and_small_lags(pool):
    rows = []
    picked = [(i, c) for t in ("k0", "k14") for i, c in enumerate(RP.small(t)) if len(c[4]) == 8]
    assert len(picked) == 6 and all(not c[6] for _, c in picked)
    # predictions and held-out scores: the mirror's slips and the tie swap, the latter a family of its own in the table
    pred = list(pool.map(RP.predict_job, [c for _, c in picked]))
    jobs = [(c, slip) for _, c in picked for slip in RP.PREDICT_SLIPS]
    bad = list(pool.map(RP.predict_slip_job, jobs))
    for (case, slip), got in zip(jobs, bad):
        ref, good = pred[[c[0] for _, c in picked].index(case[0])]
        em = RP.e_mirror(ref, good)
        ratios = {q: _ratio(PH.err(v, getattr(ref, q)), ref.bar[q], em[q], case[0]) for q, v in got.items()}
        if slip == "tie_swap":                         # the predictions and the held-out score each have to catch it
            rows.append(("tie swap, predict", slip, case[0], *max(ratios["mu"], ratios["var"], key=lambda x: x[0])))
            rows.append(("tie swap, held-out", slip, case[0], *ratios["held"]))
        else:
            rows.append(("predictions", slip, case[0], *max(ratios.values(), key=lambda x: x[0])))
    # leave-one-out: the variance and the density it moves
    loo = list(pool.map(RP.loo_job, [c for _, c in picked]))
    for (_, case), (ref, good), got in zip(picked, loo, pool.map(RP.loo_slip_job, [(c, "loo_var_raw") for _, c in picked])):
        em = RP.e_mirror(ref, good)
        best = max((_ratio(PH.err(got[q], getattr(ref, q)), ref.bar[q], em[q], case[0]) for q in ("var", "lp")), key=lambda x: x[0])
        rows.append(("leave-one-out", "loo_var_raw", case[0], best[0], best[1]))
    # draws; draw_test_noise_raw where the case has test noise
    draw = list(pool.map(RP.sample_job, [(c, i) for i, c in picked]))
    jobs = [(c, i, slip) for i, c in picked for slip in NS.SLIPS if not (slip == "draw_test_noise_raw" and i % 2)]
    for (case, i, slip), got in zip(jobs, pool.map(RP.sample_slip_job, jobs)):
        ref, good = draw[[c[0] for _, c in picked].index(case[0])]
        r, active = _ratio(PH.err(got, ref.draws), ref.bar, float(np.max(PH.err(good, ref.draws))), case[0])
        rows.append(("draws", slip, case[0], r, active))
    # the resampled gradient: the subset cells at L = 8, and handle_sigma_b (it needs marginalised offsets) at L = 4
    rp = [c for t in ("k0", "k14") for c in RC.small_cases(t) if len(c[4]) == 8]
    four = [c for t in ("k0", "k14") for c in RC.small_cases(t) if len(c[4]) == 4 and c[7] <= 120 and c[6]]
    gref = RP.regrad_references(pool, rp + four)
    jobs = [(c, r, "lag_from_merged") for c in rp for r in RN.SUBSET_CELLS] + [(c, r, "handle_sigma_b") for c in four for r in (1, 3)]
    for (case, r, slip), g in zip(jobs, pool.map(RP.regrad_slip_job, jobs)):
        ref, ll, good = gref[(case[0], r)]
        ratio, active = _ratio(RP.grad_error(g, ref), H.bar(ref), RP.grad_error(good, ref), case[0])
        rows.append(("resampled gradient" if slip == "lag_from_merged" else "resampled gradient (L = 4)", slip, "%s cell %d" % (case[0], r),
                     ratio, active))
    assert all(math.isfinite(r[3]) for r in rows)
    RC.slip_table([r for r in rows if "L = 4" not in r[0]], ("L8-b0-k0", "L8-b0-k14"))
    RC.slip_table([r for r in rows if "L = 4" in r[0]], ("L4-b1-k0", "L4-b1-k14"))
