"""The numpy mirror (gpcc_amd.markov) of the entries with a per-row noise model or a per-row data set against the extended-precision
references over tests/_markov_regime_noise_cases.py: the regime cases with a noise model, the OU twins without cross-band ties, the
resampled cells.  It shows that the references alone stay within the bars and that every condition on the cases holds: the tiers'
medians, the twins free of ties, the subset cells with a tie of three bands left, info == 0 everywhere (asserted where the jobs run).
In the control tier (k = 0) the mirror is held to each family's existing bar as it stands; in the other tiers the bar is
max(existing, 16 e_mirror), trivial for the mirror itself, and what is printed per pair (-s) is how far the existing bar is exceeded.
One injected slip per family has to miss its bar by a factor of two at L = 8, k = 14."""
import math
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _grad_highprec as H
import _markov_noise_cases as NC
import _markov_noise_hess_full_cases as NF
import _markov_regime_cases as RC
import _markov_regime_noise_cases as RN
import _markov_resample_cases as SC

pytestmark = pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)

K_TIERS = RC.TIERS[:4]
RHO_TIERS = RC.TIERS[4:]


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


def test_tiers_noise_models_twins_and_subset_cells():
    for name, m in RC.check_tiers().items():
        print("tier %-10s median lambda x lag %.3g (decade %g .. %g), %d cases" % (name, m, *RC.DECADE[name], len(RC.tier(name))))
    cases = RN.cases()
    assert [c[0] for c in cases] == [c[0] for c in RC.cases()]
    for idx, c in enumerate(cases):
        kappa, nu = c[8], c[9]
        L = len(c[4])
        assert kappa.shape == nu.shape == (L,) and (kappa >= 0).all() and (kappa <= 2).all() and (nu >= 0).all() and (nu <= 0.05).all()
        assert (idx % 2 == 0) or (kappa[0] == 0.0 and nu[0] == 0.01)
        assert (idx % 3 != 2) or (kappa[-1] == 1.0 and nu[-1] == 0.0)
    twins = RN.twins()
    assert len(twins) == 12 and {RC.TIER[c[0]] for c in twins} == set(K_TIERS)
    for c in twins:
        own = [b for b in (np.unique(np.asarray(a), return_counts=True)[1] for a in c[2][0]) if (b > 1).any()]
        assert not RC.shared_times(c[2][0], c[3]) and not RN.tied(c) and own, c[0]              # ties inside a band stay
    seen = 0
    for tier in RC.TIERS:
        for c in RN.resample_cases(tier):
            Y, counts = RN.realisations(c)
            L = len(c[4])
            for r in RN.cells(c):
                red = RN.reduced_case(c, r)
                assert all(len(a) >= 2 for a in red[2][0]) and (r in RN.SUBSET_CELLS) == (red[7] < c[7]), (c[0], r)
                if L >= 3 and r in RN.SUBSET_CELLS:
                    assert all(RN.subset_condition(c[2][0], c[3], counts, r)), (c[0], r)
                    seen += 1
    assert seen == 2 * 6 * 4 + 18                       # L = 4 and 8, three kernels, four k tiers, two cells; the 18 N = 370 cases
    for key, seed in sorted(RN._seed.items()):
        print("realisations of the shape N = %d, L = %d: seed %d" % (*key, seed))


@pytest.mark.parametrize("tier", RC.TIERS)
def test_noise_value_and_gradient(oracle, pool, tier):
    cases = RN.cases(tier)
    refs = RN.grad_references(pool, cases)
    worst = {q: RC.Worst("mirror noise %s, tier %s" % (q, tier)) for q in ("value", "grad", "noise")}
    for case in cases:
        b = RN.GradBars(oracle, case, refs[case[0]])
        b.add(worst, b.mirror_ll, b.mirror_grad)
    RC.report(worst.values())                            # (in the control tier: under the existing bars as they stand)


@pytest.mark.parametrize("tier", K_TIERS)
def test_noise_hessians_and_twins(pool, tier):
    """The mirror's full noise Hessian per block on the N <= 120 cases that ship and on the tier's three twins; OU rows with a
    cross-band tie: NaN in the tau entries and only there; a twin: every entry finite.  The twins' plain Hessian and Fisher matrix
    (RC.hess_job) per block, the tau blocks included.  At L = 8 the 28 off-diagonal (tau, tau) reference entries are pairwise distinct by
    more than their bar."""
    cases = [c for c in RN.cases(tier, small=True) if RN.ships_hessian(c)]
    twins = RN.twins(tier)
    assert len(cases) == 8 and len(twins) == 3
    refs = RN.hess_references(pool, cases + twins)
    plain = RC.hess_references(pool, [c[:8] for c in twins])
    worst = {w: RC.Worst("mirror %s, tier %s" % (w, tier)) for w in ("noise Hessian", "twin noise Hessian", "twin plain Hessian", "twin Fisher")}
    for case in cases + twins:
        cid, L = case[0], len(case[4])
        ref, mh = refs[cid]
        twin = cid.endswith("-twin")
        tau = NF.tau_mask(L)
        assert np.array_equal(np.isnan(mh), tau if RN.tied(case) else np.zeros_like(tau)) and RN.tied(case) == (case[1] == "OU" and not twin), cid
        for b, e, existing, em in RN.hess_pairs(ref, case, mh, mh, NF.BLOCKS):
            RC.add_pair(worst["twin noise Hessian" if twin else "noise Hessian"], cid, b, e, existing, em)
        if twin:
            pref, hyper_bars, ph, pf = plain[cid]
            assert not pref.ties and np.isfinite(ph).all() and np.isfinite(pf).all(), cid
            pairs = {}
            for which, got in (("H", ph), ("F", pf)):
                for q, e, existing, em in RC.hess_pairs(pref, hyper_bars, case[:8], which, got, got):
                    pairs[q] = RC.regime_bar(existing, em, cid)[0]
                    RC.add_pair(worst["twin plain Hessian" if which == "H" else "twin Fisher"], cid, q, e, existing, em)
            assert {"H at", "H rt", "H tt", "F at", "F rt", "F tt"} <= set(pairs), cid
            if L == 8:
                tt = dict((b, RC.regime_bar(ex, em, cid)[0]) for b, _, ex, em in RN.hess_pairs(ref, case, mh, mh, ("tt",)))["tt"]
                for name, gap in (("noise", RN.tau_pairs_distinct(ref.H, L, tt)), ("plain", RN.tau_pairs_distinct(pref.H, L, pairs["H tt"]))):
                    print("%s: the 28 off-diagonal (tau, tau) entries of the %s reference differ by at least %.3g (bar %.3g)" % (cid, name, *gap))
                    assert gap[0] > gap[1], (cid, name, gap)
    RC.report(worst.values())


@pytest.mark.parametrize("tier", RC.TIERS)
def test_resampled_cells(oracle, pool, tier):
    cases = RN.resample_cases(tier)
    assert len(cases) == (9 if tier in K_TIERS else 6)
    refs = RN.cell_references(pool, cases)
    worst = {w: RC.Worst("mirror %s, tier %s" % (w, tier)) for w in ("resampled", "realisations")}
    for case in cases:
        for r in RN.cells(case):
            ref, bar, ll, multi = refs[(case[0], r)]
            RC.add_pair(worst["resampled"], case[0], "cell %d (%s)" % (r, SC.KINDS[r]), RN.rel(ll, ref), bar, RN.rel(ll, ref))
            assert (multi is not None) == RN.same_model(case, r)
            if multi is not None:
                RC.add_pair(worst["realisations"], case[0], "cell %d (%s)" % (r, SC.KINDS[r]), RN.rel(multi, ref), bar, RN.rel(multi, ref))
    RC.report(w for w in worst.values() if w.pairs)


# ---- one slip per family is caught on the regime cases, at L = 8 and k = 14 -----------------------------------------------------------
_table = RC.slip_table


def test_slips_are_caught_at_eight_bands_and_small_lags(oracle, pool):
    rows = []
    # the noise gradient: every L = 8 case of k = 0 and k = 14
    picked = [c for t in ("k0", "k14") for c in RN.cases(t, small=True) if len(c[4]) == 8]
    assert len(picked) == 6
    refs = RN.grad_references(pool, picked)
    bad = list(pool.map(RN.grad_slip_job, [(c, s) for c in picked for s in NC.SLIPS]))
    for i, case in enumerate(picked):
        b = RN.GradBars(oracle, case, refs[case[0]])
        for j, slip in enumerate(NC.SLIPS):
            e = b.errors(*bad[i * len(NC.SLIPS) + j])
            bars = {q: RC.regime_bar(b.existing[q], b.e_mirror[q], case[0]) for q in e}
            q = max(e, key=lambda q: e[q] / bars[q][0])
            rows.append(("noise gradient", slip, case[0], e[q] / float(bars[q][0]), bars[q][1]))
    # the full noise Hessian: the Matern-3/2 case and the OU twin at L = 8 (the OU case itself is NaN in every block the slips touch)
    hp = [c for t in ("k0", "k14") for c in RN.cases(t, "matern32", True) + RN.twins(t) if len(c[4]) == 8]
    assert len(hp) == 4
    hrefs = RN.hess_references(pool, hp)
    jobs = [(c, slip, NF.pairs_of(8, blocks)) for c in hp for slip, blocks in NF.SLIPS.items()]
    for (case, slip, _), out in zip(jobs, pool.map(NF.slip_job, jobs)):
        ref, mh = hrefs[case[0]]
        assert out[3] == 0
        got = np.where(np.isnan(out[2]), ref.H, out[2])                            # (the pairs that were not walked)
        best = max(((e / float(RC.regime_bar(ex, em, case[0])[0]), RC.regime_bar(ex, em, case[0])[1])
                    for b, e, ex, em in RN.hess_pairs(ref, case, got, mh, NF.SLIPS[slip])), key=lambda x: x[0])
        rows.append(("noise Hessian", slip, case[0], best[0], best[1]))
    # the per-row data sets: the subset cells of the L = 8 cases
    rp = [c for t in ("k0", "k14") for c in RC.small_cases(t) if len(c[4]) == 8]
    cref = RN.cell_references(pool, rp)
    jobs = [(c, r, slip) for c in rp for r in RN.SUBSET_CELLS for slip in RN.RESAMPLE_SLIPS]
    for (case, r, slip), ll in zip(jobs, pool.map(RN.resample_slip_job, jobs)):
        ref, bar, good, _ = cref[(case[0], r)]
        b, active = RC.regime_bar(bar, RN.rel(good, ref), case[0])
        rows.append(("resampled", slip, "%s cell %d" % (case[0], r), RN.rel(ll, ref) / float(b), active))
    assert all(math.isfinite(r[3]) for r in rows)
    _table(rows, ("L8-b0-k0", "L8-b0-k14"))
