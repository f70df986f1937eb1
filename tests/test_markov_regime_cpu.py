"""The numpy mirror (gpcc_amd.markov) against the extended-precision references over tests/_markov_regime_cases.py: lambda x lag down to
5e-8 by compressing the times, rho up to 3e5, and 4 and 8 bands with three or more bands tied on one shifted time.  Per case and quantity
the mirror's error, the family's existing bar, their ratio and e_mirror are printed (-s); in the control tier (k = 0) every existing
bar holds as it stands; in the other tiers the bar is max(existing, 16 e_mirror) (the module's docstring), and the mirror's injected
slips are rejected under exactly that bar in every tier where their effect does not vanish analytically."""
import math
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import _grad_highprec as H
import _markov_grad_cases as GC
import _markov_hess_full_cases as FC
import _markov_regime_cases as RC
import _predict_highprec as PH
from gpcc_amd import markov

pytestmark = pytest.mark.skipif(not H.EXTENDED, reason=H.SKIP_REASON)

VALUE_SLIPS = ("order", "no_q", "var_n", "no_offset")
# slip -> ({tier where it need not be rejected}, why).  Nothing else is exempt.
EXEMPT = {"grad no_dpinf": (("rho300000",), "dPinf/drho's entries in the observed row are -2 lambda^2 / (3 rho) (Matern-5/2; none for OU and "
                          "Matern-3/2): they fall as rho^-3 and are below the bar at rho = 3e5 (error / bar 1e5, 65, 0.25 at rho = 3e3, 3e4, 3e5)")}


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


@pytest.fixture(scope="module")
def bars(oracle, pool):
    """{case id: RC.Bars}: every case's extended reference (info == 0 asserted there), the mirror's value and gradient, the bars."""
    cases = RC.cases()
    return {c[0]: RC.Bars(oracle, c, job) for c, job in zip(cases, pool.map(RC.value_grad_job, cases))}


def test_tiers_and_ties():
    """Every tier's median lambda x lag lies in its decade; the multi-band ties are there (asserted while the cases are built)."""
    for name, m in RC.check_tiers().items():
        print("tier %-10s median lambda x lag %.3g (decade %g .. %g), %d cases" % (name, m, *RC.DECADE[name], len(RC.tier(name))))
    for c in RC.cases():
        for a in list(c[2][0]) + [c[3]]:
            assert np.array_equal(np.asarray(a) * 2.0 ** RC.K_OF[c[0]] * 1024.0, np.round(np.asarray(a) * 2.0 ** RC.K_OF[c[0]] * 1024.0)), c[0]


@pytest.mark.parametrize("tier", RC.TIERS)
def test_value_and_gradient(bars, tier):
    """The mirror's value and gradient of every case against _grad_highprec.evaluate."""
    wv, wg = RC.Worst("mirror value, tier %s" % tier), RC.Worst("mirror gradient, tier %s" % tier)
    for case in RC.tier(tier):
        cid, k, data, delays, alpha, rho, mb, N = case
        b = bars[cid]
        assert b.mirror_ll == markov.loglik(k, *data, delays, alpha, rho, mb)[0], cid
        ev, eg = b.e_mirror_value, b.e_mirror_grad
        print("%-30s value: error %.3g existing bar %.3g ratio %.3g e_mirror %.3g | gradient: error %.3g (%.3g of max|g|) existing bar %.3g "
              "ratio %.3g e_mirror %.3g" % (cid, ev, b.value_existing, ev / b.value_existing, ev, eg, eg / np.max(np.abs(b.ref.grad)),
                                           b.grad_existing, eg / b.grad_existing, eg))
        if tier == RC.CONTROL:       # every existing bar as it stands, no new term
            assert b.value == b.value_existing and b.grad == b.grad_existing and not b.value_active and not b.grad_active
            assert ev <= b.value_existing and H.ratio(b.mirror_grad, b.ref) <= 1.0, cid
        wv.add(b.value_ratio(b.mirror_ll), cid, b.value_active)
        wg.add(b.grad_ratio(b.mirror_grad), cid, b.grad_active)
    RC.report([wv, wg])


@pytest.mark.parametrize("tier", RC.TIERS)
def test_slips_are_rejected_in_every_tier(bars, tier):
    """Each slip of the mirror's value and gradient is rejected by at least one case of the tier under the bar that the tier's device
    test uses; per slip and tier the number of rejecting cases and the closest miss among them are printed.  EXEMPT lists the slips
    whose effect vanishes analytically in a tier, each with its reason."""
    cases = [c for c in RC.tier(tier) if c[7] <= (RC.SMALL if tier.startswith("k") else 370)]      # (the smaller shapes: the mirror's passes are slow)
    assert len(cases) == (9 if tier.startswith("k") else 6)
    seen = {}
    for case in cases:
        cid, k, data, delays, alpha, rho, mb, N = case
        b = bars[cid]
        for slip in VALUE_SLIPS:
            if slip in ("var_n", "no_offset") and not mb:
                continue                      # (both touch the marginalised offsets alone)
            bad, _ = markov.loglik(k, *data, delays, alpha, rho, mb, _slip=slip)
            seen.setdefault(slip, []).append((b.value_ratio(bad) if math.isfinite(bad) else math.inf, cid))
        for slip in GC.SLIPS:
            if slip == "one_sided" and k != "OU":
                continue                      # (the mirror applies it to OU alone: the Matern kernels are C^1 and have one tie order)
            g = markov.loglik_grad(k, *data, delays, alpha, rho, mb, _slip=slip)[1]
            seen.setdefault("grad " + slip, []).append((b.grad_ratio(g), cid))
    assert set(seen) == set(VALUE_SLIPS) | {"grad " + s for s in GC.SLIPS}
    for slip, (tiers, why) in EXEMPT.items():
        assert why and slip in seen and set(tiers) <= set(RC.TIERS) - {RC.CONTROL}
    missed = []
    for slip, ratios in sorted(seen.items()):
        rejecting = [x for x in ratios if x[0] > 1.0]
        exempt = tier in EXEMPT.get(slip, ((), ""))[0]
        close = min(rejecting) if rejecting else max(ratios)
        print("tier %-10s slip %-18s rejected by %2d of %2d cases; closest miss: error / bar %.3g (%s); largest %.3g%s"
              % (tier, slip, len(rejecting), len(ratios), close[0], close[1], max(ratios)[0], "  EXEMPT: " + EXEMPT[slip][1] if exempt else ""))
        if not rejecting and not exempt:
            missed.append((tier, slip, max(ratios)))
    assert not missed, missed


# ---- the other families at the N <= 120 shapes ------------------------------------------------------------------------------------
def _control(tier, r, what):
    """In the control tier add_pair's bar is the existing one: the mirror passes it as it stands."""
    if tier == RC.CONTROL:
        assert r <= 1.0, what


@pytest.mark.parametrize("tier", RC.TIERS[:4])
def test_hessians_and_fisher(pool, tier):
    """The mirror's hyper block, full Hessian and Fisher matrix per block (_hess_highprec, the bars of _markov_hess_cases /
    _markov_hess_full_cases / _markov_fisher_cases); OU rows: NaN in the tau entries and only there (every case has cross-band ties)."""
    cases = [c for c in RC.small_cases(tier) if RC.ships_hessian(c)]
    assert len(cases) == 8
    refs = RC.hess_references(pool, cases)
    worst = {w: RC.Worst("mirror %s, tier %s" % (n, tier)) for w, n in (("hyper", "Hessian block"), ("H", "full Hessian"), ("F", "Fisher"))}
    for case in cases:
        cid, k, data, delays, alpha, rho, mb, N = case
        ref, hyper_bars, mh, mf = refs[cid]
        L = len(alpha)
        assert ref.ties, cid
        tau = FC.tau_mask(L)
        for m in (mh, mf):
            assert np.array_equal(np.isnan(m), tau if k == "OU" else np.zeros_like(tau)), cid
        for which, got in (("hyper", mh[:L + 1, :L + 1]), ("H", mh), ("F", mf)):
            for q, e, existing, em in RC.hess_pairs(ref, hyper_bars, case, which, got, got):
                _control(tier, RC.add_pair(worst[which], cid, q, e, existing, em), (cid, q))
    cid, k, data, delays, alpha, rho, mb, N = cases[0]
    assert np.array_equal(markov.loglik_hess_hyper(k, *data, delays, alpha, rho, mb)[2], refs[cid][2][:len(alpha) + 1, :len(alpha) + 1])
    RC.report(worst.values())


@pytest.mark.parametrize("tier", RC.TIERS[:4])
def test_predict_heldout_postb_loo_and_draws(oracle, pool, tier):
    """The mirror's predictions, held-out value, postb (_predict_highprec: its bar holds the mirror's error as e_second already),
    leave-one-out quantities (_loo_highprec's bar times the filter's factor) and one draw (_sample_highprec)."""
    cases = RC.small_cases(tier)
    assert len(cases) == 9
    pred = list(pool.map(RC.predict_job, cases))
    loo = list(pool.map(RC.loo_job, cases))
    draw = list(pool.map(RC.sample_job, [(c, 900 + i, 0) for i, c in enumerate(cases)]))
    worst = {w: RC.Worst("mirror %s, tier %s" % (w, tier)) for w in ("predict", "held-out", "postb", "loo", "draws")}
    group = {"mu": "predict", "var": "predict", "held": "held-out", "pmu": "postb", "pS": "postb"}
    for case, p, (lref, lmir), d in zip(cases, pred, loo, draw):
        cid, mb = case[0], case[6]
        assert set(p.bar) == {"mu", "var", "held"} | ({"pmu", "pS"} if mb else set()) and p.second == "mirror", cid
        for q in p.bar:
            # (the mirror's own error: what e_second measured)
            _control(tier, RC.add_pair(worst[group[q]], cid, q, p.e_second[q], p.bar[q], p.e_second[q]), (cid, q))
        for q in ("mu", "var", "lp", "loo", "mix_lp", "mix_loo"):
            e = PH.err(lmir[q], getattr(lref, q))
            _control(tier, RC.add_pair(worst["loo"], cid, "loo " + q, e, lref.bar[q] * lref.scale, float(np.max(e))), (cid, q))
        assert d.second == "mirror"
        _control(tier, RC.add_pair(worst["draws"], cid, "draw", d.e_second, d.base, d.e_second), cid)
    RC.report(worst.values())
