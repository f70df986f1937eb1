"""The prediction family on the device against the extended-precision reference (tests/_predict_highprec.py), under its bar
16 max(e_witness, e_second, n 2^-53 terms) -- measured on the CPU, nothing of it from the device, no cond term and no 1e-10 floor
(tests/test_predict_highprec_cpu.py shows what it rejects):

  the 72 cases of _markov_predict_cases.cpu_cases()  (N = 110, L = 1 .. 3, both b-modes, rho in {0.1, 3, 20, 300}; ties, "before" and plain
      layouts; repeated and unsorted test times; bands without test points)
      dense entries        predict_batch, heldout_loglik_batch, posterior_offsets (marginalised b); and again with rbf on the L = 2 cases
      linear-time entries  predict_markov_batch, heldout_loglik_markov_batch, posterior_offsets_markov_batch (marginalised b)
  tile and path edges of the dense entries: test_gpu_predict_batch.GEOMETRY and test_gpu_heldout.GEOMETRY at N in {2, 127, 128, 129, 385}
      (test blocks of 1, 127, 128, 129 and 300 points; 8 x 16 with bands without test points; 385 the first size past the single-launch
      family), OU and matern52, both b-modes, one row each.  (N = 1024 and beyond stay with their present references: a longdouble
      factorisation of that size does not fit a test of a few seconds.)
  one mutation check per family on the device's own output: var - 1e-8 must miss the variance bar, and the first test point's mean under
      the neighbouring band's mean must miss the mean bar.

References are cached per case (_predict_highprec.case_reference).  Every group prints its worst error / bar in a line that starts
with "highprec"; profiles/predict/highprec_parity.log keeps them."""
import numpy as np
import pytest

import _grad_witness as W
import _markov_cases as MC
import _markov_predict_cases as PC
import _predict_highprec as PH
import gpcc_amd
import test_gpu_heldout as TH
import test_gpu_predict_batch as TP

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not PH.EXTENDED, reason=PH.SKIP_REASON)]

KERN = {"OU": gpcc_amd.OU, "rbf": gpcc_amd.rbf, "matern32": gpcc_amd.matern32, "matern52": gpcc_amd.matern52}
CASES = PC.cpu_cases()
EDGES = (2, 127, 128, 129, 385)
EDGE_KERNELS = ("OU", "matern52")


def _dense(case, kernel=None):
    """{quantity: the dense entries' value} of a case."""
    cid, k, data, delays, alpha, rho, mb, tests = case
    with gpcc_amd.Objective(*data, KERN[kernel or k], marginalise_b=mb) as obj:
        mu, var, _, info, _, _ = obj.predict_batch(delays[None, :], alpha[None, :], [rho], tests[0])
        held, _, infoh, _, refit = obj.heldout_loglik_batch(delays[None, :], alpha[None, :], [rho], *tests)
        assert info[0] == 0 and infoh[0] == 0 and not refit.any(), cid
        out = {"mu": mu[0], "var": var[0], "held": held[0]}
        if mb:
            out["pmu"], out["pS"] = obj.posterior_offsets(delays, alpha, rho)
    return out


def _markov(case):
    """{quantity: the linear-time entries' value} of a case."""
    cid, k, data, delays, alpha, rho, mb, tests = case
    with gpcc_amd.Objective(*data, KERN[k], marginalise_b=mb) as obj:
        mu, var, _, info, _, _ = obj.predict_markov_batch(delays[None, :], alpha[None, :], [rho], tests[0])
        held, _, infoh, _ = obj.heldout_loglik_markov_batch(delays[None, :], alpha[None, :], [rho], *tests)
        assert info[0] == 0 and infoh[0] == 0, cid
        out = {"mu": mu[0], "var": var[0], "held": held[0]}
        if mb:
            pmu, pS, _, infop = obj.posterior_offsets_markov_batch(delays[None, :], alpha[None, :], [rho])
            assert infop[0] == 0, cid
            out["pmu"], out["pS"] = pmu[0], pS[0]
    return out


def _compare(oracle, family, entries, cases, kernel=None):
    worst = {}
    for case in cases:
        ref = PH.case_reference(oracle, case, kernel)
        got = entries(case) if kernel is None else entries(case, kernel)
        assert set(got) == set(ref.bar), case[0]
        for what, value in got.items():
            r = ref.ratio(what, value)
            print("%s %s %s: error / bar %.3g" % (family, what, case[0] + ("" if kernel is None else " as " + kernel), r))
            group = "highprec %s %s %s L = %d" % (family, what, kernel or case[1], len(case[2][0]))
            worst.setdefault(what, PH.Worst(group)).add(r, case[0])
    PH.report(worst.values())                            # (every figure is printed before the first assertion)


def _select(kernel, L):
    return [c for c in CASES if c[1] == kernel and len(c[2][0]) == L]


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_cases_dense(oracle, kernel, L):
    cases = _select(kernel, L)
    assert len(cases) == 2 * len(MC.RHOS)
    _compare(oracle, "dense", _dense, cases)


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("kernel", MC.KERNELS)
def test_cases_markov(oracle, kernel, L):
    cases = _select(kernel, L)
    assert len(cases) == 2 * len(MC.RHOS)
    _compare(oracle, "linear-time", _markov, cases)


@pytest.mark.parametrize("data_of", MC.KERNELS)
def test_cases_dense_rbf(oracle, data_of):
    """The dense entries with the rbf kernel on the L = 2 cases (those of each Markov kernel have their own light curves)."""
    _compare(oracle, "dense", _dense, _select(data_of, 2), kernel="rbf")


def _edge_rows(module, N):
    """[(kernel, marginalise_b, data, delays, alpha, rho, Nt, seed of the test set)]: the first row of the module's own parity test."""
    Nl, Nt = module.GEOMETRY[N]
    data = W.ragged_data(Nl, seed=N)
    out = []
    for ki, name in enumerate(module.KERNELS):
        for mb in (True, False):
            if name in EDGE_KERNELS:
                delays, alpha, rho = W.random_params(len(Nl), 2, seed=N + 10 * ki + mb)
                out.append((name, mb, data, delays[0], alpha[0], rho[0], Nt, N + ki))
    assert len(out) == 4
    return out


@pytest.mark.parametrize("N", EDGES)
def test_tile_edges_predict(oracle, N):
    worst = {w: PH.Worst("highprec dense %s edges N = %d, T = %d" % (w, N, sum(TP.GEOMETRY[N][1]))) for w in ("mu", "var")}
    for name, mb, data, delays, alpha, rho, Nt, seed in _edge_rows(TP, N):
        ttest = TP._tests(data[0], delays, Nt, seed=seed)
        ref = PH.reference(oracle, name, data, delays, alpha, rho, mb, (ttest, None, None), want=("predict",))
        with gpcc_amd.Objective(*data, KERN[name], marginalise_b=mb) as obj:
            mu, var, _, info, _, _ = obj.predict_batch(delays[None, :], alpha[None, :], [rho], ttest)
        assert info[0] == 0
        ratios = {"mu": ref.ratio("mu", mu[0]), "var": ref.ratio("var", var[0])}
        print("dense edges N = %d %s b%d (%s): error / bar mu %.3g, var %.3g" % (N, name, mb, ref.second, ratios["mu"], ratios["var"]))
        for w in worst:
            worst[w].add(ratios[w], (name, mb))
    PH.report(worst.values())


@pytest.mark.parametrize("N", EDGES)
def test_tile_edges_heldout(oracle, N):
    worst = PH.Worst("highprec dense held-out edges N = %d, T = %d" % (N, sum(TH.GEOMETRY[N][1])))
    for name, mb, data, delays, alpha, rho, Nt, seed in _edge_rows(TH, N):
        tests = TH._testset(data[0], data[1], delays, Nt, seed=seed)
        ref = PH.reference(oracle, name, data, delays, alpha, rho, mb, tests, want=("heldout",))
        with gpcc_amd.Objective(*data, KERN[name], marginalise_b=mb) as obj:
            held, _, info, _, refit = obj.heldout_loglik_batch(delays[None, :], alpha[None, :], [rho], *tests)
        assert info[0] == 0 and not refit.any()
        r = ref.ratio("held", held[0])
        print("dense edges N = %d %s b%d (%s): error / bar held-out %.3g" % (N, name, mb, ref.second, r))
        worst.add(r, (name, mb))
    PH.report([worst])


@pytest.mark.parametrize("family,entries", [("dense", _dense), ("linear-time", _markov)])
def test_mutations_miss_the_bar(oracle, family, entries):
    """On the device's own output at the Matern-3/2 cases with two bands (both b-modes, every rho): the variance without JITTER and the
    first test point's mean under the other band's mean must miss their bars; the output itself passes them."""
    low = {"var": np.inf, "mu": np.inf}
    for case in _select("matern32", 2):
        ref = PH.case_reference(oracle, case)
        got = entries(case)
        assert ref.ratio("var", got["var"]) <= 1.0 and ref.ratio("mu", got["mu"]) <= 1.0, case[0]
        b = int(ref.bs[0])
        mu = got["mu"].copy()
        mu[0] += ref.mean[(b + 1) % 2] - ref.mean[b]
        r = {"var": ref.ratio("var", got["var"] - 1e-8), "mu": ref.ratio("mu", mu)}
        for what in r:
            low[what] = min(low[what], r[what])
            assert r[what] > 1.0, (case[0], what, r[what])
    print("highprec %s mutations: smallest error / bar of var - 1e-8 %.3g, of the first mean under the other band's mean %.3g"
          % (family, low["var"], low["mu"]))
