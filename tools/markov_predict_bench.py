#!/usr/bin/env python3
"""Rates of the linear-time post-fit entries (gpcc_predict_markov_batch, gpcc_heldout_loglik_markov_batch) against their dense
namesakes (gpcc_predict_batch, gpcc_heldout_loglik_batch) on the same inputs in the same run, the two paths alternating; prints one
JSON line per measurement.

  python tools/markov_predict_bench.py [--log profiles/markov/predict_bench.log] [--quick]
      predictions   N = 4096, L = 2, 64 delays, T = 2 x 512; README size N = 110, 101 delays, T = 2 x 201; N = 16384, Matern-5/2, 64
                    delays (no dense fp64 counterpart: alone)
      held-out      the 5-fold split N = 4096 -> 3276 / 820, 64 delays; README size, one fold
      performcv_grid, 5 folds, 101 delays, iterations = 1000, both solvers
  python tools/markov_predict_bench.py --profile-run     the N = 4096 prediction call after a warm-up, for rocprofv3 --kernel-trace --stats

Timing: a warm-up of every timed shape, then `rounds` rounds of (a window of linear-time calls, a window of dense calls), each window at
least `window` seconds of blocking calls; the median over the rounds of the windows' mean time per call."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LINES = []


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    LINES.append(line)


def sweep(Nl, M, seed=1, **kw):
    from gpcc_amd import synthetic
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=seed, **kw)
    alpha, rho = synthetic.default_hyperparameters(y)
    grid = np.linspace(0.0, 20.0, M)
    return (t, y, s), np.stack([np.zeros(M), grid], 1), np.tile(alpha, (M, 1)), np.full(M, rho)


def window(fn, seconds, max_calls):
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds or n >= max_calls:
            return dt / n


def alternate(fast, slow, rounds, seconds, max_slow=50):
    fast()
    if slow:
        slow()
    tf, ts = [], []
    for _ in range(rounds):
        tf.append(window(fast, seconds, 100000))
        if slow:
            ts.append(window(slow, seconds, max_slow))
    return float(np.median(tf)), (float(np.median(ts)) if slow else None), tf, ts


def predictions(name, Nl, M, T, kernel, rounds, seconds, dense=True, **kw):
    import gpcc_amd
    data, delays, alpha, rho = sweep(Nl, M, **kw)
    hi = max(np.max(a) for a in data[0])
    tt = [np.linspace(-0.02 * hi, 1.02 * hi, T)] * len(Nl)
    w = np.ones(M)
    with gpcc_amd.Objective(*data, kernel) as obj:
        fast = lambda: obj.predict_markov_batch(delays, alpha, rho, tt, weights=w)
        slow = (lambda: obj.predict_batch(delays, alpha, rho, tt, weights=w)) if dense else None
        tf, ts, af, as_ = alternate(fast, slow, rounds, seconds)
        rf = fast()
        diff = None
        if dense:
            rs = slow()
            diff = [float(np.max(np.abs(rf[0] - rs[0]))), float(np.max(np.abs(rf[1] - rs[1])))]
    emit(what="predictions: " + name, N=int(sum(Nl)), M=M, T=T * len(Nl), kernel=kernel.name, markov_rows_per_s=M / tf,
         dense_rows_per_s=(M / ts if dense else None), ratio=(ts / tf if dense else None), markov_ms_per_call=1e3 * tf,
         dense_ms_per_call=(1e3 * ts if dense else None), markov_ms_rounds=[1e3 * x for x in af], dense_ms_rounds=[1e3 * x for x in as_],
         max_abs_diff_mu_var=diff, failed=int((rf[3] != 0).sum()))


def heldout(name, Nl, M, kernel, rounds, seconds, **kw):
    import gpcc_amd
    from gpcc_amd import fit
    data, delays, alpha, rho = sweep(Nl, M, **kw)
    folds = fit.cvindices(Nl, 5, 1)
    (ttr, ytr, str_), (tte, yte, ste) = fit._split(*data, folds, 0)
    w = np.ones(M)
    with gpcc_amd.Objective(ttr, ytr, str_, kernel) as obj:
        fast = lambda: obj.heldout_loglik_markov_batch(delays, alpha, rho, tte, yte, ste, weights=w)
        slow = lambda: obj.heldout_loglik_batch(delays, alpha, rho, tte, yte, ste, weights=w)
        tf, ts, af, as_ = alternate(fast, slow, rounds, seconds)
        rf, rs = fast(), slow()
    emit(what="held-out: " + name, N_train=int(sum(len(a) for a in ttr)), T=int(sum(len(a) for a in tte)), M=M, kernel=kernel.name,
         markov_rows_per_s=M / tf, dense_rows_per_s=M / ts, ratio=ts / tf, markov_ms_per_call=1e3 * tf, dense_ms_per_call=1e3 * ts,
         markov_ms_rounds=[1e3 * x for x in af], dense_ms_rounds=[1e3 * x for x in as_],
         max_rel_diff=float(np.max(np.abs(rf[0] - rs[0]) / np.abs(rs[0]))), failed=int((rf[2] != 0).sum()))


def crossvalidation(rounds):
    import gpcc_amd
    from gpcc_amd import fit, synthetic
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    grid = np.arange(0.0, 20.01, 0.2)
    cand = np.stack([np.zeros_like(grid), grid], 1)
    run = lambda solver: fit.performcv_grid(t, y, s, candidatedelays=cand, kernel=gpcc_amd.OU, iterations=1000, solver=solver)
    out = {}
    for solver in ("markov", "dense"):
        run(solver)
    for _ in range(rounds):
        for solver in ("markov", "dense"):
            t0 = time.perf_counter()
            cv = run(solver)
            out.setdefault(solver, []).append(time.perf_counter() - t0)
            out[solver + "_mix"] = float(cv.mix.sum())
    emit(what="performcv_grid, 5 folds, 101 delays, iterations = 1000, N = 110", markov_ms=1e3 * float(np.median(out["markov"])),
         dense_ms=1e3 * float(np.median(out["dense"])), markov_ms_rounds=[1e3 * x for x in out["markov"]],
         dense_ms_rounds=[1e3 * x for x in out["dense"]], mix_sum_markov=out["markov_mix"], mix_sum_dense=out["dense_mix"])


def main():
    import gpcc_amd
    if "--profile-run" in sys.argv:
        data, delays, alpha, rho = sweep([2048, 2048], 64)
        hi = max(np.max(a) for a in data[0])
        tt = [np.linspace(-0.02 * hi, 1.02 * hi, 512)] * 2
        with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
            for _ in range(4):
                obj.predict_markov_batch(delays, alpha, rho, tt, weights=np.ones(64))
        return
    quick = "--quick" in sys.argv
    rounds, seconds = (2, 0.3) if quick else (5, 1.0)
    emit(what="build", info=gpcc_amd.build_info())
    predictions("N = 4096", [2048, 2048], 64, 512, gpcc_amd.matern32, rounds, seconds)
    predictions("README size", [60, 50], 101, 201, gpcc_amd.OU, rounds, seconds, gap_band=1, span=20.0)
    predictions("N = 16384 (no dense fp64 counterpart)", [8192, 8192], 64, 512, gpcc_amd.matern52, rounds, seconds, dense=False)
    heldout("N = 4096, one of 5 folds", [2048, 2048], 64, gpcc_amd.matern32, rounds, seconds)
    heldout("README size, one of 5 folds", [60, 50], 101, gpcc_amd.OU, rounds, seconds, gap_band=1, span=20.0)
    crossvalidation(2 if quick else 5)
    if "--log" in sys.argv:
        path = sys.argv[sys.argv.index("--log") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tools/markov_predict_bench.py: the linear-time post-fit entries against the dense ones, same inputs, same run, "
                    "alternating windows (MI355X)\n")
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
