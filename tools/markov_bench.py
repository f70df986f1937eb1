#!/usr/bin/env python3
"""Rates of gpcc_loglik_markov_batch (the linear-time log-likelihood of the OU / Matern kernels) against the dense path
(gpcc_loglik_batch) on the same inputs in the same run; prints one JSON line per measurement and a summary.

  python tools/markov_bench.py [--log profiles/markov/markov_bench.log] [--quick]
      N = 4096, Matern-3/2, L = 2, 1024 delays (the headline batch)              evaluations/s of both
      N = 110, 101 delays (the README sweep); M = 1 at N = 384 / 1024 / 4096     both
      full fit, 512 delays, iterations = 30, N = 4096                            fitted grid points/s, fit_markov 0 and 1
      N = 16384, Matern-5/2, 64 delays against the fp32 dense path               both
  python tools/markov_bench.py --profile-run     one headline batch after a warm-up, for rocprofv3 --kernel-trace --stats

Timing: a warm-up call, then the median of `reps` timed calls (host wall clock around blocking calls)."""
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


def sweep(N, M, L=2, seed=1):
    from gpcc_amd import synthetic
    Nl = [N // L + (1 if l < N % L else 0) for l in range(L)]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=seed)
    alpha, rho = synthetic.default_hyperparameters(y)
    grid = np.linspace(0.0, 20.0, M)
    return (t, y, s), np.stack([np.zeros(M), grid], 1), np.tile(alpha, (M, 1)), np.full(M, rho)


def median_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def both(name, N, M, kernel, reps_markov, reps_dense, precision="fp64"):
    import gpcc_amd
    data, delays, alpha, rho = sweep(N, M)
    with gpcc_amd.Objective(*data, kernel, precision=precision) as obj:
        tm = median_time(lambda: obj.loglik_markov_batch(delays, alpha, rho), reps_markov)
        lm, im = obj.loglik_markov_batch(delays, alpha, rho)
        td = median_time(lambda: obj.loglik_batch(delays, alpha, rho), reps_dense)
        ld, idn = obj.loglik_batch(delays, alpha, rho)
    ok = (im == 0) & (idn == 0)
    emit(what=name, N=N, M=M, kernel=kernel.name, dense_precision=precision, markov_evals_per_s=M / tm[0], dense_evals_per_s=M / td[0],
         ratio=td[0] / tm[0], markov_ms=[1e3 * x for x in tm], dense_ms=[1e3 * x for x in td], reps=[reps_markov, reps_dense],
         max_rel_diff=float(np.max(np.abs(lm[ok] - ld[ok]) / np.abs(ld[ok]))), failed=int((~ok).sum()))


def fit_rate(N, G, iterations, kernel, quick):
    import gpcc_amd
    data, delays, _, _ = sweep(N, G)
    out = {}
    with gpcc_amd.Objective(*data, kernel) as obj:
        for flag in ((1,) if quick else (1, 0)):
            obj.set_option("fit_markov", flag)
            t0 = time.perf_counter()
            ll, alpha, rho, info, its, (f_calls, rounds) = obj.grid_loglik(delays, iterations)
            dt = time.perf_counter() - t0
            out[flag] = dict(points_per_s=G / dt, seconds=dt, f_calls=f_calls, rounds=rounds, best=float(np.max(ll)),
                             argmax=int(np.argmax(ll)))
    emit(what="full fit", N=N, delays=G, iterations=iterations, kernel=kernel.name, fit_markov_1=out.get(1), fit_markov_0=out.get(0),
         ratio=(out[1]["points_per_s"] / out[0]["points_per_s"]) if 0 in out else None)


def main():
    import gpcc_amd
    if "--profile-run" in sys.argv:
        data, delays, alpha, rho = sweep(4096, 1024)
        with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
            for _ in range(4):
                obj.loglik_markov_batch(delays, alpha, rho)
        return
    quick = "--quick" in sys.argv
    emit(what="build", info=gpcc_amd.build_info())
    both("headline", 4096, 1024, gpcc_amd.matern32, 20, 1 if quick else 2)
    both("README sweep", 110, 101, gpcc_amd.matern32, 200, 200)
    for N in (384, 1024, 4096):
        both("single evaluation", N, 1, gpcc_amd.matern32, 50, 50)
    both("cfg5 size", 16384, 64, gpcc_amd.matern52, 5, 1, precision="fp32")
    fit_rate(4096, 512, 30, gpcc_amd.matern32, quick)
    if "--log" in sys.argv:
        path = sys.argv[sys.argv.index("--log") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tools/markov_bench.py: gpcc_loglik_markov_batch against gpcc_loglik_batch, same inputs, same run (MI355X)\n")
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
