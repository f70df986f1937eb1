#!/usr/bin/env python3
"""Times gpcc_loglik_grad_markov_resampled_batch (the gradient of rows with their own parameters and their own resampled data set, one
linear-time pass) against the routes beside it, same inputs, same run; prints one JSON line per measurement.  A measurement, not a
gate: every ratio is stated whatever it is, also where the new entry loses.

  python tools/markov_resample_grad_bench.py [--log profiles/markov/resample_grad_bench.log] [--quick]
      (a) README size: N = 110, OU, 101 delays, R = 1000, one gradient per (realisation, delay), flux randomisation and subset selection
      (b) N = 4096, Matern-3/2, 1024 delays x R = 8 and R = 64
      (c) N = 16384, Matern-5/2, 256 delays x R = 4
          ... each, in the same run, against gpcc_loglik_markov_resampled_batch on the same rows (what the gradient costs over the
          value), against gpcc_loglik_grad_markov_batch on the same number of rows (one data set: what the per-lane data source costs)
          and against the loop of R fresh handles it replaces (create, gpcc_loglik_grad_markov_batch, close: timed whole).  The rows are
          realisation-major; the gradient entry is also timed with the same rows in a scrambled order (lanes of a wave on different
          realisations read scattered 16-byte pairs)
      (d) the refit: fit.realisation_refits at README size, R = 100, 101 delays, warm start, optimiser "bfgs" against "neldermead" (30
          iterations each: rounds, f_calls, wall time, mean final log-likelihood), and fit.realisation_peaks on the same R from the
          BFGS refit

Timing: host wall clock around blocking calls; each measurement runs in a fresh process of its own, the entries before its loop.  The
entries: after a warm-up call of each, 5 alternating windows of `calls` calls, median window.  The loop is timed whole, `loops` times,
median.  (a) to (c) run without marginalise_b and with own means, so that every route computes the same numbers; the largest
disagreement with the loop, relative to max|g| of the row, is printed."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from markov_grad_bench import WINDOWS, alternate, sweep  # noqa: E402
from markov_resample_bench import med, reduced  # noqa: E402

LINES = []


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    LINES.append(line)


def measure(name, N, M, kernel, R, calls, loops):
    import gpcc_amd
    from gpcc_amd import markov, synthetic
    (t, y, s), delays, alpha, rho = sweep(N, M)
    Y, counts = synthetic.resample(y, s, R, seed=R)
    mean, vb = markov.resample_constants(t, Y, counts, False)
    g, r = np.tile(np.arange(M), R), np.repeat(np.arange(R), M)          # realisation-major rows
    dg, ag, rg = delays[g], alpha[g], rho[g]
    sc = np.random.default_rng(1).permutation(M * R)                     # the same rows, scrambled

    def loop():
        out = np.empty((R, M, 2 * len(t) + 1))
        for k in range(R):
            with gpcc_amd.Objective(*reduced(t, s, Y, counts, k), kernel, marginalise_b=False) as fresh:
                out[k] = fresh.loglik_grad_markov_batch(delays, alpha, rho)[1]
        return out

    with gpcc_amd.Objective(t, y, s, kernel, marginalise_b=False) as obj:
        flat, cflat = obj.realisations(Y), np.concatenate(counts, axis=1)
        kw = dict(counts=cflat, center=mean, sigma_b=vb)
        fns = [lambda: obj.loglik_grad_markov_resampled(flat, dg, ag, rg, r, **kw),
               lambda: obj.loglik_grad_markov_resampled(flat, dg[sc], ag[sc], rg[sc], r[sc], **kw),
               lambda: obj.loglik_markov_resampled(flat, dg, ag, rg, r, **kw),
               lambda: obj.loglik_grad_markov_batch(dg, ag, rg)]
        tg, tsc, tv, tp = alternate(fns, [calls] * len(fns))
        ll, grad, info = fns[0]()
        l2, g2, _ = fns[1]()
        scrambled_same = bool(np.array_equal(g2, grad[sc]) and np.array_equal(l2, ll[sc]))
    return lambda: _finish(name, N, M, kernel, R, calls, loops, loop, tg, tsc, tv, tp, grad, info, scrambled_same)


def _finish(name, N, M, kernel, R, calls, loops, loop, tg, tsc, tv, tp, grad, info, scrambled_same):
    ref = loop()
    tl = []
    for _ in range(loops):
        t0 = time.perf_counter()
        loop()
        tl.append(time.perf_counter() - t0)
    grad = grad.reshape(ref.shape)
    emit(what=name, N=N, M=M, R=R, rows=M * R, kernel=kernel.name, resampled_grad_ms=[1e3 * x for x in tg],
         resampled_grad_scrambled_ms=[1e3 * x for x in tsc], resampled_value_ms=[1e3 * x for x in tv],
         plain_grad_same_rows_ms=[1e3 * x for x in tp], loop_ms=[1e3 * x for x in sorted(tl)], grads_per_s=M * R / med(tg),
         ratio_grad_over_value=med(tg) / med(tv), ratio_grad_over_plain_grad=med(tg) / med(tp), ratio_scrambled_over_realisation_major=med(tsc) / med(tg),
         ratio_loop_over_resampled_grad=med(tl) / med(tg), calls_per_window=calls, windows=WINDOWS, loops=loops,
         scrambled_rows_bitwise_the_same=scrambled_same,
         max_diff_from_the_loop_of_max_g=float(np.max(np.abs(grad - ref) / np.max(np.abs(ref), axis=2, keepdims=True))),
         failed=int((info != 0).sum()))


def refit(R, iterations):
    import gpcc_amd
    from gpcc_amd import fit, synthetic
    (t, y, s), cand, _, _ = sweep(110, 101)
    Y, counts = synthetic.resample(y, s, R, seed=3)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        res = fit.gpcc_grid(t, y, s, kernel=gpcc_amd.OU, candidatedelays=cand, iterations=100, objective=obj, solver="markov")
        start = (res.alpha, res.rho)
        out, secs = {}, {}
        for o in ("bfgs", "neldermead"):
            fit.realisation_refits(obj, cand, [a[:2] for a in Y], [c[:2] for c in counts], iterations=2, start=start, optimiser=o)   # warm-up
            t0 = time.perf_counter()
            out[o] = fit.realisation_refits(obj, cand, Y, counts, iterations=iterations, start=start, optimiser=o)
            secs[o] = time.perf_counter() - t0
        t0 = time.perf_counter()
        pk = fit.realisation_peaks(obj, cand, Y, counts, start=out["bfgs"], iterations=iterations)
        t_peaks = time.perf_counter() - t0
    b, n = out["bfgs"], out["neldermead"]
    emit(what="refit, README size", N=110, G=101, R=R, iterations=iterations, kernel="OU", bfgs_s=secs["bfgs"], neldermead_s=secs["neldermead"],
         bfgs_rounds=int(b.rounds), bfgs_f_calls=int(b.f_calls), neldermead_rounds=int(n.rounds), neldermead_f_calls=int(n.f_calls),
         bfgs_mean_loglikel=float(b.loglikel.mean()), neldermead_mean_loglikel=float(n.loglikel.mean()),
         bfgs_cells_converged=int(b.converged.sum()), cells=R * 101, bfgs_cells_at_least_neldermead=int((b.loglikel >= n.loglikel).sum()),
         ratio_neldermead_over_bfgs_s=secs["neldermead"] / secs["bfgs"])
    cell = b.delays.map_index
    emit(what="peaks, README size", N=110, G=101, R=R, iterations=iterations, kernel="OU", peaks_s=t_peaks, rounds=int(pk.rounds),
         f_calls=int(pk.f_calls), converged=int(pk.converged.sum()), mean_gain_over_the_cell=float(np.mean(pk.loglikel - pk.start_loglikel)),
         grid_spacing=float(cand[1, 1] - cand[0, 1]), std_of_the_cells_delay=float(np.std(cand[cell, 1])), std_of_the_peaks_delay=float(np.std(pk.delays[:, 1])),
         mean_abs_move_from_the_cell=float(np.mean(np.abs(pk.delays[:, 1] - cand[cell, 1]))),
         note="OU has kinks in tau where shifted times cross: a realisation that stalls on one ends with converged = False at its best point")


def jobs(quick):
    import gpcc_amd
    out = [lambda: measure("README size", 110, 101, gpcc_amd.OU, 1000 if not quick else 32, 5, 1 if quick else 3)]
    if not quick:
        out += [lambda R=R: measure("N = 4096, 1024 delays", 4096, 1024, gpcc_amd.matern32, R, 2, 3) for R in (8, 64)]
        out += [lambda: measure("N = 16384, 256 delays", 16384, 256, gpcc_amd.matern52, 4, 1, 1)]
    return out + [lambda: (lambda: refit(100 if not quick else 4, 30))]


def main():
    import subprocess
    import gpcc_amd
    quick = "--quick" in sys.argv
    if "--child" in sys.argv:                       # one measurement: the entries first, then its loop of fresh handles
        jobs(quick)[int(sys.argv[sys.argv.index("--child") + 1])]()()
        return 0
    emit(what="build", info=gpcc_amd.build_info())
    for k in range(len(jobs(quick))):               # one fresh process per measurement, one after the other (tools/markov_resample_bench.py)
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(k)] + (["--quick"] if quick else []),
                             stdout=subprocess.PIPE, text=True)
        for line in run.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                LINES.append(line)
        if run.returncode:
            return run.returncode
    if "--log" in sys.argv:
        path = sys.argv[sys.argv.index("--log") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tools/markov_resample_grad_bench.py: gpcc_loglik_grad_markov_resampled_batch against gpcc_loglik_markov_resampled_batch and "
                    "gpcc_loglik_grad_markov_batch on the same rows and against R fresh handles with one gpcc_loglik_grad_markov_batch call each, "
                    "same inputs, same run (MI355X);\n# entries: 5 alternating windows of `calls_per_window` blocking calls, median window; the "
                    "loop: timed whole, `loops` times; then realisation_refits by both optimisers and realisation_peaks; build %s\n"
                    % gpcc_amd.build_info())
            f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
