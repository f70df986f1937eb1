#!/usr/bin/env python3
"""Times gpcc_loglik_markov_resampled_batch (rows with their own parameters and their own resampled data set, one linear-time pass)
against the routes beside it, same inputs, same run; prints one JSON line per measurement.  A measurement, not a gate: every ratio is
stated whatever it is, also where the new entry loses.

  python tools/markov_resample_bench.py [--log profiles/markov/resample_bench.log] [--quick]
      (a) README size: N = 110, OU, 101 delays, R = 1000, one evaluation per (realisation, delay) -- flux randomisation alone, and
          with random subset selection
      (b) N = 4096, Matern-3/2, 1024 delays x R = 8 and R = 64
          ... each against the loop of R fresh handles (create, gpcc_loglik_markov_batch, close: timed whole) and, without subset
          selection, against gpcc_loglik_markov_multi_batch on the same Y: the shared-covariance route, which shows what
          un-sharing the covariance recursion costs
      (c) the refit: fit.realisation_refits at README size, R = 100, 30 iterations, warm start, against 100
          gpcc_grid(solver="markov") runs on fresh handles (timed whole, once each way after a warm-up of the library)

Timing: host wall clock around blocking calls; each measurement runs in a fresh process of its own, the entries before its loop.  The two entries: after a warm-up call of each, 5 alternating windows of `calls`
calls, median window.  The loop is timed whole, `loops` times, median.  (a) and (b) run without marginalise_b and with own means, so
that every route computes the same numbers (the realisations' means are computed once, outside the timed calls); their largest relative disagreement is printed."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from markov_grad_bench import WINDOWS, alternate, sweep  # noqa: E402

LINES = []


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    LINES.append(line)


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def reduced(t, s, Y, counts, r):
    keep = [c[r] > 0 for c in counts]
    return ([np.asarray(a)[k] for a, k in zip(t, keep)], [a[r][k] for a, k in zip(Y, keep)],
            [np.asarray(a)[k] / np.sqrt(c[r][k]) for a, k, c in zip(s, keep, counts)])


def measure(name, N, M, kernel, R, calls, loops, subset):
    import gpcc_amd
    from gpcc_amd import markov, synthetic
    (t, y, s), delays, alpha, rho = sweep(N, M)
    Y, counts = synthetic.resample(y, s, R, seed=R, subset=subset)
    mean, vb = markov.resample_constants(t, Y, counts, False)          # each realisation's own band means, once (as fit.realisation_refits does)
    g, r = np.tile(np.arange(M), R), np.repeat(np.arange(R), M)          # realisation-major rows
    dg, ag, rg = delays[g], alpha[g], rho[g]

    def loop():
        out = np.empty((R, M))
        for k in range(R):
            with gpcc_amd.Objective(*reduced(t, s, Y, counts, k), kernel, marginalise_b=False) as fresh:
                out[k] = fresh.loglik_markov_batch(delays, alpha, rho)[0]
        return out

    with gpcc_amd.Objective(t, y, s, kernel, marginalise_b=False) as obj:
        flat, cflat = obj.realisations(Y), (np.concatenate(counts, axis=1) if subset else None)
        fns = [lambda: obj.loglik_markov_resampled(flat, dg, ag, rg, r, counts=cflat, center=mean, sigma_b=vb)]
        if not subset:
            fns.append(lambda: obj.loglik_markov_realisations(flat, delays, alpha, rho))
        fns.append(lambda: obj.loglik_markov_batch(delays, alpha, rho))
        times = alternate(fns, [calls] * len(fns))
        tr, ts = times[0], times[-1]
        tm = times[1] if not subset else None
        ll, info = obj.loglik_markov_resampled(flat, dg, ag, rg, r, counts=cflat, center=mean, sigma_b=vb)
        multi = obj.loglik_markov_realisations(flat, delays, alpha, rho)[0] if not subset else None
        scratch = obj.get_option("markov_resample_bytes") + obj.get_option("markov_resample_upload_bytes")
    return lambda: _finish(name, N, M, kernel, R, calls, loops, subset, loop, tr, tm, ts, ll, info, multi, scratch)


def _finish(name, N, M, kernel, R, calls, loops, subset, loop, tr, tm, ts, ll, info, multi, scratch):
    ref = loop()
    tl = []
    for _ in range(loops):
        t0 = time.perf_counter()
        loop()
        tl.append(time.perf_counter() - t0)
    ok = info == 0
    ll = ll.reshape(R, M)
    emit(what=name, N=N, M=M, R=R, rows=M * R, kernel=kernel.name, subset=bool(subset), resampled_ms=[1e3 * x for x in tr],
         multi_ms=None if tm is None else [1e3 * x for x in tm], single_call_ms=[1e3 * x for x in ts], loop_ms=[1e3 * x for x in sorted(tl)],
         rows_per_s=M * R / med(tr), ratio_loop_over_resampled=med(tl) / med(tr),
         ratio_resampled_over_multi=None if tm is None else med(tr) / med(tm), ratio_resampled_over_R_single_calls=med(tr) / (R * med(ts)),
         scratch_bytes=int(scratch), calls_per_window=calls, windows=WINDOWS, loops=loops,
         max_rel_diff_from_the_loop=float(np.max(np.abs(ll - ref) / np.abs(ref))),
         max_rel_diff_from_multi=None if multi is None else float(np.max(np.abs(ll - multi.T) / np.abs(multi.T))), failed=int((~ok).sum()))


def refit(R, iterations):
    import gpcc_amd
    from gpcc_amd import fit, synthetic
    (t, y, s), cand, _, _ = sweep(110, 101)
    Y, counts = synthetic.resample(y, s, R, seed=3)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        res = fit.gpcc_grid(t, y, s, kernel=gpcc_amd.OU, candidatedelays=cand, iterations=100, objective=obj, solver="markov")
        fit.realisation_refits(obj, cand, [a[:2] for a in Y], [c[:2] for c in counts], iterations=2, start=(res.alpha, res.rho))   # warm-up
        t0 = time.perf_counter()
        out = fit.realisation_refits(obj, cand, Y, counts, iterations=iterations, start=(res.alpha, res.rho))
        t_refit = time.perf_counter() - t0
    return lambda: _refit_loop(R, iterations, t, s, Y, counts, cand, out, t_refit)


def _refit_loop(R, iterations, t, s, Y, counts, cand, out, t_refit):
    import gpcc_amd
    from gpcc_amd import fit
    t0 = time.perf_counter()
    grids = []
    for k in range(R):
        red = reduced(t, s, Y, counts, k)
        with gpcc_amd.Objective(*red, gpcc_amd.OU) as fresh:
            grids.append(fit.gpcc_grid(*red, kernel=gpcc_amd.OU, candidatedelays=cand, iterations=iterations, objective=fresh,
                                       solver="markov").loglikel)
    t_loop = time.perf_counter() - t0
    grids = np.array(grids)
    emit(what="refit, README size", N=110, G=101, R=R, iterations=iterations, kernel="OU", refit_s=t_refit, loop_of_gpcc_grid_s=t_loop,
         ratio_loop_over_refit=t_loop / t_refit, f_calls=int(out.f_calls), rounds=int(out.rounds),
         rows_per_s_whole_fit=out.f_calls / t_refit, mean_gain_over_the_start=float(np.mean(out.loglikel - out.start_loglikel)),
         mean_refit_minus_cold_grid=float(np.mean(out.loglikel - grids)),
         note="the loop's gpcc_grid starts cold (random candidates, native engine); the refit starts warm and drives Nelder-Mead from numpy")


def jobs(quick):
    import gpcc_amd
    out = [lambda sub=sub: measure("README size", 110, 101, gpcc_amd.OU, 1000 if not quick else 32, 10, 1 if quick else 3, sub) for sub in (False, True)]
    if not quick:
        out += [lambda R=R: measure("N = 4096, 1024 delays", 4096, 1024, gpcc_amd.matern32, R, 2, 3, False) for R in (8, 64)]
    return out + [lambda: refit(100 if not quick else 4, 30)]


def main():
    import subprocess
    import gpcc_amd
    quick = "--quick" in sys.argv
    if "--child" in sys.argv:                       # one measurement: the entries first, then its loop of fresh handles
        jobs(quick)[int(sys.argv[sys.argv.index("--child") + 1])]()()
        return 0
    # One fresh process per measurement, one after the other.  In one process the second measurement's calls were slow throughout -- 26
    # against 2.1 ms for the README size with subset selection, 2.9 against 0.13 ms for the gpcc_loglik_markov_batch call beside it --
    # whether or not a loop of fresh handles had run before: what an earlier, destroyed handle leaves behind is the open question of
    # DESIGN.md 4.20, and not the entries'.
    emit(what="build", info=gpcc_amd.build_info())
    for k in range(len(jobs(quick))):
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
            f.write("# tools/markov_resample_bench.py: gpcc_loglik_markov_resampled_batch against R fresh handles with one gpcc_loglik_markov_batch "
                    "call each and against gpcc_loglik_markov_multi_batch, same inputs, same run (MI355X);\n# entries: 5 alternating windows of "
                    "`calls_per_window` blocking calls, median window; the loop: timed whole, `loops` times; build %s\n" % gpcc_amd.build_info())
            f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
