#!/usr/bin/env python3
"""Times gpcc_loglik_hess_noise_markov_batch (the Hessian over [alpha, rho, kappa, nu] of rows with their own noise model, DESIGN.md
4.26) against the plain block and against the loop it replaces, same inputs, same run; prints one JSON line per measurement.  A
measurement, not a gate: no ratio is fixed in advance, every one is stated whatever it is.

  python tools/markov_noise_hess_bench.py [--log profiles/markov/noise_hess_bench.log] [--quick]
      README size: N = 110, OU, 101 delays;  N = 4096, Matern-3/2, L = 2, 1024 rows;  N = 16384, Matern-5/2, 64 rows.  For each:
      (i)   the new entry on rows that carry D = 8 distinct noise models (row m: model m mod D): (3L+1)(3L+2)/2 = 28 pair slots
      (ii)  gpcc_loglik_hess_hyper_markov_batch on the same rows (the handle's error bars): (L+1)(L+2)/2 = 6 pair slots
      (iii) the loop the feature replaces: central differences of gpcc_loglik_grad_noise_markov_batch in the 2L noise parameters (4L
            calls on all rows) for the noise rows and columns, plus, per distinct (kappa, nu), a fresh handle on effective_std and (ii)
            on its rows for the (alpha, rho) block

Timing: host wall clock around blocking calls; each workload runs in a fresh process of its own.  (i) and (ii): after a warm-up call
of each, 5 alternating windows of `calls` calls, median window.  The loop is timed whole, `loops` times, median."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from markov_grad_bench import WINDOWS, alternate, sweep  # noqa: E402

LINES = []
D = 8


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    LINES.append(line)


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def measure(name, N, M, kernel, calls, loops):
    import gpcc_amd
    from gpcc_amd import fit
    (t, y, s), delays, alpha, rho = sweep(N, M)
    L = 2
    n = 3 * L + 1
    rg = np.random.default_rng(N)
    models = np.concatenate([rg.uniform(0.5, 2.0, (D, L)), rg.uniform(0.2, 1.0, (D, L)) * np.array([np.mean(a ** 2) for a in s])], 1)
    which = np.arange(M) % D
    kappa, nu = np.ascontiguousarray(models[which, :L]), np.ascontiguousarray(models[which, L:])
    idx = list(range(L + 1)) + list(range(2 * L + 1, 4 * L + 1))
    h = 1e-4

    with gpcc_amd.Objective(t, y, s, kernel) as obj:
        def loop():
            H = np.empty((M, n, n))
            for c in range(2 * L):                  # the noise rows and columns: central differences of the gradient entry
                e = np.zeros((M, 2 * L))
                e[:, c] = h * np.concatenate([kappa, nu], 1)[:, c]
                gp = obj.loglik_grad_markov_noise_batch(delays, alpha, rho, kappa + e[:, :L], nu + e[:, L:])[1][:, idx]
                gm = obj.loglik_grad_markov_noise_batch(delays, alpha, rho, kappa - e[:, :L], nu - e[:, L:])[1][:, idx]
                H[:, :, L + 1 + c] = H[:, L + 1 + c, :] = (gp - gm) / (2 * e[:, c])[:, None]
            for k in range(D):                      # the (alpha, rho) block: a fresh handle per distinct noise model
                rows = which == k
                with gpcc_amd.Objective(t, y, fit.effective_std(s, models[k, :L], models[k, L:]), kernel) as fresh:
                    H[rows, :L + 1, :L + 1] = fresh.loglik_hess_hyper_markov_batch(delays[rows], alpha[rows], rho[rows])[2]
            return H

        tn, tp = alternate([lambda: obj.loglik_hess_markov_noise_batch(delays, alpha, rho, kappa, nu),
                            lambda: obj.loglik_hess_hyper_markov_batch(delays, alpha, rho)], [calls] * 2)
        ll, grad, hess, info = obj.loglik_hess_markov_noise_batch(delays, alpha, rho, kappa, nu)
        ref = loop()
        tl = []
        for _ in range(loops):
            t0 = time.perf_counter()
            loop()
            tl.append(time.perf_counter() - t0)
    ok = info == 0
    scale = np.max(np.abs(hess[ok]), axis=(1, 2), keepdims=True)
    emit(what=name, N=N, M=M, kernel=kernel.name, distinct_noise_models=D, noise_hess_ms=[1e3 * x for x in tn], plain_hess_ms=[1e3 * x for x in tp],
         loop_ms=[1e3 * x for x in sorted(tl)], rows_per_s=M / med(tn), ratio_noise_over_plain_hess=med(tn) / med(tp),
         ratio_loop_over_noise_hess=med(tl) / med(tn), slots_noise_over_plain="%d/%d = %.3f" % (n * (n + 1) // 2, (L + 1) * (L + 2) // 2,
                                                                                             n * (n + 1) / ((L + 1) * (L + 2))),
         waves="%d" % (((M + 63) // 64) * (n * (n + 1) // 2)), calls_per_window=calls, windows=WINDOWS, loops=loops,
         max_diff_from_the_loop_of_max_abs_H=float(np.max(np.abs(hess[ok] - ref[ok]) / scale)), failed=int((~ok).sum()))


def jobs(quick):
    import gpcc_amd
    out = [lambda: measure("README size", 110, 101, gpcc_amd.OU, 100, 3)]
    if not quick:
        out += [lambda: measure("N = 4096, 1024 rows", 4096, 1024, gpcc_amd.matern32, 10, 3),
                lambda: measure("N = 16384, 64 rows", 16384, 64, gpcc_amd.matern52, 3, 3)]
    return out


def main():
    import subprocess
    import gpcc_amd
    quick = "--quick" in sys.argv
    if "--child" in sys.argv:
        jobs(quick)[int(sys.argv[sys.argv.index("--child") + 1])]()
        return 0
    emit(what="build", info=gpcc_amd.build_info())
    for k in range(len(jobs(quick))):               # one fresh process per workload, one after the other (tools/markov_noise_bench.py)
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
            f.write("# tools/markov_noise_hess_bench.py: gpcc_loglik_hess_noise_markov_batch against gpcc_loglik_hess_hyper_markov_batch on the same "
                    "rows and against the loop it replaces (central differences of the noise gradient entry plus the plain block on a fresh handle per "
                    "distinct noise model), same inputs, same run (MI355X);\n# entries: 5 alternating windows of `calls_per_window` blocking calls, "
                    "median window; the loop: timed whole, `loops` times; build %s\n" % gpcc_amd.build_info())
            f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
