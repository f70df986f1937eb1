#!/usr/bin/env python3
"""Times gpcc_loglik_hess_full_noise_markov_batch (the full Hessian over [alpha, rho, tau, kappa, nu] of rows with their own noise model,
DESIGN.md 4.27) against the plain full Hessian and against the loop it replaces, same inputs, same run; prints one JSON line per
measurement.  A measurement, not a gate: no ratio is fixed in advance, every one is stated whatever it is.

  python tools/markov_noise_hess_tau_bench.py [--log profiles/markov/noise_hess_full_bench.log] [--quick]
      README size: N = 110, OU, 101 delays;  N = 4096, Matern-3/2, L = 2, 1024 and 64 rows;  N = 16384, Matern-5/2, 64 rows.  For each:
      (i)   the new entry on rows that carry D = 8 distinct noise models (row m: model m mod D): the gradient's launches, the block's
            (3L+1)(3L+2)/2 = 28 pair slots and the 3L^2 + L + L(L+1)/2 = 17 pair slots with a tau
      (ii)  gpcc_loglik_hess_markov_batch on the same rows at kappa = 1, nu = 0 (the handle's error bars): (L+1)(L+2)/2 = 6 slots of
            the (alpha, rho) block and L^2 + L + L(L+1)/2 = 9 slots with a tau
      (iii) the loop the feature replaces for the rows of tau: five-point central differences of gpcc_loglik_grad_noise_markov_batch
            in each tau (4L calls on all rows)

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
    (t, y, s), delays, alpha, rho = sweep(N, M)
    L = 2
    W = 4 * L + 1
    rg = np.random.default_rng(N)
    models = np.concatenate([rg.uniform(0.5, 2.0, (D, L)), rg.uniform(0.2, 1.0, (D, L)) * np.array([np.mean(a ** 2) for a in s])], 1)
    which = np.arange(M) % D
    kappa, nu = np.ascontiguousarray(models[which, :L]), np.ascontiguousarray(models[which, L:])
    h = 1e-3 * float(np.median(rho))       # the tau step: a fraction of the time scale

    with gpcc_amd.Objective(t, y, s, kernel) as obj:
        def loop():
            rows = np.empty((M, L, W))
            for l in range(L):              # the rows of tau: five-point central differences of the gradient entry in tau_l
                e = np.zeros((M, L))
                e[:, l] = h
                f = [obj.loglik_grad_markov_noise_batch(delays + q * e, alpha, rho, kappa, nu)[1] for q in (1, -1, 2, -2)]
                rows[:, l, :] = (8 * (f[0] - f[1]) - (f[2] - f[3])) / (12 * h)
            return rows

        tn, tp = alternate([lambda: obj.loglik_hess_full_markov_noise_batch(delays, alpha, rho, kappa, nu),
                            lambda: obj.loglik_hess_markov_batch(delays, alpha, rho)], [calls] * 2)
        ll, grad, hess, info = obj.loglik_hess_full_markov_noise_batch(delays, alpha, rho, kappa, nu)
        ref = loop()
        tl = []
        for _ in range(loops):
            t0 = time.perf_counter()
            loop()
            tl.append(time.perf_counter() - t0)
    ok = (info == 0) & np.isfinite(hess).all(axis=(1, 2))
    got = hess[:, L + 1:2 * L + 1, :]
    scale = np.max(np.abs(got[ok]), axis=(1, 2), keepdims=True)
    new_slots, block_slots = 3 * L * L + L + L * (L + 1) // 2, (3 * L + 1) * (3 * L + 2) // 2
    plain_slots = L * L + L + L * (L + 1) // 2 + (L + 1) * (L + 2) // 2
    emit(what=name, N=N, M=M, kernel=kernel.name, distinct_noise_models=D, noise_hess_full_ms=[1e3 * x for x in tn],
         plain_hess_full_ms=[1e3 * x for x in tp], loop_ms=[1e3 * x for x in sorted(tl)], rows_per_s=M / med(tn),
         ratio_noise_full_over_plain_full=med(tn) / med(tp), ratio_loop_over_noise_full=med(tl) / med(tn),
         slots_noise_over_plain="%d/%d = %.3f" % (new_slots + block_slots, plain_slots, (new_slots + block_slots) / plain_slots),
         waves_new_kernel="%d" % (((M + 63) // 64) * new_slots), calls_per_window=calls, windows=WINDOWS, loops=loops,
         max_diff_of_the_tau_rows_from_the_loop_of_max_abs=float(np.max(np.abs(got[ok] - ref[ok]) / scale)),
         failed_or_tied=int((~ok).sum()))


def jobs(quick):
    import gpcc_amd
    out = [lambda: measure("README size", 110, 101, gpcc_amd.OU, 100, 3)]
    if not quick:
        out += [lambda: measure("N = 4096, 1024 rows", 4096, 1024, gpcc_amd.matern32, 10, 3),
                lambda: measure("N = 4096, 64 rows", 4096, 64, gpcc_amd.matern32, 10, 3),
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
            f.write("# tools/markov_noise_hess_tau_bench.py: gpcc_loglik_hess_full_noise_markov_batch against gpcc_loglik_hess_markov_batch on the same "
                    "rows at kappa = 1, nu = 0 and against the loop it replaces (five-point central differences of the noise gradient entry in each "
                    "tau), same inputs, same run (MI355X);\n# entries: 5 alternating windows of `calls_per_window` blocking calls, median window; the "
                    "loop: timed whole, `loops` times; build %s\n" % gpcc_amd.build_info())
            f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
