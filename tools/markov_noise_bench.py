#!/usr/bin/env python3
"""Times gpcc_loglik_noise_markov_batch and gpcc_loglik_grad_noise_markov_batch (rows with their own parameters and their own noise
model kappa^2 sigma^2 + nu) against the routes beside them, same inputs, same run; prints one JSON line per
measurement.  A measurement, not a gate: every ratio is stated whatever it is, also where the new entries lose.

  python tools/markov_noise_bench.py [--log profiles/markov/noise_bench.log] [--quick]
      README size: N = 110, OU, 101 delays;  N = 4096, Matern-3/2, 1024 rows;  N = 16384, Matern-5/2, 64 rows.  For each:
      (a) the value entry against gpcc_loglik_markov_batch on the same rows at kappa = 1, nu = 0 (bitwise the same numbers): what the
          feature costs -- one fma and two LDS reads a step, 44 L instead of 28 L bytes of LDS a lane
      (b) the value entry on rows that carry D = 8 distinct noise models (row m: model m mod D) against the loop a user needs without
          it: per distinct (kappa, nu) a fresh handle on effective_std, one gpcc_loglik_markov_batch call on its rows, close
      (c) the gradient entry (4L+1 entries; 4L+1 slots, OU 5L+1) against gpcc_loglik_grad_markov_batch (2L+1 entries; 2L+1 slots, OU
          3L+1) on the same rows at kappa = 1, nu = 0

Timing: host wall clock around blocking calls; each workload runs in a fresh process of its own.  The entries: after a warm-up call of
each, 5 alternating windows of `calls` calls, median window.  The loop is timed whole, `loops` times, median."""
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
    ou = kernel.name == "OU"
    rg = np.random.default_rng(N)
    models = np.concatenate([rg.uniform(0.5, 2.0, (D, L)), rg.uniform(0.0, 1.0, (D, L)) * np.array([np.mean(a ** 2) for a in s])], 1)
    which = np.arange(M) % D
    kappa, nu = np.ascontiguousarray(models[which, :L]), np.ascontiguousarray(models[which, L:])
    one, zero = np.ones((M, L)), np.zeros((M, L))

    def loop():
        out = np.empty(M)
        for k in range(D):
            rows = which == k
            with gpcc_amd.Objective(t, y, fit.effective_std(s, models[k, :L], models[k, L:]), kernel) as fresh:
                out[rows] = fresh.loglik_markov_batch(delays[rows], alpha[rows], rho[rows])[0]
        return out

    with gpcc_amd.Objective(t, y, s, kernel) as obj:
        tn1, tp, tnd, tng, tpg = alternate([lambda: obj.loglik_markov_noise_batch(delays, alpha, rho, one, zero),
                                            lambda: obj.loglik_markov_batch(delays, alpha, rho),
                                            lambda: obj.loglik_markov_noise_batch(delays, alpha, rho, kappa, nu),
                                            lambda: obj.loglik_grad_markov_noise_batch(delays, alpha, rho, one, zero),
                                            lambda: obj.loglik_grad_markov_batch(delays, alpha, rho)], [calls] * 5)
        unit, uinfo = obj.loglik_markov_noise_batch(delays, alpha, rho, one, zero)
        plain, pinfo = obj.loglik_markov_batch(delays, alpha, rho)
        ll, info = obj.loglik_markov_noise_batch(delays, alpha, rho, kappa, nu)
    ref = loop()
    tl = []
    for _ in range(loops):
        t0 = time.perf_counter()
        loop()
        tl.append(time.perf_counter() - t0)
    slots_noise, slots_plain = (5 * L + 1, 3 * L + 1) if ou else (4 * L + 1, 2 * L + 1)
    emit(what=name, N=N, M=M, kernel=kernel.name, distinct_noise_models=D,
         noise_value_unit_ms=[1e3 * x for x in tn1], plain_value_ms=[1e3 * x for x in tp], noise_value_ms=[1e3 * x for x in tnd],
         noise_grad_ms=[1e3 * x for x in tng], plain_grad_ms=[1e3 * x for x in tpg], loop_ms=[1e3 * x for x in sorted(tl)],
         rows_per_s=M / med(tnd), ratio_noise_over_plain_value=med(tn1) / med(tp), ratio_loop_over_noise_value=med(tl) / med(tnd),
         ratio_noise_over_plain_grad=med(tng) / med(tpg), slots_noise_over_plain="%d/%d = %.3f" % (slots_noise, slots_plain, slots_noise / slots_plain),
         calls_per_window=calls, windows=WINDOWS, loops=loops, unit_noise_bitwise_plain=bool(np.array_equal(unit, plain) and np.array_equal(uinfo, pinfo)),
         max_rel_diff_from_the_loop=float(np.max(np.abs(ll - ref) / np.abs(ref))), failed=int((info != 0).sum()))


def jobs(quick):
    import gpcc_amd
    out = [lambda: measure("README size", 110, 101, gpcc_amd.OU, 200, 3)]
    if not quick:
        out += [lambda: measure("N = 4096, 1024 rows", 4096, 1024, gpcc_amd.matern32, 20, 3),
                lambda: measure("N = 16384, 64 rows", 16384, 64, gpcc_amd.matern52, 5, 3)]
    return out


def main():
    import subprocess
    import gpcc_amd
    quick = "--quick" in sys.argv
    if "--child" in sys.argv:
        jobs(quick)[int(sys.argv[sys.argv.index("--child") + 1])]()
        return 0
    emit(what="build", info=gpcc_amd.build_info())
    for k in range(len(jobs(quick))):               # one fresh process per workload, one after the other (tools/markov_resample_bench.py)
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
            f.write("# tools/markov_noise_bench.py: gpcc_loglik_noise_markov_batch against gpcc_loglik_markov_batch on the same rows, against the "
                    "loop of fresh handles on effective_std, and its gradient against gpcc_loglik_grad_markov_batch, same inputs, same run "
                    "(MI355X);\n# entries: 5 alternating windows of `calls_per_window` blocking calls, median window; the loop: timed whole, "
                    "`loops` times; build %s\n" % gpcc_amd.build_info())
            f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
