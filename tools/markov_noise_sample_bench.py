#!/usr/bin/env python3
"""Times the linear-time joint posterior draws under a per-row noise model (gpcc_sample_noise_markov_batch) against the
plain entry and against the loop it replaces, same inputs, same run; prints one JSON line per measurement.  A measurement, not a gate:
every ratio is stated whatever it is.

  python tools/markov_noise_sample_bench.py [--log profiles/markov/noise_sample_bench.log] [--quick]
      the shapes of tools/markov_sample_bench.py, mixture draws over weighted rows:
      README size: N = 110, OU, 101 delays, T = 2 x 201, 10 000 draws;  N = 4096, Matern-3/2, 64 rows, T = 2 x 512, 4096 draws;
      N = 16384, Matern-5/2, the same rows, test set and draws.  For each size:
      (a) the noise entry at kappa = 1, nu = 0 against the plain entry on the same rows (bitwise the same numbers): what the feature
          costs -- one fma and two LDS reads a training step, 16 L more bytes of LDS a lane
      (b) the noise entry on rows that each carry their own noise model
      (c) the loop it replaces: the rows picked on the host, per drawn row a fresh handle on effective_std, one plain one-row call for
          that row's draws, close

Timing: host wall clock around blocking calls; each size runs in a fresh process of its own.  The entries: after a warm-up call of each,
5 alternating windows of `calls` calls, median window.  The loop is timed whole, `loops` times, median."""
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


def measure(name, N, M, kernel, Tl, S, calls, loops):
    import gpcc_amd
    from gpcc_amd import fit, rng
    (t, y, s), delays, alpha, rho = sweep(N, M)
    L, seed = 2, 1
    rg = np.random.default_rng(N)
    kappa = rg.uniform(0.5, 2.0, (M, L))
    nu = rg.uniform(0.0, 1.0, (M, L)) * np.array([np.mean(a ** 2) for a in s])
    one, zero = np.ones((M, L)), np.zeros((M, L))
    hi = max(np.max(a) for a in t)
    tt = [np.linspace(-0.02 * hi, 1.02 * hi, Tl) for _ in range(L)]
    st = [np.full(Tl, float(np.mean(s[l]))) for l in range(L)]
    w = np.exp(-0.5 * ((np.arange(M) - 0.4 * M) / (0.2 * M)) ** 2)

    def loop():
        """The rows on the host, then per drawn row a fresh handle on its effective error bars and one plain call for its draws."""
        rows = rng.pick_rows(seed, S, w)
        out = np.empty((S, L * Tl))
        for m in np.unique(rows):
            sel = rows == m
            with gpcc_amd.Objective(t, y, fit.effective_std(s, kappa[m], nu[m]), kernel) as fresh:
                out[sel] = fresh.sample_markov_batch(delays[m:m + 1], alpha[m:m + 1], rho[m:m + 1], tt, int(sel.sum()), seed, weights=[1.0],
                                                     sigmatest=fit.effective_std(st, kappa[m], nu[m]))[0]
        return out, rows

    with gpcc_amd.Objective(t, y, s, kernel) as obj:
        unit = lambda: obj.sample_markov_noise_batch(delays, alpha, rho, one, zero, tt, S, seed, sigmatest=st, weights=w)      # noqa: E731
        plain = lambda: obj.sample_markov_batch(delays, alpha, rho, tt, S, seed, sigmatest=st, weights=w)                     # noqa: E731
        noise = lambda: obj.sample_markov_noise_batch(delays, alpha, rho, kappa, nu, tt, S, seed, sigmatest=st, weights=w)    # noqa: E731
        tu, tp, tn = alternate([unit, plain, noise], [calls] * 3)
        got, ru, rp = noise(), unit(), plain()
    tl = []
    for _ in range(loops):
        t0 = time.perf_counter()
        ref, rows = loop()
        tl.append(time.perf_counter() - t0)
    bitwise = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ru, rp))
    emit(what=name, N=N, M=M, T=L * Tl, S=S, kernel=kernel.name, rows_drawn=int(len(np.unique(rows))), noise_unit_ms=[1e3 * x for x in tu],
         plain_ms=[1e3 * x for x in tp], noise_ms=[1e3 * x for x in tn], loop_ms=[1e3 * x for x in sorted(tl)],
         ratio_noise_unit_over_plain=med(tu) / med(tp), ratio_noise_over_plain=med(tn) / med(tp), ratio_loop_over_noise=med(tl) / med(tn),
         noise_draws_per_s=S / med(tn), calls_per_window=calls, windows=WINDOWS, loops=loops, unit_noise_bitwise_plain=bool(bitwise),
         same_draw_rows_as_the_loop=bool(np.array_equal(rows, got[1])), failed=int(((got[3] != 0) & (got[3] != -14)).sum()),
         max_gap_of_the_draws_means_from_the_loop=float(np.max(np.abs(got[0].mean(0) - ref.mean(0)))))


def jobs(quick):
    import gpcc_amd
    out = [lambda: measure("README size", 110, 101, gpcc_amd.OU, 201, 10000, 3, 1)]
    if not quick:
        out += [lambda: measure("N = 4096, 64 rows", 4096, 64, gpcc_amd.matern32, 512, 4096, 2, 1),
                lambda: measure("N = 16384, 64 rows", 16384, 64, gpcc_amd.matern52, 512, 4096, 1, 1)]
    return out


def main():
    import subprocess
    import gpcc_amd
    quick = "--quick" in sys.argv
    if "--child" in sys.argv:
        jobs(quick)[int(sys.argv[sys.argv.index("--child") + 1])]()
        return 0
    emit(what="build", info=gpcc_amd.build_info())
    for k in range(len(jobs(quick))):               # one fresh process per size, one after the other (tools/markov_noise_predict_bench.py)
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
            f.write("# tools/markov_noise_sample_bench.py: gpcc_sample_noise_markov_batch at kappa = 1, nu = 0 against gpcc_sample_markov_batch, "
                    "on rows with their own noise model, and against the loop of fresh handles on effective_std, same inputs, same run "
                    "(MI355X);\n# entries: 5 alternating windows of `calls_per_window` blocking calls, median window; the loop: timed whole, "
                    "`loops` times; build %s\n" % gpcc_amd.build_info())
            f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
