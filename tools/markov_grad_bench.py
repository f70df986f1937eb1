#!/usr/bin/env python3
"""Rates of gpcc_loglik_grad_markov_batch (the linear-time gradient of the OU / Matern kernels) against the dense gradient
(gpcc_loglik_grad_batch) on the same inputs in the same run; prints one JSON line per measurement.

  python tools/markov_grad_bench.py [--log profiles/markov/grad_bench.log] [--quick]
      N = 4096, Matern-3/2, L = 2, 1024 delays (the headline batch)         value+gradient evaluations/s of both; floor: ratio >= 10
      N = 2048, 256 delays; N = 110, 1000 delays                            both
      one call at N = 110 / 1024 / 4096                                     latency of both
      N = 16384, Matern-5/2, 64 delays                                      the linear-time rate and the handle's bytes (no dense gradient)
  python tools/markov_grad_bench.py --profile-run     one headline batch after a warm-up, for rocprofv3 --kernel-trace --stats

Timing: host wall clock around blocking calls.  After a warm-up call of each path, `windows` (5) windows per path, the two paths
ALTERNATING; a window is `calls` calls back to back; the figure is the median window."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LINES = []
WINDOWS = 5
FLOOR = 10.0


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    LINES.append(line)


def sweep(N, M, L=2, seed=1):
    from gpcc_amd import synthetic
    Nl = [N // L + (1 if l < N % L else 0) for l in range(L)]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=seed)
    alpha, rho = synthetic.default_hyperparameters(y)
    grid = np.linspace(0.0, 20.0, M) if M > 1 else np.array([7.3])
    return (t, y, s), np.stack([np.zeros(M), grid], 1), np.tile(alpha, (M, 1)), np.full(M, rho)


def window(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) / calls


def alternate(fns, calls):
    """Per path the per-call seconds of WINDOWS windows, the paths alternating -> [sorted seconds] per path."""
    for fn in fns:
        fn()
    out = [[] for _ in fns]
    for _ in range(WINDOWS):
        for i, (fn, c) in enumerate(zip(fns, calls)):
            out[i].append(window(fn, c))
    return [sorted(o) for o in out]


def both(name, N, M, kernel, calls_markov, calls_dense):
    import gpcc_amd
    data, delays, alpha, rho = sweep(N, M)
    with gpcc_amd.Objective(*data, kernel) as obj:
        tm, td = alternate([lambda: obj.loglik_grad_markov_batch(delays, alpha, rho), lambda: obj.loglik_grad_batch(delays, alpha, rho)],
                           [calls_markov, calls_dense])
        lm, gm, im = obj.loglik_grad_markov_batch(delays, alpha, rho)
        ld, gd, idn = obj.loglik_grad_batch(delays, alpha, rho)
    ok = (im == 0) & (idn == 0)
    scale = np.max(np.abs(gd[ok]), axis=1, keepdims=True)
    med = lambda v: v[len(v) // 2]
    emit(what=name, N=N, M=M, kernel=kernel.name, markov_grads_per_s=M / med(tm), dense_grads_per_s=M / med(td), ratio=med(td) / med(tm),
         markov_ms=[1e3 * x for x in tm], dense_ms=[1e3 * x for x in td], calls_per_window=[calls_markov, calls_dense], windows=WINDOWS,
         max_grad_diff_of_max_g=float(np.max(np.abs(gm[ok] - gd[ok]) / scale)), failed=int((~ok).sum()))
    return med(td) / med(tm)


def markov_only(name, N, M, kernel, calls):
    import torch
    import gpcc_amd
    data, delays, alpha, rho = sweep(N, M)
    torch.cuda.synchronize()
    with gpcc_amd.Objective(*data, kernel) as obj:
        free0, _ = torch.cuda.mem_get_info(0)
        (tm,) = alternate([lambda: obj.loglik_grad_markov_batch(delays, alpha, rho)], [calls])
        free1, _ = torch.cuda.mem_get_info(0)
        tv = sorted(window(lambda: obj.loglik_markov_batch(delays, alpha, rho), calls) for _ in range(WINDOWS))
        _, _, info = obj.loglik_grad_markov_batch(delays, alpha, rho)
        built = obj.get_option("workspace_slots") != obj.get_option("slots_per_stream")
    emit(what=name, N=N, M=M, kernel=kernel.name, markov_grads_per_s=M / tm[len(tm) // 2], markov_values_per_s=M / tv[len(tv) // 2],
         markov_ms=[1e3 * x for x in tm], value_ms=[1e3 * x for x in tv], handle_growth_bytes=int(free0 - free1), workspace_built=bool(built),
         failed=int((info != 0).sum()))


def main():
    import gpcc_amd
    if "--profile-run" in sys.argv:
        data, delays, alpha, rho = sweep(4096, 1024)
        with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
            for _ in range(4):
                obj.loglik_grad_markov_batch(delays, alpha, rho)
        return 0
    quick = "--quick" in sys.argv
    emit(what="build", info=gpcc_amd.build_info())
    ratio = both("headline", 4096, 1024, gpcc_amd.matern32, 4, 1)
    emit(what="floor", shape="headline", ratio=ratio, floor=FLOOR, holds=bool(ratio >= FLOOR))
    if not quick:
        both("mid batch", 2048, 256, gpcc_amd.matern32, 8, 2)
        both("README size batch", 110, 1000, gpcc_amd.matern32, 20, 200)
        for N in (110, 1024, 4096):
            both("single evaluation", N, 1, gpcc_amd.matern32, 20, 20)
        markov_only("no dense gradient", 16384, 64, gpcc_amd.matern52, 2)
    if "--log" in sys.argv:
        path = sys.argv[sys.argv.index("--log") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tools/markov_grad_bench.py: gpcc_loglik_grad_markov_batch against gpcc_loglik_grad_batch, same inputs, same run (MI355X);\n"
                    "# per path 5 alternating windows of `calls_per_window` blocking calls, median window; build %s\n" % gpcc_amd.build_info())
            f.write("\n".join(LINES) + "\n")
    return 0 if ratio >= FLOOR else 1


if __name__ == "__main__":
    sys.exit(main())
