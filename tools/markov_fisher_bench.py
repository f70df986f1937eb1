#!/usr/bin/env python3
"""Rates of gpcc_loglik_fisher_markov_batch (the linear-time Fisher information of the OU / Matern kernels) against the dense Hessian
entry (gpcc_loglik_hess_batch, the only dense source of the Fisher information) on the same inputs in the same run; prints one JSON
line per measurement.

  python tools/markov_fisher_bench.py [--log profiles/markov/fisher_bench.log] [--quick]
      N = 4096, Matern-3/2, L = 2, 64 rows (the headline batch)          rows/s of both; floor: ratio >= 10
      one call at N = 110 / 1024 / 4096                                  latency of both
      N = 16384, Matern-5/2, 64 delays                                   ms per call and the handle's bytes (no dense Hessian fits)

Timing: host wall clock around blocking calls.  After a warm-up call of each path, `windows` (5) windows per path, the two paths
ALTERNATING; a window is `calls` calls back to back; the figure is the median window."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from markov_grad_bench import WINDOWS, alternate, sweep, window  # noqa: E402

LINES = []
FLOOR = 10.0


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    LINES.append(line)


def med(v):
    return v[len(v) // 2]


def both(name, N, M, kernel, calls_markov, calls_dense):
    import gpcc_amd
    data, delays, alpha, rho = sweep(N, M)
    with gpcc_amd.Objective(*data, kernel) as obj:
        tm, td = alternate([lambda: obj.loglik_fisher_markov_batch(delays, alpha, rho),
                            lambda: obj.loglik_hess_batch(delays, alpha, rho)], [calls_markov, calls_dense])
        lm, gm, fm, im = obj.loglik_fisher_markov_batch(delays, alpha, rho)
        ld, gd, hd, fd, idn = obj.loglik_hess_batch(delays, alpha, rho)
    ok = (im == 0) & (idn == 0) & np.isfinite(fm).all(axis=(1, 2))
    scale = np.max(np.abs(fd[ok]), axis=(1, 2), keepdims=True)
    ratio = med(td) / med(tm)
    emit(what=name, N=N, M=M, kernel=kernel.name, markov_rows_per_s=M / med(tm), dense_rows_per_s=M / med(td), ratio=ratio,
         markov_ms=[1e3 * x for x in tm], dense_ms=[1e3 * x for x in td], calls_per_window=[calls_markov, calls_dense], windows=WINDOWS,
         max_fisher_diff_of_max_f=float(np.max(np.abs(fm[ok] - fd[ok]) / scale)), failed=int((~ok).sum()))
    return ratio


def markov_only(name, N, M, kernel, calls):
    import torch
    import gpcc_amd
    data, delays, alpha, rho = sweep(N, M)
    torch.cuda.synchronize()
    with gpcc_amd.Objective(*data, kernel) as obj:
        free0, _ = torch.cuda.mem_get_info(0)
        (tm,) = alternate([lambda: obj.loglik_fisher_markov_batch(delays, alpha, rho)], [calls])
        free1, _ = torch.cuda.mem_get_info(0)
        tg = sorted(window(lambda: obj.loglik_grad_markov_batch(delays, alpha, rho), calls) for _ in range(WINDOWS))
        fisher, info = obj.loglik_fisher_markov_batch(delays, alpha, rho)[2:]
        built = obj.get_option("workspace_slots") != obj.get_option("slots_per_stream")
    lo = float(min(np.linalg.eigvalsh(f).min() / np.max(np.abs(f)) for f in fisher[info == 0]))
    emit(what=name, N=N, M=M, kernel=kernel.name, markov_rows_per_s=M / med(tm), markov_ms=[1e3 * x for x in tm],
         grad_ms=[1e3 * x for x in tg], handle_growth_bytes=int(free0 - free1), workspace_built=bool(built),
         smallest_eigenvalue_of_max_f=lo, failed=int((info != 0).sum()))


def main():
    import gpcc_amd
    quick = "--quick" in sys.argv
    emit(what="build", info=gpcc_amd.build_info())
    ratio = both("headline", 4096, 64, gpcc_amd.matern32, 4, 1)
    emit(what="floor", shape="headline", ratio=ratio, floor=FLOOR, holds=bool(ratio >= FLOOR))
    if not quick:
        for N in (110, 1024, 4096):
            both("single evaluation", N, 1, gpcc_amd.matern32, 20, 5)
        markov_only("no dense Hessian", 16384, 64, gpcc_amd.matern52, 2)
    if "--log" in sys.argv:
        path = sys.argv[sys.argv.index("--log") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tools/markov_fisher_bench.py: gpcc_loglik_fisher_markov_batch against gpcc_loglik_hess_batch, same inputs, same run "
                    "(MI355X);\n# per path 5 alternating windows of `calls_per_window` blocking calls, median window; build %s\n"
                    % gpcc_amd.build_info())
            f.write("\n".join(LINES) + "\n")
    return 0 if ratio >= FLOOR else 1


if __name__ == "__main__":
    sys.exit(main())
