#!/usr/bin/env python3
"""Rates of gpcc_loglik_hess_hyper_markov_batch (the linear-time (alpha, rho) block of the Hessian of the OU / Matern kernels) against
the dense block (gpcc_loglik_hess_hyper_batch) on the same inputs in the same run; prints one JSON line per measurement.

  python tools/markov_hess_bench.py [--log profiles/markov/hess_bench.log] [--quick]
      N = 4096, Matern-3/2, L = 2, 1024 rows (the headline batch)       rows/s of both, the dense entry on 64 of the rows; floor: ratio >= 10
      one call at N = 110 / 1024 / 4096                                  latency of both
      gpcc_grid at N = 4096, 512 delays, iterations = 30, solver markov  seconds and Newton rounds per delay with evidence_solver="markov",
                                                                         and with the dense evidence on 64 of the delays
      N = 16384, Matern-5/2, 64 delays                                   ms per call and the handle's bytes (no dense Hessian fits)
  python tools/markov_hess_bench.py --profile-run     one headline batch after a warm-up, for rocprofv3 --kernel-trace --stats

Timing: host wall clock around blocking calls.  After a warm-up call of each path, `windows` (5) windows per path, the two paths
ALTERNATING; a window is `calls` calls back to back; the figure is the median window."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from markov_grad_bench import WINDOWS, alternate, sweep, window  # noqa: E402

LINES = []
FLOOR = 10.0
DENSE_ROWS = 64        # the dense entry's measured batch


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    LINES.append(line)


def med(v):
    return v[len(v) // 2]


def both(name, N, M, kernel, calls_markov, calls_dense, dense_rows=None):
    import gpcc_amd
    data, delays, alpha, rho = sweep(N, M)
    D = min(M, dense_rows or M)
    with gpcc_amd.Objective(*data, kernel) as obj:
        tm, td = alternate([lambda: obj.loglik_hess_hyper_markov_batch(delays, alpha, rho),
                            lambda: obj.loglik_hess_hyper_batch(delays[:D], alpha[:D], rho[:D])], [calls_markov, calls_dense])
        lm, gm, hm, im = obj.loglik_hess_hyper_markov_batch(delays[:D], alpha[:D], rho[:D])
        ld, gd, hd, _, idn = obj.loglik_hess_hyper_batch(delays[:D], alpha[:D], rho[:D])
    ok = (im == 0) & (idn == 0)
    scale = np.max(np.abs(hd[ok]), axis=(1, 2), keepdims=True)
    ratio = (M / med(tm)) / (D / med(td))
    emit(what=name, N=N, M=M, dense_rows=D, kernel=kernel.name, markov_rows_per_s=M / med(tm), dense_rows_per_s=D / med(td), ratio=ratio,
         markov_ms=[1e3 * x for x in tm], dense_ms=[1e3 * x for x in td], calls_per_window=[calls_markov, calls_dense], windows=WINDOWS,
         max_hess_diff_of_max_h=float(np.max(np.abs(hm[ok] - hd[ok]) / scale)), failed=int((~ok).sum()))
    return ratio


def markov_only(name, N, M, kernel, calls):
    import torch
    import gpcc_amd
    data, delays, alpha, rho = sweep(N, M)
    torch.cuda.synchronize()
    with gpcc_amd.Objective(*data, kernel) as obj:
        free0, _ = torch.cuda.mem_get_info(0)
        (tm,) = alternate([lambda: obj.loglik_hess_hyper_markov_batch(delays, alpha, rho)], [calls])
        free1, _ = torch.cuda.mem_get_info(0)
        tg = sorted(window(lambda: obj.loglik_grad_markov_batch(delays, alpha, rho), calls) for _ in range(WINDOWS))
        info = obj.loglik_hess_hyper_markov_batch(delays, alpha, rho)[3]
        built = obj.get_option("workspace_slots") != obj.get_option("slots_per_stream")
    emit(what=name, N=N, M=M, kernel=kernel.name, markov_rows_per_s=M / med(tm), markov_ms=[1e3 * x for x in tm], grad_ms=[1e3 * x for x in tg],
         handle_growth_bytes=int(free0 - free1), workspace_built=bool(built), failed=int((info != 0).sum()))


def end_to_end(N, G, iterations, kernel):
    import gpcc_amd
    from gpcc_amd import fit
    data, cand, _, _ = sweep(N, G)
    out = {}
    with gpcc_amd.Objective(*data, kernel) as obj:
        for label, es, rows in (("markov", "markov", G), ("dense", None, DENSE_ROWS)):
            fit.gpcc_grid(*data, kernel=kernel, candidatedelays=cand[:4], iterations=2, objective=obj, engine="native", solver="markov",
                          evidence="laplace", evidence_solver=es)       # warm-up: buffers and code objects
            t0 = time.perf_counter()
            fonly = fit.gpcc_grid(*data, kernel=kernel, candidatedelays=cand[:rows], iterations=iterations, objective=obj, engine="native",
                                  solver="markov")
            t1 = time.perf_counter()
            res = fit.gpcc_grid(*data, kernel=kernel, candidatedelays=cand[:rows], iterations=iterations, objective=obj, engine="native",
                                solver="markov", evidence="laplace", evidence_solver=es)
            t2 = time.perf_counter()
            out[label] = dict(delays=rows, fit_s=t1 - t0, fit_and_evidence_s=t2 - t1, evidence_s=(t2 - t1) - (t1 - t0),
                              newton_rounds_per_delay=float(np.mean(res.laplace_rounds)), converged=int((res.laplace_info == 0).sum()))
    emit(what="end to end", N=N, kernel=kernel.name, iterations=iterations, **{k + "_" + kk: vv for k, v in out.items() for kk, vv in v.items()})


def main():
    import gpcc_amd
    if "--profile-run" in sys.argv:
        data, delays, alpha, rho = sweep(4096, 1024)
        with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
            for _ in range(4):
                obj.loglik_hess_hyper_markov_batch(delays, alpha, rho)
        return 0
    quick = "--quick" in sys.argv
    emit(what="build", info=gpcc_amd.build_info())
    ratio = both("headline", 4096, 1024, gpcc_amd.matern32, 4, 1, dense_rows=DENSE_ROWS)
    emit(what="floor", shape="headline", ratio=ratio, floor=FLOOR, holds=bool(ratio >= FLOOR))
    if not quick:
        for N in (110, 1024, 4096):
            both("single evaluation", N, 1, gpcc_amd.matern32, 20, 5)
        end_to_end(4096, 512, 30, gpcc_amd.matern32)
        markov_only("no dense Hessian", 16384, 64, gpcc_amd.matern52, 2)
    if "--log" in sys.argv:
        path = sys.argv[sys.argv.index("--log") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tools/markov_hess_bench.py: gpcc_loglik_hess_hyper_markov_batch against gpcc_loglik_hess_hyper_batch, same inputs, same run "
                    "(MI355X);\n# per path 5 alternating windows of `calls_per_window` blocking calls, median window; build %s\n"
                    % gpcc_amd.build_info())
            f.write("\n".join(LINES) + "\n")
    return 0 if ratio >= FLOOR else 1


if __name__ == "__main__":
    sys.exit(main())
