#!/usr/bin/env python3
"""Rates of the linear-time joint posterior draws (gpcc_sample_markov_batch) against the dense draws (gpcc_sample_batch) on the same
inputs in the same run, the two paths alternating; prints one JSON line per measurement.

  python tools/markov_sample_bench.py [--log profiles/markov/sample_bench.log] [--quick]
      README size   N = 110, 101 weighted delays, T = 2 x 201, 10 000 mixture draws
      N = 4096      L = 2, T = 2 x 512, 4096 mixture draws over 64 weighted rows
      N = 16384     Matern-5/2, the same test set and draws (no dense fp64 counterpart: alone)
  python tools/markov_sample_bench.py --profile-run     the N = 4096 call after a warm-up, for rocprofv3 --kernel-trace --stats

Timing: a warm-up of every timed shape, then `rounds` rounds of (a window of linear-time calls, a window of dense calls), each window at
least `window` seconds of blocking calls; the median over the rounds of the windows' mean time per call."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from markov_predict_bench import LINES, alternate, emit, sweep


def draws(name, Nl, M, T, S, kernel, rounds, seconds, dense=True, **kw):
    import gpcc_amd
    data, delays, alpha, rho = sweep(Nl, M, **kw)
    hi = max(np.max(a) for a in data[0])
    tt = [np.linspace(-0.02 * hi, 1.02 * hi, T)] * len(Nl)
    w = np.exp(-0.5 * ((np.arange(M) - 0.4 * M) / (0.2 * M)) ** 2)
    with gpcc_amd.Objective(*data, kernel) as obj:
        fast = lambda: obj.sample_markov_batch(delays, alpha, rho, tt, S, 1, weights=w)
        slow = (lambda: obj.sample_batch(delays, alpha, rho, tt, S, 1, weights=w, fallback=False)) if dense else None
        tf, ts, af, as_ = alternate(fast, slow, rounds, seconds)
        rf = fast()
        drawn = int((rf[3] != -14).sum())
        same_rows, mean_gap = None, None
        if dense:
            rs = slow()
            same_rows = bool(np.array_equal(rf[1], rs[1]))
            mean_gap = float(np.max(np.abs(rf[0].mean(0) - rs[0].mean(0))))
    emit(what="draws: " + name, N=int(sum(Nl)), M=M, T=T * len(Nl), S=S, kernel=kernel.name, rows_drawn=drawn,
         markov_ms_per_call=1e3 * tf, dense_ms_per_call=(1e3 * ts if dense else None), ratio=(ts / tf if dense else None),
         markov_draws_per_s=S / tf, dense_draws_per_s=(S / ts if dense else None), markov_ms_rounds=[1e3 * x for x in af],
         dense_ms_rounds=[1e3 * x for x in as_], same_draw_rows=same_rows, max_gap_of_the_draws_means=mean_gap,
         failed=int(((rf[3] != 0) & (rf[3] != -14)).sum()))


def main():
    import gpcc_amd
    if "--profile-run" in sys.argv:
        data, delays, alpha, rho = sweep([2048, 2048], 64)
        hi = max(np.max(a) for a in data[0])
        tt = [np.linspace(-0.02 * hi, 1.02 * hi, 512)] * 2
        w = np.exp(-0.5 * ((np.arange(64) - 0.4 * 64) / (0.2 * 64)) ** 2)
        with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
            for _ in range(3):
                obj.sample_markov_batch(delays, alpha, rho, tt, 4096, 1, weights=w)
        return
    quick = "--quick" in sys.argv
    rounds, seconds = (2, 0.3) if quick else (5, 1.0)
    emit(what="build", info=gpcc_amd.build_info())
    draws("README size", [60, 50], 101, 201, 10000, gpcc_amd.OU, rounds, seconds, gap_band=1, span=20.0)
    draws("N = 4096", [2048, 2048], 64, 512, 4096, gpcc_amd.matern32, rounds, seconds)
    draws("N = 16384 (no dense fp64 counterpart)", [8192, 8192], 64, 512, 4096, gpcc_amd.matern52, rounds, seconds, dense=False)
    if "--log" in sys.argv:
        path = sys.argv[sys.argv.index("--log") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tools/markov_sample_bench.py: the linear-time draws against the dense draws, same inputs, same run, alternating "
                    "windows (MI355X)\n")
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
