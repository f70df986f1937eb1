#!/usr/bin/env python3
"""Times gpcc_loglik_markov_multi_batch (R flux realisations per parameter row in one linear-time pass) against the route it replaces:
R fresh handles and R gpcc_loglik_markov_batch calls on the same inputs in the same run; prints one JSON line per measurement.  A
measurement, not a gate: the ratio is stated whatever it is.

  python tools/markov_multi_bench.py [--log profiles/markov/multi_bench.log] [--quick]
      README size: N = 110, OU, 101 delays, R = 1000
      N = 4096, Matern-3/2, 1024 delays, R in {1, RB, 64}      (R = 1: the cost of the pack pass over gpcc_loglik_markov_batch)
      N = 16384, Matern-5/2, 64 delays, R = 64
      ... and at R = RB the time per step of a wave against gpcc_markov_eval's (call time / N: with at most one wave per CU the
      call is N dependent steps of every wave at once)

Timing: host wall clock around blocking calls.  The new entry and one gpcc_loglik_markov_batch call on the handle: after a warm-up
call of each, 5 alternating windows of `calls` calls, median window.  The loop of fresh handles (create, call, close, per
realisation) is timed whole, `loops` times, median.  No marginalise_b and own means, so that both routes compute the same numbers;
their largest relative disagreement is printed."""
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


def measure(name, N, M, kernel, R, calls, loops):
    import gpcc_amd
    from gpcc_amd import synthetic
    (t, y, s), delays, alpha, rho = sweep(N, M)
    Y = synthetic.flux_randomise(y, s, R, seed=R)

    def loop():
        out = np.empty((M, R))
        for r in range(R):
            with gpcc_amd.Objective(t, [a[r] for a in Y], s, kernel, marginalise_b=False) as fresh:
                out[:, r] = fresh.loglik_markov_batch(delays, alpha, rho)[0]
        return out

    with gpcc_amd.Objective(t, y, s, kernel, marginalise_b=False) as obj:
        rb = obj.get_option("markov_multi_block")
        flat = obj.realisations(Y)
        tm, ts = alternate([lambda: obj.loglik_markov_realisations(flat, delays, alpha, rho),
                            lambda: obj.loglik_markov_batch(delays, alpha, rho)], [calls, calls])
        ll, info = obj.loglik_markov_realisations(flat, delays, alpha, rho)
        scratch = obj.get_option("markov_multi_bytes")
    ref = loop()
    tl = []
    for _ in range(loops):
        t0 = time.perf_counter()
        loop()
        tl.append(time.perf_counter() - t0)
    ok = info == 0
    emit(what=name, N=N, M=M, R=R, RB=int(rb), kernel=kernel.name, multi_ms=[1e3 * x for x in tm], single_call_ms=[1e3 * x for x in ts],
         loop_ms=[1e3 * x for x in sorted(tl)], cells_per_s=M * R / med(tm), ratio_loop_over_multi=med(tl) / med(tm),
         ratio_R_single_calls_over_multi=R * med(ts) / med(tm), multi_over_single_call=med(tm) / med(ts),
         step_us_multi=1e6 * med(tm) / N, step_us_eval=1e6 * med(ts) / N, scratch_bytes=int(scratch), calls_per_window=calls,
         windows=WINDOWS, loops=loops, max_rel_diff_of_the_routes=float(np.max(np.abs(ll[ok] - ref[ok]) / np.abs(ref[ok]))),
         failed=int((~ok).sum()))


def main():
    import gpcc_amd
    quick = "--quick" in sys.argv
    emit(what="build", info=gpcc_amd.build_info())
    measure("README size", 110, 101, gpcc_amd.OU, 1000 if not quick else 64, 10, 1 if quick else 3)
    if not quick:
        with gpcc_amd.Objective(*sweep(64, 1)[0], gpcc_amd.matern32, marginalise_b=False) as obj:
            rb = int(obj.get_option("markov_multi_block"))
        for R in (1, rb, 64):
            measure("N = 4096, 1024 delays", 4096, 1024, gpcc_amd.matern32, R, 4, 3)
        measure("N = 16384, 64 delays", 16384, 64, gpcc_amd.matern52, 64, 2, 3)
    if "--log" in sys.argv:
        path = sys.argv[sys.argv.index("--log") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tools/markov_multi_bench.py: gpcc_loglik_markov_multi_batch against R fresh handles and R gpcc_loglik_markov_batch calls, "
                    "same inputs, same run (MI355X);\n# multi and single call: 5 alternating windows of `calls_per_window` blocking calls, "
                    "median window; the loop: timed whole, `loops` times; build %s\n" % gpcc_amd.build_info())
            f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
