#!/usr/bin/env python3
"""Cost of the exact leave-one-out entries (gpcc_loo_batch, gpcc_loo_markov_batch) against the calls they sit beside, on the same inputs
in the same run, the two sides alternating; prints one JSON line per measurement.

  python tools/loo_bench.py [--log profiles/loo/loo_bench.log] [--quick]
      dense         gpcc_loo_batch against gpcc_loglik_grad_batch on the same rows (it runs that call's launches without
                    gpcc_grad_tiles, plus one read of X): N = 4096, L = 2, 64 rows; README size N = 110, 101 rows
      linear time   gpcc_loo_markov_batch against gpcc_predict_markov_batch with the training times as test points (T = N: about the
                    same work): N = 4096, 64 rows; N = 16384, Matern-5/2, 64 rows
      today         what a user must do without the entries, once, at the README size: N handles with one point removed each, and a
                    held-out call of the 101 delays on each
  python tools/loo_bench.py --only linear     the linear-time pair alone, in a process that has held no dense handle (after
                                              a dense N = 4096 handle in the same process the linear-time call is 4x slower; open)
  python tools/loo_bench.py --profile-run     the two N = 4096 calls, three times, for rocprofv3 --kernel-trace --stats
                                              (gpcc_loo_diag reads 67 MB per row there: its achieved bandwidth)

Timing: a warm-up of every timed shape, then `rounds` rounds of (a window of leave-one-out calls, a window of the other call), each
window at least `window` seconds of blocking calls; the median over the rounds of the windows' mean time per call."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LINES = []


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    LINES.append(line)


def sweep(Nl, M, seed=1, **kw):
    from gpcc_amd import synthetic
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=seed, **kw)
    alpha, rho = synthetic.default_hyperparameters(y)
    grid = np.linspace(0.0, 20.0, M)
    return (t, y, s), np.stack([np.zeros(M), grid], 1), np.tile(alpha, (M, 1)), np.full(M, rho)


def window(fn, seconds, max_calls):
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds or n >= max_calls:
            return dt / n


def alternate(a, b, rounds, seconds, max_calls=100000):
    a()
    b()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(a, seconds, max_calls))
        tb.append(window(b, seconds, max_calls))
    return float(np.median(ta)), float(np.median(tb)), ta, tb


def dense(name, Nl, M, kernel, rounds, seconds, **kw):
    import gpcc_amd
    data, delays, alpha, rho = sweep(Nl, M, **kw)
    w = np.ones(M)
    with gpcc_amd.Objective(*data, kernel) as obj:
        loo = lambda: obj.loo_batch(delays, alpha, rho, weights=w)
        grad = lambda: obj.loglik_grad_batch(delays, alpha, rho)
        tl, tg, al, ag = alternate(loo, grad, rounds, seconds)
        res, (gl, _, gi) = loo(), grad()
    N = int(sum(Nl))
    emit(what="dense: " + name, N=N, M=M, kernel=kernel.name, loo_ms_per_call=1e3 * tl, grad_ms_per_call=1e3 * tg, loo_over_grad=tl / tg,
         loo_ms_rounds=[1e3 * x for x in al], grad_ms_rounds=[1e3 * x for x in ag], loglik_bitwise=bool(np.array_equal(res.loglik, gl)),
         failed=int((res.info != 0).sum()), diag_read_MB_per_row=8e-6 * N * (N + 128) / 2)


def linear(name, Nl, M, kernel, rounds, seconds, **kw):
    import gpcc_amd
    data, delays, alpha, rho = sweep(Nl, M, **kw)
    w = np.ones(M)
    tt = [np.asarray(a, np.float64) for a in data[0]]
    with gpcc_amd.Objective(*data, kernel) as obj:
        loo = lambda: obj.loo_markov_batch(delays, alpha, rho, weights=w)
        pred = lambda: obj.predict_markov_batch(delays, alpha, rho, tt, weights=w)
        tl, tp, al, ap = alternate(loo, pred, rounds, seconds)
        res = loo()
    emit(what="linear time: " + name, N=int(sum(Nl)), M=M, T=int(sum(Nl)), kernel=kernel.name, loo_ms_per_call=1e3 * tl,
         predict_ms_per_call=1e3 * tp, loo_over_predict=tl / tp, loo_ms_rounds=[1e3 * x for x in al],
         predict_ms_rounds=[1e3 * x for x in ap], failed=int((res.info != 0).sum()))


def today(rounds):
    """N = 110 handles with one point removed each plus a held-out call of the 101 delays on each, once; against one gpcc_loo_batch
    and one gpcc_loo_markov_batch of the same rows (median of `rounds` calls)."""
    import gpcc_amd
    data, delays, alpha, rho = sweep([60, 50], 101, gap_band=1, span=20.0)
    t, y, s = data
    N = 110
    lp = np.empty((101, N))
    t0 = time.perf_counter()
    i = 0
    for l in range(2):
        for j in range(len(t[l])):
            keep = np.arange(len(t[l])) != j
            tr = [[a[keep] if b == l else a for b, a in enumerate(arrs)] for arrs in (t, y, s)]
            te = [[a[j:j + 1] if b == l else a[:0] for b, a in enumerate(arrs)] for arrs in (t, y, s)]
            with gpcc_amd.Objective(*tr, gpcc_amd.OU) as obj:
                lp[:, i] = obj.heldout_loglik_batch(delays, alpha, rho, *te)[0]
            i += 1
    t_today = time.perf_counter() - t0
    with gpcc_amd.Objective(*data, gpcc_amd.OU) as obj:
        obj.loo_batch(delays, alpha, rho)
        obj.loo_markov_batch(delays, alpha, rho)
        td, tm = [], []
        for _ in range(rounds):
            t0 = time.perf_counter()
            res = obj.loo_batch(delays, alpha, rho)
            td.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            obj.loo_markov_batch(delays, alpha, rho)
            tm.append(time.perf_counter() - t0)
    # (the removed-point fits centre the band on its own mean and take the offsets' prior from its own variance, and the held-out
    # score adds JITTER: the two are the same quantity only up to those)
    emit(what="today: N one-point-removed handles + held-out calls, README size (N = 110, 101 delays)", today_ms=1e3 * t_today,
         loo_batch_ms=1e3 * float(np.median(td)), loo_markov_batch_ms=1e3 * float(np.median(tm)),
         speedup_dense=t_today / float(np.median(td)), speedup_linear=t_today / float(np.median(tm)),
         max_abs_diff_lp=float(np.max(np.abs(lp - res.lp))))


def main():
    import gpcc_amd
    if "--profile-run" in sys.argv:
        data, delays, alpha, rho = sweep([2048, 2048], 64)
        with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
            for _ in range(3):
                obj.loo_batch(delays, alpha, rho, weights=np.ones(64))
                obj.loo_markov_batch(delays, alpha, rho, weights=np.ones(64))
        return
    quick = "--quick" in sys.argv
    rounds, seconds = (2, 0.3) if quick else (5, 1.0)
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    emit(what="build", info=gpcc_amd.build_info())
    if only in (None, "dense"):
        dense("N = 4096", [2048, 2048], 64, gpcc_amd.matern32, rounds, seconds)
        dense("README size", [60, 50], 101, gpcc_amd.OU, rounds, seconds, gap_band=1, span=20.0)
    if only in (None, "linear"):
        linear("N = 4096", [2048, 2048], 64, gpcc_amd.matern32, rounds, seconds)
        linear("N = 16384", [8192, 8192], 64, gpcc_amd.matern52, rounds, seconds)
    if only in (None, "today"):
        today(2 if quick else 5)
    if "--log" in sys.argv:
        path = sys.argv[sys.argv.index("--log") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tools/loo_bench.py: the leave-one-out entries against the gradient call (dense) and the predictive call at T = N "
                    "(linear time), same inputs, same run, alternating windows (MI355X)\n")
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
