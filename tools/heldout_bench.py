#!/usr/bin/env python3
"""Rates of gpcc_heldout_loglik_batch (the held-out log-likelihood at a batch of delays and its delay average) on the device; prints one
JSON line.

  python tools/heldout_bench.py                  rows/s at N = 4096 split 5-fold (train 3276, test 820), L = 2, M = 64 (Matern-3/2,
                                                 fp64, with weights); the README size (N = 110, 101 delays, one fold's test split, OU):
                                                 one call against the loop of single-row Predictor(ttest, ytest, stest) it replaces;
                                                 and a whole 5-fold performcv_grid with iterations = 1000, split into fits and scoring
  python tools/heldout_bench.py --profile-run    one large batch of 64 after a warm-up batch of 8, for rocprofv3 --kernel-trace --stats
                                                 (run it under the profiler on its own)
  python tools/heldout_bench.py --kernel-stats <kernel_stats.csv>
                                                 each kernel's time per row from such a run"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

PROFILE_M, PROFILE_WARM = 64, 8
KERNELS = ("gpcc_heldout_finish", "gpcc_heldout_mix", "gpcc_panel_update", "gpcc_diag_factor", "gpcc_panel_trsm", "gpcc_assemble_tiles")


def split_problem(N=4096, M=64, seed=1):
    """N points in two bands split 5-fold: fold 1 of cvindices is the test set (820 points), the rest the training set (3276)."""
    from gpcc_amd import fit, synthetic
    t, y, s, _ = synthetic.simulate_lightcurves([N // 2, N - N // 2], seed=seed)
    folds = fit.cvindices([len(a) for a in t], 5, 1)
    (ttr, ytr, st), (tte, yte, ste) = fit._split(t, y, s, folds, 0)
    alpha, rho = synthetic.default_hyperparameters(ytr)
    grid = np.linspace(0.0, 20.0, M)
    delays = np.stack([np.zeros(M), grid], 1)
    w = np.exp(-0.5 * ((grid - 2.0) / 2.0) ** 2)
    return (ttr, ytr, st), (tte, yte, ste), delays, np.tile(alpha, (M, 1)), np.full(M, rho), w


def main():
    import gpcc_amd
    from gpcc_amd import fit, synthetic
    if "--kernel-stats" in sys.argv:
        import csv
        path = sys.argv[sys.argv.index("--kernel-stats") + 1]
        rows = PROFILE_M + PROFILE_WARM   # (the trace holds both batches)
        out = {}
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                for k in KERNELS:
                    if k in name:
                        e = out.setdefault(k, {"calls": 0, "total_ms": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_ms"] += float(row["TotalDurationNs"]) * 1e-6
        for k, e in out.items():
            e["per_row_ms"] = round(e["total_ms"] / rows, 5)
            e["total_ms"] = round(e["total_ms"], 3)
        tot = sum(e["per_row_ms"] for e in out.values())
        print(json.dumps({"build": gpcc_amd.build_info(), "N_train": 3276, "T": 820, "rows": rows, "kernels": out,
                          "sum_per_row_ms": round(tot, 4)}))
        return
    tr, te, delays, alpha, rho, w = split_problem()
    if "--profile-run" in sys.argv:
        with gpcc_amd.Objective(*tr, gpcc_amd.matern32) as obj:
            k = PROFILE_WARM
            obj.heldout_loglik_batch(delays[:k], alpha[:k], rho[:k], *te, weights=w[:k])
            obj.heldout_loglik_batch(delays, alpha, rho, *te, weights=w)
        return
    res = {"build": gpcc_amd.build_info(), "precision": "fp64"}
    M = len(rho)
    with gpcc_amd.Objective(*tr, gpcc_amd.matern32) as obj:
        obj.heldout_loglik_batch(delays, alpha, rho, *te, weights=w)   # warm-up (buffers, code objects)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            obj.heldout_loglik_batch(delays, alpha, rho, *te, weights=w)
            ts.append(time.perf_counter() - t0)
        slots = obj.get_option("heldout_slots")
    res["n4096_split"] = {"N_train": sum(len(a) for a in tr[0]), "T": sum(len(a) for a in te[0]), "L": 2, "M": M, "kernel": "matern32",
                          "rows_per_s": round(M / float(np.median(ts)), 1), "call_ms_median": round(1e3 * float(np.median(ts)), 2),
                          "heldout_slots": int(slots), "target_rows_per_s": 1000.0}
    # README size: one fold's split of the two-band sweep, 101 delays
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    folds = fit.cvindices([60, 50], 5, 1)
    (ttr, ytr, str_), (tte, yte, ste) = fit._split(t, y, s, folds, 0)
    alpha0, rho0 = synthetic.default_hyperparameters(ytr)
    grid = np.arange(0.0, 20.01, 0.2)
    G = len(grid)
    delays = np.stack([np.zeros(G), grid], 1)
    alpha, rho = np.tile(alpha0, (G, 1)), np.full(G, rho0)
    w = np.exp(-0.5 * ((grid - 2.0) / 1.0) ** 2)
    with gpcc_amd.Objective(ttr, ytr, str_, gpcc_amd.OU) as obj:
        obj.heldout_loglik_batch(delays, alpha, rho, tte, yte, ste, weights=w)
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            obj.heldout_loglik_batch(delays, alpha, rho, tte, yte, ste, weights=w)
            ts.append(time.perf_counter() - t0)
        fit.Predictor(obj, delays[0], alpha[0], rho[0])(tte, yte, ste)
        t0 = time.perf_counter()
        for g in range(G):
            fit.Predictor(obj, delays[g], alpha[g], rho[g])(tte, yte, ste)
        tl = time.perf_counter() - t0
    res["readme_fold"] = {"N_train": sum(len(a) for a in ttr), "T": sum(len(a) for a in tte), "delays": G, "kernel": "OU",
                          "call_ms_median": round(1e3 * float(np.median(ts)), 3), "predictor_loop_ms": round(1e3 * tl, 2),
                          "speedup": round(tl / float(np.median(ts)), 1), "target_call_ms": 1.0, "target_speedup": 30.0}
    # a whole 5-fold performcv_grid (iterations = 1000): fits against held-out scoring
    cand = delays
    tfit = [0.0]
    theld = [0.0]
    grid_fit, held_fn = fit.gpcc_grid, gpcc_amd.Objective.heldout_loglik_batch

    def timed_fit(*a, **k):
        t0 = time.perf_counter()
        r = grid_fit(*a, **k)
        tfit[0] += time.perf_counter() - t0
        return r

    def timed_held(*a, **k):
        t0 = time.perf_counter()
        r = held_fn(*a, **k)
        theld[0] += time.perf_counter() - t0
        return r

    fit.gpcc_grid, gpcc_amd.Objective.heldout_loglik_batch = timed_fit, timed_held
    try:
        t0 = time.perf_counter()
        cv = fit.performcv_grid(t, y, s, candidatedelays=cand, kernel=gpcc_amd.OU, iterations=1000)
        tcv = time.perf_counter() - t0
    finally:
        fit.gpcc_grid, gpcc_amd.Objective.heldout_loglik_batch = grid_fit, held_fn
    res["readme_performcv_grid"] = {"folds": 5, "delays": G, "iterations": 1000, "total_ms": round(1e3 * tcv, 1),
                                    "fits_ms": round(1e3 * tfit[0], 1), "heldout_ms": round(1e3 * theld[0], 2),
                                    "mix": [round(float(v), 4) for v in cv.mix]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
