#!/usr/bin/env python3
"""Rates of gpcc_sample_batch (joint posterior draws of the light curves, per row or mixed over the delay posterior) on the device;
prints one JSON line.

  python tools/sample_bench.py                   the README size (N = 110 in two bands, 101 delays weighted by getprobabilities of a
                                                 gpcc_grid fit, T = 2 x 201, S = 10 000 mixture draws, OU): one call against the host
                                                 loop of Objective.predict + numpy Cholesky + matmul over the drawn rows; and the large
                                                 case (N = 4096, L = 2, 64 rows of positive weight, T = 2 x 512, S = 4096, Matern-3/2):
                                                 factorised rows/s end to end
  python tools/sample_bench.py --profile-run     per-row mode, M = 8, S = 1024, N = 4096, T = 2 x 512, after a warm-up call, for
                                                 rocprofv3 --kernel-trace --stats (run it under the profiler on its own)
  python tools/sample_bench.py --kernel-stats <kernel_stats.csv>
                                                 gpcc_sample_tiles' share of the fp64 matrix peak from such a run"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

PROFILE_M, PROFILE_S, PROFILE_T = 8, 1024, 1024
FP64_MATRIX_PEAK = 78.6e12   # MI355X: dense fp64 matrix FLOP/s
KERNELS = ("gpcc_sample_tiles", "gpcc_sample_mean", "gpcc_heldout_finish", "gpcc_panel_update", "gpcc_diag_factor", "gpcc_panel_trsm",
           "gpcc_assemble_tiles")


def large_problem(N=4096, M=64, seed=1):
    from gpcc_amd import synthetic
    t, y, s, _ = synthetic.simulate_lightcurves([N // 2, N - N // 2], seed=seed)
    alpha, rho = synthetic.default_hyperparameters(y)
    grid = np.linspace(0.0, 20.0, M)
    delays = np.stack([np.zeros(M), grid], 1)
    w = np.exp(-0.5 * ((grid - 2.0) / 4.0) ** 2)
    span = max(float(np.max(a)) for a in t)
    tt = [np.linspace(0.0, span, 512), np.linspace(0.0, span, 512)]
    return (t, y, s), delays, np.tile(alpha, (M, 1)), np.full(M, rho), w, tt


def tiles_flops(T, S, M):
    """MFMA FLOPs of gpcc_sample_tiles: per row, test tile J and 128-draw block, sum_{K <= J} a 128 x 128 x 128 product (the diagonal
    tile counted whole, as the waves' bounds round it)."""
    ntT = (T + 127) // 128
    nblk = (S + 127) // 128
    return M * nblk * sum(J + 1 for J in range(ntT)) * 2 * 128 ** 3


def main():
    import gpcc_amd
    from gpcc_amd import fit, synthetic
    if "--kernel-stats" in sys.argv:
        import csv
        path = sys.argv[sys.argv.index("--kernel-stats") + 1]
        out = {}
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                for k in KERNELS:
                    if k in name:
                        e = out.setdefault(k, {"calls": 0, "total_ms": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_ms"] += float(row["TotalDurationNs"]) * 1e-6
        res = {"build": gpcc_amd.build_info(), "N": 4096, "T": PROFILE_T, "M": PROFILE_M, "S": PROFILE_S, "kernels": out}
        if "gpcc_sample_tiles" in out:
            e = out["gpcc_sample_tiles"]
            calls = 2   # the warm-up call and the measured one run the same work
            per_call_s = e["total_ms"] * 1e-3 / calls
            fl = tiles_flops(PROFILE_T, PROFILE_S, PROFILE_M)
            res["sample_tiles"] = {"ms_per_call": round(1e3 * per_call_s, 3), "tflops": round(fl / per_call_s / 1e12, 2),
                                   "share_of_fp64_matrix_peak": round(fl / per_call_s / FP64_MATRIX_PEAK, 3), "target_share": 0.3}
        print(json.dumps(res))
        return
    data, delays, alpha, rho, w, tt = large_problem()
    if "--profile-run" in sys.argv:
        k = PROFILE_M
        with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
            for _ in range(2):
                obj.sample_batch(delays[:k], alpha[:k], rho[:k], tt, PROFILE_S, seed=1, fallback=False)
        return
    res = {"build": gpcc_amd.build_info(), "precision": "fp64"}
    # README size
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    grid = np.arange(0.0, 20.01, 0.2)
    cand = np.stack([np.zeros_like(grid), grid], 1)
    fr = fit.gpcc_grid(t, y, s, kernel=gpcc_amd.OU, candidatedelays=cand, iterations=1000, rhomin=0.1, rhomax=20.0)
    p = gpcc_amd.getprobabilities(fr.loglikel)
    tg = np.linspace(-2.0, 22.0, 201)
    bands = [tg, tg]
    S = 10000
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        obj.sample_batch(cand, fr.alpha, fr.rho, bands, S, 1, weights=p, fallback=False)
        ts = []
        for i in range(20):
            t0 = time.perf_counter()
            _, rows, _, _ = obj.sample_batch(cand, fr.alpha, fr.rho, bands, S, 1 + i, weights=p, fallback=False)
            ts.append(time.perf_counter() - t0)
        drawn = np.unique(rows)
        # the host loop it replaces: per drawn row, the dense predictive, a numpy Cholesky and the product with its normals
        from gpcc_amd import rng
        z = rng.normals(1, 2 * len(tg), np.arange(S), rng.MIXROW)
        t0 = time.perf_counter()
        for m in drawn:
            mu, Sig = obj.predict(cand[m], fr.alpha[m], fr.rho[m], bands)
            sel = rows == m
            mu[None, :] + z[sel] @ np.linalg.cholesky(Sig).T
        tl = time.perf_counter() - t0
    res["readme"] = {"N": 110, "T": 402, "delays": len(grid), "drawn_rows": int(len(drawn)), "S": S, "kernel": "OU",
                     "call_ms_median": round(1e3 * float(np.median(ts)), 3), "host_loop_ms": round(1e3 * tl, 2),
                     "speedup": round(tl / float(np.median(ts)), 1), "target_call_ms": 3.0, "target_speedup": 30.0}
    # large: 64 rows of positive weight, S = 4096 mixture draws
    S = 4096
    with gpcc_amd.Objective(*data, gpcc_amd.matern32) as obj:
        obj.sample_batch(delays, alpha, rho, tt, S, 1, weights=w, fallback=False)
        ts = []
        for i in range(3):
            t0 = time.perf_counter()
            _, rows, _, info = obj.sample_batch(delays, alpha, rho, tt, S, 2 + i, weights=w, fallback=False)
            ts.append(time.perf_counter() - t0)
        nrows = int((info != -14).sum())
    res["n4096"] = {"N": 4096, "T": 1024, "L": 2, "M": len(rho), "factorised_rows": nrows, "S": S, "kernel": "matern32",
                    "call_ms_median": round(1e3 * float(np.median(ts)), 2),
                    "rows_per_s": round(nrows / float(np.median(ts)), 1), "target_rows_per_s": 800.0}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
