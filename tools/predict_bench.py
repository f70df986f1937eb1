#!/usr/bin/env python3
"""Rates of gpcc_predict_batch (the posterior predictive at a batch of delays and its delay average) on the device; prints one JSON line.

  python tools/predict_bench.py                  rows/s at N = 4096, L = 2, M = 64, T = 2 x 512 (Matern-3/2, fp64, with weights), and
                                                 the README sweep (N = 110, 101 delays, T = 2 x 201, OU): one call against the loop of
                                                 Objective.predict it replaces
  python tools/predict_bench.py --profile-run    one N = 4096 batch of 64 after a warm-up batch of 8, for rocprofv3 --kernel-trace --stats
                                                 (run it under the profiler on its own)
  python tools/predict_bench.py --kernel-stats <kernel_stats.csv>
                                                 each kernel's time per row from such a run and, for gpcc_pred_tiles, its fraction of the
                                                 fp64 matrix peak by the MFMA flops it issues (counted below from the shapes)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FP64_MFMA_PEAK_TFLOPS = 78.6   # MI355X fp64 matrix peak (vendor sheet, as bench.py)
MFMA_FLOPS = 2 * 16 * 16 * 4   # one v_mfma_f64_16x16x4_f64
PROFILE_N, PROFILE_M, PROFILE_WARM, PROFILE_T = 4096, 64, 8, 512
KERNELS = ("gpcc_pred_tiles", "gpcc_pred_finish", "gpcc_pred_mix", "gpcc_grad_trtri", "gpcc_grad_copy", "gpcc_grad_w",
           "gpcc_panel_update", "gpcc_diag_factor", "gpcc_panel_trsm", "gpcc_assemble_tiles")


def pred_tiles_flops(nt, ntT):
    """MFMA flops gpcc_pred_tiles issues per row: per (I, J), I full tiles of X (8 waves x 32 k-steps x 8 MFMAs) and the triangular
    X_II (wave w: 4 (w + 1) k-steps x 8 MFMAs) -- csrc/gpcc_pred.hip.h."""
    per_j = sum(I * 8 * 32 * 8 + sum(4 * (w + 1) * 8 for w in range(8)) for I in range(nt))
    return per_j * ntT * MFMA_FLOPS


def problem(N, M, T, seed=1):
    from gpcc_amd import synthetic
    t, y, s, _ = synthetic.simulate_lightcurves([N // 2, N - N // 2], seed=seed)
    alpha, rho = synthetic.default_hyperparameters(y)
    grid = np.linspace(0.0, 20.0, M)
    delays = np.stack([np.zeros(M), grid], 1)
    span = max(float(np.max(a)) for a in t)
    tt = np.linspace(-5.0, span + 5.0, T)
    w = np.exp(-0.5 * ((grid - 2.0) / 2.0) ** 2)
    return (t, y, s), delays, np.tile(alpha, (M, 1)), np.full(M, rho), [tt, tt], w


def main():
    import gpcc_amd
    if "--kernel-stats" in sys.argv:
        import csv
        path = sys.argv[sys.argv.index("--kernel-stats") + 1]
        rows = PROFILE_M + PROFILE_WARM   # (the trace holds both batches)
        flops = pred_tiles_flops(PROFILE_N // 128, 2 * PROFILE_T // 128)
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
            if k == "gpcc_pred_tiles":
                tf = flops * rows / (e["total_ms"] * 1e-3) / 1e12
                e["mfma_tflops"] = round(tf, 2)
                e["frac_fp64_peak"] = round(tf / FP64_MFMA_PEAK_TFLOPS, 4)
            e["total_ms"] = round(e["total_ms"], 3)
        print(json.dumps({"build": gpcc_amd.build_info(), "N": PROFILE_N, "T": 2 * PROFILE_T, "rows": rows, "kernels": out}))
        return
    if "--profile-run" in sys.argv:
        d, delays, alpha, rho, tt, w = problem(PROFILE_N, PROFILE_M, PROFILE_T)
        with gpcc_amd.Objective(*d, gpcc_amd.matern32) as obj:
            k = PROFILE_WARM
            obj.predict_batch(delays[:k], alpha[:k], rho[:k], tt, weights=w[:k])
            obj.predict_batch(delays, alpha, rho, tt, weights=w)
        return
    res = {"build": gpcc_amd.build_info(), "precision": "fp64"}
    d, delays, alpha, rho, tt, w = problem(4096, 64, 512)
    with gpcc_amd.Objective(*d, gpcc_amd.matern32) as obj:
        obj.predict_batch(delays, alpha, rho, tt, weights=w)   # warm-up (buffers, code objects)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            obj.predict_batch(delays, alpha, rho, tt, weights=w)
            ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        obj.loglik_grad_batch(delays, alpha, rho)
        tg = time.perf_counter() - t0
    res["n4096"] = {"N": 4096, "L": 2, "M": 64, "T": 1024, "kernel": "matern32", "rows_per_s": round(64 / float(np.median(ts)), 1),
                    "call_ms_median": round(1e3 * float(np.median(ts)), 2), "value_and_grad_per_s": round(64 / tg, 1),
                    "target_rows_per_s": 500.0}
    from gpcc_amd import synthetic
    t, y, s, _ = synthetic.simulate_lightcurves([60, 50], seed=1, gap_band=1, span=20.0)
    alpha0, rho0 = synthetic.default_hyperparameters(y)
    grid = np.arange(0.0, 20.01, 0.2)
    G = len(grid)
    delays = np.stack([np.zeros(G), grid], 1)
    alpha, rho = np.tile(alpha0, (G, 1)), np.full(G, rho0)
    tq = np.linspace(-1.0, 21.0, 201)
    w = np.exp(-0.5 * ((grid - 2.0) / 1.0) ** 2)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        obj.predict_batch(delays, alpha, rho, [tq, tq], weights=w)
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            obj.predict_batch(delays, alpha, rho, [tq, tq], weights=w)
            ts.append(time.perf_counter() - t0)
        obj.predict(delays[0], alpha[0], rho[0], [tq, tq])
        t0 = time.perf_counter()
        for g in range(G):
            obj.predict(delays[g], alpha[g], rho[g], [tq, tq])
        tl = time.perf_counter() - t0
    res["readme_sweep"] = {"N": 110, "delays": G, "T": 402, "kernel": "OU", "call_ms_median": round(1e3 * float(np.median(ts)), 3),
                           "predict_loop_ms": round(1e3 * tl, 2), "speedup": round(tl / float(np.median(ts)), 1),
                           "target_call_ms": 2.0, "target_speedup": 10.0}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
