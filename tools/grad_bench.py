#!/usr/bin/env python3
"""Rates of gpcc_loglik_grad_batch (value and gradient) on the device; prints one JSON line.

  python tools/grad_bench.py                 value+gradient evaluations/s (N = 4096 / 1024 delays, 2048 / 256, 110 / 1000;
                                             Matern-3/2, fp64), the value alone on the same batches, single-call latency at
                                             N = 110, 1024, 4096
  python tools/grad_bench.py --profile-run   one N = 4096 / 256-delay gradient batch after a warm-up, for
                                             rocprofv3 --kernel-trace --stats (run it under the profiler on its own)
  python tools/grad_bench.py --kernel-stats <kernel_stats.csv>
                                             each gradient kernel's time from such a run and its fraction of the fp64 matrix
                                             peak by the MFMA flops it issues (counted below from the shapes)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FP64_MFMA_PEAK_TFLOPS = 78.6   # MI355X fp64 matrix peak (vendor sheet, as bench.py)
MFMA_FLOPS = 2 * 16 * 16 * 4   # one v_mfma_f64_16x16x4_f64
PROFILE_N, PROFILE_M, PROFILE_WARM = 4096, 256, 8   # the profiled run: a warm-up batch of 8, then 256 evaluations


def mfma_flops(nt):
    """MFMA flops issued per evaluation by gpcc_grad_trtri and gpcc_grad_tiles (csrc/gpcc_grad.hip.h) for nt tile rows."""
    diag_first = sum((16 * w + 16) // 4 for w in range(8)) * 8   # k-steps x 8 MFMAs, over the 8 waves (triangular X_II)
    second = sum(4 * (8 - cb) for cb in range(8)) * 8
    trtri = 0
    for j in range(nt - 1):
        for I in range(j + 1, nt):
            trtri += (I - j - 1) * 32 * 8 * 8 + diag_first + second
    diag_tiles = sum((128 - 16 * w) // 4 for w in range(8)) * 8
    tiles = 0
    for I in range(nt):
        for J in range(I + 1):
            tiles += (nt - 1 - I) * 32 * 8 * 8 + diag_tiles
    return {"gpcc_grad_trtri": trtri * MFMA_FLOPS, "gpcc_grad_tiles": tiles * MFMA_FLOPS}


def data(N, L=2, seed=1):
    from gpcc_amd import synthetic
    Nl = [N // L + (1 if l < N % L else 0) for l in range(L)]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=seed)
    return t, y, s


def sweep(N, M):
    """A delay grid at fixed hyper-parameters (the README's sweep)."""
    from gpcc_amd import synthetic
    t, y, s = data(N)
    alpha, rho = synthetic.default_hyperparameters(y)
    grid = np.linspace(0.0, 20.0, M)
    return (t, y, s), np.stack([np.zeros(M), grid], 1), np.tile(alpha, (M, 1)), np.full(M, rho)


def rate(obj, fn, delays, alpha, rho, reps):
    fn(delays, alpha, rho)   # warm-up (workspace, code objects)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn(delays, alpha, rho)
    return reps * len(rho) / (time.perf_counter() - t0)


def main():
    import gpcc_amd
    if "--kernel-stats" in sys.argv:
        import csv
        path = sys.argv[sys.argv.index("--kernel-stats") + 1]
        nt = PROFILE_N // 128
        flops = mfma_flops(nt)
        evals = PROFILE_M + PROFILE_WARM   # (the trace holds both batches)
        out = {}
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                for k in ("gpcc_grad_trtri", "gpcc_grad_copy", "gpcc_grad_w", "gpcc_grad_tiles", "gpcc_grad_finish"):
                    if k in name:
                        ns = float(row["TotalDurationNs"])
                        e = out.setdefault(k, {"calls": 0, "total_ms": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_ms"] += ns * 1e-6
        for k, e in out.items():
            e["per_evaluation_ms"] = round(e["total_ms"] / evals, 5)
            if k in flops:
                tf = flops[k] * evals / (e["total_ms"] * 1e-3) / 1e12
                e["mfma_tflops"] = round(tf, 2)
                e["frac_fp64_peak"] = round(tf / FP64_MFMA_PEAK_TFLOPS, 4)
            e["total_ms"] = round(e["total_ms"], 3)
        print(json.dumps({"build": gpcc_amd.build_info(), "N": PROFILE_N, "evaluations": evals, "kernels": out}))
        return
    if "--profile-run" in sys.argv:
        d, delays, alpha, rho = sweep(PROFILE_N, PROFILE_M)
        with gpcc_amd.Objective(*d, gpcc_amd.matern32) as obj:
            obj.loglik_grad_batch(delays[:PROFILE_WARM], alpha[:PROFILE_WARM], rho[:PROFILE_WARM])
            obj.loglik_grad_batch(delays, alpha, rho)
        return
    res = {"build": gpcc_amd.build_info(), "kernel": "matern32", "precision": "fp64", "rates": [], "latency_ms": []}
    targets = {4096: 600.0}
    for N, M, reps in ((4096, 1024, 2), (2048, 256, 4), (110, 1000, 10)):
        d, delays, alpha, rho = sweep(N, M)
        with gpcc_amd.Objective(*d, gpcc_amd.matern32) as obj:
            g = rate(obj, obj.loglik_grad_batch, delays, alpha, rho, reps)
            v = rate(obj, obj.loglik_batch, delays, alpha, rho, reps)
        res["rates"].append({"N": N, "delays": M, "value_and_grad_per_s": round(g, 1), "value_only_per_s": round(v, 1),
                             "target_value_and_grad_per_s": targets.get(N)})
    for N, reps in ((110, 50), (1024, 20), (4096, 5)):
        d, delays, alpha, rho = sweep(N, 1)
        with gpcc_amd.Objective(*d, gpcc_amd.matern32) as obj:
            obj.loglik_grad_batch(delays, alpha, rho)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                obj.loglik_grad_batch(delays, alpha, rho)
                ts.append((time.perf_counter() - t0) * 1e3)
            tv = []
            for _ in range(reps):
                t0 = time.perf_counter()
                obj.loglik_batch(delays, alpha, rho)
                tv.append((time.perf_counter() - t0) * 1e3)
        res["latency_ms"].append({"N": N, "value_and_grad_median": round(float(np.median(ts)), 3),
                                  "value_only_median": round(float(np.median(tv)), 3)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
