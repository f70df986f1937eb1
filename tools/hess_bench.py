#!/usr/bin/env python3
"""Rates of gpcc_loglik_hess_batch (value, gradient, Hessian and Fisher information) on the device; prints one JSON line.

  python tools/hess_bench.py                 Hessian evaluations/s at N = 4096 with L = 2 and 3 (batches of 64), at the README sizes
                                             (N = 110 with two bands, 150 with three, as simulatedata draws them; 1000 delays), and
                                             single-call latency at N = 110, 1024, 4096 (Matern-3/2, fp64)
  python tools/hess_bench.py --profile-run   one N = 4096 / L = 2 batch of 64 after a warm-up batch of 8, for
                                             rocprofv3 --kernel-trace --stats (run it under the profiler on its own)
  python tools/hess_bench.py --kernel-stats <kernel_stats.csv>
                                             each Hessian kernel's time from such a run and, for the matrix kernels, its fraction of
                                             the fp64 matrix peak by the MFMA flops it issues (counted below from the shapes)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FP64_MFMA_PEAK_TFLOPS = 78.6   # MI355X fp64 matrix peak (vendor sheet, as bench.py)
MFMA_FLOPS = 2 * 16 * 16 * 4   # one v_mfma_f64_16x16x4_f64
PROFILE_N, PROFILE_L, PROFILE_M, PROFILE_WARM = 4096, 2, 64, 8
KERNELS = ("gpcc_hess_ctab", "gpcc_hess_u", "gpcc_hess_z", "gpcc_hess_gemm", "gpcc_hess_trace", "gpcc_hess_finish",
           "gpcc_grad_trtri", "gpcc_grad_tiles", "gpcc_grad_w", "gpcc_grad_copy", "gpcc_grad_finish")


def mfma_flops(nt, L):
    """MFMA flops issued per evaluation by gpcc_hess_gemm (P nt^2 tiles, 2 x 16 k-steps of 8 MFMAs per wave per tile of K) and
    gpcc_hess_ctab (the loop of gpcc_grad_tiles) -- csrc/gpcc_hess.hip.h."""
    P = 2 * L + 1
    gemm = P * nt * nt * nt * 8 * 32 * 8
    diag_tiles = sum((128 - 16 * w) // 4 for w in range(8)) * 8
    ctab = sum((nt - 1 - I) * 32 * 8 * 8 + diag_tiles for I in range(nt) for J in range(I + 1))
    return {"gpcc_hess_gemm": gemm * MFMA_FLOPS, "gpcc_hess_ctab": ctab * MFMA_FLOPS}


def data(N, L, seed=1):
    from gpcc_amd import synthetic
    Nl = [N // L + (1 if l < N % L else 0) for l in range(L)]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=seed)
    return t, y, s


def sweep(N, L, M):
    """A delay grid at fixed hyper-parameters (the README's sweep)."""
    from gpcc_amd import synthetic
    t, y, s = data(N, L)
    alpha, rho = synthetic.default_hyperparameters(y)
    grid = np.linspace(0.0, 20.0, M)
    delays = np.zeros((M, L))
    for l in range(1, L):
        delays[:, l] = grid * l
    return (t, y, s), delays, np.tile(alpha, (M, 1)), np.full(M, rho)


def rate(fn, delays, alpha, rho, reps):
    fn(delays, alpha, rho)   # warm-up (buffers, code objects)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn(delays, alpha, rho)
    return reps * len(rho) / (time.perf_counter() - t0)


def main():
    import gpcc_amd
    if "--kernel-stats" in sys.argv:
        import csv
        path = sys.argv[sys.argv.index("--kernel-stats") + 1]
        flops = mfma_flops(PROFILE_N // 128, PROFILE_L)
        evals = PROFILE_M + PROFILE_WARM   # (the trace holds both batches)
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
            e["per_evaluation_ms"] = round(e["total_ms"] / evals, 5)
            if k in flops:
                tf = flops[k] * evals / (e["total_ms"] * 1e-3) / 1e12
                e["mfma_tflops"] = round(tf, 2)
                e["frac_fp64_peak"] = round(tf / FP64_MFMA_PEAK_TFLOPS, 4)
            e["total_ms"] = round(e["total_ms"], 3)
        print(json.dumps({"build": gpcc_amd.build_info(), "N": PROFILE_N, "L": PROFILE_L, "evaluations": evals, "kernels": out}))
        return
    if "--profile-run" in sys.argv:
        d, delays, alpha, rho = sweep(PROFILE_N, PROFILE_L, PROFILE_M)
        with gpcc_amd.Objective(*d, gpcc_amd.matern32) as obj:
            obj.loglik_hess_batch(delays[:PROFILE_WARM], alpha[:PROFILE_WARM], rho[:PROFILE_WARM])
            obj.loglik_hess_batch(delays, alpha, rho)
        return
    res = {"build": gpcc_amd.build_info(), "kernel": "matern32", "precision": "fp64", "rates": [], "latency_ms": []}
    targets = {(4096, 2): 40.0}
    for N, L, M, reps in ((4096, 2, 64, 2), (4096, 3, 64, 1), (110, 2, 1000, 5), (150, 3, 1000, 5)):
        d, delays, alpha, rho = sweep(N, L, M)
        with gpcc_amd.Objective(*d, gpcc_amd.matern32) as obj:
            h = rate(obj.loglik_hess_batch, delays, alpha, rho, reps)
            g = rate(obj.loglik_grad_batch, delays, alpha, rho, reps)
            slots = obj.get_option("hess_slots")
        res["rates"].append({"N": N, "L": L, "delays": M, "hessian_per_s": round(h, 1), "value_and_grad_per_s": round(g, 1),
                             "hess_slots": slots, "target_hessian_per_s": targets.get((N, L))})
    for N, reps in ((110, 50), (1024, 20), (4096, 5)):
        d, delays, alpha, rho = sweep(N, 2, 1)
        with gpcc_amd.Objective(*d, gpcc_amd.matern32) as obj:
            obj.loglik_hess_batch(delays, alpha, rho)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                obj.loglik_hess_batch(delays, alpha, rho)
                ts.append((time.perf_counter() - t0) * 1e3)
        res["latency_ms"].append({"N": N, "hessian_median": round(float(np.median(ts)), 3)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
