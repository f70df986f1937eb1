#!/usr/bin/env python3
"""Rates of the hyper-parameter-block Hessian and of the Laplace evidence on the device; prints one JSON line.

  python tools/laplace_bench.py                 block (gpcc_loglik_hess_hyper_batch) against full (gpcc_loglik_hess_batch) Hessian
                                                evaluations/s at N = 4096, L = 2 and 3 (batches of 64, Matern-3/2); the README sweeps
                                                (N = 110 with 101 delays, N = 150 with 111 x 111 delays; iterations = 1000, OU): wall time
                                                of gpcc_grid_loglik alone and followed by gpcc_laplace_evidence, Newton rounds per delay
  python tools/laplace_bench.py --profile-run   one N = 4096 / L = 2 block batch of 64 after a warm-up batch of 8, for
                                                rocprofv3 --kernel-trace --stats (run it under the profiler on its own); the kernel split
                                                comes from tools/hess_bench.py --kernel-stats <kernel_stats.csv>"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

PROFILE_N, PROFILE_L, PROFILE_M, PROFILE_WARM = 4096, 2, 64, 8


def sweep(N, L, M):
    from gpcc_amd import synthetic
    Nl = [N // L + (1 if l < N % L else 0) for l in range(L)]
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=1)
    alpha, rho = synthetic.default_hyperparameters(y)
    grid = np.linspace(0.0, 20.0, M)
    delays = np.zeros((M, L))
    for l in range(1, L):
        delays[:, l] = grid * l
    return (t, y, s), delays, np.tile(alpha, (M, 1)), np.full(M, rho)


def rate(fn, delays, alpha, rho, reps):
    fn(delays, alpha, rho)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn(delays, alpha, rho)
    return reps * len(rho) / (time.perf_counter() - t0)


def readme_sweep(Nl, grids):
    """the README's sweep: simulated light curves, a candidate-delay grid, the native fit, then the Laplace evidence"""
    import gpcc_amd
    from gpcc_amd import synthetic
    t, y, s, _ = synthetic.simulate_lightcurves(Nl, seed=1, gap_band=1, span=20.0 if len(Nl) == 2 else None)
    mesh = np.meshgrid(*grids, indexing="ij")
    cand = np.stack([np.zeros(mesh[0].size)] + [m.ravel() for m in mesh], 1)
    with gpcc_amd.Objective(t, y, s, gpcc_amd.OU) as obj:
        obj.grid_loglik(cand[:4], 10)                     # warm-up
        obj.laplace_evidence(cand[:4], np.ones((4, len(Nl))), np.full(4, 2.0))
        t0 = time.perf_counter()
        ll, alpha, rho, info, its, _ = obj.grid_loglik(cand, 1000)
        t1 = time.perf_counter()
        _, _, _, logz, _, linfo, rounds, (evals, batches) = obj.laplace_evidence(cand, alpha, rho)
        t2 = time.perf_counter()
    codes = {str(int(c)): int((linfo == c).sum()) for c in np.unique(linfo)}
    return {"N": int(sum(Nl)), "L": len(Nl), "delays": int(len(cand)), "fit_s": round(t1 - t0, 3), "fit_plus_laplace_s": round(t2 - t0, 3),
            "laplace_s": round(t2 - t1, 3), "newton_rounds_mean": round(float(rounds.mean()), 3), "newton_rounds_max": int(rounds.max()),
            "laplace_batches": int(batches), "laplace_info_counts": codes}


def main():
    import gpcc_amd
    if "--profile-run" in sys.argv:
        d, delays, alpha, rho = sweep(PROFILE_N, PROFILE_L, PROFILE_M)
        with gpcc_amd.Objective(*d, gpcc_amd.matern32) as obj:
            obj.loglik_hess_hyper_batch(delays[:PROFILE_WARM], alpha[:PROFILE_WARM], rho[:PROFILE_WARM])
            obj.loglik_hess_hyper_batch(delays, alpha, rho)
        return
    res = {"build": gpcc_amd.build_info(), "kernel": "matern32", "precision": "fp64", "rates": [], "sweeps": []}
    targets = {(4096, 2): 70.0}
    for N, L, M, reps in ((4096, 2, 64, 2), (4096, 3, 64, 1)):
        d, delays, alpha, rho = sweep(N, L, M)
        with gpcc_amd.Objective(*d, gpcc_amd.matern32) as obj:
            b = rate(obj.loglik_hess_hyper_batch, delays, alpha, rho, reps)
            f = rate(obj.loglik_hess_batch, delays, alpha, rho, reps)
        res["rates"].append({"N": N, "L": L, "batch": M, "block_hessian_per_s": round(b, 1), "full_hessian_per_s": round(f, 1),
                             "speedup": round(b / f, 3), "target_block_per_s": targets.get((N, L))})
    res["sweeps"].append(readme_sweep([60, 50], [np.arange(0.0, 20.01, 0.2)]))
    res["sweeps"].append(readme_sweep([50, 50, 50], [np.linspace(0.0, 10.0, 111), np.linspace(0.0, 10.0, 111)]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
