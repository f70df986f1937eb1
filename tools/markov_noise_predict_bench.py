#!/usr/bin/env python3
"""Times the four post-fit entries under a per-row noise model (gpcc_predict_noise_markov_batch, gpcc_heldout_loglik_noise_markov_batch,
gpcc_posterior_offsets_noise_markov_batch, gpcc_loo_noise_markov_batch) against their plain counterparts and against
the loop they replace, same inputs, same run; prints one JSON line per measurement.  A measurement, not a gate: every ratio is stated
whatever it is.

  python tools/markov_noise_predict_bench.py [--log profiles/markov/noise_predict_bench.log] [--quick]
      README size: N = 110, OU, 101 delays, T = 2 x 201;  N = 4096, Matern-3/2, 64 rows, T = 2 x 512;  N = 16384, Matern-5/2, 64 rows,
      T = 2 x 512.  For each size and each of the four entries (all with the mixture's weights):
      (a) the noise entry at kappa = 1, nu = 0 against the plain entry on the same rows (bitwise the same numbers): what the feature
          costs -- one fma and two LDS reads a step, 16 L more bytes of LDS a lane
      (b) the noise entry on rows that each carry their own noise model
      (c) the loop it replaces: per row a fresh handle on effective_std, one plain one-row call, close, and the mixture on the host

Timing: host wall clock around blocking calls; each size runs in a fresh process of its own.  The entries: after a warm-up call of each,
5 alternating windows of `calls` calls, median window.  The loop is timed whole, `loops` times, median."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from markov_grad_bench import WINDOWS, alternate, sweep  # noqa: E402

LINES = []
ENTRIES = ("predict", "heldout", "postb", "loo")


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    LINES.append(line)


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def measure(name, N, M, kernel, Tl, calls, loops):
    import gpcc_amd
    from gpcc_amd import fit
    (t, y, s), delays, alpha, rho = sweep(N, M)
    L = 2
    rg = np.random.default_rng(N)
    kappa = rg.uniform(0.5, 2.0, (M, L))
    nu = rg.uniform(0.0, 1.0, (M, L)) * np.array([np.mean(a ** 2) for a in s])
    one, zero = np.ones((M, L)), np.zeros((M, L))
    hi = max(np.max(a) for a in t)
    tt = [np.linspace(-0.02 * hi, 1.02 * hi, Tl) for _ in range(L)]
    yt = [np.mean(y[l]) + np.std(y[l]) * rg.standard_normal(Tl) for l in range(L)]
    st = [np.full(Tl, float(np.mean(s[l]))) for l in range(L)]
    w = rg.uniform(0.1, 1.0, M)
    p = w / w.sum()
    loo_out = ("lp", "loo", "mix_lp", "mix_loo", "loglik", "info")

    def plain(obj, e, d, a, r, stt, ww):
        if e == "predict":
            return obj.predict_markov_batch(d, a, r, tt, weights=ww)
        if e == "heldout":
            return obj.heldout_loglik_markov_batch(d, a, r, tt, yt, stt, weights=ww)
        if e == "postb":
            return obj.posterior_offsets_markov_batch(d, a, r)
        return obj.loo_markov_batch(d, a, r, weights=ww, outputs=loo_out if ww is not None else ("lp", "loo", "loglik", "info"))

    def noise(obj, e, k, v):
        if e == "predict":
            return obj.predict_markov_noise_batch(delays, alpha, rho, tt, k, v, weights=w)
        if e == "heldout":
            return obj.heldout_loglik_markov_noise_batch(delays, alpha, rho, tt, yt, st, k, v, weights=w)
        if e == "postb":
            return obj.posterior_offsets_markov_noise_batch(delays, alpha, rho, k, v)
        return obj.loo_markov_noise_batch(delays, alpha, rho, k, v, weights=w, outputs=loo_out)

    def loop(e):
        """Per row a fresh handle on its effective error bars and one plain call; the mixture on the host -> the headline number."""
        rows = []
        for m in range(M):
            with gpcc_amd.Objective(t, y, fit.effective_std(s, kappa[m], nu[m]), kernel) as fresh:
                rows.append(plain(fresh, e, delays[m:m + 1], alpha[m:m + 1], rho[m:m + 1], fit.effective_std(st, kappa[m], nu[m]), None))
        if e == "predict":
            mu, var = np.stack([r_[0][0] for r_ in rows]), np.stack([r_[1][0] for r_ in rows])
            mean = p @ mu
            return mean, p @ (var + (mu - mean) ** 2)
        if e == "heldout":
            x = np.log(p) + np.array([r_[0][0] for r_ in rows])
            return x.max() + np.log(np.sum(np.exp(x - x.max())))
        if e == "postb":
            return np.stack([r_[0][0] for r_ in rows])
        x = np.log(p)[:, None] - np.stack([r_.lp[0] for r_ in rows])
        return float(np.sum(-(x.max(axis=0) + np.log(np.sum(np.exp(x - x.max(axis=0)), axis=0)))))

    with gpcc_amd.Objective(t, y, s, kernel) as obj:
        fns = []
        for e in ENTRIES:
            fns += [lambda e=e: noise(obj, e, one, zero), lambda e=e: plain(obj, e, delays, alpha, rho, st, w), lambda e=e: noise(obj, e, kappa, nu)]
        times = alternate(fns, [calls] * len(fns))
        got = {e: noise(obj, e, kappa, nu) for e in ENTRIES}
        unit = {e: noise(obj, e, one, zero) for e in ENTRIES}
        base = {e: plain(obj, e, delays, alpha, rho, st, w) for e in ENTRIES}
    head = {"predict": lambda r_: (r_[4], r_[5]), "heldout": lambda r_: r_[3], "postb": lambda r_: r_[0], "loo": lambda r_: r_.mix_loo}
    for i, e in enumerate(ENTRIES):
        tu, tp, tn = times[3 * i], times[3 * i + 1], times[3 * i + 2]
        tl = []
        for _ in range(loops):
            t0 = time.perf_counter()
            ref = loop(e)
            tl.append(time.perf_counter() - t0)
        a, b = np.concatenate([np.ravel(x) for x in np.atleast_1d(head[e](got[e]))]), np.concatenate([np.ravel(x) for x in np.atleast_1d(ref)])
        fields = (lambda r_: [getattr(r_, f) for f in loo_out]) if e == "loo" else (lambda r_: list(r_))
        bitwise = all(np.array_equal(np.asarray(x), np.asarray(z), equal_nan=True) for x, z in zip(fields(unit[e]), fields(base[e])))
        emit(what=name, entry=e, N=N, M=M, T=L * Tl, kernel=kernel.name, noise_unit_ms=[1e3 * x for x in tu], plain_ms=[1e3 * x for x in tp],
             noise_ms=[1e3 * x for x in tn], loop_ms=[1e3 * x for x in sorted(tl)], ratio_noise_unit_over_plain=med(tu) / med(tp),
             ratio_noise_over_plain=med(tn) / med(tp), ratio_loop_over_noise=med(tl) / med(tn), calls_per_window=calls, windows=WINDOWS,
             loops=loops, unit_noise_bitwise_plain=bool(bitwise), max_rel_diff_from_the_loop=float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))))


def jobs(quick):
    import gpcc_amd
    out = [lambda: measure("README size", 110, 101, gpcc_amd.OU, 201, 20, 1)]
    if not quick:
        out += [lambda: measure("N = 4096, 64 rows", 4096, 64, gpcc_amd.matern32, 512, 5, 1),
                lambda: measure("N = 16384, 64 rows", 16384, 64, gpcc_amd.matern52, 512, 3, 1)]
    return out


def main():
    import subprocess
    import gpcc_amd
    quick = "--quick" in sys.argv
    if "--child" in sys.argv:
        jobs(quick)[int(sys.argv[sys.argv.index("--child") + 1])]()
        return 0
    emit(what="build", info=gpcc_amd.build_info())
    for k in range(len(jobs(quick))):               # one fresh process per size, one after the other (tools/markov_noise_bench.py)
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(k)] + (["--quick"] if quick else []),
                             stdout=subprocess.PIPE, text=True)
        for line in run.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                LINES.append(line)
        if run.returncode:
            return run.returncode
    if "--log" in sys.argv:
        path = sys.argv[sys.argv.index("--log") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# tools/markov_noise_predict_bench.py: the four noise-model post-fit entries at kappa = 1, nu = 0 against their plain "
                    "counterparts, on rows with their own noise model, and against the loop of fresh handles on effective_std with host "
                    "mixing, same inputs, same run (MI355X);\n# entries: 5 alternating windows of `calls_per_window` blocking calls, median "
                    "window; the loop: timed whole, `loops` times; build %s\n" % gpcc_amd.build_info())
            f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
