// gpcc_markov_noise_sample.hip.h -- joint posterior draws in linear time of rows that each carry their own (tau, alpha, rho) AND their
// own NOISE MODEL, for gfx950: gpcc_sample_noise_markov_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py
// (sample_noise) is the same algorithm in numpy.  The model is gpcc_markov_noise.hip.h's: point i of band l of row m is observed with
//     v_i = kappa_{m,l}^2 sigma_i^2 + nu_{m,l}
// and the band means and Sigma_b stay the handle's.  The four steps of gpcc_markov_sample.hip.h change in one place each:
//   prior draw   r~_i = alpha_b x~_1(s_i) + b~_b + sqrt(v_i) xi, v_i = fma(kappa_b^2, sigma_i^2, nu_b) formed on the lane;
//   correction   the walk's filter updates with the same v_i; the weights are gpcc_markov_combine_w's, unchanged, on the taps of
//                gpcc_markov_noise_taps<P, NOFF, GPCC_MKP_TAP> (the combine reads tap records only);
//   result       with sigmatest a test point of band b is a replicated observation under the fitted model, its noise
//                sqrt(JITTER + fma(kappa_b^2, sigma*^2, nu_b)) xi from the staged rounded product sigma*^2; without sigmatest
//                (`latent`) the draw is the latent curve, its noise sqrt(JITTER) xi, and nu is NOT added;
//   normals      unchanged: the same Philox stream and counters (e, s, m, 2), e naming the POINT.
// So a row's draws are, to rounding, gpcc_markov_draw's on a fresh handle created with the error bars sqrt(v_i), sigmatest mapped the
// same way, with the same seed.  At kappa = 1, nu = 0 the fma returns its operand exactly, the lane's correctly rounded
// sqrt(JITTER + sigma*^2) is the number the plain host stages, and every statement has gpcc_markov_draw's operands: the draws are its
// bits.
//
// A SIBLING BODY: gpcc_markov_noise_draw<P, NOFF> is gpcc_markov_draw (gpcc_markov_sample.hip.h) statement for statement, with the
// mapped variance handed to the unedited gpcc_mks_advance, gpcc_mk_transition, gpcc_mk_propagate, gpcc_mk_update and cursor
// (gpcc_mkp_rewind, gpcc_mkp_next), one call site of each.  (One walk templated on a variance policy was built first: the plain
// instantiations did not keep their registers under it -- DESIGN.md 4.30 has the numbers -- so gpcc_markov_draw stays as it is.)  A
// lane's kappa^2 and nu live in LDS, [band][thread], carved BEHIND the plain kernel's region (gpcc_mksn_lds_bytes): 16 more bytes per
// lane and band, 56 L in all.  gpcc_mknp_load_noise's check is not read here: a row whose kappa or nu is negative or not finite has
// info = -3 from the tap launch of the same call, which makes its mu -- and so its draws -- NaN; a lane writes its own column of the
// scratch only, so no other row is touched.
#pragma once
#include "gpcc_markov_noise_pred.hip.h"
#include "gpcc_markov_sample.hip.h"

// GpccMarkovDrawArgs (the host fills both through one function) and the rows' noise model; tpts holds t*[T] | sigma*^2[T] (raw)
struct GpccMarkovNoiseDrawArgs : GpccMarkovDrawArgs {
    const double *kappa, *nu;              // the (compacted) rows: Mc x L each
    int latent;                            // sigmatest == NULL: the test noise is sqrt(JITTER) xi
};

// dynamic LDS of a workgroup of `threads` lanes: the plain kernel's region first, kappa^2 and nu behind it
static inline size_t gpcc_mksn_lds_bytes(int N, int T, int L, int threads, bool stage)
{
    return gpcc_mks_lds_bytes(N, T, L, threads, stage) + (size_t)GPCC_MARKOV_NOISE_LANE_BYTES * L * threads;
}

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_noise_draw(const GpccMarkovNoiseDrawArgs a)
{
    constexpr int NS = P + NOFF;
    extern __shared__ __attribute__((aligned(16))) double gpcc_mksn_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x, L = a.L, N = a.N, T = a.T;
    // staged: t[N] | sigma^2[N] | t*[T] | sigma*^2[T] (doubles), then perm[N] | tperm[T] (ints, padded to a double), then the lanes' arrays
    const long nd = 2L * N + 2L * T, ni = ((long)N + T + 1) / 2;
    double *shead = gpcc_mksn_lds + (a.stage ? nd + ni : 0);         // [2L][nthr]: training bands, then test bands
    double *stau = shead + 2 * L * nthr, *salpha = stau + L * nthr;
    int *scur = (int *)(salpha + L * nthr);                          // [2L][nthr]
    double *sk2 = (double *)(scur + 2 * L * nthr), *snu = sk2 + L * nthr;   // behind gpcc_markov_draw's region (8-byte aligned)
    if (a.stage) {
        int *li = (int *)(gpcc_mksn_lds + nd);
        for (int i = tid; i < N; i += nthr) {
            gpcc_mksn_lds[i] = a.pts[i];
            gpcc_mksn_lds[N + i] = a.pts[2L * N + i];
            li[i] = a.perm[i];
        }
        for (int i = tid; i < T; i += nthr) {
            gpcc_mksn_lds[2L * N + i] = a.tpts[i];
            gpcc_mksn_lds[2L * N + T + i] = a.tpts[T + i];
            li[N + i] = a.tperm[i];
        }
    }
    const double *pt = a.stage ? (const double *)gpcc_mksn_lds : a.pts;
    const double *ps2 = a.stage ? (const double *)(gpcc_mksn_lds + N) : a.pts + 2L * N;
    const double *tt = a.stage ? (const double *)(gpcc_mksn_lds + 2L * N) : a.tpts;
    const double *ts2 = tt + T;
    const int *perm = a.stage ? (const int *)(gpcc_mksn_lds + nd) : a.perm;
    const int *tperm = a.stage ? perm + N : a.tperm;

    const int slot = (int)blockIdx.x * nthr + tid;                   // < lstride: every lane owns a column of the scratch
    const bool valid = slot < a.lanes;
    const long lane = a.lane0 + (valid ? slot : a.lanes - 1);
    const long m_ = a.lane_row[lane];
    const int lrow = (int)(m_ - a.row0);
    const unsigned long long sdraw = (unsigned long long)a.lane_s[lane];
    const unsigned long long word = a.mixture ? ~0ULL : (unsigned long long)a.row_word[m_];
    const double rho = a.rho[m_];
    gpcc_mk_load_row(a, m_, rho, stau, salpha, nthr, tid);
    gpcc_mknp_load_noise(a, m_, sk2, snu, nthr, tid);
    __syncthreads();

    // the offsets' draw: block N + T
    double bt[NOFF > 0 ? NOFF : 1];
    bt[0] = 0.0;
    if constexpr (NOFF > 0) {
        double z[4];
        gpccrng::normal4_stream(a.seed, (unsigned long long)N + T, sdraw, word, GPCC_MKS_STREAM, z);
#pragma unroll
        for (int c = 0; c < NOFF; ++c) bt[c] = sqrt(a.sigma_b[c]) * z[c];
    }
    double *rt = a.rt + slot, *acc = a.acc + slot;
    const long ls = a.lstride, ms = a.mstride;
    const GpccMkpLane cur = {pt, tt, shead, stau, scur, nthr, tid};

#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        const bool rev = pass == 1;
        gpcc_mkp_rewind<true>(a, cur, rev);
        double lam, lam2, Q[P][P], mu[NS], C[NS][NS], x[P];
        gpcc_mk_init<P, NOFF>(rho, a.sigma_b, lam, lam2, Q, mu, C);
#pragma unroll
        for (int i = 0; i < P; ++i) x[i] = 0.0;
        double ll = 0.0, sprev = 0.0, xprev = 0.0;
        int jt = 0;          // updates so far
        for (int j = 0; j < N + T; ++j) {
            const GpccMkpPoint p = gpcc_mkp_next(a, cur, rev, true);
            const bool is_test = p.is_test;
            const int band = p.band, i = p.i;
            const double key = p.key;
            const double al = salpha[band * nthr + tid];
            double boff = 0.0;
#pragma unroll
            for (int c = 0; c < NOFF; ++c) boff = (band == c) ? bt[c] : boff;
            // forward: the point's normals, the simulated state brought to the point
            double z3 = 0.0;
            if (!rev) {
                double z[4];
                const unsigned long long e = is_test ? (unsigned long long)N + tperm[i] : (unsigned long long)perm[i];
                gpccrng::normal4_stream(a.seed, e, sdraw, word, GPCC_MKS_STREAM, z);
                gpcc_mks_advance<P>(lam, lam2, Q, j == 0, j == 0 ? 0.0 : key - xprev, z, x);
                xprev = key;
                z3 = z[3];
            }
            const double d = (jt == 0) ? 0.0 : key - sprev;
            double A[P][P];
            gpcc_mk_transition<P>(lam, lam2, d, A);
            if (is_test) {
                // the filter's mean propagated to the test point, on a copy, against the weights of this direction
                const double *wr = a.w + (((long)pass * T + i) * NS) * ms + lrow;
                double dot = 0.0;
#pragma unroll
                for (int i2 = 0; i2 < P; ++i2) {
                    double m2 = 0.0;
#pragma unroll
                    for (int k = 0; k < P; ++k) m2 += A[i2][k] * mu[k];
                    dot += wr[(long)i2 * ms] * m2;
                }
#pragma unroll
                for (int c = 0; c < NOFF; ++c) dot += wr[(long)(P + c) * ms] * mu[P + c];
                double *o = acc + (long)tperm[i] * ls;
                if (!rev) {
                    // a replicated observation under the row's model, or (latent) the curve itself: nu is not added then
                    const double vt = a.latent ? GPCC_MKP_JITTER
                                               : GPCC_MKP_JITTER + fma(sk2[band * nthr + tid], ts2[i], snu[band * nthr + tid]);
                    *o = al * x[0] + boff + sqrt(vt) * z3 - dot;
                } else {
                    *o -= dot;
                }
                continue;
            }
            const double v = fma(sk2[band * nthr + tid], ps2[i], snu[band * nthr + tid]);
            double r;
            if (!rev) {
                r = al * x[0] + boff + sqrt(v) * z3;
                rt[(long)i * ls] = r;
            } else {
                r = rt[(long)i * ls];
            }
            sprev = key;
            gpcc_mk_propagate<P, NOFF>(A, Q, mu, C);
            gpcc_mk_update<P, NOFF>(band, al, r, v, mu, C, ll);
            ++jt;
        }
    }
}

// WHAT SHIPS: every <P, NOFF>.  Registers per lane (tools/kernel_resources.py, profiles/markov/kernel_resources_noise_sample.log), no
// scratch memory in any of them: see DESIGN.md 4.30.
struct GpccMkShipsNoiseSample { static constexpr int max_noff[3] = {GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS}; };

// ---- launch (gpcc_markov_noise_sample_inst.hip: an object of its own) ----
// grid (g.blocks): one lane per draw
hipError_t gpcc_mksn_launch_draw(const GpccMkLaunch &g, const GpccMarkovNoiseDrawArgs &a);
