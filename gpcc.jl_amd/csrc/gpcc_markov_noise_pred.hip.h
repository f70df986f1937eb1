// gpcc_markov_noise_pred.hip.h -- linear-time predictions, held-out log-likelihoods, the offsets' posterior and leave-one-out scores of
// rows that each carry their own (tau, alpha, rho) AND their own NOISE MODEL, for gfx950: gpcc_predict_noise_markov_batch,
// gpcc_heldout_loglik_noise_markov_batch, gpcc_posterior_offsets_noise_markov_batch and gpcc_loo_noise_markov_batch of
// include/gpcc_hip.h; gpcc.jl_amd/markov.py (predict_noise, heldout_noise, posterior_offsets_noise, loo_noise) is the
// same algorithm in numpy.  The model is gpcc_markov_noise.hip.h's: point i of band l of row m is observed with the variance
//     v_i = kappa_{m,l}^2 sigma_i^2 + nu_{m,l}
// and the band means and Sigma_b stay the handle's, so a row's outputs are those of a fresh handle created with the error bars sqrt(v_i).
//
// gpcc_markov_noise_taps<P, NOFF, MODE>: gpcc_markov_taps (gpcc_markov_pred.hip.h) with s2' = fma(kappa_b^2, s2, nu_b) handed to the
//   unedited gpcc_mk_update.  A TRAINING point's s2 is sigma_i^2; a TEST point that is an observation (MODE = GPCC_MKP_UPDATE, the
//   held-out union filter) is staged with its raw sigma*^2 and enters with fma(kappa_b^2, sigma*^2, nu_b) + JITTER: at kappa = 1,
//   nu = 0 that is the sum the host of gpcc_heldout_loglik_markov_batch stages.  A tapped test point (MODE = GPCC_MKP_TAP) has no
//   variance: the latent curve's var* = h'P_s h + JITTER feels the noise model through the training updates only, and the combine is
//   gpcc_markov_combine itself.
// gpcc_markov_noise_loo_taps<P, NOFF>: gpcc_markov_loo_taps (gpcc_markov_loo.hip.h) likewise.  Its combine is gpcc_markov_loo_combine
//   instantiated on GpccMarkovNoiseLooCombineArgs: var_i = h'P_s h + fma(kappa_b^2, sigma_i^2, nu_b), the lane's expression.
// At kappa = 1, nu = 0 the fma returns s2 exactly and every statement has the plain kernel's operands: the outputs are its bits.
//
// A lane's kappa^2 and nu live in LDS, [band][thread], carved AFTER the plain kernel's region (gpcc_mkp_lds_bytes /
// gpcc_mkl_lds_bytes): 16 more bytes per lane and band, 56 L for the prediction layout, 44 L for the leave-one-out layout.  The
// cursor (gpcc_mkp_*), gpcc_mk_load_row and the filter's step functions are used unedited, one call site of each per kernel.  A kappa
// or nu that is negative or not finite: info = -3, after -1 (alpha) and -2 (rho), as gpcc_mkn_open (whose GpccMkLane these layouts
// do not have).
#pragma once
#include "gpcc_markov_loo.hip.h"
#include "gpcc_markov_noise.hip.h"

// GpccMarkovPredArgs' fields under the same names (the host fills both through one function) and the rows' noise model
struct GpccMarkovNoisePredArgs {
    const double *pts;                     // t[N] | r[N] | sigma^2[N], as GpccMarkovArgs
    const double *tpts;                    // test points, each band sorted by time: t[T] (TAP), t[T] | r[T] | sigma*^2 [T] (UPDATE: raw)
    const double *delays, *alpha, *rho;    // the batch's rows: M x L, M x L, M
    double *out_loglik;
    int *out_info;
    double *tap;
    double *ll2;
    int *info2, *at2;
    double *fin;
    int M, L, N, T, stage;
    int row0, rows, mstride;
    int off[GPCC_MARKOV_MAXL + 1], toff[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
    const double *kappa, *nu;              // the batch's rows: M x L each
};

// GpccMarkovLooArgs' fields and the rows' noise model
struct GpccMarkovNoiseLooArgs {
    const double *pts;
    const double *delays, *alpha, *rho;
    double *out_loglik;
    int *out_info;
    double *tap;
    int M, L, N, stage;
    int row0, rows, mstride;
    int off[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
    const double *kappa, *nu;              // the batch's rows: M x L each
};

// GpccMarkovLooCombineArgs' fields and the rows' noise model: what gpcc_markov_loo_combine is instantiated on for these rows
struct GpccMarkovNoiseLooCombineArgs {
    const double *tap, *alpha, *rho;
    const double *pts;
    const int *pband, *pperm;
    double *mu, *var, *lp;
    int L, N, row0, rows, mstride;
    double mean_b[GPCC_MARKOV_MAXL], sigma_b[GPCC_MARKOV_MAX_OFFSETS];
    const double *kappa, *nu;              // the batch's rows: M x L each
};

// dynamic LDS of a workgroup of `threads` lanes: the plain kernel's region first, kappa^2 and nu behind it
static inline size_t gpcc_mknp_lds_bytes(int N, int T, int tw, int L, int threads, bool stage)
{
    return gpcc_mkp_lds_bytes(N, T, tw, L, threads, stage) + (size_t)GPCC_MARKOV_NOISE_LANE_BYTES * L * threads;
}
static inline size_t gpcc_mknl_lds_bytes(int N, int L, int threads, bool stage)
{
    return gpcc_mkl_lds_bytes(N, L, threads, stage) + (size_t)GPCC_MARKOV_NOISE_LANE_BYTES * L * threads;
}

// the lane's kappa^2 and nu of row m to sk2, snu ([band][thread]); true: one of them is negative or not finite (gpcc_mkn_open's check)
template <class ARGS>
__device__ __forceinline__ bool gpcc_mknp_load_noise(const ARGS &a, long m, double *sk2, double *snu, int nthr, int tid)
{
    bool bad = false;
    for (int l = 0; l < a.L; ++l) {
        const double k = a.kappa[m * a.L + l], v = a.nu[m * a.L + l];
        bad = bad || !(k >= 0.0 && k < __builtin_inf()) || !(v >= 0.0 && v < __builtin_inf());
        sk2[l * nthr + tid] = k * k;
        snu[l * nthr + tid] = v;
    }
    return bad;
}

template <int P, int NOFF, int MODE>
__global__ void __launch_bounds__(256) gpcc_markov_noise_taps(const GpccMarkovNoisePredArgs a)
{
    constexpr int NS = P + NOFF, NREC = NS + NS * (NS + 1) / 2, TW = MODE == GPCC_MKP_TAP ? 1 : 3;
    extern __shared__ __attribute__((aligned(16))) double gpcc_mknp_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x, L = a.L, N = a.N, T = a.T;
    const int kind = blockIdx.y;                                  // uniform per workgroup
    const bool rev = MODE == GPCC_MKP_TAP && kind == 1;           // descending shifted time
    const bool use_tests = MODE == GPCC_MKP_TAP || kind == 1;     // (the training-only lane of UPDATE walks no test stream)
    const long nstage = a.stage ? 3L * N + (long)TW * T : 0;
    double *shead = gpcc_mknp_lds + nstage;                       // [2L][nthr]: training bands, then test bands
    double *stau = shead + 2 * L * nthr, *salpha = stau + L * nthr;
    int *scur = (int *)(salpha + L * nthr);                       // [2L][nthr]
    double *sk2 = (double *)(scur + 2 * L * nthr), *snu = sk2 + L * nthr;   // behind gpcc_markov_taps' region (8-byte aligned)
    if (a.stage) {
        for (int i = tid; i < 3 * N; i += nthr) gpcc_mknp_lds[i] = a.pts[i];
        for (int i = tid; i < TW * T; i += nthr) gpcc_mknp_lds[3L * N + i] = a.tpts[i];
    }
    const double *pts = a.stage ? (const double *)gpcc_mknp_lds : a.pts;
    const double *tpts = a.stage ? (const double *)(gpcc_mknp_lds + 3L * N) : a.tpts;

    const int lrow = (int)blockIdx.x * nthr + tid;
    const bool valid = lrow < a.rows;
    const long m_ = a.row0 + (valid ? lrow : a.rows - 1);
    const double rho = a.rho[m_];
    int info = gpcc_mk_load_row(a, m_, rho, stau, salpha, nthr, tid);
    info = (gpcc_mknp_load_noise(a, m_, sk2, snu, nthr, tid) && info == 0) ? -3 : info;
    __syncthreads();
    const GpccMkpLane cur = {pts, tpts, shead, stau, scur, nthr, tid};
    gpcc_mkp_rewind<true>(a, cur, rev);

    double lam, lam2, Q[P][P], mu[NS], C[NS][NS];
    gpcc_mk_init<P, NOFF>(rho, a.sigma_b, lam, lam2, Q, mu, C);

    double ll = 0.0, sprev = 0.0;
    int jt = 0, at = 0;         // jt: updates so far
    const int total = N + (use_tests ? T : 0);
    for (int j = 0; j < total; ++j) {
        // the point taken: its band, key, residual and reported variance (a tapped test point has none and ends the step)
        const GpccMkpPoint p = gpcc_mkp_next(a, cur, rev, use_tests);
        const int i = p.i;
        double r, s2;
        if (p.is_test) {
            if constexpr (MODE == GPCC_MKP_TAP) {
                // the state after the training points before this test point, propagated to it: on a copy
                const double d = (jt == 0) ? 0.0 : p.key - sprev;
                double A[P][P], mu2[NS], C2[NS][NS];
                gpcc_mk_transition<P>(lam, lam2, d, A);
#pragma unroll
                for (int i2 = 0; i2 < NS; ++i2) {
                    mu2[i2] = mu[i2];
#pragma unroll
                    for (int k = 0; k < NS; ++k) C2[i2][k] = C[i2][k];
                }
                gpcc_mk_propagate<P, NOFF>(A, Q, mu2, C2);
                if (valid) {
                    double *rec = a.tap + (((long)kind * T + i) * NREC) * a.mstride + lrow;
#pragma unroll
                    for (int i2 = 0; i2 < NS; ++i2) rec[(long)i2 * a.mstride] = mu2[i2];
                    int c = NS;
#pragma unroll
                    for (int i2 = 0; i2 < NS; ++i2)
#pragma unroll
                        for (int k = i2; k < NS; ++k) rec[(long)(c++) * a.mstride] = C2[i2][k];
                }
                continue;
            }
            r = MODE == GPCC_MKP_TAP ? 0.0 : tpts[T + i];
            s2 = MODE == GPCC_MKP_TAP ? 0.0 : tpts[2 * T + i];
            at = (info == 0) ? i : at;
        } else {
            r = pts[N + i];
            s2 = pts[2 * N + i];
        }
        // one filter step, as in gpcc_markov_eval, on the mapped variance (a test observation: plus JITTER, as the plain host stages it)
        const double al = salpha[p.band * nthr + tid];
        double v = fma(sk2[p.band * nthr + tid], s2, snu[p.band * nthr + tid]);
        if constexpr (MODE == GPCC_MKP_UPDATE) v = p.is_test ? v + GPCC_MKP_JITTER : v;
        const double d = (jt == 0) ? 0.0 : p.key - sprev;
        sprev = p.key;
        double A[P][P];
        gpcc_mk_transition<P>(lam, lam2, d, A);
        gpcc_mk_propagate<P, NOFF>(A, Q, mu, C);
        const bool ok = gpcc_mk_update<P, NOFF>(p.band, al, r, v, mu, C, ll);
        info = (info == 0 && !ok) ? jt + 1 : info;   // first predictive variance that is not positive and finite
        ++jt;
    }
    if (!valid) return;
    const long row = a.row0 + lrow;
    if (kind == 0) {
        a.out_loglik[row] = info ? __builtin_nan("") : ll;
        a.out_info[row] = info;
        if constexpr (NOFF > 0)
            if (a.fin) {
                int c = 0;
#pragma unroll
                for (int i2 = 0; i2 < NOFF; ++i2) a.fin[(long)(c++) * a.M + row] = mu[P + i2];
#pragma unroll
                for (int i2 = 0; i2 < NOFF; ++i2)
#pragma unroll
                    for (int k = i2; k < NOFF; ++k) a.fin[(long)(c++) * a.M + row] = C[P + i2][P + k];
            }
    } else if constexpr (MODE == GPCC_MKP_UPDATE) {
        a.ll2[row] = ll;
        a.info2[row] = info;
        a.at2[row] = at;
    }
}

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_noise_loo_taps(const GpccMarkovNoiseLooArgs a)
{
    constexpr int NS = P + NOFF, NREC = NS + NS * (NS + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) double gpcc_mknl_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x, L = a.L, N = a.N;
    const int kind = blockIdx.y;          // uniform per workgroup
    const bool rev = kind == 1;           // the reverse of the merged order
    double *shead = gpcc_mknl_lds + (a.stage ? 3L * N : 0);
    double *stau = shead + L * nthr, *salpha = stau + L * nthr;
    int *scur = (int *)(salpha + L * nthr);
    double *sk2 = (double *)(scur + L * nthr), *snu = sk2 + L * nthr;   // behind gpcc_markov_loo_taps' region (L nthr is even)
    if (a.stage)
        for (int i = tid; i < 3 * N; i += nthr) gpcc_mknl_lds[i] = a.pts[i];
    const double *pts = a.stage ? (const double *)gpcc_mknl_lds : a.pts;

    const int lrow = (int)blockIdx.x * nthr + tid;
    const bool valid = lrow < a.rows;
    const long m_ = a.row0 + (valid ? lrow : a.rows - 1);
    const double rho = a.rho[m_];
    int info = gpcc_mk_load_row(a, m_, rho, stau, salpha, nthr, tid);
    info = (gpcc_mknp_load_noise(a, m_, sk2, snu, nthr, tid) && info == 0) ? -3 : info;
    __syncthreads();
    const GpccMkpLane cur = {pts, nullptr, shead, stau, scur, nthr, tid};
    gpcc_mkp_rewind<false>(a, cur, rev);

    double lam, lam2, Q[P][P], mu[NS], C[NS][NS];
    gpcc_mk_init<P, NOFF>(rho, a.sigma_b, lam, lam2, Q, mu, C);

    double ll = 0.0, sprev = 0.0;
    for (int j = 0; j < N; ++j) {
        // the next point: on ties the lowest band forward, the highest backward
        const GpccMkpPoint p = gpcc_mkp_next<true>(a, cur, rev);
        const int b = p.band, i = p.i;
        const double s = p.key, r = pts[N + i], al = salpha[b * nthr + tid];
        const double s2 = fma(sk2[b * nthr + tid], pts[2 * N + i], snu[b * nthr + tid]);
        const double d = (j == 0) ? 0.0 : s - sprev;
        sprev = s;

        double A[P][P];
        gpcc_mk_transition<P>(lam, lam2, d, A);
        gpcc_mk_propagate<P, NOFF>(A, Q, mu, C);
        if (valid) {   // the state at s_i before point i enters
            double *rec = a.tap + (((long)kind * N + i) * NREC) * a.mstride + lrow;
#pragma unroll
            for (int i2 = 0; i2 < NS; ++i2) rec[(long)i2 * a.mstride] = mu[i2];
            int c = NS;
#pragma unroll
            for (int i2 = 0; i2 < NS; ++i2)
#pragma unroll
                for (int k = i2; k < NS; ++k) rec[(long)(c++) * a.mstride] = C[i2][k];
        }
        const bool ok = gpcc_mk_update<P, NOFF>(b, al, r, s2, mu, C, ll);
        info = (info == 0 && !ok) ? j + 1 : info;   // first predictive variance that is not positive and finite
    }
    if (valid && kind == 0) {
        const long row = a.row0 + lrow;
        a.out_loglik[row] = info ? __builtin_nan("") : ll;
        a.out_info[row] = info;
    }
}

// WHAT SHIPS: every <P, NOFF>.  Registers per lane (tools/kernel_resources.py, profiles/markov/kernel_resources_noise_pred.log), no
// scratch memory in any of them: see DESIGN.md 4.29.
struct GpccMkShipsNoisePred { static constexpr int max_noff[3] = {GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS}; };

// ---- launches (gpcc_markov_noise_pred_inst.hip: an object of its own) ----
// mode GPCC_MKP_TAP / GPCC_MKP_UPDATE (two kernels); grid (g.blocks, ny)
hipError_t gpcc_mknp_launch_taps(const GpccMkLaunch &g, int mode, int ny, const GpccMarkovNoisePredArgs &a);
// grid (g.blocks, 2): the forward and the backward filter
hipError_t gpcc_mknl_launch_taps(const GpccMkLaunch &g, const GpccMarkovNoiseLooArgs &a);
// gpcc_markov_loo_combine on the noise model's Args: grid (N, ceil(rows / 64)), 64 threads
hipError_t gpcc_mknl_launch_combine(int p, int noff, const GpccMarkovNoiseLooCombineArgs &a, hipStream_t s);
