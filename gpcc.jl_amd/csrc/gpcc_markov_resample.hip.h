// gpcc_markov_resample.hip.h -- the linear-time log-likelihood of rows that each carry their own (tau, alpha, rho) AND their own
// RESAMPLED DATA SET on the handle's cadence, for gfx950: gpcc_loglik_markov_resampled_batch of include/gpcc_hip.h, DESIGN.md 4.24;
// gpcc.jl_amd/markov.py (loglik_resampled) is the same algorithm in numpy.  It is gpcc_markov_eval with the data read per lane:
// flux randomisation with a refit per realisation, random subset selection (RSS) and, with marginalise_b, each realisation's own
// Sigma_b.
//
// Dropping points from the L-way merge does not change the order of the points that remain, and a point drawn n times is the same
// point with variance sigma^2 / n.  So the handle's times, their staging and the merge cursor stay shared by every lane; what a lane
// reads of ITS realisation at a step is one aligned 16-byte pair rv[real N + i] = {residual, effective variance} that
// gpcc_markov_resample_pack wrote, i the index of the merged point in the handle's sorted light curves.  A DROPPED POINT is marked by a
// NEGATIVE VARIANCE (sigma^2 = 0 is a legal input and sigma^2 / n is never negative): the lane moves the cursor past it and does
// nothing more -- no transition, no propagate, no update, not even the point's 1/2 log 2 pi.
//
// ONE LANE PER ROW, rows along x exactly as in gpcc_markov_eval: the same gpcc_mk_open / gpcc_mk_next<false>, the same LDS, the same
// launch shapes, and gpcc_mk_init / gpcc_mk_transition / gpcc_mk_propagate / gpcc_mk_update unedited.  The lane keeps the shifted time
// of its last KEPT point: the lag of a kept point is s - s_kept (0 at the first kept point), one subtraction, the lag the reduced data
// set would see -- not a product of transitions over the skipped points.  The lag gpcc_mk_next forms, the staged r and the staged
// sigma^2 are not read.  With a realisation that is the handle's own y, counts of 1 and the handle's means and Sigma_b every statement
// has gpcc_markov_eval's operands.  info counts positions among the kept points, as a fresh handle of the reduced data would.  No
// atomics, no communication between lanes: a row's value depends on its own parameters and its own realisation only, whatever M, R,
// the order of the rows (lanes of a wave on one realisation read nearby pairs, which the caches serve; any other order is as correct)
// and the launch shape.
#pragma once
#include "gpcc_markov.hip.h"

struct GpccMarkovResampleArgs {
    const double *pts;                     // (GpccMarkovArgs' fields, for the shared cursor; only the t third of pts is read)
    const double *delays, *alpha, *rho;
    double *out_loglik;                    // [M]
    int *out_info;                         // [M]
    int M, L, N, stage;
    int off[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];   // (not read: every realisation has its own, sigb)
    const double2 *rv;                     // [R][N]: {residual, sigma^2 / count} of sorted point i of realisation r; .y < 0: dropped
    const int *real;                       // [M]: the realisation of row m, checked on the host to lie in [0, R)
    const double *sigb;                    // [R][L]: the offsets' prior variances of each realisation (read with NOFF > 0 only)
};

// the pack kernel's: Y [R][N] in the order gpcc_create took y, count [R][N] or NULL (all 1), mean [R][L], perm[i] = the caller's
// position of sorted point i, sig2 = the sigma^2 third of the handle's sorted light curves
struct GpccMarkovResamplePackArgs {
    const double *Y, *mean, *sig2;
    const int *count, *perm;
    double2 *rv;
    long total;                            // R N
    int N, L;
    int off[GPCC_MARKOV_MAXL + 1];
};

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_resample(const GpccMarkovResampleArgs a)
{
    constexpr int NS = P + NOFF;
    extern __shared__ __attribute__((aligned(16))) double gpcc_mkr_lds[];
    const GpccMkLane ln = gpcc_mk_open(a, gpcc_mkr_lds);

    const long real = a.real[ln.valid ? ln.row : a.M - 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
#pragma unroll
    for (int c = 0; c < GPCC_MARKOV_MAX_OFFSETS; ++c) sigma_b[c] = 0.0;
#pragma unroll
    for (int c = 0; c < NOFF; ++c) sigma_b[c] = a.sigb[real * a.L + c];   // (NOFF > 0: NOFF == L)
    double lam, lam2, Q[P][P], mu[NS], C[NS][NS];
    gpcc_mk_init<P, NOFF>(ln.rho, sigma_b, lam, lam2, Q, mu, C);
    const double2 *rv = a.rv + real * a.N;

    double ll = 0.0, sprev = 0.0, skept = 0.0;
    int info = ln.info, kept = 0;
    for (int j = 0; j < a.N; ++j) {
        const GpccMkPoint p = gpcc_mk_next<false>(a, ln, j, sprev);   // (leaves the point's shifted time in sprev)
        const double2 v = rv[ln.scur[p.b * ln.nthr + ln.tid] - 1];    // the point taken: the cursor has moved past it
        if (v.y < 0.0) continue;                                      // dropped from this lane's realisation
        const double d = kept ? sprev - skept : 0.0;
        skept = sprev;
        ++kept;
        double A[P][P];
        gpcc_mk_transition<P>(lam, lam2, d, A);
        gpcc_mk_propagate<P, NOFF>(A, Q, mu, C);
        const bool ok = gpcc_mk_update<P, NOFF>(p.b, p.al, v.x, v.y, mu, C, ll);
        info = (info == 0 && !ok) ? kept : info;   // first kept point whose predictive variance is not positive and finite
    }
    if (ln.valid) {
        a.out_loglik[ln.row] = info ? __builtin_nan("") : ll;
        a.out_info[ln.row] = info;
    }
}

// WHAT SHIPS: every <P, NOFF> of the filter.  Registers per lane (tools/kernel_resources.py,
// profiles/markov/kernel_resources_resample.log), no scratch memory in any of them: see DESIGN.md 4.24.
struct GpccMkShipsResample { static constexpr int max_noff[3] = {GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS}; };

// gpcc_markov_resample_pack on ceil(R N / 256) workgroups (gpcc_markov_resample_inst.hip: the object with P = 1)
hipError_t gpcc_markov_resample_pack_launch(const GpccMarkovResamplePackArgs &a, hipStream_t s);
// gpcc_markov_resample<g.p, g.noff> on the grid (g.blocks)
hipError_t gpcc_markov_resample_launch(const GpccMkLaunch &g, const GpccMarkovResampleArgs &a);
