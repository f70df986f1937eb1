// gpcc_markov_resample_grad.hip.h -- the exact linear-time gradient of the log-likelihood of rows that each carry their own
// (tau, alpha, rho) AND their own RESAMPLED DATA SET on the handle's cadence, for gfx950: gpcc_loglik_grad_markov_resampled_batch of
// include/gpcc_hip.h; gpcc.jl_amd/markov.py (loglik_grad_resampled) is the same algorithm in numpy.  It is
// gpcc_markov_grad (gpcc_markov_grad.hip.h: the forward sensitivities, the slots, the first / last pair of OU) over the data source of
// gpcc_markov_resample (gpcc_markov_resample.hip.h: one packed 16-byte pair {residual, sigma^2 / count} per step, a negative variance
// marks a dropped point), the gradient of the log-likelihood of a fresh handle on the reduced data set: band means and Sigma_b are
// constants of the data.
//
// gpcc_markov_resample_grad<P, NOFF>: ONE LANE PER (ROW, PARAMETER SLOT), the slot being blockIdx.y, exactly the slots of
// gpcc_markov_grad: L alpha, one rho, L tau (OU: 2L, averaged by gpcc_markov_grad's finish kernel).  The walk is gpcc_mkg_walk itself,
// instantiated on this header's data policy GpccMkrData where gpcc_markov_grad instantiates it on GpccMkOwnData; what the policy does:
//   skip      a pair with .y < 0 is not in the lane's data: no transition, no tangent step, no update (the cursor has moved past it)
//   lag       s - s_kept, one subtraction, 0 at the first kept point: the lag the reduced data set would see
//   tau       the lag's tangent is [band of the last KEPT point == tb] - [b == tb], 0 at the first kept point: the walk keeps bprev
//             over the skipped points, and `first` is the policy's
//   Sigma_b   the realisation's own sigb[real L + c] in gpcc_mk_init
//   ties      the cursor's ranked rule orders kept and dropped points alike; a tie with a dropped point is no tie, since the dropped
//             point takes no step, and two kept points that tie across a dropped one are neighbours with lag 0 in either order
// The staged r and sigma^2 and the lag gpcc_mk_next forms are not read.  With a realisation that is the handle's own y, counts of 1 and
// the handle's means and Sigma_b every statement has gpcc_markov_grad's operands.  Value and info are gpcc_markov_resample's, of the same
// call (info counts positions among the kept points); the finish kernel reads them.  No atomics, no communication between lanes.
#pragma once
#include "gpcc_markov_grad.hip.h"
#include "gpcc_markov_resample.hip.h"

// GpccMarkovGradArgs (the cursor, the slots, the finish kernel take it as it is) and the data source of GpccMarkovResampleArgs
struct GpccMarkovResampleGradArgs : GpccMarkovGradArgs {
    const double2 *rv;                     // [R][N]: {residual, sigma^2 / count} of sorted point i of realisation r; .y < 0: dropped
    const int *real;                       // [M]: the realisation of row m, checked on the host to lie in [0, R)
    const double *sigb;                    // [R][L]: the offsets' prior variances of each realisation (read with NOFF > 0 only)
};

// the data policy of a lane with its own realisation (gpcc_markov_grad.hip.h, beside GpccMkOwnData)
struct GpccMkrData {
    static constexpr bool resampled = true;
    const double2 *rv;                     // the lane's realisation: [N]
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
    double skept;                          // the shifted time of the last kept point
    int kept;                              // kept points so far
    // s: the shifted time of the point taken, p (the cursor has moved past it)
    __device__ __forceinline__ GpccMkObs take(const GpccMkLane &ln, const GpccMkPoint &p, int, double s)
    {
        const double2 v = rv[ln.scur[p.b * ln.nthr + ln.tid] - 1];
        GpccMkObs o = {v.x, v.y, kept ? s - skept : 0.0, kept == 0, !(v.y < 0.0)};
        if (o.kept) {
            skept = s;
            ++kept;
        }
        return o;
    }
};

template <int NOFF>
__device__ __forceinline__ GpccMkrData gpcc_mkr_open(const GpccMarkovResampleGradArgs &a, const GpccMkLane &ln)
{
    GpccMkrData dt;
    const long real = a.real[ln.valid ? ln.row : a.M - 1];
#pragma unroll
    for (int c = 0; c < GPCC_MARKOV_MAX_OFFSETS; ++c) dt.sigma_b[c] = 0.0;
#pragma unroll
    for (int c = 0; c < NOFF; ++c) dt.sigma_b[c] = a.sigb[real * a.L + c];   // (NOFF > 0: NOFF == L)
    dt.rv = a.rv + real * a.N;
    dt.skept = 0.0;
    dt.kept = 0;
    return dt;
}

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_resample_grad(const GpccMarkovResampleGradArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double gpcc_mkrg_lds[];
    const GpccMkLane ln = gpcc_mk_open(a, gpcc_mkrg_lds);
    const GpccMkrData dt = gpcc_mkr_open<NOFF>(a, ln);
    const int L = a.L;

    // what this workgroup differentiates (uniform)
    const int slot = blockIdx.y;
    double dll;
    if (slot < L) {
        dll = gpcc_mkg_walk<P, NOFF, GPCC_MKG_ALPHA>(a, ln, GpccMkPlain(), slot, -1, 0, dt);
    } else if (slot == L) {
        dll = gpcc_mkg_walk<P, NOFF, GPCC_MKG_RHO>(a, ln, GpccMkPlain(), -1, -1, 0, dt);
    } else {
        const int q = slot - L - 1, tb = a.twice ? q >> 1 : q;
        dll = gpcc_mkg_walk<P, NOFF, GPCC_MKG_TAU>(a, ln, GpccMkPlain(), tb, a.twice ? tb : -1, (q & 1) ? L : -1, dt);
    }
    if (ln.valid) a.slot[(long)slot * a.M + ln.row] = dll;
}

// WHAT SHIPS: every <P, NOFF> of the filter.  Registers per lane (tools/kernel_resources.py,
// profiles/markov/kernel_resources_resample_grad.log), no scratch memory in any of them: see DESIGN.md 4.28.
struct GpccMkShipsResampleGrad { static constexpr int max_noff[3] = {GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS}; };

// grid (g.blocks, slots) of gpcc_markov_resample_grad<g.p, g.noff>, then gpcc_markov_grad's finish kernel over the M rows
// (gpcc_markov_resample_grad_inst.hip: one object per P)
hipError_t gpcc_markov_resample_grad_launch(const GpccMkLaunch &g, int slots, const GpccMarkovResampleGradArgs &a);
