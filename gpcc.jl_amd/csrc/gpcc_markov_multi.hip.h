// gpcc_markov_multi.hip.h -- the linear-time log-likelihood of MANY flux realisations per parameter row for gfx950:
// gpcc_loglik_markov_multi_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py (loglik_realisations) is the same algorithm
// in numpy.  It is the filter of gpcc_markov.hip.h with a second data axis: "one factorisation, many right-hand sides" in linear time.
//
// In a step of the filter nothing but the state mean, the innovation eps = r - h'mu, eps^2 / S and mu += Ph eps / S reads a flux: the
// merge, the transition A, the covariance recursion C, the predictive variance S, 1 / S, log S and the gain Ph / S depend on the row
// (tau, alpha, rho) and on the times and error bars alone.  A lane therefore carries ONE covariance recursion and drives RB means
// through it, one per realisation, summing RB log-likelihoods: the flux-dependent part is P^2 + 3 NS + 6 fp64 operations a step and
// realisation beside the few hundred of the step.
//
// ONE LANE PER (ROW, BLOCK OF RB REALISATIONS): rows along x exactly as in gpcc_markov_eval (same cursor, same LDS, same launch shapes),
// blocks of realisations along blockIdx.y.  The walk is gpcc_mk_open / gpcc_mk_next<false>, the covariance gpcc_mk_init /
// gpcc_mk_transition / gpcc_mk_propagate, all unedited; gpcc_mk_update is NOT used and not edited (its contraction fixes the bits of
// every other entry): gpcc_mk_update_multi below is its sibling.  What is computed per realisation is written with explicit fma(), so
// that every realisation of a block is the same sequence of roundings whatever the compiler does with the unrolled loop: cell (m, r) of
// the result is bitwise the same in any block, at any position in it, for any M, R, chunk and launch shape.  It is NOT bitwise
// gpcc_markov_eval's value of the same data: another statement order, the same bar.
//
// THE RESIDUALS (R x N doubles) do not fit the LDS beside the staged t and sigma^2; they are read through the caches from a packed
// buffer that gpcc_markov_multi_pack writes: point-major within a block, res[(block N + i) RB + k] = Y[block RB + k][perm[i]] -
// mean[block RB + k][band(i)], i the index of the point in the handle's sorted light curves.  A lane's read at a step is one aligned run
// of RB doubles, and the lanes of a wave sit at nearby i.  The tail block is padded with copies of its last realisation; padded
// realisations are computed and not stored.  A flux that is not finite is packed as NaN, so that its column (and no other) is NaN.
// The staged r of the handle's own data is never read.  info depends on the row only: block 0 stores it.  No atomics, no communication
// between lanes.
#pragma once
#include "gpcc_markov.hip.h"

struct GpccMarkovMultiArgs {
    const double *pts;                     // (GpccMarkovArgs' fields, for the shared cursor; the r third of pts is not read)
    const double *delays, *alpha, *rho;
    double *out_loglik;                    // [M][ldo]: row m, realisation r of this chunk at m * ldo + r
    int *out_info;                         // [M]
    int M, L, N, stage;
    int off[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
    const double *res;                     // the packed residuals of this chunk: [blocks][N][RB]
    long ldo;
    int R;                                 // realisations of this chunk (the last block holds R - (blocks - 1) RB of them)
};

// the pack kernel's: Y [R][N] in the order gpcc_create took y, mean [R][L], perm[i] = the caller's position of sorted point i
struct GpccMarkovMultiPackArgs {
    const double *Y, *mean;
    const int *perm;
    double *res;
    int R, N, L, rb, blocks;
    int off[GPCC_MARKOV_MAXL + 1];
};

// predict, the means: mu_k <- A mu_k on the P process components of each realisation's mean (the offsets do not move)
template <int P, int NOFF, int RB>
__device__ __forceinline__ void gpcc_mk_propagate_means(const double (&A)[P][P], double (&mu)[RB][P + NOFF])
{
#pragma unroll
    for (int k = 0; k < RB; ++k) {
        double t1[P];
#pragma unroll
        for (int i2 = 0; i2 < P; ++i2) {
            double acc = A[i2][0] * mu[k][0];
#pragma unroll
            for (int q = 1; q < P; ++q) acc = fma(A[i2][q], mu[k][q], acc);
            t1[i2] = acc;
        }
#pragma unroll
        for (int i2 = 0; i2 < P; ++i2) mu[k][i2] = t1[i2];
    }
}

// update with h = alpha_b e_1 + e_{P + b} for RB realisations at once: Ph, S, 1 / S and log S once (gpcc_mk_update's statements), then
// per realisation eps, the log-density and the mean; false: the predictive variance is not positive and finite (the row's, not a
// realisation's)
template <int P, int NOFF, int RB>
__device__ __forceinline__ bool gpcc_mk_update_multi(int b, double al, const double (&r)[RB], double s2, double (&mu)[RB][P + NOFF],
                                                     double (&C)[P + NOFF][P + NOFF], double (&ll)[RB])
{
    constexpr int NS = P + NOFF;
    double Ph[NS];
#pragma unroll
    for (int i2 = 0; i2 < NS; ++i2) {
        double acc = al * GPCC_MK_SYM(C, i2, 0);
#pragma unroll
        for (int c = 0; c < NOFF; ++c) acc += (b == c) ? GPCC_MK_SYM(C, i2, P + c) : 0.0;
        Ph[i2] = acc;
    }
    double S = al * Ph[0] + s2;
#pragma unroll
    for (int c = 0; c < NOFF; ++c) S += (b == c) ? Ph[P + c] : 0.0;
    const bool ok = S > 0.0 && S < __builtin_inf();
    const double inv = 1.0 / S, base = 1.8378770664093453 + log(S);
#pragma unroll
    for (int k = 0; k < RB; ++k) {
        double hm = al * mu[k][0];
#pragma unroll
        for (int c = 0; c < NOFF; ++c) hm += (b == c) ? mu[k][P + c] : 0.0;
        const double eps = r[k] - hm, g = eps * inv;
        ll[k] = fma(-0.5, fma(eps, g, base), ll[k]);
#pragma unroll
        for (int i2 = 0; i2 < NS; ++i2) mu[k][i2] = fma(Ph[i2], g, mu[k][i2]);
    }
#pragma unroll
    for (int i2 = 0; i2 < NS; ++i2) {
        const double ki = Ph[i2] * inv;
#pragma unroll
        for (int k = i2; k < NS; ++k) C[i2][k] -= ki * Ph[k];
    }
    return ok;
}

template <int P, int NOFF, int RB>
__global__ void __launch_bounds__(256) gpcc_markov_multi(const GpccMarkovMultiArgs a)
{
    constexpr int NS = P + NOFF;
    static_assert(RB == 1 || RB % 2 == 0, "a block is read as runs of two doubles");
    extern __shared__ __attribute__((aligned(16))) double gpcc_mkm_lds[];
    const GpccMkLane ln = gpcc_mk_open(a, gpcc_mkm_lds);

    double lam, lam2, Q[P][P], mu0[NS], C[NS][NS], mu[RB][NS], ll[RB];
    gpcc_mk_init<P, NOFF>(ln.rho, a.sigma_b, lam, lam2, Q, mu0, C);
#pragma unroll
    for (int k = 0; k < RB; ++k) {
        ll[k] = 0.0;
#pragma unroll
        for (int i2 = 0; i2 < NS; ++i2) mu[k][i2] = 0.0;
    }
    const double *res = a.res + (long)blockIdx.y * a.N * RB;

    double sprev = 0.0;
    int info = ln.info;
    for (int j = 0; j < a.N; ++j) {
        const GpccMkPoint p = gpcc_mk_next<false>(a, ln, j, sprev);
        const long i = ln.scur[p.b * ln.nthr + ln.tid] - 1;   // the point taken: the cursor has moved past it
        double r[RB];
        if constexpr (RB == 1) {
            r[0] = res[i];
        } else {
            const double2 *run = (const double2 *)(res + i * RB);
#pragma unroll
            for (int k = 0; k < RB / 2; ++k) {
                const double2 v = run[k];
                r[2 * k] = v.x;
                r[2 * k + 1] = v.y;
            }
        }
        double A[P][P];
        gpcc_mk_transition<P>(lam, lam2, p.d, A);
        gpcc_mk_propagate<P, NOFF>(A, Q, mu0, C);      // (the covariance; mu0 stays 0 and costs nothing)
        gpcc_mk_propagate_means<P, NOFF, RB>(A, mu);
        const bool ok = gpcc_mk_update_multi<P, NOFF, RB>(p.b, p.al, r, p.s2, mu, C, ll);
        info = (info == 0 && !ok) ? j + 1 : info;
    }
    if (ln.valid) {
        const long r0 = (long)blockIdx.y * RB;
#pragma unroll
        for (int k = 0; k < RB; ++k)
            if (r0 + k < a.R) a.out_loglik[ln.row * a.ldo + r0 + k] = info ? __builtin_nan("") : ll[k];
        if (blockIdx.y == 0) a.out_info[ln.row] = info;
    }
}

// WHAT SHIPS: every <P, NOFF> of the filter, each with RB = 8 realisations per lane.  Registers per lane (tools/kernel_resources.py,
// profiles/markov/kernel_resources.log), no scratch memory in any of them: see DESIGN.md 4.23.
struct GpccMkShipsMulti {
    static constexpr int max_noff[3] = {GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS};
    static constexpr int rb(int /* p */, int /* noff */) { return 8; }
};

// the realisations a lane of <p, noff> carries; 0: not shipped
static inline int gpcc_markov_multi_rb(int p, int noff)
{
    return gpcc_mk_ships<GpccMkShipsMulti>(p, noff) ? GpccMkShipsMulti::rb(p, noff) : 0;
}

// gpcc_markov_multi_pack on (ceil(N / 256), blocks) (gpcc_markov_multi_inst.hip: the object with P = 1)
hipError_t gpcc_markov_multi_pack_launch(const GpccMarkovMultiPackArgs &a, hipStream_t s);
// gpcc_markov_multi<g.p, g.noff, rb> on the grid (g.blocks, blocks)
hipError_t gpcc_markov_multi_launch(const GpccMkLaunch &g, int blocks, const GpccMarkovMultiArgs &a);
