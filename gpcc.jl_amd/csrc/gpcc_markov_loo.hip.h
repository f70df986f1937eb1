// gpcc_markov_loo.hip.h -- exact leave-one-out predictive scores of the Markov kernels (OU, Matern-3/2, Matern-5/2) in linear time for
// gfx950: gpcc_loo_markov_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py (loo) is the same algorithm in numpy.  The
// state-space model and the filter's step (gpcc_mk_*) are gpcc_markov.hip.h's, the small inverse gpcc_markov_pred.hip.h's; nothing is
// approximated.
//
// The posterior of the process at training point i given every OTHER observation is the two-filter combine of DESIGN.md 4.16 taken at
// the point itself: the forward filter's state propagated to s_i BEFORE the update with point i, and the backward filter's likewise.
//
// gpcc_markov_loo_taps<P, NOFF>: ONE LANE PER (ROW, blockIdx.y).  blockIdx.y = 0: the filter of gpcc_markov_eval over the L-way merge
//   of the bands in ascending shifted time (the lowest band first on ties); 1: the same points in exactly the reverse order
//   (descending shifted time, the highest band first on ties, each band from its last point), lags |d| -- so every other point, tied
//   or not, is on exactly one side of i.  The cursor is gpcc_markov_pred.hip.h's one-stream gpcc_mkp_next<true>: NOT
//   gpcc_markov_taps' rule, which takes the lowest band in both directions.  At each point the state after gpcc_mk_propagate and
//   before gpcc_mk_update is stored to the scratch [direction][point][component][row] (a wave's stores coalesce); the filter's chain
//   is gpcc_markov_eval's, one call site of each step function, so lane 0's log-likelihood and info are its bits.  The direction is
//   uniform per workgroup.  Lanes beyond the chunk's rows compute its last row again and store nothing.
// gpcc_markov_loo_combine<P, NOFF>: one lane per (row, point): P_s = (P_f^-1 + P_b^-1 - P0^-1)^-1, m_s = P_s (P_f^-1 m_f + P_b^-1 m_b),
//   scaled by diag(P0)^-1/2, the backward state mapped by D = diag(1, -1, 1); with h of the point's band
//       mu_i = h'm_s + mean(y_band),  var_i = h'P_s h + sigma_i^2,  lp_i = -(log 2 pi + log var_i + (y_i - mu_i)^2 / var_i) / 2,
//   written at the point's position in the caller's order.  A pivot that is not positive and finite writes NaN.
// gpcc_markov_loo_rows: per row, info = N + i for the first point (caller's order) whose variance is not positive and finite, NaN
//   where the row failed, and loo = sum_i lp_i in a fixed order.
// No atomics, no communication between rows: a row's bits do not depend on M, the chunking, the row order or the launch shape.
#pragma once
#include "gpcc_markov_pred.hip.h"

struct GpccMarkovLooArgs {
    const double *pts;                     // t[N] | r[N] | sigma^2[N], as GpccMarkovArgs
    const double *delays, *alpha, *rho;    // the batch's rows: M x L, M x L, M
    double *out_loglik;                    // lane 0: per row of the batch
    int *out_info;
    double *tap;                           // [2][N][NS + NS (NS + 1) / 2][mstride]
    int M, L, N, stage;                    // stage: copy pts to LDS first
    int row0, rows, mstride;               // the chunk: rows row0 .. row0 + rows - 1 of the batch, row stride of tap
    int off[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
};

struct GpccMarkovLooCombineArgs {
    const double *tap, *alpha, *rho;       // alpha, rho: the batch's rows
    const double *pts;                     // as above (r and sigma^2 of the sorted points)
    const int *pband, *pperm;              // per sorted point: its band and its position in the caller's order
    double *mu, *var, *lp;                 // [rows][N], the caller's order
    int L, N, row0, rows, mstride;
    double mean_b[GPCC_MARKOV_MAXL], sigma_b[GPCC_MARKOV_MAX_OFFSETS];
};

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_loo_taps(const GpccMarkovLooArgs a)
{
    constexpr int NS = P + NOFF, NREC = NS + NS * (NS + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) double gpcc_mkl_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x, L = a.L, N = a.N;
    const int kind = blockIdx.y;          // uniform per workgroup
    const bool rev = kind == 1;           // the reverse of the merged order
    double *shead = gpcc_mkl_lds + (a.stage ? 3L * N : 0);
    double *stau = shead + L * nthr, *salpha = stau + L * nthr;
    int *scur = (int *)(salpha + L * nthr);
    if (a.stage)
        for (int i = tid; i < 3 * N; i += nthr) gpcc_mkl_lds[i] = a.pts[i];
    const double *pts = a.stage ? (const double *)gpcc_mkl_lds : a.pts;

    const int lrow = (int)blockIdx.x * nthr + tid;
    const bool valid = lrow < a.rows;
    const long m_ = a.row0 + (valid ? lrow : a.rows - 1);
    const double rho = a.rho[m_];
    int info = gpcc_mk_load_row(a, m_, rho, stau, salpha, nthr, tid);
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
        const double s = p.key, r = pts[N + i], s2 = pts[2 * N + i], al = salpha[b * nthr + tid];
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

// one lane per (row of the chunk, sorted point): grid (N, ceil(rows / 64)), 64 threads -- the point on grid.x, which has no 65535
// limit (gpcc_create takes N up to 65536).  The arithmetic is gpcc_markov_combine's (gpcc_markov_pred.hip.h) up to h'm_s and h'P_s h,
// copied and not shared so that the existing kernel keeps its bits: a fix to either belongs in both.
// ARGS: GpccMarkovLooCombineArgs, or GpccMarkovNoiseLooCombineArgs (gpcc_markov_noise_pred.hip.h: the same fields and the rows' kappa,
// nu), on which the point's variance is the one its row's noise model gives it; the plain instantiation compiles the statements it had.
template <int P, int NOFF, class ARGS = GpccMarkovLooCombineArgs>
__global__ void __launch_bounds__(64) gpcc_markov_loo_combine(const ARGS a)
{
    constexpr int NS = P + NOFF, NREC = NS + NS * (NS + 1) / 2;
    const int lrow = (int)blockIdx.y * 64 + (int)threadIdx.x, pj = blockIdx.x;
    if (lrow >= a.rows) return;
    const long row = a.row0 + lrow;
    const int qb = a.pband[pj];
    const double rho = a.rho[row], al = a.alpha[row * a.L + qb];
    const double lam = gpcc_mk_rate<P>(rho);
    // sc = diag(P0)^-1/2; sgn = D, the time reversal of the backward state
    double sc[NS], sgn[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) { sc[i] = 1.0; sgn[i] = 1.0; }
    if constexpr (P == 2) sc[1] = 1.0 / lam;
    if constexpr (P == 3) { sc[1] = 1.7320508075688772 / lam; sc[2] = 1.0 / (lam * lam); }
    if constexpr (P >= 2) sgn[1] = -1.0;
#pragma unroll
    for (int c = 0; c < NOFF; ++c) sc[P + c] = 1.0 / sqrt(a.sigma_b[c]);

    double Lam[NS][NS], eta[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        eta[i] = 0.0;
#pragma unroll
        for (int j = 0; j < NS; ++j) Lam[i][j] = 0.0;
    }
    bool ok = true;
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        const double *rec = a.tap + (((long)dir * a.N + pj) * NREC) * a.mstride + lrow;
        double m[NS], F[NS][NS], Fi[NS][NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) m[i] = rec[(long)i * a.mstride] * sc[i] * (dir ? sgn[i] : 1.0);
        int c = NS;
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int j = i; j < NS; ++j) {
                const double v = rec[(long)(c++) * a.mstride] * (sc[i] * sc[j]) * (dir ? sgn[i] * sgn[j] : 1.0);
                F[i][j] = F[j][i] = v;
            }
        ok = gpcc_mkp_spd_inverse<NS>(F, Fi) && ok;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            double v = 0.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                v += Fi[i][j] * m[j];
                Lam[i][j] += Fi[i][j];
            }
            eta[i] += v;
        }
    }
    // - inv(P0), scaled: the identity, except Matern-5/2's (f, f'') block [[1, -1/3], [-1/3, 1]]^-1 = [[9/8, 3/8], [3/8, 9/8]]
#pragma unroll
    for (int i = 0; i < NS; ++i) Lam[i][i] -= (P == 3 && (i == 0 || i == 2)) ? 1.125 : 1.0;
    if constexpr (P == 3) {
        Lam[0][2] -= 0.375;
        Lam[2][0] -= 0.375;
    }
    double Ps[NS][NS];
    ok = gpcc_mkp_spd_inverse<NS>(Lam, Ps) && ok;
    // h scaled: alpha e_1 + sqrt(Sigma_b) e_{P + band}
    double h[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) h[i] = 0.0;
    h[0] = al;
#pragma unroll
    for (int c = 0; c < NOFF; ++c) h[P + c] = (qb == c) ? sqrt(a.sigma_b[c]) : 0.0;
    double mean = 0.0, var = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double pe = 0.0, ph = 0.0;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            pe += Ps[i][j] * eta[j];
            ph += Ps[i][j] * h[j];
        }
        mean += h[i] * pe;
        var += h[i] * ph;
    }
    if constexpr (std::is_same_v<ARGS, GpccMarkovLooCombineArgs>) {
        var += a.pts[2L * a.N + pj];
    } else {   // the tap lane's expression: fma(kappa_b^2, sigma_i^2, nu_b)
        const double k = a.kappa[row * a.L + qb];
        var += fma(k * k, a.pts[2L * a.N + pj], a.nu[row * a.L + qb]);
    }
    ok = ok && var > 0.0 && var < __builtin_inf() && mean == mean;
    const double e = a.pts[(long)a.N + pj] - mean, nan = __builtin_nan("");   // y_i - mu_i: the residual against the band mean
    const long o = (long)lrow * a.N + a.pperm[pj];
    a.mu[o] = ok ? mean + a.mean_b[qb] : nan;
    a.var[o] = ok ? var : nan;
    a.lp[o] = ok ? -0.5 * (1.8378770664093453 + log(var) + e * e / var) : nan;
}

static inline size_t gpcc_mkl_lds_bytes(int N, int L, int threads, bool stage) { return gpcc_markov_lds_bytes(N, L, threads, stage); }

// ---- launches (gpcc_markov_loo_inst.hip: an object of its own) ----
// grid (g.blocks, 2): the forward and the backward filter
hipError_t gpcc_mkl_launch_taps(const GpccMkLaunch &g, const GpccMarkovLooArgs &a);
// grid (N, ceil(rows / 64)), 64 threads
hipError_t gpcc_mkl_launch_combine(int p, int noff, const GpccMarkovLooCombineArgs &a, hipStream_t s);
// per row of the chunk (mu, var, lp: [rows][N]): a failed filter (info != 0) makes the row NaN; else the first NaN of var (caller's
// order, i from 0) sets info = N + i + 1 and makes the row NaN; loo[row0 + row] = sum_i lp_i (NaN for a failed row)
hipError_t gpcc_mkl_launch_rows(double *mu, double *var, double *lp, double *loo, int *info, int N, int row0, int rows, hipStream_t s);
