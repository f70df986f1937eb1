// gpcc_markov_pred.hip.h -- linear-time predictions, held-out log-likelihoods and the offsets' posterior of the Markov kernels (OU,
// Matern-3/2, Matern-5/2) for gfx950: gpcc_predict_markov_batch, gpcc_heldout_loglik_markov_batch and
// gpcc_posterior_offsets_markov_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py (predict, heldout,
// posterior_offsets) is the same algorithm in numpy.  The state-space model and the filter's step (gpcc_mk_*) are gpcc_markov.hip.h's;
// nothing is approximated.  This file owns the walk in either direction over training and test bands (GpccMkpLane, gpcc_mkp_rewind,
// gpcc_mkp_next), which gpcc_markov_draw and gpcc_markov_loo_taps share.
//
// gpcc_markov_taps<P, NOFF, MODE>: ONE LANE PER (ROW, blockIdx.y).  The filter of gpcc_markov_eval with the same register-resident
// state and the same functions, walking a 2L-way merge: L training streams that update the state and L test streams.
//   MODE = GPCC_MKP_TAP     blockIdx.y = 0: the forward filter (ascending shifted time); 1: the backward filter (descending shifted
//                           time, lags |d|; the process reversed in time is the same process with f' negated, which the combine
//                           applies).  A test point is tapped: a COPY of the state is propagated to it and stored to the scratch
//                           [direction][test point][component][row], so that a wave's stores coalesce; the filter's own chain is not
//                           split, so lane 0's log-likelihood is bitwise gpcc_markov_eval's.  Ties in shifted time (gpcc_mkp_next): a
//                           training point that ties with a test point is on the forward side only (forward: training first;
//                           backward: test first).
//   MODE = GPCC_MKP_UPDATE  blockIdx.y = 0: the training filter alone; 1: the filter over training U test, the test points being
//                           observations (residual and variance from tpts).  Their difference is the held-out log-likelihood.
//                           Lane 0 can store the offset block of its final state (the offsets' posterior).
// The direction is uniform per workgroup, never a per-lane branch.  Lanes beyond the chunk's rows compute its last row again and store
// nothing.  No atomics, no communication between lanes: a row's bits do not depend on M, the chunking, the row order or the launch.
//
// gpcc_markov_combine<P, NOFF>: one lane per (row, test point): P_s = (P_f^-1 + P_b^-1 - P0^-1)^-1, m_s = P_s (P_f^-1 m_f + P_b^-1 m_b)
// with everything scaled by diag(P0)^-1/2 (Sigma_b is ~1e4 times the process variance), three Cholesky factorisations of n <= 7 in
// registers; mu* = h'm_s + mean(y_band), var* = h'P_s h + JITTER.  A pivot that is not positive and finite writes NaN;
// gpcc_markov_rowinfo turns the first NaN of a row into info = N + j and the whole row into NaN.
#pragma once
#include "gpcc_markov.hip.h"

#define GPCC_MKP_TAP 1
#define GPCC_MKP_UPDATE 2
#define GPCC_MKP_LANE_BYTES 40             /* per lane and band: two heads, tau, alpha (doubles) and two cursors (ints) */
#define GPCC_MKP_JITTER 1e-8

// GpccMarkovArgs' fields under the same names (the host fills both through one template) and what the test points add.  Not derived from
// it: the kernel-argument layout that gives moves the register allocation of gpcc_markov_taps<.., GPCC_MKP_UPDATE>
struct GpccMarkovPredArgs {
    const double *pts;                     // t[N] | r[N] | sigma^2[N], as GpccMarkovArgs
    const double *tpts;                    // test points, each band sorted by time: t[T] (TAP), t[T] | r[T] | sigma^2 + JITTER [T] (UPDATE)
    const double *delays, *alpha, *rho;    // the batch's rows: M x L, M x L, M
    double *out_loglik;                    // lane 0: per row of the batch
    int *out_info;
    double *tap;                           // TAP: [2][T][NS + NS (NS + 1) / 2][mstride]
    double *ll2;                           // UPDATE, lane 1: per row of the batch; info2: its merged position of failure, at2: the test
    int *info2, *at2;                      //   point (sorted index) met there or last before it
    double *fin;                           // lane 0, or NULL: [NOFF + NOFF (NOFF + 1) / 2][M], the offset block of the final state
    int M, L, N, T, stage;                 // stage: copy pts and tpts to LDS first
    int row0, rows, mstride;               // the chunk: rows row0 .. row0 + rows - 1 of the batch, row stride of tap
    int off[GPCC_MARKOV_MAXL + 1], toff[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
};

struct GpccMarkovCombineArgs {
    const double *tap, *alpha, *rho;       // alpha, rho: the batch's rows
    const int *tband, *tperm;              // per sorted test point: its band and its position in the caller's order
    double *mu, *var;                      // [rows][T], the caller's order
    int L, T, row0, rows, mstride;
    double mean_b[GPCC_MARKOV_MAXL], sigma_b[GPCC_MARKOV_MAX_OFFSETS];
};

static inline size_t gpcc_mkp_lds_bytes(int N, int T, int tw, int L, int threads, bool stage)
{
    return (stage ? (size_t)24 * N + (size_t)8 * tw * T : 0) + (size_t)GPCC_MKP_LANE_BYTES * L * threads;
}

// ---- the walk in either direction, shared by gpcc_markov_taps below, gpcc_markov_draw (gpcc_markov_sample.hip.h) and
// gpcc_markov_loo_taps (gpcc_markov_loo.hip.h).  A stream is L bands of sorted points (band l: off[l] .. off[l + 1] - 1) with its
// cursors and heads in L slots of the lane's arrays: the training stream in slots 0 .. L - 1, the test stream in L .. 2L - 1.  A head
// is the KEY of the band's next point: its shifted time walking forward, minus that walking backward (rev), so the smallest key is
// next and a lag is a difference of keys.  Each kernel stages its points in its own layout and names the two time arrays ----

struct GpccMkpLane {
    const double *t, *tt;                  // the times of the training and of the test points (LDS when staged)
    double *shead, *stau;                  // LDS: heads [slot][thread], tau [band][thread]
    int *scur;                             // LDS: cursors [slot][thread]
    int nthr, tid;
};

// the point taken: of the test stream or not, its band, its index and its key
struct GpccMkpPoint {
    bool is_test;
    int band, i;
    double key;
};

// every band's cursor to its first point of the direction (rev: its last), and its head; TESTS: both streams, else the training one
template <bool TESTS, class ARGS>
__device__ __forceinline__ void gpcc_mkp_rewind(const ARGS &a, const GpccMkpLane &c, bool rev)
{
    const int L = a.L, nthr = c.nthr, tid = c.tid;
    for (int l = 0; l < L; ++l) {
        const int i0 = rev ? a.off[l + 1] - 1 : a.off[l];
        c.scur[l * nthr + tid] = i0;
        const double base = c.t[i0] - c.stau[l * nthr + tid];
        c.shead[l * nthr + tid] = rev ? -base : base;
        if constexpr (TESTS) {
            const int q0 = rev ? a.toff[l + 1] - 1 : a.toff[l];
            c.scur[(L + l) * nthr + tid] = q0;
            if (a.toff[l + 1] > a.toff[l]) {
                const double tb = c.tt[q0] - c.stau[l * nthr + tid];
                c.shead[(L + l) * nthr + tid] = rev ? -tb : tb;
            }
        }
    }
}

// one stream's merge (slots slot0 .. slot0 + L - 1): b, the band with points left whose head has the smallest key (-1: none left),
// and the key s.  Ties: the lowest band in both directions; REVERSE_TIES: the highest band when rev
template <bool REVERSE_TIES>
__device__ __forceinline__ void gpcc_mkp_pick(const GpccMkpLane &c, const int (&off)[GPCC_MARKOV_MAXL + 1], int L, int slot0, bool rev, int &b,
                                              double &s)
{
    b = -1;
    s = 0.0;
    for (int l = 0; l < L; ++l) {
        const double sl = c.shead[(slot0 + l) * c.nthr + c.tid];
        const int i = c.scur[(slot0 + l) * c.nthr + c.tid];
        const bool live = rev ? i >= off[l] : i < off[l + 1];
        const bool take = live && (b < 0 || sl < s || (REVERSE_TIES && rev && sl == s));
        b = take ? l : b;
        s = take ? sl : s;
    }
}

// takes the point at the head of the slot at k (= slot * nthr + tid): its index; the cursor moves on
__device__ __forceinline__ int gpcc_mkp_advance(const GpccMkpLane &c, int k, bool rev)
{
    const int i = c.scur[k];
    c.scur[k] = i + (rev ? -1 : 1);
    return i;
}

// the head at k once point i of band b of the training (TEST: the test) stream is taken: the key of the band's next point, if any
template <bool TEST, class ARGS>
__device__ __forceinline__ void gpcc_mkp_refill(const ARGS &a, const GpccMkpLane &c, int k, int b, int i, bool rev)
{
    const double *t = c.t;
    const int *off = a.off;
    if constexpr (TEST) {
        t = c.tt;
        off = a.toff;
    }
    if (rev ? i - 1 >= off[b] : i + 1 < off[b + 1]) {
        const double base = t[i + (rev ? -1 : 1)] - c.stau[b * c.nthr + c.tid];
        c.shead[k] = rev ? -base : base;
    }
}

// one step over both streams (use_tests false: the training stream alone).  A training point goes first on ties, except walking
// backward, where the tying training point belongs to the forward side
template <class ARGS>
__device__ __forceinline__ GpccMkpPoint gpcc_mkp_next(const ARGS &a, const GpccMkpLane &c, bool rev, bool use_tests)
{
    int b, q = -1;
    double s, sq = 0.0;
    gpcc_mkp_pick<false>(c, a.off, a.L, 0, rev, b, s);
    if (use_tests) gpcc_mkp_pick<false>(c, a.toff, a.L, a.L, rev, q, sq);
    GpccMkpPoint p;
    p.is_test = q >= 0 && (b < 0 || sq < s || (rev && sq == s));
    p.band = p.is_test ? q : b;
    p.key = p.is_test ? sq : s;
    const int k = (p.is_test ? a.L + q : b) * c.nthr + c.tid;
    p.i = gpcc_mkp_advance(c, k, rev);
    if (p.is_test)
        gpcc_mkp_refill<true>(a, c, k, q, p.i, rev);
    else
        gpcc_mkp_refill<false>(a, c, k, b, p.i, rev);
    return p;
}

// one step over the training stream alone, with the tie rule as a parameter: REVERSE_TIES makes the backward walk the exact reverse
// of the forward one, which gpcc_markov_loo_taps needs and the two-stream walks do not have (markov.py mirrors both rules)
template <bool REVERSE_TIES, class ARGS>
__device__ __forceinline__ GpccMkpPoint gpcc_mkp_next(const ARGS &a, const GpccMkpLane &c, bool rev)
{
    GpccMkpPoint p;
    p.is_test = false;
    gpcc_mkp_pick<REVERSE_TIES>(c, a.off, a.L, 0, rev, p.band, p.key);
    p.i = gpcc_mkp_advance(c, p.band * c.nthr + c.tid, rev);
    gpcc_mkp_refill<false>(a, c, p.band * c.nthr + c.tid, p.band, p.i, rev);
    return p;
}

template <int P, int NOFF, int MODE>
__global__ void __launch_bounds__(256) gpcc_markov_taps(const GpccMarkovPredArgs a)
{
    constexpr int NS = P + NOFF, NREC = NS + NS * (NS + 1) / 2, TW = MODE == GPCC_MKP_TAP ? 1 : 3;
    extern __shared__ __attribute__((aligned(16))) double gpcc_mkp_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x, L = a.L, N = a.N, T = a.T;
    const int kind = blockIdx.y;                                  // uniform per workgroup
    const bool rev = MODE == GPCC_MKP_TAP && kind == 1;           // descending shifted time
    const bool use_tests = MODE == GPCC_MKP_TAP || kind == 1;     // (the training-only lane of UPDATE walks no test stream)
    const long nstage = a.stage ? 3L * N + (long)TW * T : 0;
    double *shead = gpcc_mkp_lds + nstage;                        // [2L][nthr]: training bands, then test bands
    double *stau = shead + 2 * L * nthr, *salpha = stau + L * nthr;
    int *scur = (int *)(salpha + L * nthr);                       // [2L][nthr]
    if (a.stage) {
        for (int i = tid; i < 3 * N; i += nthr) gpcc_mkp_lds[i] = a.pts[i];
        for (int i = tid; i < TW * T; i += nthr) gpcc_mkp_lds[3L * N + i] = a.tpts[i];
    }
    const double *pts = a.stage ? (const double *)gpcc_mkp_lds : a.pts;
    const double *tpts = a.stage ? (const double *)(gpcc_mkp_lds + 3L * N) : a.tpts;

    const int lrow = (int)blockIdx.x * nthr + tid;
    const bool valid = lrow < a.rows;
    const long m_ = a.row0 + (valid ? lrow : a.rows - 1);
    const double rho = a.rho[m_];
    int info = gpcc_mk_load_row(a, m_, rho, stau, salpha, nthr, tid);
    __syncthreads();
    const GpccMkpLane cur = {pts, tpts, shead, stau, scur, nthr, tid};
    gpcc_mkp_rewind<true>(a, cur, rev);

    double lam, lam2, Q[P][P], mu[NS], C[NS][NS];
    gpcc_mk_init<P, NOFF>(rho, a.sigma_b, lam, lam2, Q, mu, C);

    double ll = 0.0, sprev = 0.0;
    int jt = 0, at = 0;         // jt: updates so far
    const int total = N + (use_tests ? T : 0);
    for (int j = 0; j < total; ++j) {
        // the point taken: its band, key, residual and variance (a tapped test point has none and ends the step)
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
        // one filter step, as in gpcc_markov_eval
        const double al = salpha[p.band * nthr + tid];
        const double d = (jt == 0) ? 0.0 : p.key - sprev;
        sprev = p.key;
        double A[P][P];
        gpcc_mk_transition<P>(lam, lam2, d, A);
        gpcc_mk_propagate<P, NOFF>(A, Q, mu, C);
        const bool ok = gpcc_mk_update<P, NOFF>(p.band, al, r, s2, mu, C, ll);
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

// inv(A) of a symmetric positive definite A (full storage) by Cholesky, everything in registers; false: a pivot is not positive and finite
template <int NS>
__device__ __forceinline__ bool gpcc_mkp_spd_inverse(const double (&A)[NS][NS], double (&Inv)[NS][NS])
{
    double G[NS][NS], Gi[NS][NS];   // lower factor and its inverse
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= G[j][k] * G[j][k];
        ok = ok && d > 0.0 && d < __builtin_inf();
        const double g = sqrt(d), ig = 1.0 / g;
        G[j][j] = g;
#pragma unroll
        for (int i = j + 1; i < NS; ++i) {
            double v = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= G[i][k] * G[j][k];
            G[i][j] = v * ig;
        }
        // column j of inv(G) above and on the diagonal is known once row j of G is: Gi[j][c] = -(sum_{k<j} G[j][k] Gi[k][c]) / g
        Gi[j][j] = ig;
#pragma unroll
        for (int c = 0; c < j; ++c) {
            double v = 0.0;
#pragma unroll
            for (int k = c; k < j; ++k) v += G[j][k] * Gi[k][c];
            Gi[j][c] = -v * ig;
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = i; j < NS; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = j; k < NS; ++k) v += Gi[k][i] * Gi[k][j];
            Inv[i][j] = Inv[j][i] = v;
        }
    return ok;
}

// one lane per (row of the chunk, sorted test point): grid (ceil(rows / 64), T), 64 threads
// (gpcc_markov_loo_combine of gpcc_markov_loo.hip.h carries a copy of this arithmetic: a fix here belongs there too)
template <int P, int NOFF>
__global__ void __launch_bounds__(64) gpcc_markov_combine(const GpccMarkovCombineArgs a)
{
    constexpr int NS = P + NOFF, NREC = NS + NS * (NS + 1) / 2;
    const int lrow = (int)blockIdx.x * 64 + (int)threadIdx.x, tj = blockIdx.y;
    if (lrow >= a.rows) return;
    const long row = a.row0 + lrow;
    const int qb = a.tband[tj];
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
        const double *rec = a.tap + (((long)dir * a.T + tj) * NREC) * a.mstride + lrow;
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
    ok = ok && var == var && mean == mean;
    const long o = (long)lrow * a.T + a.tperm[tj];
    a.mu[o] = ok ? mean + a.mean_b[qb] : __builtin_nan("");
    a.var[o] = ok ? var + GPCC_MKP_JITTER : __builtin_nan("");
}

// ---- launches (gpcc_markov_pred_inst.hip: an object of its own) ----
// mode GPCC_MKP_TAP / GPCC_MKP_UPDATE (two kernels); grid (g.blocks, ny)
hipError_t gpcc_mkp_launch_taps(const GpccMkLaunch &g, int mode, int ny, const GpccMarkovPredArgs &a);
// grid (ceil(rows / 64), T), 64 threads
hipError_t gpcc_mkp_launch_combine(int p, int noff, const GpccMarkovCombineArgs &a, hipStream_t s);
// per row of the chunk: a failed training filter (info != 0) makes the row NaN; else the first NaN of the row (caller's order, j from
// 0) sets info = N + j + 1 and makes the row NaN
hipError_t gpcc_mkp_launch_rowinfo(double *mu, double *var, int *info, int N, int T, int row0, int rows, hipStream_t s);
// the running mixture of gpcc_predict_batch over the chunk's rows in row order; mix: 6 x T (W, mean, S, V, mix_mu, mix_var), zeroed
// before the first chunk; last: writes mix_mu and mix_var
hipError_t gpcc_mkp_launch_mix(const double *mu, const double *var, const double *p, double *mix, int T, int row0, int rows, int last,
                               hipStream_t s);
// heldout[m] = ll2 - loglik (NaN where either filter failed; the union filter's failure sets info = N + tperm[at2] + 1), then, with p,
// gpcc_heldout_loglik_batch's row-order log-sum-exp into mix[3]
hipError_t gpcc_mkp_launch_heldout_finish(const double *loglik, int *info, const double *ll2, const int *info2, const int *at2,
                                          const int *tperm, double *heldout, const double *p, double *mix, int N, int M, hipStream_t s);
