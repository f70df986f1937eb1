// gpcc_markov_sample.hip.h -- joint posterior draws of the Markov kernels (OU, Matern-3/2, Matern-5/2) in linear time for gfx950:
// gpcc_sample_markov_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py (prior_draw, sample) is the same algorithm in
// numpy.  Matheron's rule: a posterior draw is a prior draw plus the posterior-mean correction of the prior draw's synthetic data,
//   f*_j = mu_j + g~_j - c_j + sqrt(JITTER + sigma*_j^2) xi,
// mu the mean of gpcc_predict_markov_batch, (r~, g~) a draw of the prior at the training and test points and c the smoother of 4.16
// applied to r~.  The filter's step is gpcc_markov.hip.h's (gpcc_mk_*), unchanged; no T x T factor, no N^2 workspace.
//
// gpcc_markov_combine_w<P, NOFF>: gpcc_markov_combine with one more output.  The smoother's covariances do not depend on the data, so
// c_j = w_f,j . m_f,j + w_b,j . m_b,j with w_dir,j = sc o D_dir o (P_dir^-1 P_s h) per (row, test point): 2 NS doubles next to mu and var,
// in the taps' layout [direction][test point][component][row].  (A kernel of its own: gpcc_markov_combine keeps its code object.)
//
// gpcc_markov_draw<P, NOFF>: ONE LANE PER (ROW, DRAW), gpcc_markov_taps' lane -- state in registers, cursors / heads / tau / alpha in
// LDS [band][thread], the points staged in LDS when they fit (in this kernel's own layout) -- walking the merged training and test
// points twice, each time with the shared cursor of gpcc_markov_pred.hip.h (gpcc_mkp_rewind, gpcc_mkp_next).
//   forward   the point's Philox block (counter (e, s, m, 2): e the POINT, not the merged position) gives four normals; the simulated
//             state x~ <- A(d) x~ + C xi[0 .. P) with C C' = Pinf - A Pinf A' (gpcc_mks_advance; A = 0 at the first point; d = 0 gives
//             C = 0: tied points share one state).  Training point: r~ = alpha x~_1 + b~ + sigma xi[3] goes to the scratch [point][lane] and
//             through the filter step in place of r.  Test point: acc = g~ + sqrt(JITTER + sigma*^2) xi[3] - w_f . (the filter's mean
//             propagated to it, on a copy) goes to the scratch [test point][lane].
//   backward  the filter over r~ read back, descending: acc -= w_b . (its mean propagated to the test point).
// gpcc_markov_draw_finish adds mu and transposes acc through LDS into the caller's rows.  The host sorts the lanes by row, so a wave's
// lanes mostly share tau, alpha and the merge.  No atomics, no communication between lanes: a draw's bits depend on the seed, the
// row's parameters, s and the row word m alone -- not on M, S, the chunking or the launch.
//
// The process noise Q = Pinf - A Pinf A' of the simulated state is NOT formed by that difference where the lag is small (the filter's
// own propagation, gpcc_mk_propagate, is left as it is): see gpcc_mks_advance.
#pragma once
#include "gpcc_markov_pred.hip.h"
#include "gpcc_rng.h"

#define GPCC_MKS_STREAM 2                  /* word 3 of the Philox counter: 0 the dense normals, 1 the row picks */
#define GPCC_MKS_POINT_BYTES 20            /* staged per training or test point: time, sigma^2 or noise sd (doubles), the point's index (int) */
#define GPCC_MKS_SCRATCH_BYTES ((long)128 << 20)
#define GPCC_MKS_SERIES_MAX 1.0            /* the largest x = lambda d whose process noise takes the series (markov.SIM_SERIES_MAX) */
#define GPCC_MKS_SERIES_TERMS 26           /* the tail after 26 terms at y = 2 is below 1e-20 of the sum (markov.SIM_SERIES_TERMS) */

struct GpccMarkovDrawArgs {
    const double *pts;                     // t[N] | r[N] | sigma^2[N], as GpccMarkovArgs (r is not read)
    const int *perm;                       // [N]: sorted training point -> its index in gpcc_create's flattened order
    const double *tpts;                    // t*[T] | sqrt(JITTER + sigma*^2)[T], each band sorted by time
    const int *tperm;                      // [T]: sorted test point -> its index in the caller's flattened order
    const double *delays, *alpha, *rho;    // the (compacted) rows: Mc x L, Mc x L, Mc
    const double *w;                       // gpcc_markov_combine_w's weights of the row chunk: [2][T][NS][mstride]
    const int *lane_row, *lane_s;          // per lane of the call: its row (compacted) and its draw index s
    const int *row_word;                   // per compacted row: the row word m of its counters (per-row mode)
    double *rt, *acc;                      // scratch [N][lstride], [T][lstride]: acc in the CALLER's test order
    unsigned long long seed;
    int mixture;                           // the row word is 2^64 - 1
    int L, N, T, stage;
    int row0, mstride;                     // the row chunk: w holds rows row0 .. of the compacted batch, row stride mstride
    int lane0, lanes, lstride;             // the lane chunk: lanes lane0 .. lane0 + lanes - 1, lane stride of the scratch
    int off[GPCC_MARKOV_MAXL + 1], toff[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
};

struct GpccMarkovCombineWArgs {
    GpccMarkovCombineArgs c;
    double *w;                             // [2][T][NS][mstride]
};

struct GpccMarkovDrawFinishArgs {
    const double *mu, *acc;                // mu: [rows of the chunk][T]; acc: [T][lstride]
    const int *lane_row, *lane_out;        // per lane of the call: its row (compacted), its row of `draws`
    double *draws;                         // [D][T]
    int T, row0, lane0, lanes, lstride;
};

static inline size_t gpcc_mks_lds_bytes(int N, int T, int L, int threads, bool stage)
{
    return (stage ? (size_t)GPCC_MKS_POINT_BYTES * ((size_t)N + T) + 8 : 0) + (size_t)GPCC_MKP_LANE_BYTES * L * threads;
}

// j[k] = int_0^x u^k e^-2u du = gamma(k + 1, y) / 2^(k+1), y = 2x, k = 0 .. K, without cancellation: the top one by the all-positive
// series y^(K+1) e^-y sum_m y^m / ((K + 1) ... (K + 1 + m)), the others by gamma(k, y) = (gamma(k + 1, y) + y^k e^-y) / k
template <int K>
__device__ __forceinline__ void gpcc_mks_gammas(double x, double (&j)[K + 1])
{
    const double y = 2.0 * x, e = exp(-y);
    double term = 1.0 / (K + 1), acc = term, yp[K + 2];
#pragma unroll 1
    for (int m = 1; m < GPCC_MKS_SERIES_TERMS; ++m) {
        term = term * y / (double)(K + 1 + m);
        acc += term;
    }
    yp[0] = 1.0;
#pragma unroll
    for (int k = 1; k <= K + 1; ++k) yp[k] = yp[k - 1] * y;
    double g = yp[K + 1] * e * acc, half = 0.5;
    double gk[K + 1];
    gk[K] = g;
#pragma unroll
    for (int k = K; k > 0; --k) gk[k - 1] = (gk[k] + yp[k] * e) / (double)k;
#pragma unroll
    for (int k = 0; k <= K; ++k) {
        j[k] = gk[k] * half;
        half *= 0.5;
    }
}

// x~ a lag d later: x~ <- A x~ + C z[0 .. P), C C' = Q = Pinf - A Pinf A', factored in the units of diag(Pinf)^1/2.  Formed by that
// difference Q is a cancellation from a unit diagonal: at a small lag x = lambda d its diagonal is ~x^5, x^3, x (Matern-5/2) and
// drowns in the rounding of A.  For x <= GPCC_MKS_SERIES_MAX it is evaluated as what it is, Q = q int_0^d a(s) a(s)' ds with a(s) the
// last column of A(s) (q = 2 lambda, 4 lambda^3, 16 lambda^5 / 3): scaled and with u = lambda s
//     OU           1 - e^-2x
//     Matern-3/2   4 int b b' e^-2u du,        b = (u, 1 - u)
//     Matern-5/2   16/3 int b b' e^-2u du,     b = (u^2 / 2, sqrt3 u (1 - u / 2), 1 - 2u + u^2 / 2)
// every integral from gpcc_mks_gammas: each entry to a few eps of sqrt(Q_ii Q_jj) (markov.process_noise_scaled).  Beyond, where Q is
// of the order of Pinf, and at the first point (first: the stationary draw, A = 0) by the difference.  The factor is eliminated from
// the LAST component (the largest pivot) to the first, so C is upper triangular; a pivot that is not > 0 gives a zero column.
template <int P>
__device__ __forceinline__ void gpcc_mks_advance(double lam, double lam2, const double (&Pinf)[P][P], bool first, double d, const double *z,
                                                 double (&x)[P])
{
    double A[P][P], sc[P], G[P][P];
    gpcc_mk_transition<P>(lam, lam2, d, A);
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int k = 0; k < P; ++k) A[i][k] = first ? 0.0 : A[i][k];
    sc[0] = 1.0;
    if constexpr (P == 2) sc[1] = 1.0 / lam;
    if constexpr (P == 3) { sc[1] = 1.7320508075688772 / lam; sc[2] = 1.0 / lam2; }
    const double xl = lam * d;
    if (!first && xl <= GPCC_MKS_SERIES_MAX) {
        if constexpr (P == 1) {
            G[0][0] = -expm1(-2.0 * xl);
        } else if constexpr (P == 2) {
            double j[3];
            gpcc_mks_gammas<2>(xl, j);
            G[0][0] = 4.0 * j[2];
            G[0][1] = 4.0 * (j[1] - j[2]);
            G[1][1] = 4.0 * (j[0] - 2.0 * j[1] + j[2]);
        } else {
            double j[5];
            gpcc_mks_gammas<4>(xl, j);
            const double c = 16.0 / 3.0, s3 = 1.7320508075688772;
            G[0][0] = c * 0.25 * j[4];
            G[0][1] = c * (0.5 * s3) * (j[3] - 0.5 * j[4]);
            G[0][2] = c * (0.5 * j[2] - j[3] + 0.25 * j[4]);
            G[1][1] = c * 3.0 * (j[2] - j[3] + 0.25 * j[4]);
            G[1][2] = c * s3 * (j[1] - 2.5 * j[2] + 1.5 * j[3] - 0.25 * j[4]);
            G[2][2] = c * (j[0] - 4.0 * j[1] + 5.0 * j[2] - 2.0 * j[3] + 0.25 * j[4]);
        }
    } else {
        // B = A Pinf, Q = Pinf - B A' (scaled, upper triangle)
        double B[P][P];
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int k = 0; k < P; ++k) {
                double acc = 0.0;
#pragma unroll
                for (int q = 0; q < P; ++q) acc += A[i][q] * Pinf[q][k];
                B[i][k] = acc;
            }
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int k = i; k < P; ++k) {
                double acc = 0.0;
#pragma unroll
                for (int q = 0; q < P; ++q) acc += B[i][q] * A[k][q];
                G[i][k] = (Pinf[i][k] - acc) * (sc[i] * sc[k]);
            }
    }
    // in place: G <- the upper factor U, U U' = G, eliminated from the last component; zero columns where the pivot is not > 0
#pragma unroll
    for (int jj = 0; jj < P; ++jj) {
        const int j = P - 1 - jj;
        double piv = G[j][j];
#pragma unroll
        for (int k = j + 1; k < P; ++k) piv -= G[j][k] * G[j][k];
        const bool ok = piv > 0.0 && piv < __builtin_inf();
        const double g = ok ? sqrt(piv) : 0.0;
        G[j][j] = g;
#pragma unroll
        for (int i = 0; i < j; ++i) {
            double v = G[i][j];
#pragma unroll
            for (int k = j + 1; k < P; ++k) v -= G[i][k] * G[j][k];
            G[i][j] = ok ? v / g : 0.0;
        }
    }
    double xn[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        double ax = 0.0, cz = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) ax += A[i][k] * x[k];
#pragma unroll
        for (int k = i; k < P; ++k) cz += G[i][k] * z[k];
        xn[i] = ax + cz / sc[i];
    }
#pragma unroll
    for (int i = 0; i < P; ++i) x[i] = xn[i];
}

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_draw(const GpccMarkovDrawArgs a)
{
    constexpr int NS = P + NOFF;
    extern __shared__ __attribute__((aligned(16))) double gpcc_mks_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x, L = a.L, N = a.N, T = a.T;
    // staged: t[N] | sigma^2[N] | t*[T] | sd*[T] (doubles), then perm[N] | tperm[T] (ints, padded to a double), then the lanes' arrays
    const long nd = 2L * N + 2L * T, ni = ((long)N + T + 1) / 2;
    double *shead = gpcc_mks_lds + (a.stage ? nd + ni : 0);          // [2L][nthr]: training bands, then test bands
    double *stau = shead + 2 * L * nthr, *salpha = stau + L * nthr;
    int *scur = (int *)(salpha + L * nthr);                          // [2L][nthr]
    if (a.stage) {
        int *li = (int *)(gpcc_mks_lds + nd);
        for (int i = tid; i < N; i += nthr) {
            gpcc_mks_lds[i] = a.pts[i];
            gpcc_mks_lds[N + i] = a.pts[2L * N + i];
            li[i] = a.perm[i];
        }
        for (int i = tid; i < T; i += nthr) {
            gpcc_mks_lds[2L * N + i] = a.tpts[i];
            gpcc_mks_lds[2L * N + T + i] = a.tpts[T + i];
            li[N + i] = a.tperm[i];
        }
    }
    const double *pt = a.stage ? (const double *)gpcc_mks_lds : a.pts;
    const double *ps2 = a.stage ? (const double *)(gpcc_mks_lds + N) : a.pts + 2L * N;
    const double *tt = a.stage ? (const double *)(gpcc_mks_lds + 2L * N) : a.tpts;
    const double *tsd = tt + T;
    const int *perm = a.stage ? (const int *)(gpcc_mks_lds + nd) : a.perm;
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
                if (!rev) *o = al * x[0] + boff + tsd[i] * z3 - dot;
                else *o -= dot;
                continue;
            }
            double r;
            if (!rev) {
                r = al * x[0] + boff + sqrt(ps2[i]) * z3;
                rt[(long)i * ls] = r;
            } else {
                r = rt[(long)i * ls];
            }
            sprev = key;
            gpcc_mk_propagate<P, NOFF>(A, Q, mu, C);
            gpcc_mk_update<P, NOFF>(band, al, r, ps2[i], mu, C, ll);
            ++jt;
        }
    }
}

// gpcc_markov_combine (gpcc_markov_pred.hip.h) with the weights of the two filters' means as a third output
template <int P, int NOFF>
__global__ void __launch_bounds__(64) gpcc_markov_combine_w(const GpccMarkovCombineWArgs aw)
{
    constexpr int NS = P + NOFF, NREC = NS + NS * (NS + 1) / 2;
    const GpccMarkovCombineArgs &a = aw.c;
    const int lrow = (int)blockIdx.x * 64 + (int)threadIdx.x, tj = blockIdx.y;
    if (lrow >= a.rows) return;
    const long row = a.row0 + lrow;
    const int qb = a.tband[tj];
    const double rho = a.rho[row], al = a.alpha[row * a.L + qb];
    const double lam = gpcc_mk_rate<P>(rho);
    double sc[NS], sgn[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) { sc[i] = 1.0; sgn[i] = 1.0; }
    if constexpr (P == 2) sc[1] = 1.0 / lam;
    if constexpr (P == 3) { sc[1] = 1.7320508075688772 / lam; sc[2] = 1.0 / (lam * lam); }
    if constexpr (P >= 2) sgn[1] = -1.0;
#pragma unroll
    for (int c = 0; c < NOFF; ++c) sc[P + c] = 1.0 / sqrt(a.sigma_b[c]);

    double Lam[NS][NS], eta[NS], Fi[2][NS][NS];
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
        double m[NS], F[NS][NS];
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
        ok = gpcc_mkp_spd_inverse<NS>(F, Fi[dir]) && ok;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            double v = 0.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                v += Fi[dir][i][j] * m[j];
                Lam[i][j] += Fi[dir][i][j];
            }
            eta[i] += v;
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) Lam[i][i] -= (P == 3 && (i == 0 || i == 2)) ? 1.125 : 1.0;
    if constexpr (P == 3) {
        Lam[0][2] -= 0.375;
        Lam[2][0] -= 0.375;
    }
    double Ps[NS][NS];
    ok = gpcc_mkp_spd_inverse<NS>(Lam, Ps) && ok;
    double h[NS], ph[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) h[i] = 0.0;
    h[0] = al;
#pragma unroll
    for (int c = 0; c < NOFF; ++c) h[P + c] = (qb == c) ? sqrt(a.sigma_b[c]) : 0.0;
    double mean = 0.0, var = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double pe = 0.0, p2 = 0.0;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            pe += Ps[i][j] * eta[j];
            p2 += Ps[i][j] * h[j];
        }
        ph[i] = p2;
        mean += h[i] * pe;
        var += h[i] * p2;
    }
    ok = ok && var == var && mean == mean;
    const long o = (long)lrow * a.T + a.tperm[tj];
    a.mu[o] = ok ? mean + a.mean_b[qb] : __builtin_nan("");
    a.var[o] = ok ? var + GPCC_MKP_JITTER : __builtin_nan("");
    // w_dir = sc o D_dir o (P_dir^-1 P_s h): c = w_f . m_f + w_b . m_b on the UNSCALED, unflipped tapped means
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        double *wr = aw.w + (((long)dir * a.T + tj) * NS) * a.mstride + lrow;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            double v = 0.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) v += Fi[dir][i][j] * ph[j];
            wr[(long)i * a.mstride] = v * sc[i] * (dir ? sgn[i] : 1.0);
        }
    }
}

// ---- launches (gpcc_markov_sample_inst.hip: an object of its own) ----
// grid (ceil(rows / 64), T), 64 threads
hipError_t gpcc_mks_launch_combine(int p, int noff, const GpccMarkovCombineWArgs &a, hipStream_t s);
// grid (g.blocks): one lane per draw
hipError_t gpcc_mks_launch_draw(const GpccMkLaunch &g, const GpccMarkovDrawArgs &a);
// draws[lane_out][j] = mu[row][j] + acc[j][lane]: 64 x 64 tiles of (lane, test point) transposed through LDS
hipError_t gpcc_mks_launch_finish(const GpccMarkovDrawFinishArgs &a, hipStream_t s);
