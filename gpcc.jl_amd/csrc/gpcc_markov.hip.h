// gpcc_markov.hip.h -- the exact linear-time log-likelihood of the Markov kernels (OU, Matern-3/2, Matern-5/2) for gfx950:
// gpcc_loglik_markov_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py is the same algorithm in numpy.  This file owns
// the Kalman filter itself (gpcc_mk_init, gpcc_mk_transition, gpcc_mk_propagate, gpcc_mk_update) and the forward walk over the data
// around it (GpccMkLane, gpcc_mk_open, gpcc_mk_next).  Nine kernels walk the data around the one step.  Six go forward once and share
// this file's cursor: gpcc_markov_eval below, gpcc_markov_grad, gpcc_markov_hess, gpcc_markov_hess_tau, gpcc_markov_multi and
// gpcc_markov_resample (their own headers; gpcc_markov_multi carries many realisations' means through one covariance recursion and has
// its own update; gpcc_markov_resample reads each lane's own resampled data and skips the points it drops).  Three
// go forward and backward and share the cursor of gpcc_markov_pred.hip.h (GpccMkpLane, gpcc_mkp_next): gpcc_markov_taps there,
// gpcc_markov_draw (gpcc_markov_sample.hip.h) and gpcc_markov_loo_taps (gpcc_markov_loo.hip.h).  The merged order -- the lowest band
// first on ties, and each exception to it -- is written in those two places only.
//
// f with one of these kernels is a stationary Gauss-Markov process of state dimension P = 1, 2, 3 (f, f', f''), so with all
// observations merged in the order of their shifted times s = t - tau_band, K = alpha alpha' k(s - s') + Sobs (+ B) is the covariance
// of a linear-Gaussian state-space model and logpdf(MvNormal(bbar, K), Y) is the sum of the Kalman filter's one-step predictive
// log-densities: O(N P^2) work and O(1) memory per evaluation, nothing approximated.  The marginalised offsets b_l are NOFF = L
// more states that never move (prior variance 100 var(y_l)); more than GPCC_MARKOV_MAX_OFFSETS = 4 of them do not fit a lane's
// registers: gpcc_loglik_markov_batch returns GPCC_ERR_UNSUPPORTED for marginalise_b with L > 4 (without marginalise_b any L <= 8).
//
// ONE LANE PER EVALUATION.  The filter is N dependent steps of ~100-300 fp64 operations; nothing inside one evaluation is worth a
// wave.  A lane keeps the mean (P + NOFF) and the upper triangle of the covariance ((P + NOFF)(P + NOFF + 1) / 2 doubles, 7 + 28 at
// most) in registers -- every loop over the state is unrolled by the template parameters, every index a constant, the observed
// band's offset column chosen by selects -- and walks an L-way merge of the bands (each sorted by time once, on the host): L
// cursors, the head of each band, tau and alpha per band live in LDS, [band][thread] (a lane indexes them by its own band).  The
// light curves (t, r = y - mean, sigma^2: 24 bytes per point) are the same for every lane; they are staged in LDS when they fit
// beside that (N <= ~6500) and read from global memory through the caches otherwise -- one code path, `pts` points to either.
// A workgroup is one wave while the batch has no more waves than the chip has CUs (a 1024-delay grid spreads over 16 CUs), two or
// four waves sharing one staged copy beyond.  Lanes beyond M compute row M - 1 again and store nothing.  No atomics, no
// communication between lanes: a lane's result depends on its own (tau, alpha, rho) only, so results are bitwise the same for any M,
// any row order and any launch shape.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>

#define GPCC_MARKOV_MAX_OFFSETS 4
#define GPCC_MARKOV_MAXL 8
#define GPCC_MARKOV_LDS_MAX (156 * 1024)   /* of the CU's 160 KiB */
#define GPCC_MARKOV_LANE_BYTES 28          /* per lane and band: head, tau, alpha (doubles) and the cursor (int) */

struct GpccMarkovArgs {
    const double *pts;                     // t[N] | r[N] | sigma^2[N], bands one after the other, each sorted by t
    const double *delays, *alpha, *rho;    // M x L, M x L, M
    double *out_loglik;
    int *out_info;
    int M, L, N, stage;                    // stage: copy pts to LDS first
    int off[GPCC_MARKOV_MAXL + 1];         // band l holds points off[l] .. off[l + 1] - 1
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
};

// dynamic LDS of a workgroup of `threads` lanes
static inline size_t gpcc_markov_lds_bytes(int N, int L, int threads, bool stage)
{
    return (stage ? (size_t)24 * N : 0) + (size_t)GPCC_MARKOV_LANE_BYTES * L * threads;
}

// element (i, j) of a symmetric matrix kept in its upper triangle (constant indices after unrolling)
#define GPCC_MK_SYM(Q, i, j) ((i) <= (j) ? Q[i][j] : Q[j][i])

// ---- the filter, shared by every kernel of the linear-time path.  Everything is __forceinline__ and takes its
// arrays by reference, so that after unrolling they stay in registers; the compiler's FMA contraction of these statements, in this
// order, decides the bits of every entry point ----

// lambda: 1/rho (OU), sqrt3/rho (Matern-3/2), sqrt5/rho (Matern-5/2)
template <int P>
__device__ __forceinline__ double gpcc_mk_rate(double rho)
{
    return (P == 1 ? 1.0 : (P == 2 ? 1.7320508075688772 : 2.23606797749979)) / rho;
}

// the rate and the prior state: lam, lam2 = lam^2, Q = Pinf, mu = 0, C = blockdiag(Pinf, diag sigma_b) (C: upper triangle used)
template <int P, int NOFF>
__device__ __forceinline__ void gpcc_mk_init(double rho, const double (&sigma_b)[GPCC_MARKOV_MAX_OFFSETS], double &lam, double &lam2,
                                             double (&Q)[P][P], double (&mu)[P + NOFF], double (&C)[P + NOFF][P + NOFF])
{
    constexpr int NS = P + NOFF;
    lam = gpcc_mk_rate<P>(rho);
    lam2 = lam * lam;
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) Q[i][j] = 0.0;
    Q[0][0] = 1.0;
    if constexpr (P == 2) Q[1][1] = lam2;
    if constexpr (P == 3) {
        Q[0][2] = Q[2][0] = -lam2 / 3.0;
        Q[1][1] = lam2 / 3.0;
        Q[2][2] = lam2 * lam2;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        mu[i] = 0.0;
#pragma unroll
        for (int j = 0; j < NS; ++j) C[i][j] = (i < P && j < P) ? Q[i][j] : 0.0;
    }
#pragma unroll
    for (int c = 0; c < NOFF; ++c) C[P + c][P + c] = sigma_b[c];
}

// a lane's row m: alpha and tau to LDS, [band][thread], and the reference's argument checks (delayedCovariance.jl:3, :5-7) as
// gpcc_loglik_batch reports them: -1 (some alpha <= 0), -2 (rho <= 0), else 0.  ARGS: GpccMarkovArgs or GpccMarkovPredArgs
template <class ARGS>
__device__ __forceinline__ int gpcc_mk_load_row(const ARGS &a, long m, double rho, double *stau, double *salpha, int nthr, int tid)
{
    int info = 0;
    for (int l = 0; l < a.L; ++l) {
        const double al = a.alpha[m * a.L + l];
        if (!(al > 0.0)) info = -1;
        salpha[l * nthr + tid] = al;
        stau[l * nthr + tid] = a.delays[m * a.L + l];
    }
    if (info == 0 && rho <= 0.0) info = -2;
    return info;
}

// A = expm(F d)
template <int P>
__device__ __forceinline__ void gpcc_mk_transition(double lam, double lam2, double d, double (&A)[P][P])
{
    const double e = exp(-lam * d), x = lam * d;
    if constexpr (P == 1) {
        A[0][0] = e;
    } else if constexpr (P == 2) {
        A[0][0] = e * (1.0 + x);
        A[0][1] = e * d;
        A[1][0] = -e * lam2 * d;
        A[1][1] = e * (1.0 - x);
    } else {
        A[0][0] = e * (1.0 + x + 0.5 * x * x);
        A[0][1] = e * d * (1.0 + x);
        A[0][2] = e * 0.5 * d * d;
        A[1][0] = -e * 0.5 * lam2 * lam * d * d;
        A[1][1] = e * (1.0 + x - x * x);
        A[1][2] = e * d * (1.0 - 0.5 * x);
        A[2][0] = e * lam2 * x * (0.5 * x - 1.0);
        A[2][1] = e * lam * x * (x - 3.0);
        A[2][2] = e * (1.0 - 2.0 * x + 0.5 * x * x);
    }
}

// predict: m <- A m, C_xx <- A (C_xx - Pinf) A' + Pinf, C_xb <- A C_xb
template <int P, int NOFF>
__device__ __forceinline__ void gpcc_mk_propagate(const double (&A)[P][P], const double (&Q)[P][P], double (&mu)[P + NOFF],
                                                  double (&C)[P + NOFF][P + NOFF])
{
    double t1[P], D[P][P], T[P][P];
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) acc += A[i2][k] * mu[k];
        t1[i2] = acc;
    }
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2) mu[i2] = t1[i2];
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
        for (int k = 0; k < P; ++k) D[i2][k] = GPCC_MK_SYM(C, i2, k) - Q[i2][k];
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
        for (int k = 0; k < P; ++k) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < P; ++q) acc += A[i2][q] * D[q][k];
            T[i2][k] = acc;
        }
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
        for (int k = i2; k < P; ++k) {
            double acc = Q[i2][k];
#pragma unroll
            for (int q = 0; q < P; ++q) acc += T[i2][q] * A[k][q];
            C[i2][k] = acc;
        }
#pragma unroll
    for (int c = 0; c < NOFF; ++c) {
#pragma unroll
        for (int i2 = 0; i2 < P; ++i2) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k) acc += A[i2][k] * C[k][P + c];
            t1[i2] = acc;
        }
#pragma unroll
        for (int i2 = 0; i2 < P; ++i2) C[i2][P + c] = t1[i2];
    }
}

// update with h = alpha_b e_1 + e_{P + b}; false: the predictive variance is not positive and finite
template <int P, int NOFF>
__device__ __forceinline__ bool gpcc_mk_update(int b, double al, double r, double s2, double (&mu)[P + NOFF],
                                               double (&C)[P + NOFF][P + NOFF], double &ll)
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
    double S = al * Ph[0] + s2, hm = al * mu[0];
#pragma unroll
    for (int c = 0; c < NOFF; ++c) {
        S += (b == c) ? Ph[P + c] : 0.0;
        hm += (b == c) ? mu[P + c] : 0.0;
    }
    const bool ok = S > 0.0 && S < __builtin_inf();
    const double inv = 1.0 / S, eps = r - hm;
    ll -= 0.5 * (1.8378770664093453 + log(S) + eps * eps * inv);
    const double g = eps * inv;
#pragma unroll
    for (int i2 = 0; i2 < NS; ++i2) {
        mu[i2] += Ph[i2] * g;
        const double ki = Ph[i2] * inv;
#pragma unroll
        for (int k = i2; k < NS; ++k) C[i2][k] -= ki * Ph[k];
    }
    return ok;
}

// ---- the forward walk, shared by gpcc_markov_eval below, gpcc_markov_grad, gpcc_markov_hess, gpcc_markov_hess_tau, gpcc_markov_multi and gpcc_markov_resample: what a lane
// keeps outside its registers, the kernel's prologue (gpcc_mk_open) and the choice of the next observation (gpcc_mk_next).  ARGS:
// any argument struct with GpccMarkovArgs' fields ----

struct GpccMkLane {
    const double *pts;                     // t[N] | r[N] | sigma^2[N]: the staged copy in LDS, or global memory
    double *shead, *stau, *salpha;         // LDS, [band][thread]: the shifted time of each band's next point, tau, alpha
    int *scur;                             // LDS, [band][thread]: the index of each band's next point
    int nthr, tid;
    long row;                              // blockIdx.x * nthr + tid
    bool valid;                            // row < M; a lane beyond M walks row M - 1 and stores nothing
    double rho;
    int info;                              // gpcc_mk_load_row's
};

// the observation taken: its band, residual, variance, the band's alpha and the lag from the one before (0 at the first)
struct GpccMkPoint {
    int b;
    double r, s2, al, d;
};

// the prologue: carves the workgroup's dynamic LDS (gpcc_markov_lds_bytes), stages pts, loads the lane's row, sets the cursors
template <class ARGS>
__device__ __forceinline__ GpccMkLane gpcc_mk_open(const ARGS &a, double *lds)
{
    GpccMkLane ln;
    const int tid = ln.tid = threadIdx.x, nthr = ln.nthr = blockDim.x, L = a.L, N = a.N;
    ln.shead = lds + (a.stage ? 3L * N : 0);
    ln.stau = ln.shead + L * nthr;
    ln.salpha = ln.stau + L * nthr;
    ln.scur = (int *)(ln.salpha + L * nthr);
    if (a.stage)
        for (int i = tid; i < 3 * N; i += nthr) lds[i] = a.pts[i];
    ln.pts = a.stage ? (const double *)lds : a.pts;
    ln.row = (long)blockIdx.x * nthr + tid;
    ln.valid = ln.row < a.M;
    const long m_ = ln.valid ? ln.row : a.M - 1;
    ln.rho = a.rho[m_];
    ln.info = gpcc_mk_load_row(a, m_, ln.rho, ln.stau, ln.salpha, nthr, tid);
    __syncthreads();
    for (int l = 0; l < L; ++l) {
        ln.scur[l * nthr + tid] = a.off[l];
        ln.shead[l * nthr + tid] = ln.pts[a.off[l]] - ln.stau[l * nthr + tid];
    }
    return ln;
}

// step j: the L-way merge takes the band whose head has the smallest shifted time, the lowest band on ties, moves its cursor on,
// refills its head and forms the lag from sprev (the shifted time of step j - 1: the caller's, updated here).  RANKED, a compile-time
// rule (as a run-time one it costs gpcc_markov_eval registers): a band's rank among ties is its index, except band rb's, which is rr
// (the gradient's first / last pair, gpcc_markov_grad.hip.h)
template <bool RANKED, class ARGS>
__device__ __forceinline__ GpccMkPoint gpcc_mk_next(const ARGS &a, const GpccMkLane &ln, int j, double &sprev, int rb, int rr)
{
    const int N = a.N, nthr = ln.nthr, tid = ln.tid;
    int b = -1, rk = 0;
    double s = 0.0;
    for (int l = 0; l < a.L; ++l) {
        const double sl = ln.shead[l * nthr + tid];
        const bool live = ln.scur[l * nthr + tid] < a.off[l + 1];
        const int rl = (RANKED && l == rb) ? rr : l;
        const bool take = live && (b < 0 || sl < s || (RANKED && sl == s && rl < rk));
        b = take ? l : b;
        s = take ? sl : s;
        rk = take ? rl : rk;
    }
    const int i = ln.scur[b * nthr + tid];
    const GpccMkPoint p = {b, ln.pts[N + i], ln.pts[2 * N + i], ln.salpha[b * nthr + tid], (j == 0) ? 0.0 : s - sprev};
    ln.scur[b * nthr + tid] = i + 1;
    if (i + 1 < a.off[b + 1]) ln.shead[b * nthr + tid] = ln.pts[i + 1] - ln.stau[b * nthr + tid];
    sprev = s;
    return p;
}

// the unranked rule has no rank pair to take; the ranked one cannot be called without
template <bool RANKED, class ARGS>
__device__ __forceinline__ GpccMkPoint gpcc_mk_next(const ARGS &a, const GpccMkLane &ln, int j, double &sprev)
{
    static_assert(!RANKED, "gpcc_mk_next<true> needs the band rb and its rank rr");
    return gpcc_mk_next<false>(a, ln, j, sprev, -1, 0);
}

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_eval(const GpccMarkovArgs a)
{
    constexpr int NS = P + NOFF;
    extern __shared__ __attribute__((aligned(16))) double gpcc_mk_lds[];
    const GpccMkLane ln = gpcc_mk_open(a, gpcc_mk_lds);

    double lam, lam2, Q[P][P], mu[NS], C[NS][NS];
    gpcc_mk_init<P, NOFF>(ln.rho, a.sigma_b, lam, lam2, Q, mu, C);

    double ll = 0.0, sprev = 0.0;
    int info = ln.info;
    for (int j = 0; j < a.N; ++j) {
        const GpccMkPoint p = gpcc_mk_next<false>(a, ln, j, sprev);
        double A[P][P];
        gpcc_mk_transition<P>(lam, lam2, p.d, A);
        gpcc_mk_propagate<P, NOFF>(A, Q, mu, C);
        const bool ok = gpcc_mk_update<P, NOFF>(p.b, p.al, p.r, p.s2, mu, C, ll);
        info = (info == 0 && !ok) ? j + 1 : info;   // first predictive variance that is not positive and finite
    }
    if (ln.valid) {
        a.out_loglik[ln.row] = info ? __builtin_nan("") : ll;
        a.out_info[ln.row] = info;
    }
}

// ---- which <P, NOFF> ship, and their launch: once, for the nine families of the linear-time path ----

// What a family ships is a statement next to its kernel: a struct whose max_noff[P - 1] is the largest NOFF built for P states of the
// process (every NOFF below it is built too).  The dispatch below instantiates exactly these, so the objects hold exactly these, and
// the host refuses what gpcc_mk_ships() denies.  One that the compiler cannot keep out of scratch memory does not ship
// (tools/kernel_resources.py).  GpccMkShipsAll: every family but the two of the Hessian (gpcc_markov_hess.hip.h)
struct GpccMkShipsAll { static constexpr int max_noff[3] = {GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS}; };

template <class SHIPS>
static inline bool gpcc_mk_ships(int p, int noff)
{
    return p >= 1 && p <= 3 && noff >= 0 && noff <= SHIPS::max_noff[p - 1];
}

// one launch: the instantiation, the workgroups along x (the family's launch function knows y), the workgroup and its dynamic LDS.
// raise_lds: the handle launches this kernel for the first time, so the launch first lifts the kernel's limit of dynamic LDS above
// the default 64 KiB for the staged light curves -- on the one instantiation the handle uses, on the handle's (the current) device
struct GpccMkLaunch {
    int p, noff, blocks, threads;
    size_t lds;
    hipStream_t s;
    bool raise_lds;
};

// f(std::integral_constant<int, P>, std::integral_constant<int, NOFF>) for the runtime (p, noff), over what SHIPS ships with
// PLO <= P <= PHI (an object split by P, -DGPCC_INST_P, dispatches over its own P only); hipErrorInvalidValue for anything else
template <class SHIPS, int PLO = 1, int PHI = 3, int P = PLO, int NOFF = 0, class F>
static inline hipError_t gpcc_mk_dispatch(int p, int noff, F &&f)
{
    if constexpr (P > PHI) {
        return hipErrorInvalidValue;
    } else if constexpr (NOFF > SHIPS::max_noff[P - 1]) {
        return gpcc_mk_dispatch<SHIPS, PLO, PHI, P + 1, 0>(p, noff, f);
    } else {
        if (p == P && noff == NOFF) return f(std::integral_constant<int, P>{}, std::integral_constant<int, NOFF>{});
        return gpcc_mk_dispatch<SHIPS, PLO, PHI, P, NOFF + 1>(p, noff, f);
    }
}

// one kernel on its grid (the combine kernels: no dynamic LDS, nothing to raise)
template <class ARGS>
static inline hipError_t gpcc_mk_launch_kernel(void (*kernel)(ARGS), dim3 grid, int threads, size_t lds, hipStream_t s, bool raise_lds,
                                               const ARGS &a)
{
    if (raise_lds) {
        const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, GPCC_MARKOV_LDS_MAX);
        if (e != hipSuccess) return e;
    }
    kernel<<<grid, dim3(threads), lds, s>>>(a);
    return hipGetLastError();
}

// ... and a filter kernel on g's shape, ny workgroups along y
template <class ARGS>
static inline hipError_t gpcc_mk_launch_kernel(void (*kernel)(ARGS), const GpccMkLaunch &g, int ny, const ARGS &a)
{
    return gpcc_mk_launch_kernel(kernel, dim3(g.blocks, ny), g.threads, g.lds, g.s, g.raise_lds, a);
}

// gpcc_markov_eval<g.p, g.noff> on the grid (g.blocks) (gpcc_markov_inst.hip: its own object)
hipError_t gpcc_markov_launch(const GpccMkLaunch &g, const GpccMarkovArgs &a);
