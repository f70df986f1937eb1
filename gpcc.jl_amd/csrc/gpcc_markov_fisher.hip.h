// gpcc_markov_fisher.hip.h -- the exact linear-time expected (Fisher) information of the log-likelihood of the Markov kernels (OU,
// Matern-3/2, Matern-5/2) for gfx950: gpcc_loglik_fisher_markov_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py
// (loglik_fisher) is the same algorithm in numpy.  The filter's step (gpcc_mk_*) is gpcc_markov.hip.h's and the first-order tangents
// of the covariance (gpcc_mkg_*) are gpcc_markov_grad.hip.h's; nothing is approximated.
//
// THE RECURSION.  theta = (alpha_1..alpha_L, rho, tau_1..tau_L).  The innovation eps_k of the filter is independent of the past with
// variance S_k; its tangent eps_a = -h_a'mu - h'mu_a depends on the past only.  The expectation of -ll_ab over the data of the model is
//   I_ab = sum_k [ S_a S_b / (2 S^2) + E[eps_a eps_b] / S ].
// No data enters: the means are not carried, only their second moments (the prior mean is 0), beside C, C_a, C_b (the covariance and
// its tangents, as gpcc_markov_grad carries them):
//   M_a = E[mu_a mu'],  M_b = E[mu_b mu'],  D = E[mu_a mu_b']   (n x n, not symmetric, zero at the start),
//   Z   = E[mu mu'] = Pi - C,  Pi = blockdiag(Pinf, Sigma_b) the prior covariance: the state is stationary.
// With Abar = blockdiag(A, I), Abar_a = blockdiag(A_a, 0) (A_alpha = 0, A_rho, A_tau_l = c_l F A as in gpcc_markov_hess_tau.hip.h):
//   predict  (Z before the step)  D <- Abar D Abar' + Abar_a Z Abar_b' + Abar_a M_b' Abar' + Abar M_a Abar_b',
//            M_a <- Abar M_a Abar' + Abar_a Z Abar',  then C_a, C_b, C (gpcc_mkg_propagate, gpcc_mk_propagate)
//   update   (Z after the predict)  g = Ph / S,  g_a = (Ph)_a / S - Ph S_a / S^2,  h_a = e_1 on the observations of band a:
//            u_a = E[eps_a mu'] = -h_a'Z - h'M_a,  v_ab = E[eps_a mu_b'] = -h_a'M_b' - h'D,  v_ba = -h_b'M_a' - h'D',
//            w = E[eps_a eps_b] = h_a'Z h_b + h_a'M_b'h + h'M_a h_b + h'D h:
//            I_ab += S_a S_b / (2 S^2) + w / S,
//            D += g v_ab + v_ba'g' + w g g' + S g_a g_b',  M_a += g u_a + S g_a g',  then C_a, C_b, C (gpcc_mkg_update, gpcc_mk_update)
// On a diagonal pair M_b is M_a and is carried once.
//
// TIES.  The merged order of a row is fixed (gpcc_markov_eval's).  Matern-3/2 and -5/2 are C^1 at zero lag: exact, ties or not.  OU
// has a kink; gpcc_loglik_hess_batch's convention at an exact tie of two bands (k_s(0) = 0) is the mean of the one-sided dK's and the
// Fisher information is bilinear in them, so no filter order returns it: on a row where two points of different bands have exactly
// equal shifted times every entry with a tau index is NaN, info stays 0 and the (alpha, rho) block is exact (gpcc_markov_hess_tau's
// contract, detected the same way).  With L = 1 every c is 0 and the tau entries are exact zeros.
//
// gpcc_markov_fisher<P, NOFF>: ONE LANE PER (ROW, PAIR SLOT), a <= b, the slot being blockIdx.y: W (W + 1) / 2 slots (W = 2L + 1) in
// the order (0,0), (0,1), .., (0,W-1), (1,1), ..  A workgroup is uniform in its pair and the walk is a template on the kinds of its
// two parameters.  The state is 3 n (n + 1) / 2 + 3 n^2 doubles off the diagonal (120 at n = 5, 171 at n = 6, 231 at n = 7): in
// registers up to n = 5 and for <2, 4>; <3, 3> keeps D in LDS, [lane][entry], behind the lanes' cursors (GpccMkfLayout,
// gpcc_markov_fisher_lds_extra), so that the staged light curves shrink by 296 bytes per lane; <3, 4> does not ship.
// The lane and its merge are gpcc_markov.hip.h's (gpcc_mk_open, gpcc_mk_next<false>); the residuals are never read.
// gpcc_markov_fisher_finish writes every pair to both halves of the row's W x W block (bitwise symmetric), NaN where info != 0.
// Lanes beyond M compute row M - 1 again and store nothing.  No atomics: a row's bits depend on the row alone.
#pragma once
#include "gpcc_markov_grad.hip.h"

// GpccMarkovArgs' fields under the same names (the host fills them through one template), the slots and the blocks
struct GpccMarkovFisherArgs {
    const double *pts;
    const double *delays, *alpha, *rho;
    double *out_loglik;                    // gpcc_markov_eval's, of the same call: read by the finish kernel only
    int *out_info;
    double *slot;                          // [slots][M]
    double *fisher;                        // [M][2L + 1][2L + 1]
    int M, L, N, stage;
    int off[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
};

static inline int gpcc_markov_fisher_slots(int L) { return (2 * L + 1) * (L + 1); }

// an n x n matrix of a lane: in registers (every index a constant after unrolling), or -- IN_LDS -- in the lane's own NS * NS doubles
// of LDS (GPCC_MKF_LDS_STRIDE apart from the next lane's), read and written entry by entry
#define GPCC_MKF_LDS_STRIDE(NS) ((NS) * (NS) + 1)    /* doubles; odd: a wave's 64-bit accesses spread over the banks */
template <int NS, bool IN_LDS>
struct GpccMkfMat;
template <int NS>
struct GpccMkfMat<NS, false> {
    double v[NS][NS];
    __device__ __forceinline__ double get(int i, int k) const { return v[i][k]; }
    __device__ __forceinline__ void set(int i, int k, double x) { v[i][k] = x; }
};
template <int NS>
struct GpccMkfMat<NS, true> {
    double *p;
    __device__ __forceinline__ double get(int i, int k) const { return p[i * NS + k]; }
    __device__ __forceinline__ void set(int i, int k, double x) { p[i * NS + k] = x; }
};

// which instantiations keep D in LDS: those whose state does not fit a lane's 512 registers (n = P + NOFF >= 6 with P = 3)
template <int P, int NOFF>
struct GpccMkfLayout { static constexpr bool d_in_lds = P == 3 && NOFF >= 3; };

// the dynamic LDS of a workgroup of `threads` lanes beyond gpcc_markov_lds_bytes: D of every lane, where it lives there
static inline size_t gpcc_markov_fisher_lds_extra(int p, int noff, int threads)
{
    const int ns = p + noff;
    return (p == 3 && noff >= 3) ? (size_t)8 * GPCC_MKF_LDS_STRIDE(ns) * threads : 0;
}

// M <- Abar M Abar', Abar = blockdiag(A, I), in place
template <int P, int NOFF, class MAT>
__device__ __forceinline__ void gpcc_mkf_carry(const double (&A)[P][P], MAT &M)
{
    constexpr int NS = P + NOFF;
    double t1[P];
#pragma unroll
    for (int j = 0; j < NS; ++j) {       // the leading rows: A M
#pragma unroll
        for (int i2 = 0; i2 < P; ++i2) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k) acc += A[i2][k] * M.get(k, j);
            t1[i2] = acc;
        }
#pragma unroll
        for (int i2 = 0; i2 < P; ++i2) M.set(i2, j, t1[i2]);
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {       // the leading columns: (.) A'
#pragma unroll
        for (int i2 = 0; i2 < P; ++i2) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k) acc += M.get(i, k) * A[i2][k];
            t1[i2] = acc;
        }
#pragma unroll
        for (int i2 = 0; i2 < P; ++i2) M.set(i, i2, t1[i2]);
    }
}

// Out += Lbar X Rbar', X = M (TR: M'), Lbar = blockdiag(Lm, LI ? I : 0), Rbar = blockdiag(Rm, RI ? I : 0)
template <int P, int NOFF, bool LI, bool RI, bool TR, class MAT, class OUT>
__device__ __forceinline__ void gpcc_mkf_term(const double (&Lm)[P][P], const MAT &M, const double (&Rm)[P][P], OUT &Out)
{
    constexpr int NS = P + NOFF, NR = LI ? NS : P;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        double T[NS];                    // row i of Lbar X
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            if (i < P) {
                double acc = 0.0;
#pragma unroll
                for (int q = 0; q < P; ++q) acc += Lm[i < P ? i : 0][q] * (TR ? M.get(j, q) : M.get(q, j));
                T[j] = acc;
            } else {
                T[j] = TR ? M.get(j, i) : M.get(i, j);
            }
        }
#pragma unroll
        for (int j = 0; j < P; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < P; ++q) acc += T[q] * Rm[j][q];
            Out.set(i, j, Out.get(i, j) + acc);
        }
        if constexpr (RI) {
#pragma unroll
            for (int c = 0; c < NOFF; ++c) Out.set(i, P + c, Out.get(i, P + c) + T[P + c]);
        }
    }
}

// Z = Pi - C, Pi = blockdiag(Pinf, Sigma_b): the second moment of the filter's mean (the entries a caller does not read are not formed)
template <int P, int NOFF>
__device__ __forceinline__ void gpcc_mkf_moment(const double (&Q)[P][P], const double (&sigma_b)[GPCC_MARKOV_MAX_OFFSETS],
                                                const double (&C)[P + NOFF][P + NOFF], GpccMkfMat<P + NOFF, false> &Z)
{
    constexpr int NS = P + NOFF;
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const double pi = (i < P && j < P) ? Q[i < P ? i : 0][j < P ? j : 0] : ((i == j) ? sigma_b[i >= P ? i - P : 0] : 0.0);
            Z.v[i][j] = pi - GPCC_MK_SYM(C, i, j);
        }
}

// Ph = C h, dPh = dC h + C dh, S = h'Ph + sigma^2, dS = dh'Ph + h'dPh: the statements that open gpcc_mkg_update, repeated
// here because this walk needs the four values themselves
template <int P, int NOFF>
__device__ __forceinline__ void gpcc_mkf_gain(int b, double al, bool dh, double s2, const double (&C)[P + NOFF][P + NOFF],
                                              const double (&dC)[P + NOFF][P + NOFF], double (&Ph)[P + NOFF], double (&dPh)[P + NOFF],
                                              double &S, double &dS)
{
    constexpr int NS = P + NOFF;
#pragma unroll
    for (int i2 = 0; i2 < NS; ++i2) {
        double acc = al * GPCC_MK_SYM(C, i2, 0), dacc = al * GPCC_MK_SYM(dC, i2, 0);
#pragma unroll
        for (int c = 0; c < NOFF; ++c) {
            acc += (b == c) ? GPCC_MK_SYM(C, i2, P + c) : 0.0;
            dacc += (b == c) ? GPCC_MK_SYM(dC, i2, P + c) : 0.0;
        }
        Ph[i2] = acc;
        dPh[i2] = dacc;
    }
    S = al * Ph[0] + s2;
    dS = al * dPh[0];
#pragma unroll
    for (int c = 0; c < NOFF; ++c) {
        S += (b == c) ? Ph[P + c] : 0.0;
        dS += (b == c) ? dPh[P + c] : 0.0;
    }
    dS += dh ? 2.0 * Ph[0] : 0.0;
#pragma unroll
    for (int i2 = 0; i2 < NS; ++i2) dPh[i2] += dh ? GPCC_MK_SYM(C, i2, 0) : 0.0;
}

// row vector h'M (ROW) or column vector M h (!ROW), h = al e_1 + e_{P + b}
template <int P, int NOFF, bool ROW, class MAT>
__device__ __forceinline__ void gpcc_mkf_apply(int b, double al, const MAT &M, double (&out)[P + NOFF])
{
    constexpr int NS = P + NOFF;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        double acc = al * (ROW ? M.get(0, j) : M.get(j, 0));
#pragma unroll
        for (int c = 0; c < NOFF; ++c) acc += (b == c) ? (ROW ? M.get(P + c, j) : M.get(j, P + c)) : 0.0;
        out[j] = acc;
    }
}

// the tangent of A by a parameter of kind KIND (GPCC_MKG_*) whose lag's tangent on this step is c (a tau's); false: it is zero
template <int P, int KIND>
__device__ __forceinline__ bool gpcc_mkf_dtransition(double lam, double lam2, double d, double dlam, int c, const double (&A)[P][P],
                                                     double (&Ad)[P][P])
{
    if constexpr (KIND == GPCC_MKG_RHO) {
        gpcc_mkg_dtransition_rate<P>(lam, lam2, d, dlam, Ad);
        return true;
    } else if constexpr (KIND == GPCC_MKG_TAU) {
        gpcc_mkg_dtransition_lag<P>(lam, lam2, (double)c, A, Ad);
        return c != 0;
    } else {
#pragma unroll
        for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
            for (int k = 0; k < P; ++k) Ad[i2][k] = 0.0;
        return false;
    }
}

// one lane's walk over the merged observations for a pair whose parameters are of kinds KA, KB (GPCC_MKG_*); ia, ib: the band of an
// alpha or a tau.  DIAG: a == b.  NaN on an OU row with a cross-band tie when the pair has a tau
template <int P, int NOFF, int KA, int KB, bool DIAG>
__device__ __forceinline__ double gpcc_mkf_walk(const GpccMarkovFisherArgs &a, const GpccMkLane &ln, int ia, int ib)
{
    constexpr int NS = P + NOFF;
    const double rho = ln.rho;
    double lam, lam2, Q[P][P], mu[NS], C[NS][NS];
    gpcc_mk_init<P, NOFF>(rho, a.sigma_b, lam, lam2, Q, mu, C);
    const double dlam = -lam / rho;
    double Qa[P][P], Qb[P][P];
    gpcc_mkg_dstationary<P>(lam, lam2, KA == GPCC_MKG_RHO ? dlam : 0.0, Qa);
    gpcc_mkg_dstationary<P>(lam, lam2, KB == GPCC_MKG_RHO ? dlam : 0.0, Qb);
    // the covariance's tangents (zero, except the prior's by rho) and the moments (zero).  A diagonal pair has one tangent and one
    // M (Cb, Mb name them again; their own storage is then never touched).  The means (mu, dmu) are arguments of the shared step that
    // nothing here reads back: they and the residuals fall out of the compiled walk
    double dmu[NS], Ca[NS][NS], Cb_[NS][NS];
    GpccMkfMat<NS, false> Ma, Mb_;
    GpccMkfMat<NS, GpccMkfLayout<P, NOFF>::d_in_lds> D;
    if constexpr (GpccMkfLayout<P, NOFF>::d_in_lds) D.p = (double *)(ln.scur + a.L * ln.nthr) + (long)ln.tid * GPCC_MKF_LDS_STRIDE(NS);
    double(&Cb)[NS][NS] = DIAG ? Ca : Cb_;
    GpccMkfMat<NS, false> &Mb = DIAG ? Ma : Mb_;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        dmu[i] = 0.0;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const bool xx = i < P && j < P;
            Ca[i][j] = (KA == GPCC_MKG_RHO && xx) ? Qa[i < P ? i : 0][j < P ? j : 0] : 0.0;
            if constexpr (!DIAG) Cb[i][j] = (KB == GPCC_MKG_RHO && xx) ? Qb[i < P ? i : 0][j < P ? j : 0] : 0.0;
            Ma.v[i][j] = 0.0;
            D.set(i, j, 0.0);
            if constexpr (!DIAG) Mb.v[i][j] = 0.0;
        }
    }

    double ll = 0.0, dll = 0.0, fish = 0.0, sprev = 0.0;
    int bprev = -1;
    bool tie = false;
    for (int j = 0; j < a.N; ++j) {
        const GpccMkPoint p = gpcc_mk_next<false>(a, ln, j, sprev);
        const int b = p.b;
        const double d = p.d, al = p.al, s2 = p.s2;
        if constexpr (P == 1 && KB == GPCC_MKG_TAU) tie = tie || (j > 0 && d == 0.0 && b != bprev);
        const int ca = (KA != GPCC_MKG_TAU || j == 0) ? 0 : (int)(bprev == ia) - (int)(b == ia);
        const int cb = (KB != GPCC_MKG_TAU || j == 0) ? 0 : (int)(bprev == ib) - (int)(b == ib);
        bprev = b;

        double A[P][P], Aa[P][P], Ab_[P][P];
        double(&Ab)[P][P] = DIAG ? Aa : Ab_;
        gpcc_mk_transition<P>(lam, lam2, d, A);
        const bool ada = gpcc_mkf_dtransition<P, KA>(lam, lam2, d, dlam, ca, A, Aa);
        bool adb = ada;
        if constexpr (!DIAG) adb = gpcc_mkf_dtransition<P, KB>(lam, lam2, d, dlam, cb, A, Ab);

        // the moments' predict, from Z, M_a, M_b before it: D first
        {
            GpccMkfMat<NS, false> Z;
            gpcc_mkf_moment<P, NOFF>(Q, a.sigma_b, C, Z);
            gpcc_mkf_carry<P, NOFF>(A, D);
            if constexpr (KA != GPCC_MKG_ALPHA) {
                if (ada) {
                    if constexpr (KB != GPCC_MKG_ALPHA) {
                        if (adb) gpcc_mkf_term<P, NOFF, false, false, false>(Aa, Z, Ab, D);
                    }
                    gpcc_mkf_term<P, NOFF, false, true, true>(Aa, Mb, A, D);
                }
            }
            if constexpr (KB != GPCC_MKG_ALPHA) {
                if (adb) gpcc_mkf_term<P, NOFF, true, false, false>(A, Ma, Ab, D);
            }
            gpcc_mkf_carry<P, NOFF>(A, Ma);
            if constexpr (KA != GPCC_MKG_ALPHA) {
                if (ada) gpcc_mkf_term<P, NOFF, false, true, false>(Aa, Z, A, Ma);
            }
            if constexpr (!DIAG) {
                gpcc_mkf_carry<P, NOFF>(A, Mb);
                if constexpr (KB != GPCC_MKG_ALPHA) {
                    if (adb) gpcc_mkf_term<P, NOFF, false, true, false>(Ab, Z, A, Mb);
                }
            }
        }
        // the covariance and its tangents
        gpcc_mkg_propagate<P, NOFF, KA>(A, Aa, ada, Q, Qa, mu, C, dmu, Ca);
        if constexpr (!DIAG) gpcc_mkg_propagate<P, NOFF, KB>(A, Ab, adb, Q, Qb, mu, C, dmu, Cb);
        gpcc_mk_propagate<P, NOFF>(A, Q, mu, C);

        // the moments' update, from the state after the predict
        const bool ha = KA == GPCC_MKG_ALPHA && b == ia, hb = KB == GPCC_MKG_ALPHA && b == ib;
        {
            double Ph[NS], Pha[NS], Phb_[NS], S, Sa, Sb;
            double(&Phb)[NS] = DIAG ? Pha : Phb_;
            gpcc_mkf_gain<P, NOFF>(b, al, ha, s2, C, Ca, Ph, Pha, S, Sa);
            Sb = Sa;
            if constexpr (!DIAG) gpcc_mkf_gain<P, NOFF>(b, al, hb, s2, C, Cb, Ph, Phb, S, Sb);
            const double inv = 1.0 / S;
            double g[NS], ga[NS], gb_[NS];
            double(&gb)[NS] = DIAG ? ga : gb_;
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                g[i] = Ph[i] * inv;
                ga[i] = Pha[i] * inv - g[i] * (inv * Sa);
                if constexpr (!DIAG) gb[i] = Phb[i] * inv - g[i] * (inv * Sb);
            }
            GpccMkfMat<NS, false> Z;
            double hMa[NS], hMb_[NS], hD[NS], Dh[NS];
            double(&hMb)[NS] = DIAG ? hMa : hMb_;
            gpcc_mkf_moment<P, NOFF>(Q, a.sigma_b, C, Z);
            gpcc_mkf_apply<P, NOFF, true>(b, al, Ma, hMa);
            if constexpr (!DIAG) gpcc_mkf_apply<P, NOFF, true>(b, al, Mb, hMb);
            gpcc_mkf_apply<P, NOFF, true>(b, al, D, hD);
            gpcc_mkf_apply<P, NOFF, false>(b, al, D, Dh);
            // w = h_a'Z h_b + h_a'M_b'h + h'M_a h_b + h'D h
            double w = al * hD[0];
#pragma unroll
            for (int c = 0; c < NOFF; ++c) w += (b == c) ? hD[P + c] : 0.0;
            w += (ha ? hMb[0] : 0.0) + (hb ? hMa[0] : 0.0) + ((ha && hb) ? Z.v[0][0] : 0.0);
            fish += 0.5 * Sa * Sb * inv * inv + w * inv;
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const double vba = -(hb ? Ma.v[i][0] : 0.0) - Dh[i];     // E[eps_b mu_a']
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const double vab = -(ha ? Mb.v[k][0] : 0.0) - hD[k]; // E[eps_a mu_b']
                    D.set(i, k, D.get(i, k) + (g[i] * vab + vba * g[k] + w * g[i] * g[k] + S * ga[i] * gb[k]));
                }
            }
#pragma unroll
            for (int i = 0; i < NS; ++i)
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const double ua = -(ha ? Z.v[0][k] : 0.0) - hMa[k];
                    Ma.v[i][k] += g[i] * ua + S * ga[i] * g[k];
                    if constexpr (!DIAG) {
                        const double ub = -(hb ? Z.v[0][k] : 0.0) - hMb[k];
                        Mb.v[i][k] += g[i] * ub + S * gb[i] * g[k];
                    }
                }
        }
        gpcc_mkg_update<P, NOFF, KA>(b, al, ha, p.r, s2, mu, C, dmu, Ca, dll);
        if constexpr (!DIAG) gpcc_mkg_update<P, NOFF, KB>(b, al, hb, p.r, s2, mu, C, dmu, Cb, dll);
        gpcc_mk_update<P, NOFF>(b, al, p.r, s2, mu, C, ll);
    }
    return tie ? __builtin_nan("") : fish;
}

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_fisher(const GpccMarkovFisherArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double gpcc_mkf_lds[];
    const GpccMkLane ln = gpcc_mk_open(a, gpcc_mkf_lds);
    const int L = a.L, W = 2 * L + 1;

    // the pair of this workgroup (uniform): rows of the upper triangle one after the other
    const int slot = blockIdx.y;
    int ia = 0, rest = slot;
    while (rest >= W - ia) {
        rest -= W - ia;
        ++ia;
    }
    const int ib = ia + rest;
    const int ka = ia < L ? GPCC_MKG_ALPHA : (ia == L ? GPCC_MKG_RHO : GPCC_MKG_TAU);
    const int kb = ib < L ? GPCC_MKG_ALPHA : (ib == L ? GPCC_MKG_RHO : GPCC_MKG_TAU);
    const int ba = ka == GPCC_MKG_ALPHA ? ia : ia - L - 1, bb = kb == GPCC_MKG_ALPHA ? ib : ib - L - 1;   // the bands (rho: unused)
    double fish;
    if (ka == GPCC_MKG_ALPHA) {
        if (ia == ib) fish = gpcc_mkf_walk<P, NOFF, GPCC_MKG_ALPHA, GPCC_MKG_ALPHA, true>(a, ln, ba, bb);
        else if (kb == GPCC_MKG_ALPHA) fish = gpcc_mkf_walk<P, NOFF, GPCC_MKG_ALPHA, GPCC_MKG_ALPHA, false>(a, ln, ba, bb);
        else if (kb == GPCC_MKG_RHO) fish = gpcc_mkf_walk<P, NOFF, GPCC_MKG_ALPHA, GPCC_MKG_RHO, false>(a, ln, ba, bb);
        else fish = gpcc_mkf_walk<P, NOFF, GPCC_MKG_ALPHA, GPCC_MKG_TAU, false>(a, ln, ba, bb);
    } else if (ka == GPCC_MKG_RHO) {
        if (ia == ib) fish = gpcc_mkf_walk<P, NOFF, GPCC_MKG_RHO, GPCC_MKG_RHO, true>(a, ln, ba, bb);
        else fish = gpcc_mkf_walk<P, NOFF, GPCC_MKG_RHO, GPCC_MKG_TAU, false>(a, ln, ba, bb);
    } else {
        if (ia == ib) fish = gpcc_mkf_walk<P, NOFF, GPCC_MKG_TAU, GPCC_MKG_TAU, true>(a, ln, ba, bb);
        else fish = gpcc_mkf_walk<P, NOFF, GPCC_MKG_TAU, GPCC_MKG_TAU, false>(a, ln, ba, bb);
    }
    if (ln.valid) a.slot[(long)slot * a.M + ln.row] = fish;
}

// ---- the instantiations that ship (gpcc_markov_fisher_inst.hip: one object per P): those the compiler keeps out of scratch memory
// (the table is in DESIGN.md 4.22 and profiles/markov/kernel_resources_fisher.log).  gpcc_loglik_fisher_markov_batch returns
// GPCC_ERR_UNSUPPORTED for the others and names the dense entry ----
struct GpccMkShipsFisher { static constexpr int max_noff[3] = {4, 4, 3}; };

// gpcc_markov_fisher<g.p, g.noff> on the grid (g.blocks, slots), then the finish kernel over the M rows (gpcc_markov_fisher_inst.hip)
hipError_t gpcc_markov_fisher_launch(const GpccMkLaunch &g, int slots, const GpccMarkovFisherArgs &a);
