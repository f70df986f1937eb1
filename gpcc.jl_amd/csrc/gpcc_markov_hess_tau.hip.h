// gpcc_markov_hess_tau.hip.h -- the exact linear-time rows of tau of the Hessian of the log-likelihood of the Markov kernels (OU,
// Matern-3/2, Matern-5/2) for gfx950: gpcc_loglik_hess_markov_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py
// (loglik_hess) is the same algorithm in numpy.  The filter's step (gpcc_mk_*) is gpcc_markov.hip.h's, the first-order tangents
// (gpcc_mkg_*) are gpcc_markov_grad.hip.h's, the second-order update and the diagonal cross terms (gpcc_mkh_update, gpcc_mkh_cross)
// gpcc_markov_hess.hip.h's; nothing is approximated.
//
// THE RECURSION is gpcc_markov_hess.hip.h's with other tangents of the transition.  theta = (alpha_1..alpha_L, rho, tau_1..tau_L).  The
// merged order of a row is fixed; for the step into point i from a point of band bprev
//   c_l = -[band_i = l] + [bprev = l]  (0 at the first point: gpcc_markov_grad's dd),  F the companion matrix, F_rho = dF/drho:
//   A_alpha = 0,  A_rho as there,  A_tau_l = c_l F A,
//   A_rho,tau_l = c_l (F_rho A + F A_rho),  A_tau_l,tau_m = c_l c_m F F A,  A_alpha,. = 0,
// and every tangent of Pinf, of the prior and of h by a tau is zero.  With D = C_xx - Pinf and D_a, D_b the same of the tangents:
//   mu_ab <- A_ab mu + A_a mu_b + A_b mu_a + A mu_ab
//   C_ab  <- A_ab D A' + A D A_ab' + A_a D A_b' + A_b D A_a' + A_a D_b A' + A D_b A_a' + A_b D_a A' + A D_a A_b' + A D_ab A' (+ Pinf_ab = 0)
// written with the gradient's tangent step: (mu_ab, C_ab) moves as a tau tangent of the state does, with A_ab in place of A_tau; an
// (alpha, tau) pair's as a tau tangent of the "state" (mu_alpha, C_alpha); the A_a, A_b terms are gpcc_mkh_cross on the diagonal and
// gpcc_mkt_cross off it.  A tau tangent of A is formed only on the steps next to a point of its band.  The update is gpcc_mkh_update
// (h_a = e_1 for an alpha of the observed band only).
//
// ONE WALK, TWO KERNELS.  gpcc_mkt_walk is a template on the lane's noise policy (gpcc_markov_grad.hip.h): gpcc_markov_hess_tau
// instantiates it on GpccMkPlain over the four kinds of pair below; gpcc_markov_noise_hess_tau (gpcc_markov_noise_hess_tau.hip.h) on a lane
// with its own kappa and nu, over those four and (tau, kappa or nu), whose first tangent is a noise tangent (gpcc_markov_hess.hip.h).
//
// TIES.  Matern-3/2 and -5/2 are twice differentiable at zero lag: the fixed-order second tangent is the derivative, there is no tie
// convention.  OU is not: on a row where two points of different bands have exactly equal shifted times -- a step with d == 0 and
// band != bprev after the first -- no second derivative by tau exists, and gpcc_loglik_hess_batch's convention there (k_ss = 1 / rho^2,
// k_rs = 0) is bilinear in the one-sided dK's, so no filter order returns it.  Every lane detects the tie in its own merge and stores
// NaN in its slot: on such a row every entry with a tau index is NaN, info stays 0, and value, gradient and the (alpha, rho) block are
// untouched.  With L = 1 every c is 0 and the entries are exact zeros.
//
// gpcc_markov_hess_tau<P, NOFF>: ONE LANE PER (ROW, PAIR SLOT), the slot being blockIdx.y, so a workgroup is uniform in its pair: L^2
// + L + L (L + 1) / 2 slots in the order (alpha_a, tau_l) [a L + l], (rho, tau_l), (tau_l, tau_l), (tau_l, tau_m) l < m row by row.
// The walk is a template on the kind of pair; a diagonal pair carries three sets, the others four.  State and tangents are
// register-resident.  The lane and its merge are gpcc_markov.hip.h's (gpcc_mk_open, gpcc_mk_next<false>: gpcc_markov_eval's order;
// LDS as gpcc_markov_lds_bytes counts it); the walk keeps bprev, the lags' tangents ca / cb and OU's tie flag.
// gpcc_markov_hess_tau_finish writes the (2L+1) x (2L+1) block: the leading (L+1) x (L+1) block copied from gpcc_markov_hess_finish's
// of the same call, every tau pair to both halves (bitwise symmetric), NaN where info != 0.  Lanes beyond M compute row M - 1 again
// and store nothing.  No atomics: a row's bits depend on the row alone.
#pragma once
#include "gpcc_markov_hess.hip.h"

#define GPCC_MKT_AT 0        /* (alpha_a, tau_l) */
#define GPCC_MKT_RT 1        /* (rho, tau_l) */
#define GPCC_MKT_TT_DIAG 2   /* (tau_l, tau_l) */
#define GPCC_MKT_TT_OFF 3    /* (tau_l, tau_m), l < m */
#define GPCC_MKNT_TN 8       /* (tau_l, kappa_m or nu_m): a lane with a noise model only (gpcc_markov_noise_hess_tau.hip.h instantiates it) */

// GpccMarkovArgs' fields under the same names (the host fills them through one template), the slots and the blocks
struct GpccMarkovHessTauArgs {
    const double *pts;
    const double *delays, *alpha, *rho;
    double *out_loglik;                    // gpcc_markov_eval's, of the same call: read by the finish kernel only
    int *out_info;
    double *slot;                          // [slots][M]
    const double *hyper;                   // [M][L + 1][L + 1]: gpcc_markov_hess_finish's blocks of the same call
    double *hess;                          // [M][2L + 1][2L + 1]
    int M, L, N, stage;
    int off[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
};

static inline int gpcc_markov_hess_tau_slots(int L) { return L * L + L + L * (L + 1) / 2; }

// Out += c F_rho X, F_rho = dlam dF/dlambda: the last row of the companion matrix alone depends on lambda
template <int P>
__device__ __forceinline__ void gpcc_mkt_dcompanion_rate(double lam, double lam2, double dlam, double c, const double (&X)[P][P],
                                                         double (&Out)[P][P])
{
#pragma unroll
    for (int k = 0; k < P; ++k) {
        if constexpr (P == 1) {
            Out[0][k] -= c * dlam * X[0][k];
        } else if constexpr (P == 2) {
            Out[1][k] -= c * dlam * (2.0 * lam * X[0][k] + 2.0 * X[1][k]);
        } else {
            Out[2][k] -= c * dlam * (3.0 * lam2 * X[0][k] + 6.0 * lam * X[1][k] + 3.0 * X[2][k]);
        }
    }
}

// the terms of the second tangent's step in the two first tangents of A, from the state and the tangents BEFORE their propagation (b is
// a tau: its stationary part is zero; Qa: that of a):
// mu_ab += Aa mu_b + Ab mu_a,  C_ab,xx += Aa D Ab' + Ab D Aa' + (Aa Db + Ab Da) A' + A (Aa Db + Ab Da)',  C_ab,xb += Aa C_b,xb + Ab C_a,xb
// (D = C_xx - Q, Da = C_a,xx - Qa, Db = C_b,xx)
template <int P, int NOFF>
__device__ __forceinline__ void gpcc_mkt_cross(const double (&A)[P][P], const double (&Aa)[P][P], const double (&Ab)[P][P],
                                               const double (&Q)[P][P], const double (&Qa)[P][P], const double (&C)[P + NOFF][P + NOFF],
                                               const double (&mua)[P + NOFF], const double (&Ca)[P + NOFF][P + NOFF],
                                               const double (&mub)[P + NOFF], const double (&Cb)[P + NOFF][P + NOFF],
                                               double (&mu2)[P + NOFF], double (&C2)[P + NOFF][P + NOFF])
{
    double T[P][P], U[P][P], W[P][P], X[P][P];
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) acc += Aa[i2][k] * mub[k] + Ab[i2][k] * mua[k];
        mu2[i2] += acc;
    }
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
        for (int k = 0; k < P; ++k) {
            double acc = 0.0, acu = 0.0;
#pragma unroll
            for (int q = 0; q < P; ++q) {
                acc += Aa[i2][q] * GPCC_MK_SYM(Cb, q, k) + Ab[i2][q] * (GPCC_MK_SYM(Ca, q, k) - Qa[q][k]);
                acu += Aa[i2][q] * (GPCC_MK_SYM(C, q, k) - Q[q][k]);
            }
            T[i2][k] = acc;
            U[i2][k] = acu;
        }
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
        for (int k = 0; k < P; ++k) {
            double acc = 0.0, acx = 0.0;
#pragma unroll
            for (int q = 0; q < P; ++q) {
                acc += T[i2][q] * A[k][q];
                acx += U[i2][q] * Ab[k][q];
            }
            W[i2][k] = acc;
            X[i2][k] = acx;
        }
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
        for (int k = i2; k < P; ++k) C2[i2][k] += (X[i2][k] + X[k][i2]) + (W[i2][k] + W[k][i2]);
#pragma unroll
    for (int c = 0; c < NOFF; ++c)
#pragma unroll
        for (int i2 = 0; i2 < P; ++i2) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k) acc += Aa[i2][k] * Cb[k][P + c] + Ab[i2][k] * Ca[k][P + c];
            C2[i2][P + c] += acc;
        }
}

// one lane's walk over the merged observations for a pair of kind PAIR, every observation's variance being the noise policy's (nz.var).
// pa: the band of the pair's alpha (GPCC_MKT_AT), ta: of its first tau (GPCC_MKT_TT_OFF), tb: of its (second) tau; for GPCC_MKNT_TN tb is
// the band of the tau and pn the noise parameter, which no other kind reads.  gpcc_markov_hess_tau instantiates the four kinds without a
// noise parameter on GpccMkPlain; gpcc_markov_noise_hess_tau all five on GpccMknLane.  ARGS is the kernel's, read by the cursor as it is
// there.  NaN on an OU row with a cross-band tie
template <int P, int NOFF, int PAIR, class ARGS, class NZ>
__device__ __forceinline__ double gpcc_mkt_walk(const ARGS &a, const GpccMkLane &ln, const NZ &nz, int pa, int ta, int tb, const GpccMkhParam pn)
{
    static_assert(NZ::noise || PAIR != GPCC_MKNT_TN, "a pair with a kappa or a nu needs a lane with a noise model");
    constexpr int NS = P + NOFF;
    constexpr bool DIAG = PAIR == GPCC_MKT_TT_DIAG;
    constexpr bool TN = PAIR == GPCC_MKNT_TN;
    constexpr int KA = TN ? GPCC_MKG_NOISE : (PAIR == GPCC_MKT_AT ? GPCC_MKG_ALPHA : (PAIR == GPCC_MKT_RT ? GPCC_MKG_RHO : GPCC_MKG_TAU));
    const double rho = ln.rho;
    double lam, lam2, Q[P][P], mu[NS], C[NS][NS];
    gpcc_mk_init<P, NOFF>(rho, a.sigma_b, lam, lam2, Q, mu, C);
    // Pinf_rho (zero unless the pair has rho) and a zero block
    double Qr[P][P], Z[P][P];
    const double dlam = -lam / rho;
    gpcc_mkg_dstationary<P>(lam, lam2, PAIR == GPCC_MKT_RT ? dlam : 0.0, Qr);
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) Z[i][j] = 0.0;
    // the tangents: zero, except the prior state's by rho (Pinf_rho).  A diagonal pair has one tangent (mub, Cb name it again; its own
    // storage is then never touched)
    double mua[NS], Ca[NS][NS], mub_[NS], Cb_[NS][NS], muab[NS], Cab[NS][NS];
    double(&mub)[NS] = DIAG ? mua : mub_;
    double(&Cb)[NS][NS] = DIAG ? Ca : Cb_;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        mua[i] = muab[i] = 0.0;
        if constexpr (!DIAG) mub[i] = 0.0;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const bool xx = i < P && j < P;
            Ca[i][j] = (PAIR == GPCC_MKT_RT && xx) ? Qr[i < P ? i : 0][j < P ? j : 0] : 0.0;
            if constexpr (!DIAG) Cb[i][j] = 0.0;
            Cab[i][j] = 0.0;
        }
    }

    double ll = 0.0, dll = 0.0, hll = 0.0, sprev = 0.0;
    int bprev = -1;
    bool tie = false;
    for (int j = 0; j < a.N; ++j) {
        const GpccMkPoint p = gpcc_mk_next<false>(a, ln, j, sprev);
        const int b = p.b;
        const double d = p.d, al = p.al, r = p.r, s2 = nz.var(ln, b, p.s2);
        if constexpr (P == 1) tie = tie || (j > 0 && d == 0.0 && b != bprev);
        // the variance's tangent by the pair's noise parameter at this observation (read by the updates of a lane with a noise model only)
        double dva = 0.0;
        if constexpr (TN) dva = (b == pn.band) ? (pn.is_nu ? 1.0 : pn.dk * p.s2) : 0.0;
        // the lags' tangents by the pair's taus
        const int cb = (j == 0) ? 0 : (int)(bprev == tb) - (int)(b == tb);
        const int ca = (PAIR != GPCC_MKT_TT_OFF || j == 0) ? 0 : (int)(bprev == ta) - (int)(b == ta);
        bprev = b;
        const bool adb = cb != 0;

        // A, the first tangent of A by the pair's first parameter where it is not its tau (Aa: A_rho or A_tau_a; zero for an alpha or
        // a noise parameter), by its tau (Ab), and the second (Aab)
        double A[P][P], Aa[P][P], Ab[P][P], Aab[P][P];
        gpcc_mk_transition<P>(lam, lam2, d, A);
        gpcc_mkg_dtransition_lag<P>(lam, lam2, (double)cb, A, Ab);
        bool ada = false, adab = adb;
        if constexpr (PAIR == GPCC_MKT_RT) {
            ada = true;
            gpcc_mkg_dtransition_rate<P>(lam, lam2, d, dlam, Aa);
            gpcc_mkg_dtransition_lag<P>(lam, lam2, (double)cb, Aa, Aab);
            gpcc_mkt_dcompanion_rate<P>(lam, lam2, dlam, (double)cb, A, Aab);
        } else if constexpr (PAIR == GPCC_MKT_TT_OFF) {
            ada = ca != 0;
            adab = ada && adb;
            gpcc_mkg_dtransition_lag<P>(lam, lam2, (double)ca, A, Aa);
            gpcc_mkg_dtransition_lag<P>(lam, lam2, (double)cb, Aa, Aab);
        } else if constexpr (PAIR == GPCC_MKT_TT_DIAG) {
            ada = adb;
            gpcc_mkg_dtransition_lag<P>(lam, lam2, (double)cb, Ab, Aab);
        } else {
#pragma unroll
            for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
                for (int k = 0; k < P; ++k) Aa[i2][k] = Aab[i2][k] = 0.0;
        }
        // the step: the second tangent from the state and the tangents before it, then the tangents, then the state.  An (alpha, tau)
        // and a (tau, noise) pair's second tangent is the tau tangent of (mu_a, C_a), whose stationary part is zero; the others' that
        // of the state with A_ab, plus the terms in the first tangents of A
        {
            constexpr bool AT = PAIR == GPCC_MKT_AT || TN;
            const double(&smu)[NS] = AT ? mua : mu;
            const double(&sC)[NS][NS] = AT ? Ca : C;
            const double(&sQ)[P][P] = AT ? Z : Q;
            const double(&sA)[P][P] = AT ? Ab : Aab;
            gpcc_mkg_propagate<P, NOFF, GPCC_MKG_TAU>(A, sA, adab, sQ, Z, smu, sC, muab, Cab);
        }
        if constexpr (DIAG) {
            if (adb) gpcc_mkh_cross<P, NOFF>(A, Ab, Q, Z, C, mua, Ca, muab, Cab);
        } else if constexpr (PAIR == GPCC_MKT_RT || PAIR == GPCC_MKT_TT_OFF) {
            if (ada || adb) gpcc_mkt_cross<P, NOFF>(A, Aa, Ab, Q, Qr, C, mua, Ca, mub, Cb, muab, Cab);
        }
        {
            const double(&A1)[P][P] = DIAG ? Ab : Aa;
            gpcc_mkg_propagate<P, NOFF, KA>(A, A1, ada, Q, Qr, mu, C, mua, Ca);
        }
        if constexpr (!DIAG) gpcc_mkg_propagate<P, NOFF, GPCC_MKG_TAU>(A, Ab, adb, Q, Z, mu, C, mub, Cb);
        gpcc_mk_propagate<P, NOFF>(A, Q, mu, C);
        // the update, in the same order
        const bool ha = PAIR == GPCC_MKT_AT && b == pa;
        gpcc_mkh_update<P, NOFF, NZ::noise>(b, al, ha, false, dva, 0.0, 0.0, r, s2, mu, C, mua, Ca, mub, Cb, muab, Cab, hll);
        gpcc_mkg_update<P, NOFF, KA>(b, al, ha, r, s2, mu, C, mua, Ca, dll, dva);
        if constexpr (!DIAG) gpcc_mkg_update<P, NOFF, GPCC_MKG_TAU>(b, al, false, r, s2, mu, C, mub, Cb, dll);
        gpcc_mk_update<P, NOFF>(b, al, r, s2, mu, C, ll);
    }
    return tie ? __builtin_nan("") : hll;
}

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_hess_tau(const GpccMarkovHessTauArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double gpcc_mkt_lds[];
    const GpccMkLane ln = gpcc_mk_open(a, gpcc_mkt_lds);
    const int L = a.L;

    // the pair of this workgroup (uniform)
    const int slot = blockIdx.y;
    const GpccMkhParam none = {-1, false, 0.0};
    double hll;
    if (slot < L * L) {
        hll = gpcc_mkt_walk<P, NOFF, GPCC_MKT_AT>(a, ln, GpccMkPlain(), slot / L, -1, slot % L, none);
    } else if (slot < L * L + L) {
        hll = gpcc_mkt_walk<P, NOFF, GPCC_MKT_RT>(a, ln, GpccMkPlain(), -1, -1, slot - L * L, none);
    } else if (slot < L * L + 2 * L) {
        const int l = slot - L * L - L;
        hll = gpcc_mkt_walk<P, NOFF, GPCC_MKT_TT_DIAG>(a, ln, GpccMkPlain(), -1, l, l, none);
    } else {
        // (tau_l, tau_m), l < m, rows of the strict upper triangle one after the other
        int ta = 0, rest = slot - L * L - 2 * L;
        while (rest >= L - 1 - ta) {
            rest -= L - 1 - ta;
            ++ta;
        }
        hll = gpcc_mkt_walk<P, NOFF, GPCC_MKT_TT_OFF>(a, ln, GpccMkPlain(), -1, ta, ta + 1 + rest, none);
    }
    if (ln.valid) a.slot[(long)slot * a.M + ln.row] = hll;
}

// ---- the instantiations that ship (gpcc_markov_hess_tau_inst.hip: one object per P) are GpccMkShipsHess, those of the leading block:
// <3, 4> is refused there already (the table of this family is in DESIGN.md 4.21 and profiles/markov/kernel_resources_hess_tau.log);
// gpcc_loglik_hess_markov_batch returns GPCC_ERR_UNSUPPORTED for it and names the dense entry ----

// gpcc_markov_hess_tau<g.p, g.noff> on the grid (g.blocks, slots), then the finish kernel over the M rows (gpcc_markov_hess_tau_inst.hip)
hipError_t gpcc_markov_hess_tau_launch(const GpccMkLaunch &g, int slots, const GpccMarkovHessTauArgs &a);
