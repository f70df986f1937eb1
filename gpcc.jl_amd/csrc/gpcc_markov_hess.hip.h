// gpcc_markov_hess.hip.h -- the exact linear-time (alpha, rho) block of the Hessian of the log-likelihood of the Markov kernels (OU,
// Matern-3/2, Matern-5/2) for gfx950: gpcc_loglik_hess_hyper_markov_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py
// (loglik_hess_hyper) is the same algorithm in numpy.  The filter's step (gpcc_mk_*) is gpcc_markov.hip.h's and the first-order
// tangents (gpcc_mkg_*) are gpcc_markov_grad.hip.h's; nothing is approximated.
//
// SECOND-ORDER FORWARD SENSITIVITY.  For a pair (a, b) of theta = (alpha_1..alpha_L, rho) four sets are carried through the filter: the
// state (mu, C), its tangents by a and by b, and the second tangent (mu_ab, C_ab); the log-likelihood's second tangent is summed as
// the value is.  For alpha and rho the merged order is fixed and no kink is crossed, so there is no tie convention.
//   rho rho  d/drho = (-lambda / rho) d/dlambda, so d2/drho2 = (lambda / rho)^2 d2/dlambda2 + (2 lambda / rho^2) d/dlambda, for A and Pinf
//            in closed form per kernel (gpcc_mkh_d2transition_rate, gpcc_mkh_d2stationary); the prior's second tangent is Pinf_rhorho
//   step     the product rule on the gradient's step, written with the gradient's own tangent step:
//              alpha alpha  (mu_ab, C_ab) moves as an alpha tangent does (A only)
//              alpha rho    (mu_ab, C_ab) is the rho tangent of the "state" (mu_a, C_a), whose stationary part is zero
//              rho rho      the rho tangent step with (A_rhorho, Pinf_rhorho) in place of (A_rho, Pinf_rho), plus the cross terms
//                           2 A_rho mu_rho, 2 A_rho D A_rho' + 2 (A_rho D_rho A' + A D_rho A_rho'), 2 A_rho C_rho,xb  (gpcc_mkh_cross)
//   update   h_a = e_1 on the observations of band a, h_ab = 0:  (Ph)_a = C_a h + C h_a,  (Ph)_ab = C_ab h + C_a h_b + C_b h_a,
//            S_a = h_a'Ph + h'(Ph)_a,  S_ab = h_a'(Ph)_b + h_b'(Ph)_a + h'(Ph)_ab,  eps_a = -h_a'mu - h'mu_a,
//            eps_ab = -h_a'mu_b - h_b'mu_a - h'mu_ab,  g = eps / S, g_a = (eps_a - g S_a) / S, g_ab = (eps_ab - g_a S_b - g_b S_a - g S_ab) / S:
//            ll_ab -= (S_ab / S - S_a S_b / S^2 + 2 eps_a eps_b / S + 2 g eps_ab - 2 g (eps_a S_b + eps_b S_a) / S - g^2 S_ab
//                      + 2 g^2 S_a S_b / S) / 2,  then the second tangents of mu += Ph g and C -= k Ph', k = Ph / S
//
// ONE WALK, TWO KERNELS.  gpcc_mkh_walk and gpcc_mkh_update are templates on the lane's noise policy (gpcc_markov_grad.hip.h).
// gpcc_markov_hess instantiates them on GpccMkPlain over the four kinds of pair of alpha and rho; gpcc_markov_noise_hess
// (gpcc_markov_noise_hess.hip.h) on a lane with its own kappa and nu, over those four and the four kinds with a noise parameter, whose
// variance tangents enter S_a, S_b and S_ab.  In the plain instantiation no statement has an operand for a variance tangent.
//
// NOT HERE.  The Fisher information (its expectation needs another recursion) stays with gpcc_loglik_hess_batch /
// gpcc_loglik_hess_hyper_batch.  The rows of tau are gpcc_markov_hess_tau.hip.h's (gpcc_loglik_hess_markov_batch), built from these pieces.
//
// gpcc_markov_hess<P, NOFF>: ONE LANE PER (ROW, PAIR SLOT), a <= b, the slot being blockIdx.y: (L + 1)(L + 2) / 2 slots in the order
// (0,0), (0,1), .., (0,L), (1,1), ..  A workgroup is uniform in its pair, and the walk is a template on the kind of pair: an alpha
// alpha lane forms no tangent of A, an alpha rho lane A_rho, the rho rho lane A_rho and A_rhorho; a diagonal pair carries three sets,
// the others four.  State and tangents are register-resident (4 (n + n (n + 1) / 2) = 140 doubles at n = 7, in the unified
// 512-register file at one wave per SIMD).  The lane and its merge are gpcc_markov.hip.h's (gpcc_mk_open, gpcc_mk_next<false>:
// gpcc_markov_eval's order; LDS as gpcc_markov_lds_bytes counts it), as the primal recursion is its one filter step.  Per-slot
// results go to slot[slot][row]; gpcc_markov_hess_finish writes every pair to both halves of the row's (L+1) x (L+1) block (bitwise
// symmetric), NaN where info != 0.  Lanes beyond M compute row M - 1 again and store nothing.  No atomics: a row's bits depend on the
// row alone.
#pragma once
#include "gpcc_markov_grad.hip.h"

#define GPCC_MKH_AA_DIAG 0   /* (alpha_l, alpha_l) */
#define GPCC_MKH_AA_OFF 1    /* (alpha_l, alpha_m), l < m */
#define GPCC_MKH_AR 2        /* (alpha_l, rho) */
#define GPCC_MKH_RR 3        /* (rho, rho) */
/* the kinds that only a lane with a noise model has (gpcc_markov_noise_hess.hip.h instantiates them) */
#define GPCC_MKNH_AN 4       /* (alpha_l, kappa_m or nu_m) */
#define GPCC_MKNH_RN 5       /* (rho, kappa_m or nu_m) */
#define GPCC_MKNH_NN_DIAG 6  /* (kappa_l, kappa_l), (nu_l, nu_l) */
#define GPCC_MKNH_NN_OFF 7   /* two different noise parameters, of one band or of two */

// GpccMarkovArgs' fields under the same names (the host fills them through one template), the slots and the blocks
struct GpccMarkovHessArgs {
    const double *pts;
    const double *delays, *alpha, *rho;
    double *out_loglik;                    // gpcc_markov_eval's, of the same call: read by the finish kernel only
    int *out_info;
    double *slot;                          // [slots][M]
    double *hess;                          // [M][L + 1][L + 1]
    int M, L, N, stage;
    int off[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
};

static inline int gpcc_markov_hess_slots(int L) { return (L + 1) * (L + 2) / 2; }

// Add = c2 d2A/dlambda2, in closed form per kernel (e = exp(-lambda d), x = lambda d)
template <int P>
__device__ __forceinline__ void gpcc_mkh_d2transition_rate(double lam, double d, double c2, double (&Add)[P][P])
{
    const double x = lam * d, e = exp(-x) * c2, d2 = d * d;
    if constexpr (P == 1) {
        Add[0][0] = e * d2;
    } else if constexpr (P == 2) {
        Add[0][0] = e * d2 * (x - 1.0);
        Add[0][1] = e * d2 * d;
        Add[1][0] = e * d * (4.0 * x - 2.0 - x * x);
        Add[1][1] = e * d2 * (3.0 - x);
    } else {
        Add[0][0] = e * d2 * x * (0.5 * x - 1.0);
        Add[0][1] = e * d2 * d * (x - 1.0);
        Add[0][2] = 0.5 * e * d2 * d2;
        Add[1][0] = 0.5 * e * d * x * (6.0 * x - 6.0 - x * x);
        Add[1][1] = e * d2 * (5.0 * x - 3.0 - x * x);
        Add[1][2] = 0.5 * e * d2 * d * (4.0 - x);
        Add[2][0] = e * x * (0.5 * x * x * x - 5.0 * x * x + 12.0 * x - 6.0);
        Add[2][1] = e * d * (x * x * x - 9.0 * x * x + 18.0 * x - 6.0);
        Add[2][2] = e * d2 * (0.5 * x * x - 4.0 * x + 6.0);
    }
}

// Qdd = c2 d2Pinf/dlambda2
template <int P>
__device__ __forceinline__ void gpcc_mkh_d2stationary(double lam2, double c2, double (&Qdd)[P][P])
{
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) Qdd[i][j] = 0.0;
    if constexpr (P == 2) Qdd[1][1] = 2.0 * c2;
    if constexpr (P == 3) {
        Qdd[0][2] = Qdd[2][0] = -(2.0 / 3.0) * c2;
        Qdd[1][1] = (2.0 / 3.0) * c2;
        Qdd[2][2] = 12.0 * lam2 * c2;
    }
}

// the cross terms of the (rho, rho) step, from the state and the rho tangent BEFORE their propagation:
// mu_ab += 2 Ad dmu,  C_ab,xx += 2 Ad D Ad' + 2 (Ad dD A' + A dD Ad'),  C_ab,xb += 2 Ad dC_xb   (D = C_xx - Q, dD = dC_xx - Qd)
template <int P, int NOFF>
__device__ __forceinline__ void gpcc_mkh_cross(const double (&A)[P][P], const double (&Ad)[P][P], const double (&Q)[P][P],
                                               const double (&Qd)[P][P], const double (&C)[P + NOFF][P + NOFF],
                                               const double (&dmu)[P + NOFF], const double (&dC)[P + NOFF][P + NOFF],
                                               double (&mu2)[P + NOFF], double (&C2)[P + NOFF][P + NOFF])
{
    double T[P][P], U[P][P], W[P][P];
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) acc += Ad[i2][k] * dmu[k];
        mu2[i2] += 2.0 * acc;
    }
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
        for (int k = 0; k < P; ++k) {
            double acc = 0.0, acu = 0.0;
#pragma unroll
            for (int q = 0; q < P; ++q) {
                acc += Ad[i2][q] * (GPCC_MK_SYM(dC, q, k) - Qd[q][k]);
                acu += Ad[i2][q] * (GPCC_MK_SYM(C, q, k) - Q[q][k]);
            }
            T[i2][k] = acc;
            U[i2][k] = acu;
        }
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
        for (int k = 0; k < P; ++k) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < P; ++q) acc += T[i2][q] * A[k][q];
            W[i2][k] = acc;
        }
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
        for (int k = i2; k < P; ++k) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < P; ++q) acc += U[i2][q] * Ad[k][q];
            C2[i2][k] += 2.0 * (acc + W[i2][k] + W[k][i2]);
        }
#pragma unroll
    for (int c = 0; c < NOFF; ++c)
#pragma unroll
        for (int i2 = 0; i2 < P; ++i2) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k) acc += Ad[i2][k] * dC[k][P + c];
            C2[i2][P + c] += 2.0 * acc;
        }
}

// the second tangent of gpcc_mk_update, from the state and the two tangents BEFORE it (after the propagation).  ha, hb: this
// observation's h moves with the pair's first / second parameter (an alpha of its band).  A diagonal pair passes its tangent twice.
// NOISE: the lane carries a noise model, and the tangents of this observation's variance by the pair's parameters enter S_a, S_b and
// S_ab (dva, dvb, d2v; a noise parameter has no h-tangent).  Without one the three are not read: no statement has an operand for them
template <int P, int NOFF, bool NOISE>
__device__ __forceinline__ void gpcc_mkh_update(int b, double al, bool ha, bool hb, double dva, double dvb, double d2v, double r, double s2,
                                                const double (&mu)[P + NOFF], const double (&C)[P + NOFF][P + NOFF],
                                                const double (&mua)[P + NOFF], const double (&Ca)[P + NOFF][P + NOFF],
                                                const double (&mub)[P + NOFF], const double (&Cb)[P + NOFF][P + NOFF],
                                                double (&muab)[P + NOFF], double (&Cab)[P + NOFF][P + NOFF], double &hll)
{
    constexpr int NS = P + NOFF;
    double Ph[NS], Pha[NS], Phb[NS], Phab[NS];
#pragma unroll
    for (int i2 = 0; i2 < NS; ++i2) {
        const double c0 = GPCC_MK_SYM(C, i2, 0), a0 = GPCC_MK_SYM(Ca, i2, 0), b0 = GPCC_MK_SYM(Cb, i2, 0);
        double acc = al * c0, acca = al * a0, accb = al * b0, accab = al * GPCC_MK_SYM(Cab, i2, 0);
#pragma unroll
        for (int c = 0; c < NOFF; ++c) {
            acc += (b == c) ? GPCC_MK_SYM(C, i2, P + c) : 0.0;
            acca += (b == c) ? GPCC_MK_SYM(Ca, i2, P + c) : 0.0;
            accb += (b == c) ? GPCC_MK_SYM(Cb, i2, P + c) : 0.0;
            accab += (b == c) ? GPCC_MK_SYM(Cab, i2, P + c) : 0.0;
        }
        Ph[i2] = acc;
        Pha[i2] = acca + (ha ? c0 : 0.0);
        Phb[i2] = accb + (hb ? c0 : 0.0);
        Phab[i2] = accab + (hb ? a0 : 0.0) + (ha ? b0 : 0.0);
    }
    double S = al * Ph[0] + s2, Sa = al * Pha[0], Sb = al * Phb[0], Sab = al * Phab[0];
    if constexpr (NOISE) {      // each one expression: the product and the variance's tangent contract as S's does
        Sa = al * Pha[0] + dva;
        Sb = al * Phb[0] + dvb;
        Sab = al * Phab[0] + d2v;
    }
    double hm = al * mu[0], hma = al * mua[0], hmb = al * mub[0], hmab = al * muab[0];
#pragma unroll
    for (int c = 0; c < NOFF; ++c) {
        S += (b == c) ? Ph[P + c] : 0.0;
        Sa += (b == c) ? Pha[P + c] : 0.0;
        Sb += (b == c) ? Phb[P + c] : 0.0;
        Sab += (b == c) ? Phab[P + c] : 0.0;
        hm += (b == c) ? mu[P + c] : 0.0;
        hma += (b == c) ? mua[P + c] : 0.0;
        hmb += (b == c) ? mub[P + c] : 0.0;
        hmab += (b == c) ? muab[P + c] : 0.0;
    }
    Sa += ha ? Ph[0] : 0.0;
    Sb += hb ? Ph[0] : 0.0;
    Sab += (ha ? Phb[0] : 0.0) + (hb ? Pha[0] : 0.0);
    const double ea = -(hma + (ha ? mu[0] : 0.0)), eb = -(hmb + (hb ? mu[0] : 0.0));
    const double eab = -(hmab + (ha ? mub[0] : 0.0) + (hb ? mua[0] : 0.0));
    const double inv = 1.0 / S, g = (r - hm) * inv, ga = (ea - g * Sa) * inv, gb = (eb - g * Sb) * inv;
    const double gab = (eab - ga * Sb - gb * Sa - g * Sab) * inv;
    hll -= 0.5 * (Sab * inv - Sa * Sb * inv * inv + 2.0 * ea * eb * inv + 2.0 * g * eab - 2.0 * g * inv * (ea * Sb + eb * Sa) - g * g * Sab
                  + 2.0 * g * g * Sa * Sb * inv);
    const double inv2 = inv * inv;
#pragma unroll
    for (int i2 = 0; i2 < NS; ++i2) {
        muab[i2] += Phab[i2] * g + Pha[i2] * gb + Phb[i2] * ga + Ph[i2] * gab;
        const double ki = Ph[i2] * inv, kai = Pha[i2] * inv - ki * inv * Sa, kbi = Phb[i2] * inv - ki * inv * Sb;
        const double kabi = Phab[i2] * inv - (Pha[i2] * Sb + Phb[i2] * Sa) * inv2 - ki * inv * Sab + 2.0 * ki * inv2 * Sa * Sb;
#pragma unroll
        for (int k = i2; k < NS; ++k) Cab[i2][k] -= kabi * Ph[k] + kai * Phb[k] + kbi * Pha[k] + ki * Phab[k];
    }
}

// what a lane knows of one parameter of its pair: the band (of an alpha, kappa or nu; -1: rho) and, for a noise parameter, whether it
// is a nu and the factor of sigma_i^2 in a kappa's dvar (2 kappa).  A plain kernel's pairs read the band alone
struct GpccMkhParam {
    int band;
    bool is_nu;
    double dk;
};

// one lane's walk over the merged observations for the pair (pa, pb) of kind PAIR, every observation's variance being the noise policy's
// (nz.var).  gpcc_markov_hess instantiates the four kinds of alpha and rho on GpccMkPlain; gpcc_markov_noise_hess all eight on
// GpccMknLane.  A noise tangent has no tangent of the prior, of A or of Pinf and no h-tangent: it is propagated as an alpha's with a
// zero A-tangent, and the variance's tangents dva, dvb, d2v enter the updates instead; on (rho, noise) the second tangent moves as the
// rho tangent of the noise "state", the way (alpha, rho)'s moves.  ARGS is the kernel's, read by the cursor as it is there
template <int P, int NOFF, int PAIR, class ARGS, class NZ>
__device__ __forceinline__ double gpcc_mkh_walk(const ARGS &a, const GpccMkLane &ln, const NZ &nz, const GpccMkhParam pa, const GpccMkhParam pb)
{
    static_assert(NZ::noise || PAIR <= GPCC_MKH_RR, "a pair with a kappa or a nu needs a lane with a noise model");
    constexpr int NS = P + NOFF;
    constexpr bool DIAG = PAIR == GPCC_MKH_AA_DIAG || PAIR == GPCC_MKH_RR || PAIR == GPCC_MKNH_NN_DIAG;
    constexpr bool RHO = PAIR == GPCC_MKH_AR || PAIR == GPCC_MKH_RR || PAIR == GPCC_MKNH_RN;      // some tangent of A is formed
    constexpr bool NA = PAIR == GPCC_MKNH_NN_DIAG || PAIR == GPCC_MKNH_NN_OFF;                    // the first parameter is a noise parameter
    constexpr bool NB = NA || PAIR == GPCC_MKNH_AN || PAIR == GPCC_MKNH_RN;                       // the second one is
    constexpr bool RA = PAIR == GPCC_MKH_RR || PAIR == GPCC_MKNH_RN, RB = PAIR == GPCC_MKH_AR || PAIR == GPCC_MKH_RR;   // ... is rho
    constexpr int KA = NA ? GPCC_MKG_NOISE : (RA ? GPCC_MKG_RHO : GPCC_MKG_ALPHA);
    constexpr int KB = NB ? GPCC_MKG_NOISE : (RB ? GPCC_MKG_RHO : GPCC_MKG_ALPHA);
    const double rho = ln.rho;
    double lam, lam2, Q[P][P], mu[NS], C[NS][NS];
    gpcc_mk_init<P, NOFF>(rho, a.sigma_b, lam, lam2, Q, mu, C);
    // Pinf_rho, Pinf_rhorho = (lambda / rho)^2 d2Pinf/dlambda2 - (2 / rho) Pinf_rho, and a zero block
    double Qr[P][P], Qrr[P][P], Z[P][P];
    const double dlam = -lam / rho, c2 = dlam * dlam, c1 = -2.0 / rho;
    gpcc_mkg_dstationary<P>(lam, lam2, RHO ? dlam : 0.0, Qr);
    gpcc_mkh_d2stationary<P>(lam2, PAIR == GPCC_MKH_RR ? c2 : 0.0, Qrr);
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) {
            Qrr[i][j] += (PAIR == GPCC_MKH_RR) ? c1 * Qr[i][j] : 0.0;
            Z[i][j] = 0.0;
        }
    // the tangents: zero, except the prior state's by rho (Pinf_rho) and by (rho, rho) (Pinf_rhorho).  A diagonal pair has one tangent
    // (mub, Cb name it again; its own storage is then never touched)
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
            Ca[i][j] = (RA && xx) ? Qr[i < P ? i : 0][j < P ? j : 0] : 0.0;
            if constexpr (!DIAG) Cb[i][j] = (RB && xx) ? Qr[i < P ? i : 0][j < P ? j : 0] : 0.0;
            Cab[i][j] = (PAIR == GPCC_MKH_RR && xx) ? Qrr[i < P ? i : 0][j < P ? j : 0] : 0.0;
        }
    }

    double ll = 0.0, dll = 0.0, hll = 0.0, sprev = 0.0;
    for (int j = 0; j < a.N; ++j) {
        const GpccMkPoint p = gpcc_mk_next<false>(a, ln, j, sprev);
        const int b = p.b;
        const double d = p.d, al = p.al, r = p.r, s2 = nz.var(ln, b, p.s2);
        // the variance's tangents at this observation (read by the updates of a lane with a noise model only)
        double dva = 0.0, dvb = 0.0, d2v = 0.0;
        if constexpr (NA) dva = (b == pa.band) ? (pa.is_nu ? 1.0 : pa.dk * p.s2) : 0.0;
        if constexpr (NB) dvb = (b == pb.band) ? (pb.is_nu ? 1.0 : pb.dk * p.s2) : 0.0;
        if constexpr (PAIR == GPCC_MKNH_NN_DIAG) d2v = (b == pa.band && !pa.is_nu) ? 2.0 * p.s2 : 0.0;

        double A[P][P], Ar[P][P], Arr[P][P];
        gpcc_mk_transition<P>(lam, lam2, d, A);
        if constexpr (RHO) gpcc_mkg_dtransition_rate<P>(lam, lam2, d, dlam, Ar);
        if constexpr (PAIR == GPCC_MKH_RR) {
            gpcc_mkh_d2transition_rate<P>(lam, d, c2, Arr);
#pragma unroll
            for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
                for (int k = 0; k < P; ++k) Arr[i2][k] += c1 * Ar[i2][k];
        }
        // the step: the second tangent from the state and the tangents before it, then the tangents, then the state
        if constexpr (PAIR == GPCC_MKH_RR) {
            gpcc_mkg_propagate<P, NOFF, GPCC_MKG_RHO>(A, Arr, true, Q, Qrr, mu, C, muab, Cab);
            gpcc_mkh_cross<P, NOFF>(A, Ar, Q, Qr, C, mua, Ca, muab, Cab);
        } else if constexpr (PAIR == GPCC_MKH_AR) {
            gpcc_mkg_propagate<P, NOFF, GPCC_MKG_RHO>(A, Ar, true, Z, Z, mua, Ca, muab, Cab);
        } else if constexpr (PAIR == GPCC_MKNH_RN) {
            gpcc_mkg_propagate<P, NOFF, GPCC_MKG_RHO>(A, Ar, true, Z, Z, mub, Cb, muab, Cab);
        } else {
            gpcc_mkg_propagate<P, NOFF, GPCC_MKG_ALPHA>(A, Z, false, Q, Z, mu, C, muab, Cab);
        }
        gpcc_mkg_propagate<P, NOFF, KA>(A, Ar, RA, Q, Qr, mu, C, mua, Ca);
        if constexpr (!DIAG) gpcc_mkg_propagate<P, NOFF, KB>(A, Ar, RB, Q, Qr, mu, C, mub, Cb);
        gpcc_mk_propagate<P, NOFF>(A, Q, mu, C);
        // the update, in the same order
        const bool ha = !RA && !NA && b == pa.band, hb = !RB && !NB && b == pb.band;
        gpcc_mkh_update<P, NOFF, NZ::noise>(b, al, ha, hb, dva, dvb, d2v, r, s2, mu, C, mua, Ca, mub, Cb, muab, Cab, hll);
        gpcc_mkg_update<P, NOFF, KA>(b, al, ha, r, s2, mu, C, mua, Ca, dll, dva);
        if constexpr (!DIAG) gpcc_mkg_update<P, NOFF, KB>(b, al, hb, r, s2, mu, C, mub, Cb, dll, dvb);
        gpcc_mk_update<P, NOFF>(b, al, r, s2, mu, C, ll);
    }
    return hll;
}

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_hess(const GpccMarkovHessArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double gpcc_mkh_lds[];
    const GpccMkLane ln = gpcc_mk_open(a, gpcc_mkh_lds);
    const int L = a.L;

    // the pair of this workgroup (uniform): slot -> (pa, pb), pa <= pb, rows of the upper triangle one after the other
    const int slot = blockIdx.y;
    int pa = 0, rest = slot;
    while (rest >= L + 1 - pa) {
        rest -= L + 1 - pa;
        ++pa;
    }
    const int pb = pa + rest;
    const GpccMkhParam qa = {pa, false, 0.0}, qb = {pb, false, 0.0}, qr = {-1, false, 0.0};
    double hll;
    if (pa == L)
        hll = gpcc_mkh_walk<P, NOFF, GPCC_MKH_RR>(a, ln, GpccMkPlain(), qr, qr);
    else if (pb == L)
        hll = gpcc_mkh_walk<P, NOFF, GPCC_MKH_AR>(a, ln, GpccMkPlain(), qa, qr);
    else if (pa == pb)
        hll = gpcc_mkh_walk<P, NOFF, GPCC_MKH_AA_DIAG>(a, ln, GpccMkPlain(), qa, qa);
    else
        hll = gpcc_mkh_walk<P, NOFF, GPCC_MKH_AA_OFF>(a, ln, GpccMkPlain(), qa, qb);
    if (ln.valid) a.slot[(long)slot * a.M + ln.row] = hll;
}

// ---- the instantiations that ship (gpcc_markov_hess_inst.hip: one object per P): all but <3, 4> -- Matern-5/2 with four bands and
// marginalised offsets -- which the compiler cannot keep out of scratch memory (512 registers and 28 bytes of scratch; the table is in
// DESIGN.md 4.18 and profiles/markov/kernel_resources_hess.log): gpcc_loglik_hess_hyper_markov_batch returns GPCC_ERR_UNSUPPORTED for it
// and names the dense entry.  gpcc_markov_hess_tau (gpcc_markov_hess_tau.hip.h) ships the same: its leading block comes from here ----
struct GpccMkShipsHess { static constexpr int max_noff[3] = {GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS, 3}; };

// gpcc_markov_hess<g.p, g.noff> on the grid (g.blocks, slots), then the finish kernel over the M rows (gpcc_markov_hess_inst.hip)
hipError_t gpcc_markov_hess_launch(const GpccMkLaunch &g, int slots, const GpccMarkovHessArgs &a);
