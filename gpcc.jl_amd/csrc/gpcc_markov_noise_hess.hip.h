// gpcc_markov_noise_hess.hip.h -- the exact linear-time Hessian of the log-likelihood of rows that carry their own NOISE MODEL, over
//     theta = [alpha_1..alpha_L, rho, kappa_1..kappa_L, nu_1..nu_L],   n = 3L + 1,
// for gfx950: gpcc_loglik_hess_noise_markov_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py (loglik_hess_noise) is the
// same algorithm in numpy.  Point i of band l of row m is observed with the variance kappa_{m,l}^2 sigma_i^2 + nu_{m,l}
// (gpcc_markov_noise.hip.h).  The second-order forward sensitivity is gpcc_markov_hess.hip.h's, the noise tangent is
// gpcc_markov_noise.hip.h's; nothing is approximated.
//
// WHAT IS NEW AGAINST gpcc_mkh_walk.
//   a noise tangent in the pair   for kappa_l or nu_l the prior's, the transition's and the stationary tangent are zero: it propagates as
//            an alpha tangent does (gpcc_mkg_propagate<.., GPCC_MKG_ALPHA> with a zero A-tangent) and has no h-tangent.  At an
//            observation of band b the variance moves by dvar = [b == l] (2 kappa_l sigma_i^2 or 1); its first-order update is
//            gpcc_mkn_update
//   the update with variance tangents   gpcc_mkh_update with S_a += dvar_a, S_b += dvar_b, S_ab += d2var, where d2var = 2 sigma_i^2 on
//            (kappa_l, kappa_l) at the observations of band l and 0 for every other pair, (kappa_l, nu_l) included; everything behind
//            S, S_a, S_b, S_ab is that function's algebra (gpcc_mknh_update: a function of its own, gpcc_mkh_update is not touched)
//   kinds of pair   alpha alpha (diagonal, off-diagonal), alpha rho, rho rho: gpcc_mkh_walk's steps on the mapped variance;
//            alpha noise: no tangent of A;  rho noise: A_rho and Pinf_rho only, the second tangent moves as the rho tangent of the
//            noise "state" (the way alpha rho moves today);  noise noise (diagonal, off-diagonal): no tangent of A at all.  A noise
//            noise pair on two bands is NOT zero: the filter couples the bands.
//
// gpcc_markov_noise_hess<P, NOFF>: ONE LANE PER (ROW, PAIR SLOT), a <= b, the slot being blockIdx.y: n (n + 1) / 2 slots in upper-triangle
// row order, so a workgroup is uniform in its pair; the walk is a template on the kind of pair, a diagonal pair carries three sets, the
// others four.  State and tangents are register-resident; a lane's kappa^2 and nu are in LDS behind the shared region (gpcc_mkn_open)
// and every observation's variance is gpcc_mkn_var.  Per-slot results go to slot[slot][row]; gpcc_markov_noise_hess_finish writes every
// pair to both halves of the row's n x n block (bitwise symmetric), NaN where info != 0.  Lanes beyond M compute row M - 1 again and
// store nothing.  No atomics: a row's bits depend on the row alone.
#pragma once
#include "gpcc_markov_hess.hip.h"
#include "gpcc_markov_noise.hip.h"

#define GPCC_MKNH_AN 4        /* (alpha_l, kappa_m or nu_m) */
#define GPCC_MKNH_RN 5        /* (rho, kappa_m or nu_m) */
#define GPCC_MKNH_NN_DIAG 6   /* (kappa_l, kappa_l), (nu_l, nu_l) */
#define GPCC_MKNH_NN_OFF 7    /* two different noise parameters, of one band or of two */

// GpccMarkovNoiseArgs' fields under the same names (the shared cursor and gpcc_mkn_open read them), the pair slots and the blocks
struct GpccMarkovNoiseHessArgs {
    const double *pts;
    const double *delays, *alpha, *rho;
    double *out_loglik;                    // gpcc_markov_noise_eval's, of the same call: read by the finish kernel only
    int *out_info;
    int M, L, N, stage;
    int off[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
    const double *kappa, *nu;              // M x L each
    double *slot;                          // [slots][M]
    double *hess;                          // [M][3L + 1][3L + 1]
};

static inline int gpcc_markov_noise_hess_slots(int L) { return (3 * L + 1) * (3 * L + 2) / 2; }

// gpcc_mkh_update with variance tangents: S_a += dva, S_b += dvb, S_ab += d2v; a noise parameter has no h-tangent (its ha / hb is false)
template <int P, int NOFF>
__device__ __forceinline__ void gpcc_mknh_update(int b, double al, bool ha, bool hb, double dva, double dvb, double d2v, double r, double s2,
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
    double S = al * Ph[0] + s2, Sa = al * Pha[0] + dva, Sb = al * Phb[0] + dvb, Sab = al * Phab[0] + d2v;
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
// is a nu and the factor of sigma_i^2 in a kappa's dvar (2 kappa)
struct GpccMknhParam {
    int band;
    bool is_nu;
    double dk;
};

// one lane's walk over the merged observations for the pair (pa, pb) of kind PAIR
template <int P, int NOFF, int PAIR>
__device__ __forceinline__ double gpcc_mknh_walk(const GpccMarkovNoiseHessArgs &a, const GpccMkLane &ln, const GpccMknLane &nl,
                                                 const GpccMknhParam pa, const GpccMknhParam pb)
{
    constexpr int NS = P + NOFF;
    constexpr bool DIAG = PAIR == GPCC_MKH_AA_DIAG || PAIR == GPCC_MKH_RR || PAIR == GPCC_MKNH_NN_DIAG;
    constexpr bool RHO = PAIR == GPCC_MKH_AR || PAIR == GPCC_MKH_RR || PAIR == GPCC_MKNH_RN;      // some tangent of A is formed
    constexpr bool NA = PAIR == GPCC_MKNH_NN_DIAG || PAIR == GPCC_MKNH_NN_OFF;                    // the first parameter is a noise parameter
    constexpr bool NB = NA || PAIR == GPCC_MKNH_AN || PAIR == GPCC_MKNH_RN;                       // the second one is
    constexpr bool RA = PAIR == GPCC_MKH_RR || PAIR == GPCC_MKNH_RN, RB = PAIR == GPCC_MKH_AR || PAIR == GPCC_MKH_RR;   // ... is rho
    constexpr int KA = RA ? GPCC_MKG_RHO : GPCC_MKG_ALPHA, KB = RB ? GPCC_MKG_RHO : GPCC_MKG_ALPHA;   // (a noise tangent moves as an alpha's)
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
        const double d = p.d, al = p.al, r = p.r, s2 = gpcc_mkn_var(ln, nl, b, p.s2);
        // the variance's tangents at this observation
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
        gpcc_mknh_update<P, NOFF>(b, al, ha, hb, dva, dvb, d2v, r, s2, mu, C, mua, Ca, mub, Cb, muab, Cab, hll);
        if constexpr (NA)
            gpcc_mkn_update<P, NOFF>(b, al, dva, r, s2, mu, C, mua, Ca, dll);
        else
            gpcc_mkg_update<P, NOFF, KA>(b, al, ha, r, s2, mu, C, mua, Ca, dll);
        if constexpr (!DIAG) {
            if constexpr (NB)
                gpcc_mkn_update<P, NOFF>(b, al, dvb, r, s2, mu, C, mub, Cb, dll);
            else
                gpcc_mkg_update<P, NOFF, KB>(b, al, hb, r, s2, mu, C, mub, Cb, dll);
        }
        gpcc_mk_update<P, NOFF>(b, al, r, s2, mu, C, ll);
    }
    return hll;
}

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_noise_hess(const GpccMarkovNoiseHessArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double gpcc_mknh_lds[];
    const GpccMkLane ln = gpcc_mk_open(a, gpcc_mknh_lds);
    const GpccMknLane nl = gpcc_mkn_open(a, ln);
    const int L = a.L, n = 3 * L + 1;

    // the pair of this workgroup (uniform): slot -> (ia, ib), ia <= ib, rows of the upper triangle one after the other
    const int slot = blockIdx.y;
    int ia = 0, rest = slot;
    while (rest >= n - ia) {
        rest -= n - ia;
        ++ia;
    }
    const int ib = ia + rest;
    // theta's index -> the parameter: alpha_l, rho, kappa_l (2 kappa read from the row again), nu_l
    const long m_ = ln.valid ? ln.row : a.M - 1;
    GpccMknhParam pa, pb;
    pa.band = ia < L ? ia : (ia == L ? -1 : (ia - L - 1) % L);
    pb.band = ib < L ? ib : (ib == L ? -1 : (ib - L - 1) % L);
    pa.is_nu = ia > 2 * L;
    pb.is_nu = ib > 2 * L;
    pa.dk = (ia > L && !pa.is_nu) ? 2.0 * a.kappa[m_ * L + pa.band] : 0.0;
    pb.dk = (ib > L && !pb.is_nu) ? 2.0 * a.kappa[m_ * L + pb.band] : 0.0;
    double hll;
    if (ib < L)
        hll = ia == ib ? gpcc_mknh_walk<P, NOFF, GPCC_MKH_AA_DIAG>(a, ln, nl, pa, pb) : gpcc_mknh_walk<P, NOFF, GPCC_MKH_AA_OFF>(a, ln, nl, pa, pb);
    else if (ib == L)
        hll = ia == L ? gpcc_mknh_walk<P, NOFF, GPCC_MKH_RR>(a, ln, nl, pa, pb) : gpcc_mknh_walk<P, NOFF, GPCC_MKH_AR>(a, ln, nl, pa, pb);
    else if (ia < L)
        hll = gpcc_mknh_walk<P, NOFF, GPCC_MKNH_AN>(a, ln, nl, pa, pb);
    else if (ia == L)
        hll = gpcc_mknh_walk<P, NOFF, GPCC_MKNH_RN>(a, ln, nl, pa, pb);
    else
        hll = ia == ib ? gpcc_mknh_walk<P, NOFF, GPCC_MKNH_NN_DIAG>(a, ln, nl, pa, pb) : gpcc_mknh_walk<P, NOFF, GPCC_MKNH_NN_OFF>(a, ln, nl, pa, pb);
    if (ln.valid) a.slot[(long)slot * a.M + ln.row] = hll;
}

// ---- the instantiations that ship (gpcc_markov_noise_hess_inst.hip: one object per P): those of the plain block (GpccMkShipsHess), all
// but <3, 4>, with no scratch memory in any of them (the table is in DESIGN.md 4.26 and profiles/markov/kernel_resources_noise_hess.log).
// gpcc_loglik_hess_noise_markov_batch returns GPCC_ERR_UNSUPPORTED for what does not ship and names the dense entry on effective_std ----
struct GpccMkShipsNoiseHess { static constexpr int max_noff[3] = {GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS, 3}; };

// gpcc_markov_noise_hess<g.p, g.noff> on the grid (g.blocks, slots), then the finish kernel over the M rows (gpcc_markov_noise_hess_inst.hip)
hipError_t gpcc_markov_noise_hess_launch(const GpccMkLaunch &g, int slots, const GpccMarkovNoiseHessArgs &a);
