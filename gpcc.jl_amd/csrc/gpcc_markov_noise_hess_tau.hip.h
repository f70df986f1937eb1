// gpcc_markov_noise_hess_tau.hip.h -- the exact linear-time rows of tau of the Hessian of the log-likelihood of rows that carry their
// own NOISE MODEL, over
//     theta = [alpha_1..alpha_L, rho, tau_1..tau_L, kappa_1..kappa_L, nu_1..nu_L],   n = 4L + 1   (the gradient row's order),
// for gfx950: gpcc_loglik_hess_full_noise_markov_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py
// (loglik_hess_full_noise) is the same algorithm in numpy.  The lag tangents of the transition are gpcc_markov_hess_tau.hip.h's
// (gpcc_mkt_cross, gpcc_mkt_dcompanion_rate, gpcc_mkg_dtransition_lag), the second-order update with variance tangents is
// gpcc_markov_noise_hess.hip.h's (gpcc_mknh_update), a lane's kappa^2 and nu are gpcc_markov_noise.hip.h's (gpcc_mkn_open,
// gpcc_mkn_var); nothing is approximated.
//
// THE PAIRS are every pair with at least one tau.
//   (alpha_a, tau_l), (rho, tau_l), (tau_l, tau_l), (tau_l, tau_m) l < m   gpcc_mkt_walk's recursion, statement by statement, with two
//            changes: every observation's variance is gpcc_mkn_var(...) in place of p.s2, and the update is gpcc_mknh_update with zero
//            variance tangents (the existing kernel's instantiations stay as they are)
//   (tau_l, kappa_m), (tau_l, nu_m), all l, m   NEW.  With a the noise parameter and b = tau_l:
//            first tangent a    the prior's, the transition's and the stationary tangent are zero: it propagates as an alpha tangent
//                     does with a zero A-tangent and has no h-tangent; its first-order update is gpcc_mkn_update with
//                     dvar = [band == m] (2 kappa_m sigma_i^2 or 1)
//            first tangent b    the tau tangent: A_b = c_l F A, c_l = [bprev = l] - [band = l], 0 at the first point
//            second tangent     moves as the tau tangent of the "state" (mu_a, C_a) with a zero stationary part, the way an
//                     (alpha, tau) pair's moves; A_a = 0, so there is no cross term
//            update             gpcc_mknh_update with ha = hb = false, dva = dvar, dvb = 0, d2v = 0, then the two first-order
//                     updates and the state's
//
// TIES are gpcc_markov_hess_tau.hip.h's contract: on an OU row with a step with d == 0 and band != bprev after the first, every lane
// detects the tie in its own merge and stores NaN, so every entry with a tau index is NaN, the (tau, kappa) and (tau, nu) entries
// included; info stays 0; value, gradient and the [alpha, rho, kappa, nu] block are untouched.  Matern-3/2 and -5/2 are exact at
// ties.  With L = 1 every c is 0 and the entries are exact zeros.
//
// gpcc_markov_noise_hess_tau<P, NOFF>: ONE LANE PER (ROW, PAIR SLOT), the slot being blockIdx.y, so a workgroup is uniform in its kind
// of pair: gpcc_markov_hess_tau's L^2 + L + L (L + 1) / 2 slots in its order, then (tau_l, kappa_m) [l L + m], then (tau_l, nu_m)
// [l L + m]: 3 L^2 + L + L (L + 1) / 2 in all.  State and tangents are register-resident; the lane and its merge are
// gpcc_markov.hip.h's (gpcc_mk_open, gpcc_mk_next<false>), the noise model behind the shared region of the LDS
// (gpcc_markov_noise_lds_bytes).  gpcc_markov_noise_hess_tau_finish writes the n x n block: the [alpha, rho, kappa, nu] rows and
// columns copied from gpcc_markov_noise_hess_finish's blocks of the same call, every tau pair to both halves (bitwise symmetric), NaN
// where info != 0.  Lanes beyond M compute row M - 1 again and store nothing.  No atomics: a row's bits depend on the row alone.
#pragma once
#include "gpcc_markov_hess_tau.hip.h"
#include "gpcc_markov_noise_hess.hip.h"

#define GPCC_MKNT_TN 8       /* (tau_l, kappa_m or nu_m) */

// GpccMarkovNoiseArgs' fields under the same names (the shared cursor and gpcc_mkn_open read them), the slots and the blocks
struct GpccMarkovNoiseHessTauArgs {
    const double *pts;
    const double *delays, *alpha, *rho;
    double *out_loglik;                    // gpcc_markov_noise_eval's, of the same call: read by the finish kernel only
    int *out_info;
    int M, L, N, stage;
    int off[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
    const double *kappa, *nu;              // M x L each
    double *slot;                          // [slots][M]
    const double *noise;                   // [M][3L + 1][3L + 1]: gpcc_markov_noise_hess_finish's blocks of the same call
    double *hess;                          // [M][4L + 1][4L + 1]
};

static inline int gpcc_markov_noise_hess_tau_slots(int L) { return gpcc_markov_hess_tau_slots(L) + 2 * L * L; }

// one lane's walk over the merged observations for a pair of kind PAIR: gpcc_mkt_walk on the mapped variance for the pairs without a
// noise parameter (pa: the band of the pair's alpha, ta: of its first tau, tb: of its (second) tau); for GPCC_MKNT_TN tb is the band
// of the tau and pn the noise parameter.  NaN on an OU row with a cross-band tie
template <int P, int NOFF, int PAIR>
__device__ __forceinline__ double gpcc_mknt_walk(const GpccMarkovNoiseHessTauArgs &a, const GpccMkLane &ln, const GpccMknLane &nl, int pa,
                                                 int ta, int tb, const GpccMknhParam pn)
{
    constexpr int NS = P + NOFF;
    constexpr bool DIAG = PAIR == GPCC_MKT_TT_DIAG;
    constexpr bool TN = PAIR == GPCC_MKNT_TN;
    constexpr int KA = (PAIR == GPCC_MKT_AT || TN) ? GPCC_MKG_ALPHA : (PAIR == GPCC_MKT_RT ? GPCC_MKG_RHO : GPCC_MKG_TAU);
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
        const double d = p.d, al = p.al, r = p.r, s2 = gpcc_mkn_var(ln, nl, b, p.s2);
        if constexpr (P == 1) tie = tie || (j > 0 && d == 0.0 && b != bprev);
        // the variance's tangent by the pair's noise parameter at this observation
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
        gpcc_mknh_update<P, NOFF>(b, al, ha, false, dva, 0.0, 0.0, r, s2, mu, C, mua, Ca, mub, Cb, muab, Cab, hll);
        if constexpr (TN)
            gpcc_mkn_update<P, NOFF>(b, al, dva, r, s2, mu, C, mua, Ca, dll);
        else
            gpcc_mkg_update<P, NOFF, KA>(b, al, ha, r, s2, mu, C, mua, Ca, dll);
        if constexpr (!DIAG) gpcc_mkg_update<P, NOFF, GPCC_MKG_TAU>(b, al, false, r, s2, mu, C, mub, Cb, dll);
        gpcc_mk_update<P, NOFF>(b, al, r, s2, mu, C, ll);
    }
    return tie ? __builtin_nan("") : hll;
}

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_noise_hess_tau(const GpccMarkovNoiseHessTauArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double gpcc_mknt_lds[];
    const GpccMkLane ln = gpcc_mk_open(a, gpcc_mknt_lds);
    const GpccMknLane nl = gpcc_mkn_open(a, ln);
    const int L = a.L, plain = L * L + L + L * (L + 1) / 2;

    // the pair of this workgroup (uniform)
    const int slot = blockIdx.y;
    GpccMknhParam pn;
    pn.band = -1;
    pn.is_nu = false;
    pn.dk = 0.0;
    double hll;
    if (slot < L * L) {
        hll = gpcc_mknt_walk<P, NOFF, GPCC_MKT_AT>(a, ln, nl, slot / L, -1, slot % L, pn);
    } else if (slot < L * L + L) {
        hll = gpcc_mknt_walk<P, NOFF, GPCC_MKT_RT>(a, ln, nl, -1, -1, slot - L * L, pn);
    } else if (slot < L * L + 2 * L) {
        const int l = slot - L * L - L;
        hll = gpcc_mknt_walk<P, NOFF, GPCC_MKT_TT_DIAG>(a, ln, nl, -1, l, l, pn);
    } else if (slot < plain) {
        // (tau_l, tau_m), l < m, rows of the strict upper triangle one after the other
        int ta = 0, rest = slot - L * L - 2 * L;
        while (rest >= L - 1 - ta) {
            rest -= L - 1 - ta;
            ++ta;
        }
        hll = gpcc_mknt_walk<P, NOFF, GPCC_MKT_TT_OFF>(a, ln, nl, -1, ta, ta + 1 + rest, pn);
    } else {
        // (tau_l, kappa_m) [l L + m], then (tau_l, nu_m) [l L + m]; 2 kappa read from the row again
        const int q = slot - plain, k = q % (L * L);
        const long m_ = ln.valid ? ln.row : a.M - 1;
        pn.band = k % L;
        pn.is_nu = q >= L * L;
        pn.dk = pn.is_nu ? 0.0 : 2.0 * a.kappa[m_ * L + pn.band];
        hll = gpcc_mknt_walk<P, NOFF, GPCC_MKNT_TN>(a, ln, nl, -1, -1, k / L, pn);
    }
    if (ln.valid) a.slot[(long)slot * a.M + ln.row] = hll;
}

// ---- the instantiations that ship (gpcc_markov_noise_hess_tau_inst.hip: one object per P): those of the block of the same call
// (GpccMkShipsNoiseHess), all but <3, 4>, with no scratch memory in any of them (the table is in DESIGN.md 4.27 and
// profiles/markov/kernel_resources_noise_hess_tau.log).  gpcc_loglik_hess_full_noise_markov_batch returns GPCC_ERR_UNSUPPORTED for what
// does not ship and names the dense entry on effective_std ----
struct GpccMkShipsNoiseHessTau { static constexpr int max_noff[3] = {GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS, 3}; };

// gpcc_markov_noise_hess_tau<g.p, g.noff> on the grid (g.blocks, slots), then the finish kernel over the M rows
// (gpcc_markov_noise_hess_tau_inst.hip)
hipError_t gpcc_markov_noise_hess_tau_launch(const GpccMkLaunch &g, int slots, const GpccMarkovNoiseHessTauArgs &a);
