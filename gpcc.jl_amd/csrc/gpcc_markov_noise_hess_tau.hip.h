// gpcc_markov_noise_hess_tau.hip.h -- the exact linear-time rows of tau of the Hessian of the log-likelihood of rows that carry their
// own NOISE MODEL, over
//     theta = [alpha_1..alpha_L, rho, tau_1..tau_L, kappa_1..kappa_L, nu_1..nu_L],   n = 4L + 1   (the gradient row's order),
// for gfx950: gpcc_loglik_hess_full_noise_markov_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py
// (loglik_hess_full_noise) is the same algorithm in numpy.  The walk is gpcc_markov_hess_tau.hip.h's one definition (gpcc_mkt_walk),
// instantiated on the noise policy GpccMknLane (gpcc_markov_noise.hip.h: gpcc_mkn_open, GpccMknLane::var) where gpcc_markov_hess_tau
// instantiates it on GpccMkPlain; nothing is approximated.
//
// THE PAIRS are every pair with at least one tau.
//   (alpha_a, tau_l), (rho, tau_l), (tau_l, tau_l), (tau_l, tau_m) l < m   the plain kernel's four kinds, on the mapped variance; the
//            second-order update is the noise instantiation of gpcc_mkh_update with zero variance tangents
//   (tau_l, kappa_m), (tau_l, nu_m), all l, m   the kind GPCC_MKNT_TN, which only a lane with a noise model has.  With a the noise
//            parameter and b = tau_l:
//            first tangent a    the prior's, the transition's and the stationary tangent are zero: it propagates as an alpha tangent
//                     does with a zero A-tangent and has no h-tangent; its first-order update is gpcc_mkg_update<.., GPCC_MKG_NOISE>
//                     with dvar = [band == m] (2 kappa_m sigma_i^2 or 1)
//            first tangent b    the tau tangent: A_b = c_l F A, c_l = [bprev = l] - [band = l], 0 at the first point
//            second tangent     moves as the tau tangent of the "state" (mu_a, C_a) with a zero stationary part, the way an
//                     (alpha, tau) pair's moves; A_a = 0, so there is no cross term
//            update             gpcc_mkh_update with ha = hb = false, dva = dvar, dvb = 0, d2v = 0, then the two first-order
//                     updates and the state's
// WHAT IS HERE is what this family alone has: the Args struct, the slot count, the kernel's slot decoding, what ships and the launch.
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

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_noise_hess_tau(const GpccMarkovNoiseHessTauArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double gpcc_mknt_lds[];
    const GpccMkLane ln = gpcc_mk_open(a, gpcc_mknt_lds);
    const GpccMknLane nl = gpcc_mkn_open(a, ln);
    const int L = a.L, plain = L * L + L + L * (L + 1) / 2;

    // the pair of this workgroup (uniform)
    const int slot = blockIdx.y;
    GpccMkhParam pn;
    pn.band = -1;
    pn.is_nu = false;
    pn.dk = 0.0;
    double hll;
    if (slot < L * L) {
        hll = gpcc_mkt_walk<P, NOFF, GPCC_MKT_AT>(a, ln, nl, slot / L, -1, slot % L, pn);
    } else if (slot < L * L + L) {
        hll = gpcc_mkt_walk<P, NOFF, GPCC_MKT_RT>(a, ln, nl, -1, -1, slot - L * L, pn);
    } else if (slot < L * L + 2 * L) {
        const int l = slot - L * L - L;
        hll = gpcc_mkt_walk<P, NOFF, GPCC_MKT_TT_DIAG>(a, ln, nl, -1, l, l, pn);
    } else if (slot < plain) {
        // (tau_l, tau_m), l < m, rows of the strict upper triangle one after the other
        int ta = 0, rest = slot - L * L - 2 * L;
        while (rest >= L - 1 - ta) {
            rest -= L - 1 - ta;
            ++ta;
        }
        hll = gpcc_mkt_walk<P, NOFF, GPCC_MKT_TT_OFF>(a, ln, nl, -1, ta, ta + 1 + rest, pn);
    } else {
        // (tau_l, kappa_m) [l L + m], then (tau_l, nu_m) [l L + m]; 2 kappa read from the row again
        const int q = slot - plain, k = q % (L * L);
        const long m_ = ln.valid ? ln.row : a.M - 1;
        pn.band = k % L;
        pn.is_nu = q >= L * L;
        pn.dk = pn.is_nu ? 0.0 : 2.0 * a.kappa[m_ * L + pn.band];
        hll = gpcc_mkt_walk<P, NOFF, GPCC_MKNT_TN>(a, ln, nl, -1, -1, k / L, pn);
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
