// gpcc_markov_noise_hess.hip.h -- the exact linear-time Hessian of the log-likelihood of rows that carry their own NOISE MODEL, over
//     theta = [alpha_1..alpha_L, rho, kappa_1..kappa_L, nu_1..nu_L],   n = 3L + 1,
// for gfx950: gpcc_loglik_hess_noise_markov_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py (loglik_hess_noise) is the
// same algorithm in numpy.  Point i of band l of row m is observed with the variance kappa_{m,l}^2 sigma_i^2 + nu_{m,l}
// (gpcc_markov_noise.hip.h).  Nothing is approximated.
//
// THE WALK AND THE UPDATES are gpcc_markov_hess.hip.h's and gpcc_markov_grad.hip.h's one definition each (gpcc_mkh_walk, gpcc_mkh_update,
// gpcc_mkg_update), instantiated on the noise policy GpccMknLane where gpcc_markov_hess instantiates them on GpccMkPlain.  What a lane
// with a noise model adds to them:
//   a noise tangent in the pair   for kappa_l or nu_l the prior's, the transition's and the stationary tangent are zero: it propagates as
//            an alpha tangent does, with a zero A-tangent, and has no h-tangent.  At an observation of band b the variance moves by
//            dvar = [b == l] (2 kappa_l sigma_i^2 or 1); its first-order update is gpcc_mkg_update<.., GPCC_MKG_NOISE>
//   the variance tangents of the second-order update   S_a += dvar_a, S_b += dvar_b, S_ab += d2var, where d2var = 2 sigma_i^2 on
//            (kappa_l, kappa_l) at the observations of band l and 0 for every other pair, (kappa_l, nu_l) included; everything behind
//            S, S_a, S_b, S_ab is the one algebra
//   kinds of pair   alpha alpha (diagonal, off-diagonal), alpha rho, rho rho: the plain kernel's four, on the mapped variance;
//            alpha noise: no tangent of A;  rho noise: A_rho and Pinf_rho only, the second tangent moves as the rho tangent of the
//            noise "state" (the way alpha rho's moves);  noise noise (diagonal, off-diagonal): no tangent of A at all.  A noise
//            noise pair on two bands is NOT zero: the filter couples the bands.
// WHAT IS HERE is what this family alone has: the Args struct, the slot count, the kernel's slot decoding, what ships and the launch.
//
// gpcc_markov_noise_hess<P, NOFF>: ONE LANE PER (ROW, PAIR SLOT), a <= b, the slot being blockIdx.y: n (n + 1) / 2 slots in upper-triangle
// row order, so a workgroup is uniform in its pair; the walk is a template on the kind of pair, a diagonal pair carries three sets, the
// others four.  State and tangents are register-resident; a lane's kappa^2 and nu are in LDS behind the shared region (gpcc_mkn_open)
// and every observation's variance is GpccMknLane::var.  Per-slot results go to slot[slot][row]; gpcc_markov_noise_hess_finish writes every
// pair to both halves of the row's n x n block (bitwise symmetric), NaN where info != 0.  Lanes beyond M compute row M - 1 again and
// store nothing.  No atomics: a row's bits depend on the row alone.
#pragma once
#include "gpcc_markov_hess.hip.h"
#include "gpcc_markov_noise.hip.h"

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
    GpccMkhParam pa, pb;
    pa.band = ia < L ? ia : (ia == L ? -1 : (ia - L - 1) % L);
    pb.band = ib < L ? ib : (ib == L ? -1 : (ib - L - 1) % L);
    pa.is_nu = ia > 2 * L;
    pb.is_nu = ib > 2 * L;
    pa.dk = (ia > L && !pa.is_nu) ? 2.0 * a.kappa[m_ * L + pa.band] : 0.0;
    pb.dk = (ib > L && !pb.is_nu) ? 2.0 * a.kappa[m_ * L + pb.band] : 0.0;
    double hll;
    if (ib < L)
        hll = ia == ib ? gpcc_mkh_walk<P, NOFF, GPCC_MKH_AA_DIAG>(a, ln, nl, pa, pb) : gpcc_mkh_walk<P, NOFF, GPCC_MKH_AA_OFF>(a, ln, nl, pa, pb);
    else if (ib == L)
        hll = ia == L ? gpcc_mkh_walk<P, NOFF, GPCC_MKH_RR>(a, ln, nl, pa, pb) : gpcc_mkh_walk<P, NOFF, GPCC_MKH_AR>(a, ln, nl, pa, pb);
    else if (ia < L)
        hll = gpcc_mkh_walk<P, NOFF, GPCC_MKNH_AN>(a, ln, nl, pa, pb);
    else if (ia == L)
        hll = gpcc_mkh_walk<P, NOFF, GPCC_MKNH_RN>(a, ln, nl, pa, pb);
    else
        hll = ia == ib ? gpcc_mkh_walk<P, NOFF, GPCC_MKNH_NN_DIAG>(a, ln, nl, pa, pb) : gpcc_mkh_walk<P, NOFF, GPCC_MKNH_NN_OFF>(a, ln, nl, pa, pb);
    if (ln.valid) a.slot[(long)slot * a.M + ln.row] = hll;
}

// ---- the instantiations that ship (gpcc_markov_noise_hess_inst.hip: one object per P): those of the plain block (GpccMkShipsHess), all
// but <3, 4>, with no scratch memory in any of them (the table is in DESIGN.md 4.26 and profiles/markov/kernel_resources_noise_hess.log).
// gpcc_loglik_hess_noise_markov_batch returns GPCC_ERR_UNSUPPORTED for what does not ship and names the dense entry on effective_std ----
struct GpccMkShipsNoiseHess { static constexpr int max_noff[3] = {GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS, 3}; };

// gpcc_markov_noise_hess<g.p, g.noff> on the grid (g.blocks, slots), then the finish kernel over the M rows (gpcc_markov_noise_hess_inst.hip)
hipError_t gpcc_markov_noise_hess_launch(const GpccMkLaunch &g, int slots, const GpccMarkovNoiseHessArgs &a);
