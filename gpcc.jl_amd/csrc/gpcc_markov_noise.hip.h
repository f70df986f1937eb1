// gpcc_markov_noise.hip.h -- the linear-time log-likelihood and its gradient of rows that each carry their own (tau, alpha, rho) AND
// their own NOISE MODEL, for gfx950: gpcc_loglik_noise_markov_batch and gpcc_loglik_grad_noise_markov_batch of include/gpcc_hip.h,
// DESIGN.md 4.25; gpcc.jl_amd/markov.py (loglik_noise, loglik_grad_noise) is the same algorithm in numpy.  Point i of band l of row m
// is observed with the variance
//     v_i = kappa_{m,l}^2 sigma_i^2 + nu_{m,l}        kappa >= 0: the scale of the reported error bars, nu >= 0: an excess variance
// kappa = 1, nu = 0 is the handle's model.  The band means and Sigma_b depend on y only and stay the handle's, so a row's value is the
// value of a fresh handle created with the error bars sqrt(v_i).
//
// gpcc_markov_noise_eval<P, NOFF>: ONE LANE PER ROW, gpcc_markov_eval with s2' = fma(kappa_b^2, s2, nu_b) formed before the unedited
// gpcc_mk_update, the way gpcc_markov_resample hands over its own variance.  At kappa = 1, nu = 0 the fma returns s2 exactly and every
// statement has gpcc_markov_eval's operands.  A lane's kappa^2 and nu live in LDS, [band][thread], in a part of the workgroup's
// dynamic LDS carved AFTER the region gpcc_mk_open lays out (gpcc_markov_noise_lds_bytes): 16 more bytes per lane and band, 44 in all.
// A kappa or nu that is negative or not finite: info = -3, after -1 (alpha) and -2 (rho).
//
// gpcc_markov_noise_grad<P, NOFF>: ONE LANE PER (ROW, PARAMETER SLOT), the slot being blockIdx.y as in gpcc_markov_grad: L alpha, one
// rho, L tau (OU: 2L, the first / last pair), then L kappa and L nu.  The alpha, rho and tau slots are gpcc_mkg_walk itself, instantiated
// on this header's noise policy (GpccMknLane: every observation's variance is s2') where gpcc_markov_grad instantiates it on GpccMkPlain.
// A NOISE SLOT of band l is the easiest tangent of all: no dA, no dPinf, no dh, the lowest-band-first order; the observation variance
// alone moves,
//     dvar = [b == l] (2 kappa_l sigma_i^2  or  1)
// and enters the update's tangent through dS only: gpcc_mkg_update<.., GPCC_MKG_NOISE>.  Its propagate is an alpha's
// (gpcc_mkg_propagate<P, NOFF, GPCC_MKG_ALPHA>).
//
// WHAT IS HERE is what the noise model alone has: the policy, the Args struct, the slot count, the LDS behind the shared region, the
// noise slot's walk and the two kernels' slot decoding.
#pragma once
#include "gpcc_markov_grad.hip.h"

#define GPCC_MARKOV_NOISE_LANE_BYTES 16    /* per lane and band, beside GPCC_MARKOV_LANE_BYTES: kappa^2 and nu (doubles) */

// GpccMarkovArgs' fields under the same names (the shared cursor reads them), the noise model and the gradient's slots
struct GpccMarkovNoiseArgs {
    const double *pts;                     // t[N] | r[N] | sigma^2[N], as GpccMarkovArgs
    const double *delays, *alpha, *rho;    // M x L, M x L, M
    double *out_loglik;                    // [M]: gpcc_markov_noise_eval's; read by the finish kernel
    int *out_info;                         // [M]
    int M, L, N, stage;
    int off[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
    const double *kappa, *nu;              // M x L each
    double *slot;                          // [slots][M]: alpha_1..L, rho, tau_1..L (OU: twice), kappa_1..L, nu_1..L
    double *grad;                          // [M][4L + 1]
    int twice;                             // OU: two lanes per tau_l
};

static inline int gpcc_markov_noise_slots(int L, bool twice) { return gpcc_markov_grad_slots(L, twice) + 2 * L; }

// dynamic LDS of a workgroup of `threads` lanes: the shared region first, the family's part behind it
static inline size_t gpcc_markov_noise_lds_bytes(int N, int L, int threads, bool stage)
{
    return gpcc_markov_lds_bytes(N, L, threads, stage) + (size_t)GPCC_MARKOV_NOISE_LANE_BYTES * L * threads;
}

// a lane's noise model: kappa^2 and nu in LDS, [band][thread] (kappa itself is not kept: a kappa slot reads its one from the row again).
// It is the noise policy (gpcc_markov_grad.hip.h, beside GpccMkPlain) that the derivative walks of the noise kernels are instantiated on
struct GpccMknLane {
    static constexpr bool noise = true;
    double *sk2, *snu;                     // LDS, [band][thread]
    int info;                              // gpcc_mk_load_row's, or -3
    // the variance the lane sees at a point of band b
    __device__ __forceinline__ double var(const GpccMkLane &ln, int b, double s2) const
    {
        return fma(sk2[b * ln.nthr + ln.tid], s2, snu[b * ln.nthr + ln.tid]);
    }
};

// the family's prologue behind gpcc_mk_open: carves its part of the LDS after the shared region (which ends at the cursors, L nthr
// ints; L nthr is even for a workgroup of whole waves, so the part is 8-byte aligned), loads the lane's kappa and nu and checks them
template <class ARGS>
__device__ __forceinline__ GpccMknLane gpcc_mkn_open(const ARGS &a, const GpccMkLane &ln)
{
    GpccMknLane nl;
    const int L = a.L, nthr = ln.nthr, tid = ln.tid;
    nl.sk2 = (double *)(ln.scur + L * nthr);
    nl.snu = nl.sk2 + L * nthr;
    const long m_ = ln.valid ? ln.row : a.M - 1;
    bool bad = false;
    for (int l = 0; l < L; ++l) {
        const double k = a.kappa[m_ * L + l], v = a.nu[m_ * L + l];
        bad = bad || !(k >= 0.0 && k < __builtin_inf()) || !(v >= 0.0 && v < __builtin_inf());
        nl.sk2[l * nthr + tid] = k * k;
        nl.snu[l * nthr + tid] = v;
    }
    nl.info = (ln.info == 0 && bad) ? -3 : ln.info;
    return nl;
}

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_noise_eval(const GpccMarkovNoiseArgs a)
{
    constexpr int NS = P + NOFF;
    extern __shared__ __attribute__((aligned(16))) double gpcc_mkn_lds[];
    const GpccMkLane ln = gpcc_mk_open(a, gpcc_mkn_lds);
    const GpccMknLane nl = gpcc_mkn_open(a, ln);

    double lam, lam2, Q[P][P], mu[NS], C[NS][NS];
    gpcc_mk_init<P, NOFF>(ln.rho, a.sigma_b, lam, lam2, Q, mu, C);

    double ll = 0.0, sprev = 0.0;
    int info = nl.info;
    for (int j = 0; j < a.N; ++j) {
        const GpccMkPoint p = gpcc_mk_next<false>(a, ln, j, sprev);
        double A[P][P];
        gpcc_mk_transition<P>(lam, lam2, p.d, A);
        gpcc_mk_propagate<P, NOFF>(A, Q, mu, C);
        const bool ok = gpcc_mk_update<P, NOFF>(p.b, p.al, p.r, nl.var(ln, p.b, p.s2), mu, C, ll);
        info = (info == 0 && !ok) ? j + 1 : info;   // first predictive variance that is not positive and finite
    }
    if (ln.valid) {
        a.out_loglik[ln.row] = info ? __builtin_nan("") : ll;
        a.out_info[ln.row] = info;
    }
}

// a noise slot's walk, the one walk that only a lane with a noise model has: tb its band; a kappa slot has dvar = dk sigma^2 with
// dk = 2 kappa_tb, a nu slot (is_nu) dvar = 1.  Its tangent is propagated as an alpha's and updated by gpcc_mkg_update<.., GPCC_MKG_NOISE>
template <int P, int NOFF>
__device__ __forceinline__ double gpcc_mkn_walk_noise(const GpccMarkovNoiseArgs &a, const GpccMkLane &ln, const GpccMknLane &nl, int tb,
                                                      bool is_nu, double dk)
{
    constexpr int NS = P + NOFF;
    double lam, lam2, Q[P][P], mu[NS], C[NS][NS];
    gpcc_mk_init<P, NOFF>(ln.rho, a.sigma_b, lam, lam2, Q, mu, C);
    double Zd[P][P], dmu[NS], dC[NS][NS];
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) Zd[i][j] = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        dmu[i] = 0.0;
#pragma unroll
        for (int j = 0; j < NS; ++j) dC[i][j] = 0.0;
    }

    double ll = 0.0, dll = 0.0, sprev = 0.0;
    for (int j = 0; j < a.N; ++j) {
        const GpccMkPoint p = gpcc_mk_next<false>(a, ln, j, sprev);
        const int b = p.b;
        const double s2 = nl.var(ln, b, p.s2);
        const double dvar = (b == tb) ? (is_nu ? 1.0 : dk * p.s2) : 0.0;
        double A[P][P];
        gpcc_mk_transition<P>(lam, lam2, p.d, A);
        gpcc_mkg_propagate<P, NOFF, GPCC_MKG_ALPHA>(A, Zd, false, Q, Zd, mu, C, dmu, dC);
        gpcc_mk_propagate<P, NOFF>(A, Q, mu, C);
        gpcc_mkg_update<P, NOFF, GPCC_MKG_NOISE>(b, p.al, false, p.r, s2, mu, C, dmu, dC, dll, dvar);
        gpcc_mk_update<P, NOFF>(b, p.al, p.r, s2, mu, C, ll);
    }
    return dll;
}

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_noise_grad(const GpccMarkovNoiseArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double gpcc_mkng_lds[];
    const GpccMkLane ln = gpcc_mk_open(a, gpcc_mkng_lds);
    const GpccMknLane nl = gpcc_mkn_open(a, ln);
    const int L = a.L, ntau = a.twice ? 2 * L : L;

    // what this workgroup differentiates (uniform)
    const int slot = blockIdx.y;
    double dll;
    if (slot < L) {
        dll = gpcc_mkg_walk<P, NOFF, GPCC_MKG_ALPHA>(a, ln, nl, slot, -1, 0);
    } else if (slot == L) {
        dll = gpcc_mkg_walk<P, NOFF, GPCC_MKG_RHO>(a, ln, nl, -1, -1, 0);
    } else if (slot < L + 1 + ntau) {
        const int q = slot - L - 1, tb = a.twice ? q >> 1 : q;
        dll = gpcc_mkg_walk<P, NOFF, GPCC_MKG_TAU>(a, ln, nl, tb, a.twice ? tb : -1, (q & 1) ? L : -1);
    } else {
        const int q = slot - L - 1 - ntau, tb = q < L ? q : q - L;
        const long m_ = ln.valid ? ln.row : a.M - 1;
        dll = gpcc_mkn_walk_noise<P, NOFF>(a, ln, nl, tb, q >= L, 2.0 * a.kappa[m_ * L + tb]);
    }
    if (ln.valid) a.slot[(long)slot * a.M + ln.row] = dll;
}

// WHAT SHIPS: every <P, NOFF> of the filter, value and gradient.  Registers per lane (tools/kernel_resources.py,
// profiles/markov/kernel_resources_noise.log), no scratch memory in any of them: see DESIGN.md 4.25.
struct GpccMkShipsNoise { static constexpr int max_noff[3] = {GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS, GPCC_MARKOV_MAX_OFFSETS}; };

// ---- launches (gpcc_markov_noise_inst.hip: one object per P) ----
// gpcc_markov_noise_eval<g.p, g.noff> on the grid (g.blocks)
hipError_t gpcc_markov_noise_launch(const GpccMkLaunch &g, const GpccMarkovNoiseArgs &a);
// grid (g.blocks, slots) of gpcc_markov_noise_grad<g.p, g.noff>, then the finish kernel over the M rows
hipError_t gpcc_markov_noise_grad_launch(const GpccMkLaunch &g, int slots, const GpccMarkovNoiseArgs &a);
