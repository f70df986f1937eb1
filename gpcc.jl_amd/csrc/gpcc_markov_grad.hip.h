// gpcc_markov_grad.hip.h -- the exact linear-time gradient of the log-likelihood of the Markov kernels (OU, Matern-3/2, Matern-5/2)
// for gfx950: gpcc_loglik_grad_markov_batch of include/gpcc_hip.h; gpcc.jl_amd/markov.py (loglik_grad) is the same
// algorithm in numpy.  The state-space model and the filter's step (gpcc_mk_*) are gpcc_markov.hip.h's; nothing is approximated.
//
// FORWARD SENSITIVITY.  The derivative of the filter's log-likelihood with respect to one parameter theta is carried beside the
// filter: the tangents (dmu, dC) = d(mu, C)/d theta obey the derivative of the step, and the log-likelihood's tangent is summed as the
// value is.  The parameters enter in four places:
//   alpha_l  through h = alpha_band e_1 (+ e_{P + band}) only: dh = e_1 on the observations of band l
//   rho      through lambda (d lambda / d rho = -lambda / rho): in A(d), in Pinf and in the prior state blockdiag(Pinf, Sigma_b)
//   tau_l    through the lags only: with the merged order fixed d_i = s_i - s_{i-1}, d d_i / d tau_l = -[band_i = l] + [band_{i-1} = l]
//            (0 at the first point), and dA/dd = F A with F the companion matrix of (lambda + d/dt)^P
//   step     dC_xx <- dA D A' + A dD A' + A D dA' + dPinf (D = C_xx - Pinf, dD = dC_xx - dPinf), dmu <- dA mu + A dmu,
//            dC_xb <- dA C_xb + A dC_xb
//   update   Ph = C h, dPh = dC h + C dh, dS = 2 dh'Ph + h'dC h, deps = -dh'mu - h'dmu, g = eps / S, dg = (deps - g dS) / S:
//            dll -= (dS / S + 2 g deps - g^2 dS) / 2,  dmu += dPh g + Ph dg,  dC -= (dPh Ph' + Ph dPh') / S - Ph Ph' dS / S^2
//
// TIES IN SHIFTED TIME.  The merged order is piecewise constant in tau, so the tangent with the order fixed is a one-sided derivative
// at an exact tie between two bands.  Matern-3/2 and -5/2 are C^1 there: the one-sided value is the derivative.  OU has a kink, and
// gpcc_loglik_grad_batch returns dk/ds(0) = 0, the mean of the one-sided derivatives.  The trace formula is linear in dK, so that mean
// is (tangent with band l FIRST among tied points + tangent with band l LAST) / 2, all other bands keeping the lowest-band-first rule:
// OU computes every tau_l twice, with band l's rank among ties -1 and L, and gpcc_markov_grad_finish averages the pair.  Without ties
// both lanes walk the same order and the mean is exact.
//
// gpcc_markov_grad<P, NOFF>: ONE LANE PER (ROW, PARAMETER SLOT), the slot being blockIdx.y, so a workgroup is uniform in what it
// differentiates: L alpha slots, one rho slot, L tau slots (OU: 2L).  The body is specialised by the kind of slot: an alpha lane
// carries no dA, a tau lane forms dA only on the steps next to a point of its band, the rho lane on every step.  State and tangent
// state are register-resident (2 (n + n (n + 1) / 2) <= 70 doubles at n = 7).  The lane and its merge are gpcc_markov.hip.h's
// (gpcc_mk_open, gpcc_mk_next with the ranked tie rule; LDS as gpcc_markov_lds_bytes counts it); the walk keeps the band of the point
// before (bprev) for the lags' tangents.  The primal recursion is the one filter step of gpcc_markov.hip.h, called once.  Per-slot
// results go to slot[slot][row], so a wave's stores coalesce.  Lanes beyond M compute row M - 1 again and store nothing.  No atomics,
// no communication between lanes.
//
// ONE WALK, THREE KERNELS.  gpcc_mkg_walk is a template on the lane's noise policy and on its data policy (both below):
// gpcc_markov_grad instantiates it on GpccMkPlain and GpccMkOwnData, gpcc_markov_noise_grad (gpcc_markov_noise.hip.h) on a lane with its
// own kappa and nu for its alpha, rho and tau slots, gpcc_markov_resample_grad (gpcc_markov_resample_grad.hip.h) on a lane that reads
// its own resampled data set and skips the points it drops.
// gpcc_mkg_update has the kind GPCC_MKG_NOISE for the tangent by a kappa or a nu, which the second-order walks carry as well.
#pragma once
#include "gpcc_markov.hip.h"

#define GPCC_MKG_ALPHA 0
#define GPCC_MKG_RHO 1
#define GPCC_MKG_TAU 2
#define GPCC_MKG_NOISE 3   /* a kappa or a nu of gpcc_markov_noise.hip.h: moves as an alpha's tangent, its update has dvar in place of dh */

// THE NOISE POLICY of a walk: the variance a lane observes a point of band b with, from the handle's sigma_i^2.  Every derivative walk of
// this path (gpcc_mkg_walk, gpcc_mkh_walk, gpcc_mkt_walk) is a template on it and has one definition.  A plain lane holds nothing and
// sees sigma_i^2 itself; a lane with a noise model of its own is gpcc_markov_noise.hip.h's GpccMknLane (kappa_b^2 sigma_i^2 + nu_b).
// `noise` says at compile time whether variance tangents exist at all: where it is false no statement of a walk has an operand for them
struct GpccMkPlain {
    static constexpr bool noise = false;
    __device__ __forceinline__ double var(const GpccMkLane &, int, double s2) const { return s2; }
};

// THE DATA POLICY of the first-order walk: what a lane observes at the point the cursor took.  take() hands over the residual, the
// variance (before the noise policy), the lag from the lane's last observation and whether this is its first; kept false: the point is
// not in the lane's data set and the walk does nothing at it.  The handle's own data: gpcc_mk_next's r, s2 and d as they are, never a
// skip, no state -- after inlining the statements of the walk have the operands they had without a policy.  `resampled` says at compile
// time whose Sigma_b the prior state takes: the kernel's argument or the policy's own (gpcc_markov_resample_grad.hip.h, GpccMkrData)
struct GpccMkObs {
    double r, s2, d;
    bool first, kept;
};

struct GpccMkOwnData {
    static constexpr bool resampled = false;
    __device__ __forceinline__ GpccMkObs take(const GpccMkLane &, const GpccMkPoint &p, int j, double) { return {p.r, p.s2, p.d, j == 0, true}; }
};

// GpccMarkovArgs' fields under the same names (the host fills both through one template) and the slots
struct GpccMarkovGradArgs {
    const double *pts;                     // t[N] | r[N] | sigma^2[N], as GpccMarkovArgs
    const double *delays, *alpha, *rho;    // M x L, M x L, M
    double *out_loglik;                    // gpcc_markov_eval's, of the same call: read by the finish kernel only
    int *out_info;
    double *slot;                          // [slots][M]: alpha_1..L, rho, tau_1..L (twice: tau_1 first, tau_1 last, tau_2 first, ...)
    double *grad;                          // [M][2L + 1]
    int M, L, N, stage;
    int twice;                             // OU: two lanes per tau_l
    int off[GPCC_MARKOV_MAXL + 1];
    double sigma_b[GPCC_MARKOV_MAX_OFFSETS];
};

static inline int gpcc_markov_grad_slots(int L, bool twice) { return L + 1 + (twice ? 2 * L : L); }

// dA = dd F A: the tangent of the transition over a lag whose tangent is dd
template <int P>
__device__ __forceinline__ void gpcc_mkg_dtransition_lag(double lam, double lam2, double dd, const double (&A)[P][P], double (&Ad)[P][P])
{
#pragma unroll
    for (int k = 0; k < P; ++k) {
        if constexpr (P == 1) {
            Ad[0][k] = -dd * lam * A[0][k];
        } else if constexpr (P == 2) {
            Ad[0][k] = dd * A[1][k];
            Ad[1][k] = -dd * (lam2 * A[0][k] + 2.0 * lam * A[1][k]);
        } else {
            Ad[0][k] = dd * A[1][k];
            Ad[1][k] = dd * A[2][k];
            Ad[2][k] = -dd * (lam2 * lam * A[0][k] + 3.0 * lam2 * A[1][k] + 3.0 * lam * A[2][k]);
        }
    }
}

// dA = dlam dA/dlambda, in closed form per kernel (e = exp(-lambda d), x = lambda d)
template <int P>
__device__ __forceinline__ void gpcc_mkg_dtransition_rate(double lam, double lam2, double d, double dlam, double (&Ad)[P][P])
{
    const double x = lam * d, e = exp(-x) * dlam;
    if constexpr (P == 1) {
        Ad[0][0] = -e * d;
    } else if constexpr (P == 2) {
        Ad[0][0] = -e * d * x;
        Ad[0][1] = -e * d * d;
        Ad[1][0] = e * x * (x - 2.0);
        Ad[1][1] = e * d * (x - 2.0);
    } else {
        const double q = 3.0 * x - 3.0 - 0.5 * x * x;
        Ad[0][0] = -0.5 * e * d * x * x;
        Ad[0][1] = -e * d * d * x;
        Ad[0][2] = -0.5 * e * d * d * d;
        Ad[1][0] = 0.5 * e * x * x * (x - 3.0);
        Ad[1][1] = e * d * x * (x - 3.0);
        Ad[1][2] = 0.5 * e * d * d * (x - 3.0);
        Ad[2][0] = e * lam * x * q;
        Ad[2][1] = e * x * (6.0 * x - 6.0 - x * x);
        Ad[2][2] = e * d * q;
    }
}

// dPinf = dlam dPinf/dlambda
template <int P>
__device__ __forceinline__ void gpcc_mkg_dstationary(double lam, double lam2, double dlam, double (&Qd)[P][P])
{
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) Qd[i][j] = 0.0;
    if constexpr (P == 2) Qd[1][1] = 2.0 * lam * dlam;
    if constexpr (P == 3) {
        Qd[0][2] = Qd[2][0] = -(2.0 / 3.0) * lam * dlam;
        Qd[1][1] = (2.0 / 3.0) * lam * dlam;
        Qd[2][2] = 4.0 * lam2 * lam * dlam;
    }
}

// the tangent of gpcc_mk_propagate, from the state BEFORE it.  KIND: GPCC_MKG_ALPHA and GPCC_MKG_NOISE have neither dA nor dPinf,
// GPCC_MKG_TAU has dA where `ad`, GPCC_MKG_RHO has both
template <int P, int NOFF, int KIND>
__device__ __forceinline__ void gpcc_mkg_propagate(const double (&A)[P][P], const double (&Ad)[P][P], bool ad, const double (&Q)[P][P],
                                                   const double (&Qd)[P][P], const double (&mu)[P + NOFF],
                                                   const double (&C)[P + NOFF][P + NOFF], double (&dmu)[P + NOFF],
                                                   double (&dC)[P + NOFF][P + NOFF])
{
    double t1[P], Dd[P][P], Td[P][P];
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) acc += A[i2][k] * dmu[k];
        t1[i2] = acc;
    }
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2) dmu[i2] = t1[i2];
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
        for (int k = 0; k < P; ++k) {
            Dd[i2][k] = GPCC_MK_SYM(dC, i2, k);
            if constexpr (KIND == GPCC_MKG_RHO) Dd[i2][k] -= Qd[i2][k];
        }
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
        for (int k = 0; k < P; ++k) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < P; ++q) acc += A[i2][q] * Dd[q][k];
            Td[i2][k] = acc;
        }
#pragma unroll
    for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
        for (int k = i2; k < P; ++k) {
            double acc = 0.0;
            if constexpr (KIND == GPCC_MKG_RHO) acc = Qd[i2][k];
#pragma unroll
            for (int q = 0; q < P; ++q) acc += Td[i2][q] * A[k][q];
            dC[i2][k] = acc;
        }
#pragma unroll
    for (int c = 0; c < NOFF; ++c) {
#pragma unroll
        for (int i2 = 0; i2 < P; ++i2) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k) acc += A[i2][k] * dC[k][P + c];
            t1[i2] = acc;
        }
#pragma unroll
        for (int i2 = 0; i2 < P; ++i2) dC[i2][P + c] = t1[i2];
    }
    if constexpr (KIND == GPCC_MKG_RHO || KIND == GPCC_MKG_TAU) {
        if (ad) {
            // the dA terms: dmu += dA mu, dC_xx += dA D A' + (dA D A')', dC_xb += dA C_xb
            double T[P][P], W[P][P];
#pragma unroll
            for (int i2 = 0; i2 < P; ++i2) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < P; ++k) acc += Ad[i2][k] * mu[k];
                dmu[i2] += acc;
            }
#pragma unroll
            for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    double acc = 0.0;
#pragma unroll
                    for (int q = 0; q < P; ++q) acc += Ad[i2][q] * (GPCC_MK_SYM(C, q, k) - Q[q][k]);
                    T[i2][k] = acc;
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
                for (int k = i2; k < P; ++k) dC[i2][k] += W[i2][k] + W[k][i2];
#pragma unroll
            for (int c = 0; c < NOFF; ++c)
#pragma unroll
                for (int i2 = 0; i2 < P; ++i2) {
                    double acc = 0.0;
#pragma unroll
                    for (int k = 0; k < P; ++k) acc += Ad[i2][k] * C[k][P + c];
                    dC[i2][P + c] += acc;
                }
        }
    }
}

// the tangent of gpcc_mk_update, from the state BEFORE it (after the propagation).  dh: this observation's h moves with the lane's alpha
// (GPCC_MKG_ALPHA reads it).  dvar: the tangent of this observation's variance, [b == l] (2 kappa_l sigma_i^2 or 1) for the kappa or nu
// of band l (GPCC_MKG_NOISE reads it): it enters through dS alone, no other kind has an operand for it
template <int P, int NOFF, int KIND>
__device__ __forceinline__ void gpcc_mkg_update(int b, double al, bool dh, double r, double s2, const double (&mu)[P + NOFF],
                                                const double (&C)[P + NOFF][P + NOFF], double (&dmu)[P + NOFF],
                                                double (&dC)[P + NOFF][P + NOFF], double &dll, double dvar = 0.0)
{
    constexpr int NS = P + NOFF;
    double Ph[NS], dPh[NS];
#pragma unroll
    for (int i2 = 0; i2 < NS; ++i2) {
        double acc = al * GPCC_MK_SYM(C, i2, 0), dacc = al * GPCC_MK_SYM(dC, i2, 0);
#pragma unroll
        for (int c = 0; c < NOFF; ++c) {
            acc += (b == c) ? GPCC_MK_SYM(C, i2, P + c) : 0.0;
            dacc += (b == c) ? GPCC_MK_SYM(dC, i2, P + c) : 0.0;
        }
        Ph[i2] = acc;
        dPh[i2] = dacc;       // dC h so far
    }
    // (dvar in its place among the four, in one expression with the product, as s2 is in S's: a compile-time choice, never a + 0.0)
    double S = al * Ph[0] + s2, hm = al * mu[0], dS = KIND == GPCC_MKG_NOISE ? al * dPh[0] + dvar : al * dPh[0], dhm = al * dmu[0];
#pragma unroll
    for (int c = 0; c < NOFF; ++c) {
        S += (b == c) ? Ph[P + c] : 0.0;
        hm += (b == c) ? mu[P + c] : 0.0;
        dS += (b == c) ? dPh[P + c] : 0.0;
        dhm += (b == c) ? dmu[P + c] : 0.0;
    }
    if constexpr (KIND == GPCC_MKG_ALPHA) {
        dS += dh ? 2.0 * Ph[0] : 0.0;
        dhm += dh ? mu[0] : 0.0;
#pragma unroll
        for (int i2 = 0; i2 < NS; ++i2) dPh[i2] += dh ? GPCC_MK_SYM(C, i2, 0) : 0.0;
    }
    const double inv = 1.0 / S, g = (r - hm) * inv, dg = (-dhm - g * dS) * inv;
    dll -= 0.5 * (dS * inv - 2.0 * g * dhm - g * g * dS);
#pragma unroll
    for (int i2 = 0; i2 < NS; ++i2) {
        dmu[i2] += dPh[i2] * g + Ph[i2] * dg;
        const double ki = Ph[i2] * inv, dki = dPh[i2] * inv - ki * inv * dS;
#pragma unroll
        for (int k = i2; k < NS; ++k) dC[i2][k] -= dki * Ph[k] + ki * dPh[k];
    }
}

// one lane's walk: KIND of slot, tb: the band of an alpha or tau slot, rb / rr: the band whose rank among ties is rr instead of its
// index (rb = -1: none), handed to gpcc_mk_next<true>.  nz: the lane's noise policy, dt: its data policy (the walk's own copy: a policy
// may keep state from one observation to the next).  The alpha, rho and tau slots of gpcc_markov_grad (GpccMkPlain, GpccMkOwnData), of
// gpcc_markov_noise_grad (GpccMknLane) and of gpcc_markov_resample_grad (GpccMkrData) are this one walk; ARGS is the kernel's, read by
// the cursor as it is there
template <int P, int NOFF, int KIND, class ARGS, class NZ, class DT = GpccMkOwnData>
__device__ __forceinline__ double gpcc_mkg_walk(const ARGS &a, const GpccMkLane &ln, const NZ &nz, int tb, int rb, int rr, DT dt = DT())
{
    constexpr int NS = P + NOFF;
    const double rho = ln.rho;
    double lam, lam2, Q[P][P], mu[NS], C[NS][NS];
    if constexpr (DT::resampled)
        gpcc_mk_init<P, NOFF>(rho, dt.sigma_b, lam, lam2, Q, mu, C);
    else
        gpcc_mk_init<P, NOFF>(rho, a.sigma_b, lam, lam2, Q, mu, C);
    // the tangents: zero, except the rho lane's prior state (dPinf)
    double Qd[P][P], dmu[NS], dC[NS][NS];
    const double dlam = -lam / rho;
    gpcc_mkg_dstationary<P>(lam, lam2, KIND == GPCC_MKG_RHO ? dlam : 0.0, Qd);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        dmu[i] = 0.0;
#pragma unroll
        for (int j = 0; j < NS; ++j) dC[i][j] = (KIND == GPCC_MKG_RHO && i < P && j < P) ? Qd[i][j] : 0.0;
    }

    double ll = 0.0, dll = 0.0, sprev = 0.0;
    int bprev = -1;
    for (int j = 0; j < a.N; ++j) {
        const GpccMkPoint p = gpcc_mk_next<true>(a, ln, j, sprev, rb, rr);   // (leaves the point's shifted time in sprev)
        const int b = p.b;
        const GpccMkObs o = dt.take(ln, p, j, sprev);
        if (!o.kept) continue;   // not in the lane's data: bprev stays the band of its last observation
        const double d = o.d, s2 = nz.var(ln, b, o.s2);

        double A[P][P], Ad[P][P];
        gpcc_mk_transition<P>(lam, lam2, d, A);
        bool ad = false;
        if constexpr (KIND == GPCC_MKG_RHO) {
            ad = true;
            gpcc_mkg_dtransition_rate<P>(lam, lam2, d, dlam, Ad);
        } else if constexpr (KIND == GPCC_MKG_TAU) {
            const int dd = o.first ? 0 : (int)(bprev == tb) - (int)(b == tb);
            ad = dd != 0;
            gpcc_mkg_dtransition_lag<P>(lam, lam2, (double)dd, A, Ad);
        } else {
#pragma unroll
            for (int i2 = 0; i2 < P; ++i2)
#pragma unroll
                for (int k = 0; k < P; ++k) Ad[i2][k] = 0.0;
        }
        bprev = b;
        gpcc_mkg_propagate<P, NOFF, KIND>(A, Ad, ad, Q, Qd, mu, C, dmu, dC);
        gpcc_mk_propagate<P, NOFF>(A, Q, mu, C);
        gpcc_mkg_update<P, NOFF, KIND>(b, p.al, KIND == GPCC_MKG_ALPHA && b == tb, o.r, s2, mu, C, dmu, dC, dll);
        gpcc_mk_update<P, NOFF>(b, p.al, o.r, s2, mu, C, ll);
    }
    return dll;
}

template <int P, int NOFF>
__global__ void __launch_bounds__(256) gpcc_markov_grad(const GpccMarkovGradArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double gpcc_mkg_lds[];
    const GpccMkLane ln = gpcc_mk_open(a, gpcc_mkg_lds);
    const int L = a.L;

    // what this workgroup differentiates (uniform)
    const int slot = blockIdx.y;
    double dll;
    if (slot < L) {
        dll = gpcc_mkg_walk<P, NOFF, GPCC_MKG_ALPHA>(a, ln, GpccMkPlain(), slot, -1, 0);
    } else if (slot == L) {
        dll = gpcc_mkg_walk<P, NOFF, GPCC_MKG_RHO>(a, ln, GpccMkPlain(), -1, -1, 0);
    } else {
        const int q = slot - L - 1, tb = a.twice ? q >> 1 : q;
        dll = gpcc_mkg_walk<P, NOFF, GPCC_MKG_TAU>(a, ln, GpccMkPlain(), tb, a.twice ? tb : -1, (q & 1) ? L : -1);
    }
    if (ln.valid) a.slot[(long)slot * a.M + ln.row] = dll;
}

// ---- launches (gpcc_markov_grad_inst.hip: an object of its own) ----
// grid (g.blocks, slots) of gpcc_markov_grad<g.p, g.noff>, then the finish kernel over the M rows
hipError_t gpcc_markov_grad_launch(const GpccMkLaunch &g, int slots, const GpccMarkovGradArgs &a);
// the finish kernel alone, over the M rows of a: the rows [M][2L + 1] from the slots, for a family that fills gpcc_markov_grad's slots
hipError_t gpcc_markov_grad_finish_launch(hipStream_t s, const GpccMarkovGradArgs &a);
