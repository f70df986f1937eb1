// gpcc_pred.hip.h -- device code of the batched posterior predictive and its delay average (gpcc_predict_batch).
//
// Per row (tau, alpha, rho) and test point j (band q, time t*_j), with K = Kd + Sobs (+ B), w = K^-1 (Y - bbar) and
// kB*_ij = alpha_p alpha_q k(s_ij) (+ Sigma_b_p if p == q and b is marginalised), s_ij = (t_i - tau_p) - (t*_j - tau_q):
//     mu_j  = kB*_j' w + mu_b_q                                    (src/gpccfixdelay_marginaliseb.jl:283-285)
//     var_j = alpha_q^2 k(0) (+ Sigma_b_q) - |L^-1 kB*_j|^2 + 1e-8   (the diagonal of :275-279, JITTER :69)
// After the assembly, factorisation, triangular inverse and w of the gradient path (gpcc_grad.hip.h: X = L^-1 in the slot's lower
// tiles and linv, w in gw), a group runs:
//   gpcc_pred_tiles<KID>   per (training tile row I, test tile J): V_IJ = sum_{K <= I} X_IK kB*_KJ in the accumulators
//                          (v_mfma_f64_16x16x4_f64; the tiles of kB* generated into LDS, 64 rows at a time, as gpcc_hess_gemm generates
//                          D_theta), reduced to the 128 column sums of squares -> part[slot][I][J][128]; the workgroups of the last tile
//                          row (I = nt - 1, which generate every kB*_KJ) also form kB*_J' w
//   gpcc_pred_finish       per (slot, test point): var = (alpha_q^2 + Sigma_b_q - sum_I part) + 1e-8 with I ascending, mu = kB*' w + mu_b_q;
//                          NaN where the row failed (info != 0)
//   gpcc_pred_mix          the delay average, one thread per test point: the group's rows in row order into a running weighted mean
//                          and sum of squared deviations (West's update), so that the mixture does not depend on the grouping
// No atomics: every sum has a fixed order, so a result is bitwise repeatable.  Padded training rows (band -1) have kB* = 0 and X rows
// of the identity: their V rows are exactly zero.  Padded test points (band -1) have kB* = 0 and are never written.
#pragma once
#include "gpcc_grad.hip.h"

#define GPCC_PRED_LDW 144   // LDS row of a generated kB* tile: 128 doubles + 16 (gpcc_hess_gemm's padding)

// tt, tb: the shared test points, padded to Tp = ntT * 128 (band -1); part: nt * ntT * 128 partials per slot; mu, var: Tp per slot
// (mu holds kB*' w until the finish adds mu_b); gw: w per slot (the gradient's); mix: W, mean, S, V, then mix_mu, mix_var (Tp each)
struct GpccPredBuf {
    const double *tt, *gw;
    const int *tb;
    double *part, *mu, *var, *mix;
    int T, Tp, ntT;
    double mean_b[GPCC_MAXL];
};

// a per-band value of a kernel argument without a dynamic index into it
__device__ __forceinline__ double gpcc_pred_band_val(const double (&v)[GPCC_MAXL], int b)
{
    double r = 0.0;
#pragma unroll
    for (int l = 0; l < GPCC_MAXL; ++l) r = (b == l) ? v[l] : r;
    return r;
}

// V_IJ = sum_{K <= I} X_IK kB*_KJ (grid: cnt x nt x ntT, I descending -- the longest rows first -- then J fastest, so that the
// workgroups running together share the tile row I of X; 512 threads).  Wave w holds rows 16w .. 16w+15 of V, all 128 test columns
// (C/D: row 16w + q + 4 reg, column 16 f + lane & 15).  A operand X_IK[i][k] from the swizzled tile (gpcc_grad_trtri's read of X_IK),
// B operand kB*[k][j] from LDS.  X_II is lower triangular: wave w stops at column 16w + 15 of it.
template <int KID>
__global__ __launch_bounds__(512) void gpcc_pred_tiles(GpccCtx c, GpccGroup g, GpccPredBuf pb)
{
    const int nt = c.nt, ntT = pb.ntT;
    const long per = (long)nt * ntT;
    const int m = (int)(blockIdx.x / per), rem = (int)(blockIdx.x % per);
    const int I = nt - 1 - rem / ntT, J = rem % ntT;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m;
    if (c.info[slot] != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, q = lane >> 4;
    const int L = c.L;
    __shared__ double sD[64 * GPCC_PRED_LDW];
    __shared__ double suJ[GPCC_TILE], saJ[GPCC_TILE], sbtJ[GPCC_TILE], sal[GPCC_MAXL], sdl[GPCC_MAXL];
    __shared__ int sbJ[GPCC_TILE];
    const double *dl = g.delays + (long)(g.first + m) * L, *al = g.alpha + (long)(g.first + m) * L;
    if (tid < GPCC_TILE) {
        const long gj = (long)J * GPCC_TILE + tid;
        const int b = pb.tb[gj];
        sbJ[tid] = b;
        suJ[tid] = (b >= 0) ? pb.tt[gj] - dl[b] : 0.0;
        saJ[tid] = (b >= 0) ? al[b] : 0.0;
        sbtJ[tid] = (b >= 0) ? gpcc_fold_bterm(c, b) : 0.0;
    }
    if (tid < L) { sal[tid] = al[tid]; sdl[tid] = dl[tid]; }
    const double kscale = gpcc_kernel_scale<KID>(gpcc_kernel_const<KID>(g.rho[g.first + m]));
    const double *tiles = (const double *)c.tiles + (long)slot * c.slot_stride;
    const double *lin = (const double *)c.linv;
    const double *wv = pb.gw + (long)slot * c.Np;
    const bool with_mean = (I == nt - 1);
    double msum = 0.0;
    d4 acc[8];
#pragma unroll
    for (int f = 0; f < 8; ++f) acc[f] = d4{0.0, 0.0, 0.0, 0.0};
    const int jc = tid & 127, kr0 = tid >> 7;
    for (int K = 0; K <= I; ++K) {
        const double *XA = (K < I) ? tiles + gpcc_tile_off(I, K) : lin + gpcc_linv_off(c, slot, I);
        const int kend = (K < I) ? GPCC_TILE : 16 * w + 16;
        for (int h = 0; h < 2; ++h) {
            const int kbase = K * GPCC_TILE + 64 * h;
            __syncthreads();   // (the previous rows consumed; the column data ready)
            const int qb = sbJ[jc];
            const double uj = suJ[jc], aj = saJ[jc], btj = sbtJ[jc];
#pragma unroll 4
            for (int x = 0; x < 16; ++x) {
                const int kr = kr0 + 4 * x;
                const int p = c.band[kbase + kr];
                double v = 0.0;
                if (p >= 0 && qb >= 0) {
                    v = (sal[p] * aj) * gpcc_kernel_eval_scaled<KID>(c.t[kbase + kr] - sdl[p], uj, kscale);
                    if (p == qb) v = v + btj;
                }
                sD[kr * GPCC_PRED_LDW + jc] = v;
                if (with_mean) msum = fma(v, wv[kbase + kr], msum);
            }
            __syncthreads();
            const int kn = min(64, kend - 64 * h);   // (wave-uniform)
#pragma unroll 4
            for (int k0 = 0; k0 < kn; k0 += 4) {
                const double a = gpcc_gld(XA, 16 * w + lr, 64 * h + k0 + q);
                double b[8];
#pragma unroll
                for (int f = 0; f < 8; ++f) b[f] = sD[(k0 + q) * GPCC_PRED_LDW + 16 * f + lr];
#pragma unroll
                for (int f = 0; f < 8; ++f) acc[f] = GpccP64::mfma(a, b[f], acc[f]);
            }
        }
    }
    // column sums of squares: the four rows of a lane, the four row quarters (lanes lr + 16 q), then the eight waves in order
    __syncthreads();
    double *sred = sD, *smean = sD + 8 * GPCC_TILE;
#pragma unroll
    for (int f = 0; f < 8; ++f) {
        double s = acc[f][0] * acc[f][0];
#pragma unroll
        for (int r = 1; r < 4; ++r) s = fma(acc[f][r], acc[f][r], s);
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        if (q == 0) sred[w * GPCC_TILE + 16 * f + lr] = s;
    }
    if (with_mean) smean[kr0 * GPCC_TILE + jc] = msum;
    __syncthreads();
    if (tid < GPCC_TILE) {
        double s = sred[tid];
        for (int ww = 1; ww < 8; ++ww) s += sred[ww * GPCC_TILE + tid];
        pb.part[(((long)slot * nt + I) * ntT + J) * GPCC_TILE + tid] = s;
        if (with_mean)
            pb.mu[(long)slot * pb.Tp + (long)J * GPCC_TILE + tid] =
                ((smean[tid] + smean[GPCC_TILE + tid]) + smean[2 * GPCC_TILE + tid]) + smean[3 * GPCC_TILE + tid];
    }
}

// var and mu of every real test point of a row (grid: cnt x ntT; 128 threads); NaN where the row failed
static __global__ __launch_bounds__(GPCC_TILE) void gpcc_pred_finish(GpccCtx c, GpccGroup g, GpccPredBuf pb)
{
    const int m = (int)blockIdx.x / pb.ntT, J = (int)blockIdx.x % pb.ntT;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m, j = J * GPCC_TILE + (int)threadIdx.x;
    if (j >= pb.T) return;
    double *mu = pb.mu + (long)slot * pb.Tp, *var = pb.var + (long)slot * pb.Tp;
    if (c.info[slot] != 0) {
        mu[j] = var[j] = __builtin_nan("");
        return;
    }
    const int qb = pb.tb[j];
    const double a = g.alpha[(long)(g.first + m) * c.L + qb];
    double s = 0.0;
    for (int I = 0; I < c.nt; ++I) s += pb.part[(((long)slot * c.nt + I) * pb.ntT + J) * GPCC_TILE + threadIdx.x];
    const double cb = a * a + gpcc_fold_bterm(c, qb);   // k(0) = 1 for every kernel
    var[j] = (cb - s) + 1e-8;
    mu[j] = mu[j] + gpcc_pred_band_val(pb.mean_b, qb);
}

// The delay average over the group's rows, in row order (grid: ntT; 128 threads).  p: the normalised weights of the batch; rows with
// p = 0 are skipped (failed ones too).  State per test point: W = sum p, the weighted mean, S = sum p (mu - mean)^2 (West's update) and
// V = sum p var.  last: also writes mix_mu = mean, mix_var = (V + S) / W.  One row of weight 1 gives its own mu and var bitwise.
static __global__ __launch_bounds__(GPCC_TILE) void gpcc_pred_mix(GpccGroup g, GpccPredBuf pb, const double *p, int last)
{
    const int j = (int)blockIdx.x * GPCC_TILE + (int)threadIdx.x;
    if (j >= pb.T) return;
    const long Tp = pb.Tp;
    double W = pb.mix[j], mean = pb.mix[Tp + j], S = pb.mix[2 * Tp + j], V = pb.mix[3 * Tp + j];
    for (int m = 0; m < g.cnt; ++m) {
        const double pm = p[g.first + m];
        if (pm == 0.0) continue;
        const long o = (long)(g.slot0 + m) * Tp + j;
        const double x = pb.mu[o], v = pb.var[o];
        W += pm;
        const double d = x - mean;
        mean += (pm / W) * d;
        S += pm * d * (x - mean);
        V += pm * v;
    }
    pb.mix[j] = W; pb.mix[Tp + j] = mean; pb.mix[2 * Tp + j] = S; pb.mix[3 * Tp + j] = V;
    if (last) {
        pb.mix[4 * Tp + j] = mean;
        pb.mix[5 * Tp + j] = (V + S) / W;
    }
}
