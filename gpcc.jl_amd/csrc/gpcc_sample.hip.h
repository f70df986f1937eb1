// gpcc_sample.hip.h -- device code of the joint posterior light-curve draws (gpcc_sample_batch).
//
// Per drawn row (tau, alpha, rho) the held-out path's augmented system [training | test] (gpcc_heldout.hip.h) is factorised completely,
// with a test residual of 0 and L22's diagonal tiles kept (store_l):
//     L_aug = [ L11  0  ]      L22 = chol(Sigma_pred + JITTER I + diag(sigma*^2)),  w1 = L11^-1 (Y - bbar) in c.w
//             [ L21 L22 ]
// and one draw is  f* = bbar* + L21 w1 + L22 zeta,  zeta ~ N(0, I_T)  (src/gpccfixdelay_marginaliseb.jl:259-289 plus chol(Sigma) zeta).
//   gpcc_sample_mean    per (row, test tile J): mean_J = bbar*_band + sum_{K < ntr} L_JK w1_K, once per row and tile (not per draw)
//   gpcc_sample_tiles   per (row, test tile J, block of <= 128 of the row's draws): Y_J = sum_{K <= J} L22_JK zeta_K in
//                       v_mfma_f64_16x16x4_f64 accumulators (gpcc_pred_tiles' operand scheme: A = L22_JK from the swizzled tiles,
//                       B = zeta_K generated into LDS by Philox, gpcc_rng.h), then f* = mean_J + Y_J written for the real test rows
// Row failures (info != 0) give NaN draws; zeta is still written when asked for (the host fallback redraws with it).  No atomics:
// every sum has a fixed order, and a draw's column of the product does not depend on the other columns of its block, so a draw's
// bits depend on (seed, row, s) alone -- not on S, the grouping or the slot options.
#pragma once
#include "gpcc_pred.hip.h"
#include "gpcc_rng.h"

#define GPCC_SAMP_LDW 144   // LDS row of a generated zeta tile half: 128 doubles + 16 (gpcc_pred_tiles' padding)

// mean: slots x Tp (per slot: mean of the test rows); draws / zeta: output rows of T values; dlist: per batch row (compact order), the
// draw indices s of its draws ascending, concatenated; doff: M + 1 offsets into dlist; S: draws per row (per-row mode: output row
// m S + s); mixture: 1 -> output row s, counter row word 2^64 - 1; ntr: training tile columns (the test block starts at ntr * 128);
// nblk: the largest number of 128-draw blocks of a row of the group
struct GpccSampBuf {
    double *mean, *draws, *zeta;
    const int *dlist, *doff;
    unsigned long long seed;
    int T, Tp, ntT, ntr, S, mixture, nblk;
    double mean_b[GPCC_MAXL];
};

// mean_J of every row of the group (grid: cnt x ntT; 512 threads: thread (r, part) sums tile columns K = part, part + 4, ... of row r,
// then the four parts in order)
static __global__ __launch_bounds__(512) void gpcc_sample_mean(GpccCtx c, GpccGroup g, GpccSampBuf sb)
{
    const int m = (int)blockIdx.x / sb.ntT, J = (int)blockIdx.x % sb.ntT;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m, tid = (int)threadIdx.x, r = tid & 127, part = tid >> 7;
    if (c.info[slot] != 0) return;
    const double *tiles = (const double *)c.tiles + (long)slot * c.slot_stride;
    const double *w = c.w + (long)slot * c.Np;
    const int I = sb.ntr + J;
    double s = 0.0;
    for (int K = part; K < sb.ntr; K += 4) {
        const double *X = tiles + gpcc_tile_off(I, K);
        const double *wk = w + (long)K * GPCC_TILE;
#pragma unroll 8
        for (int col = 0; col < GPCC_TILE; ++col) s = fma(gpcc_gld(X, r, col), wk[col], s);
    }
    __shared__ double sp[512];
    sp[tid] = s;
    __syncthreads();
    if (tid < GPCC_TILE) {
        const int j = J * GPCC_TILE + r;
        const int b = c.band[(long)sb.ntr * GPCC_TILE + j];
        const double v = ((sp[r] + sp[128 + r]) + sp[256 + r]) + sp[384 + r];
        sb.mean[(long)slot * sb.Tp + j] = (b >= 0) ? gpcc_pred_band_val(sb.mean_b, b) + v : 0.0;
    }
}

// Y_J = sum_{K <= J} L22_JK zeta_K for one block of a row's draws (grid: cnt x ntT x nblk, J descending -- the longest first; 512
// threads).  Wave w holds rows 16w .. 16w+15 of Y_J, all 128 draw columns (C/D: row 16w + q + 4 reg, column 16 f + lane & 15).
// zeta_K is generated 64 rows at a time: thread (column jc, quad group qg) forms the Philox blocks qg, qg + 4, qg + 8, qg + 12 of the
// half.  L22_JJ is lower triangular (store_l writes zeros above the diagonal): wave w stops at column 16w + 15 of it.
__global__ __launch_bounds__(512) void gpcc_sample_tiles(GpccCtx c, GpccGroup g, GpccSampBuf sb)
{
    const int ntT = sb.ntT, nblk = sb.nblk;
    const long per = (long)ntT * nblk;
    const int m = (int)(blockIdx.x / per), rem = (int)(blockIdx.x % per);
    const int J = ntT - 1 - rem / nblk, d = rem % nblk;
    if (m >= g.cnt) return;
    const int row = g.first + m, slot = g.slot0 + m;
    const int n0 = sb.doff[row] + GPCC_TILE * d, nd = sb.doff[row + 1] - n0;
    if (nd <= 0) return;
    const int ncol = nd < GPCC_TILE ? nd : GPCC_TILE;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, q = lane >> 4;
    const bool ok = c.info[slot] == 0;
    __shared__ double sZ[64 * GPCC_SAMP_LDW];
    __shared__ int sOut[GPCC_TILE];
    __shared__ unsigned long long sS[GPCC_TILE];
    if (tid < GPCC_TILE) {
        const int s = (tid < ncol) ? sb.dlist[n0 + tid] : 0;
        sS[tid] = (unsigned long long)s;
        sOut[tid] = sb.mixture ? s : row * sb.S + s;
    }
    const unsigned long long mrow = sb.mixture ? ~0ULL : (unsigned long long)row;
    const double *tiles = (const double *)c.tiles + (long)slot * c.slot_stride;
    const int T = sb.T, I = sb.ntr + J;
    d4 acc[8];
#pragma unroll
    for (int f = 0; f < 8; ++f) acc[f] = d4{0.0, 0.0, 0.0, 0.0};
    const int jc = tid & 127, qg = tid >> 7;
    for (int K = (ok ? 0 : J); K <= J; ++K) {
        const double *XA = tiles + gpcc_tile_off(I, sb.ntr + K);
        const int kend = (K < J) ? GPCC_TILE : 16 * w + 16;
        for (int h = 0; h < 2; ++h) {
            __syncthreads();   // (the previous half consumed; sS ready)
            const unsigned long long s = sS[jc];
#pragma unroll 2
            for (int x = 0; x < 4; ++x) {
                const int qi = qg + 4 * x, kr = 4 * qi;                   // rows kr .. kr + 3 of the half
                const int j0 = K * GPCC_TILE + 64 * h + kr;               // their test indices
                double z[4] = {0.0, 0.0, 0.0, 0.0};
                if (jc < ncol && j0 < T) gpccrng::normal4(sb.seed, (unsigned long long)(j0 >> 2), s, mrow, z);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double v = (j0 + e < T) ? z[e] : 0.0;
                    sZ[(kr + e) * GPCC_SAMP_LDW + jc] = v;
                    if (K == J && sb.zeta && jc < ncol && j0 + e < T) sb.zeta[(long)sOut[jc] * T + j0 + e] = v;
                }
            }
            __syncthreads();
            if (!ok) continue;
            const int kn = min(64, kend - 64 * h);   // (wave-uniform)
#pragma unroll 4
            for (int k0 = 0; k0 < kn; k0 += 4) {
                const double a = gpcc_gld(XA, 16 * w + lr, 64 * h + k0 + q);
                double b[8];
#pragma unroll
                for (int f = 0; f < 8; ++f) b[f] = sZ[(k0 + q) * GPCC_SAMP_LDW + 16 * f + lr];
#pragma unroll
                for (int f = 0; f < 8; ++f) acc[f] = GpccP64::mfma(a, b[f], acc[f]);
            }
        }
    }
    // f* = mean_J + Y_J through LDS, 64 draw columns at a time (sO[col][row], stride 129), then each draw's 128 test rows contiguous
    const double *mean = sb.mean + (long)slot * sb.Tp + (long)J * GPCC_TILE;
    double *sO = sZ;
    for (int hc = 0; hc < 2; ++hc) {
        __syncthreads();
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r) sO[(16 * f + lr) * 129 + 16 * w + q + 4 * r] = acc[4 * hc + f][r];
        __syncthreads();
        for (int idx = tid; idx < 64 * GPCC_TILE; idx += 512) {
            const int col = idx >> 7, rr = idx & 127, cg = 64 * hc + col, j = J * GPCC_TILE + rr;
            if (cg < ncol && j < T) sb.draws[(long)sOut[cg] * T + j] = ok ? mean[rr] + sO[col * 129 + rr] : __builtin_nan("");
        }
    }
}
