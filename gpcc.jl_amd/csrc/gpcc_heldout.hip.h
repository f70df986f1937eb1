// gpcc_heldout.hip.h -- device code of the batched held-out log-likelihood and its delay average (gpcc_heldout_loglik_batch,
// DESIGN.md 4.13).
//
// Per row (tau, alpha, rho) the augmented system of DESIGN.md 4.5 -- the training points, then the T test points from the next tile
// boundary on -- is factorised COMPLETELY, in its own workspace slot, by the unchanged launch-per-step tile kernels (woodbury = 0):
//     [ K      kB* ]         test rows: sig2 = sigma*^2 + 1e-8 (Sobs* + JITTER), resid = y* - bbar* (the band's training offset)
//     [ kB*'   cB  ]
// The first nt tile columns leave the Schur complement Sigma_pred + JITTER I + diag(sigma*^2) in the trailing tiles and
// y* - mu_pred in z[test] (src/gpccfixdelay_marginaliseb.jl:259-325); factorising the trailing tiles as well -- the same left-looking
// loop continued to nta -- gives L22 (kept on the diagonal tiles: store_l) and w[test] = L22^-1 (y* - mu_pred).  Then
//   gpcc_heldout_finish   per row: logpdf(MvNormal(mu_pred, Sigma), y*) = -(T log 2pi + 2 sum log L22_ii + |w[test]|^2) / 2 over the T
//                         real test rows (padding never counted), in a fixed order; info = N + j for the j-th failed pivot of the test
//                         block (the training loglik stays valid), NaN where the row failed
//   gpcc_heldout_mix      the delay average log sum_m p_m exp(heldout_m): one running, max-shifted log-sum-exp over the rows in row order
//                         (rows with p = 0 skipped), carried from group to group, so that it does not depend on the grouping
// No atomics: every sum has a fixed order, so a result is bitwise repeatable.
#pragma once
#include "gpcc_kernels.hip.h"

#define GPCC_HELD_THREADS 256

// hld: heldout per batch row (M); mix: the mixture state [max, scaled sum, NaN flag, result]; T: real test points; N: training points;
// off: the first test row of the augmented system (the handle's Np)
struct GpccHeldBuf {
    double *hld, *mix;
    int T, N, off;
};

// one workgroup per row of the group (grid cnt, GPCC_HELD_THREADS threads).  g.out_info holds the training info of the first nt
// diagonal steps (gpcc_diag_factor's last step of the training block); c.info the state after the whole augmented factorisation.
static __global__ __launch_bounds__(GPCC_HELD_THREADS) void gpcc_heldout_finish(GpccCtx c, GpccGroup g, GpccHeldBuf hb)
{
    const int m = (int)blockIdx.x;
    if (m >= g.cnt) return;
    const int slot = g.slot0 + m, row = g.first + m, tid = (int)threadIdx.x;
    const int tinfo = g.out_info[row], inf = c.info[slot];
    if (tinfo != 0 || inf != 0) {   // training failure (info as gpcc_loglik_batch), or the j-th pivot of the test block: N + j
        if (tid == 0) {
            hb.hld[row] = __builtin_nan("");
            if (tinfo == 0) g.out_info[row] = hb.N + (inf - hb.off);
        }
        return;
    }
    const double *tiles = (const double *)c.tiles + (long)slot * c.slot_stride;
    const double *w = c.w + (long)slot * c.Np;
    double ls = 0.0, qs = 0.0;
    for (int j = tid; j < hb.T; j += GPCC_HELD_THREADS) {   // strided in a fixed order per thread
        const int i = hb.off + j, K = i / GPCC_TILE, r = i % GPCC_TILE;
        ls += log(tiles[gpcc_tile_off(K, K) + gpcc_elem_off<double>(r, r)]);
        qs = fma(w[i], w[i], qs);
    }
    __shared__ double sl[GPCC_HELD_THREADS], sq[GPCC_HELD_THREADS];
    sl[tid] = ls;
    sq[tid] = qs;
    __syncthreads();
    for (int h = GPCC_HELD_THREADS / 2; h > 0; h >>= 1) {   // fixed pairwise tree
        if (tid < h) {
            sl[tid] += sl[tid + h];
            sq[tid] += sq[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double log2pi = 1.8378770664093454835606594728112;
        hb.hld[row] = -((double)hb.T * log2pi + 2.0 * sl[0] + sq[0]) / 2.0;
    }
}

// The delay average over the group's rows, in row order (grid 1, one wave; thread 0 works).  p: the normalised weights of the batch.
// State: mx = the largest log p_m + heldout_m so far, s = sum exp(log p + heldout - mx), nan = a failed row with p > 0 was met.  One row
// of weight 1 gives its own value bitwise (log 1 = 0, s = 1).  first: the batch's first group (initialises the state); last: writes
// the result mix[3].
static __global__ __launch_bounds__(64) void gpcc_heldout_mix(GpccGroup g, GpccHeldBuf hb, const double *p, int first, int last)
{
    if (threadIdx.x != 0) return;
    double mx = first ? -__builtin_inf() : hb.mix[0], s = first ? 0.0 : hb.mix[1], nan = first ? 0.0 : hb.mix[2];
    for (int m = 0; m < g.cnt; ++m) {
        const double pm = p[g.first + m];
        if (pm == 0.0) continue;
        const double x = hb.hld[g.first + m];
        if (x != x) {
            nan = 1.0;
            continue;
        }
        const double lx = log(pm) + x;
        if (lx == -__builtin_inf()) continue;   // contributes nothing
        if (s == 0.0) {
            mx = lx;
            s = 1.0;
        } else if (lx <= mx) {
            s += exp(lx - mx);
        } else {
            s = fma(s, exp(mx - lx), 1.0);
            mx = lx;
        }
    }
    hb.mix[0] = mx;
    hb.mix[1] = s;
    hb.mix[2] = nan;
    if (last) hb.mix[3] = (nan != 0.0) ? __builtin_nan("") : (s == 0.0 ? -__builtin_inf() : mx + log(s));
}
